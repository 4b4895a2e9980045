"""The synchronised BatchNorm kernels of csrc/stride2.hip (ngan_bn_moments -> ngan_bn_merge_fold forward, ngan_bn_act_bwd_partial ->
ngan_bn_act_bwd_merged backward): inputs, partitions of the pixel range, fp64 references with their absolute-value twins, the
per-element bound, numpy emulations in kernel order and their deliberately wrong variants.  Shared by
tests/test_gpu_sync_bn_kernels.py (the kernels against the references) and tests/test_sync_bn_bounds_cpu.py (the emulations against
the references: it settles the constants on the CPU before any kernel is looked at, and shows that the bound can fail).

Inputs: the BatchNorm family of tests/wgan_cases.py (mean / sigma = 0, 3, 1000 by channel, channel 1 constant) with one extension:
in the designated channels (3, 4, 5; channel 0 where C = 3 or 1) the FIRST PIXEL OF EVERY PART lies six sigma from the channel mean,
on alternating sides, because every rank pivots its sums on its own first pixel.

Bound, per element:   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref,   C_ACC = 8   (as tests/wgan_cases.py)
n_round per output, read from csrc/stride2.hip (bn_stats_stage1<false> / bn_moments_finish, bn_merge_fold_kernel, chan_reduce_stage1<1> /
bn_bwd_partial_finish, bn_bwd_merged_finish / bn_act_bwd_apply):
  moments count                   exact (n_round 0, absref 0: the bound is 0)
          mean, M2                fp64 throughout; held to the fp32 form with one rounding                                        1
  merge   mean                    (float) of the fp64 merged mean                                                                 1
          rstd                    (float)(1 / sqrt(var + eps)), all fp64 inside                                                   1
          scale                   gamma * rstd: one more product                                                                  2
          shift                   beta - mean * scale                                                                             1
          running_mean / _var     (float) of the fp64 update, the unbiased factor from the global count                           1
          n_total, num_batches_tracked   exact
  bn_act_apply a                  act(fmaf(scale, y, shift)): the fma, the slope product                                          2
  bwd_partial S0, S1              fp32 sums inside a chunk (the accumulation term), the chunks and nothing after them in fp64     1
  bwd_merged gy                   k1 * (gz - m0 - xhat * m1): the subtraction, the product, k1 = gamma * rstd rounded             3
          dgamma, dbeta           (float) of this rank's own record                                                               1
          dgamma_sum, dbeta_sum   the ranks' shares added in fp64 by the test against the whole tensor's sums: every share's
                                  rounding is at most 2^-24 of its own absref, together one of the eight units of C_ACC           1
The merged statistics round once per stored value, so their counts are smaller than bn_stats's (2 / 3 / 4 / 1 / 1 / 1).

The backward starts from statistics the test fixes (the fp64 ones of the whole tensor rounded to fp32), so it is pinned independently
of the forward.  LeakyReLU takes the kernel's own sign pattern, sign(fmaf(scale, y, shift)), as in wgan_cases: no element is excluded.

RAISED lists the (output, case) whose emulated worst err / bound exceeds 0.5 with C_ACC = 8, with the next power of two that brings it
to 0.5 or below and the emulated ratio there (the convention of wgan_cases.RAISED).  No entry is specific to the outlier pivots."""
import functools

import numpy as np

import fp64_conv as R
import wgan_cases as W

SLOPE = W.SLOPE
C_ACC = W.C_ACC
f32, f64 = np.float32, np.float64
# (output, case id) -> (raised C_ACC, emulated worst err / bound at that constant)
RAISED = {
}

# (C, the ranks' pixel counts in rank order).  chunk = ceil(16384 / C) pixels per workgroup, L = 256 // C pixel lanes per channel.
CASES = [
    (1, (1,)),                          # one pixel in all: M2 = 0, no unbiased variance
    (1, (5, 278533, 1, 300)),           # L = 256: 5 pixels < L; 17 chunks of 16384 and a ragged 18th; a single pixel
    (3, (614, 1434)),                   # the 0.3 / 0.7 split, one chunk each
    (3, (10931, 40, 1)),                # chunk 5462: two chunks and a ragged third; 40 < L = 85; a single pixel
    (8, (1229, 2867)),                  # one chunk each, L = 32
    (16, (4096, 4096)),                 # an equal split (four chunks each): equal-weight means are right here and only here
    (16, (4915, 11469)),                # chunk 1024: 5 and 12 chunks (fewer than 16), both ragged
    (17, (16391, 10, 1, 964)),          # chunk 964: 17 chunks and a ragged 18th; 10 < L = 15; 1; one chunk exactly.  Two blocks of
                                        # sum_parts_f64, the second with 15 idle channels
    (64, (4920, 11480)),                # chunk 256: 20 and 45 chunks, both ragged
    (129, (1, 385, 1200)),              # L = 1 with 127 idle threads, chunk 128: a single pixel; 4 chunks; 10 chunks
    (256, (1281, 1, 63, 500)),          # L = 1, chunk 64: 20 chunks and a ragged 21st; a single pixel; under a chunk; 8 chunks
    (300, (113, 1, 1000)),              # two passes of the cbase loop, chunk 55: 3 chunks; a single pixel; 18 and a ragged 19th
    (1024, (16400,)),                   # 1025 chunks of 16 -> red_chunk's cap: 965 chunks of 17 (wgan_cases' C1024-npix16400)
]


def case_id(case):
    return f"C{case[0]}-p" + "+".join(str(p) for p in case[1])


def case_of(cid):
    return next(c for c in CASES if case_id(c) == cid)


def c_acc(name, cid):
    return float(RAISED.get((name, cid), (C_ACC, None))[0])


def edges(parts):
    return [int(v) for v in np.concatenate([[0], np.cumsum(parts)])]


def slices(parts):
    e = edges(parts)
    return [slice(a, b) for a, b in zip(e[:-1], e[1:])]


def red_chunk(npix, C):
    """(chunk, nparts) of csrc/stride2.hip's red_chunk: about 16K elements per workgroup, at most 1024 workgroups"""
    chunk = max(1, (16384 + C - 1) // C)
    nparts = (npix + chunk - 1) // chunk
    if nparts > 1024:
        chunk = (npix + 1023) // 1024
        nparts = (npix + chunk - 1) // chunk
    return chunk, nparts


def lanes_of(C):
    return 256 // C if C <= 256 else 1


def options(case):
    i = CASES.index(case)
    return dict(momentum=(0.1, 0.37)[i % 2], eps=(1e-5, 1e-3)[(i // 2) % 2], track=(i % 3) != 2)


@functools.lru_cache(maxsize=2)
def inputs(case):
    """y (npix, C), g, gamma, beta, running buffers; six / const: the designated channels"""
    C, parts = case
    npix = sum(parts)
    g = W._gen(77000 + 31 * C + npix)
    sigma = (W._rand(g, C) * f32(1.5) + f32(0.5)).astype(f32)
    mean = (np.array([0.0, 3.0, 1000.0], f32)[np.arange(C) % 3] * sigma).astype(f32)
    y = (W._randn(g, npix, C) * sigma + mean).astype(f32)
    six = [c for c in (3, 4, 5) if c < C] or ([0] if (C == 3 or (C == 1 and npix > 1)) else [])
    const = [1] if C > 1 else []
    for r, first in enumerate(edges(parts)[:-1]):
        for c in six:
            y[first, c] = mean[c] + f32(6 if r % 2 == 0 else -6) * sigma[c]
    for c in const:
        y[:, c] = f32(3.1) * sigma[c]
    return dict(y=y, g=W._randn(g, npix, C), gamma=(W._randn(g, C) * f32(0.1) + f32(1)).astype(f32),
                beta=(W._randn(g, C) * f32(0.1)).astype(f32), run_mean=W._randn(g, C), run_var=W._rand(g, C) + f32(0.5), six=six, const=const)


# ---- fp64 references ---------------------------------------------------------------------------------------------------------------
def part_moments_ref(yp):
    """{count, mean, M2} of one part alone: two-pass in fp64, the first pass about the part's first pixel (exact for a constant
    channel and for a single pixel); each (ref, absref, n_round)"""
    y64 = yp.astype(f64)
    m = y64[0] + (y64 - y64[0]).mean(0)
    dev = y64 - m
    m2 = (dev * dev).sum(0)
    n = np.array([float(yp.shape[0])])
    return {"count": (n, np.zeros(1), 0), "mean": (m, np.abs(y64).mean(0), 1), "M2": (m2, m2, 1)}


EXACT = ("n_total", "num_batches_tracked")


def merge_refs(d, o, nbt_before=0):
    """everything bn_merge_fold writes, from the whole tensor"""
    eps, mom = float(f32(o["eps"])), float(f32(o["momentum"]))
    rm, rv = (W._t(d["run_mean"]), W._t(d["run_var"])) if o["track"] else (None, None)
    args = (W._t(d["y"]), W._t(d["gamma"]), W._t(d["beta"]), eps, mom, rm, rv)
    s, a = R.bn_stats(*args), R.bn_stats_abs(*args)
    n = {"mean": 1, "rstd": 1, "scale": 2, "shift": 1, "running_mean": 1, "running_var": 1}
    out = {k: (W._n(s[k]), W._n(a[k]), n[k]) for k in n if k in s}
    out["n_total"] = (np.array([float(d["y"].shape[0])]), np.zeros(1), 0)
    out["num_batches_tracked"] = (np.array([float(nbt_before + (1 if o["track"] else 0))]), np.zeros(1), 0)
    return out


def fixed_stats(d, o):
    """the statistics handed to the backward kernels: the whole tensor's fp64 ones rounded to fp32, scale and shift formed from those"""
    s = R.bn_stats(W._t(d["y"]), W._t(d["gamma"]), W._t(d["beta"]), float(f32(o["eps"])))
    mean, rstd = W._n(s["mean"]).astype(f32), W._n(s["rstd"]).astype(f32)
    scale = (d["gamma"] * rstd).astype(f32)
    return dict(mean=mean, rstd=rstd, scale=scale, shift=(d["beta"] - mean * scale).astype(f32))


def bwd_refs(d, st, act, parts):
    """whole: {gy, dgamma, dbeta} of the whole tensor (coefficients over the global count); per part: {S0, S1} = sum gz, sum gz xhat
    over that part with the handed (global) statistics -- the record, and the rank's dbeta / dgamma share"""
    y, g = d["y"], d["g"]
    mask = W.xf_mask(y, (st["scale"], st["shift"], act))
    ty, tg, tgam, tm, tr, tmask = W._t(y), W._t(g), W._t(d["gamma"]), W._t(st["mean"]), W._t(st["rstd"]), W._t(mask)
    gy, dg, db = R.bn_act_backward(ty, tg, tgam, None, tm, tr, SLOPE, mask=tmask)
    gya, dga, dba = R.bn_act_backward_abs(ty, tg, tgam, tm, tr, tmask)
    whole = {"gy": (W._n(gy), W._n(gya), 3), "dgamma": (W._n(dg), W._n(dga), 1), "dbeta": (W._n(db), W._n(dba), 1)}
    gz = g.astype(f64) * mask
    gx = gz * ((y.astype(f64) - st["mean"].astype(f64)) * st["rstd"].astype(f64))
    per = []
    for sl in slices(parts):
        per.append({"S0": (gz[sl].sum(0), np.abs(gz[sl]).sum(0), 1), "S1": (gx[sl].sum(0), np.abs(gx[sl]).sum(0), 1)})
    return whole, per


# ---- emulations in kernel order ----------------------------------------------------------------------------------------------------
def partials(a, b, chunk, dtype, drop_ragged=False):
    """chan_reduce_stage1 / bn_stats_stage1<false>: per chunk and channel the sum of a (b None) or of a * b through an fma, in `dtype`: L
    pixel lanes per channel, each sequential over its pixels i, i + L, ..., then the lanes in order.  (nparts, C)"""
    npix, C = a.shape
    nparts = -(-npix // chunk)
    L = lanes_of(C)
    steps = -(-chunk // L)

    def lay(v):
        p = np.zeros((nparts, steps * L, C), v.dtype)
        full = npix // chunk
        p[:full, :chunk] = v[:full * chunk].reshape(full, chunk, C)
        if full < nparts:
            p[full, :npix - full * chunk] = v[full * chunk:]
        return p.reshape(nparts, steps, L, C)

    pa, pb = lay(a), None if b is None else lay(b)
    lanes = np.zeros((nparts, L, C), dtype)
    for i in range(steps):
        if pb is None:
            lanes = lanes + pa[:, i].astype(dtype)
        else:       # fp32: the product of two fp32 numbers is exact in fp64, so this is the fused form; fp64: 2^-53 apart from it
            lanes = (lanes.astype(f64) + pa[:, i].astype(f64) * pb[:, i].astype(f64)).astype(dtype)
    part = np.zeros((nparts, C), dtype)
    for l in range(L):
        part = part + lanes[:, l]
    if drop_ragged and npix % chunk:
        part = part[:-1]
    return part


def sum_parts(part, drop_lanes16=False):
    """sum_parts_f64: 16 lanes per channel, lane l adds the chunk partials l, l + 16, ... in order, then the 16 lane sums in order.
    drop_lanes16: every lane stops after its first partial (the partials from 16 on are lost)"""
    nparts, C = part.shape
    lanes = np.zeros((16, C), f64)
    for k in range(min(nparts, 16) if drop_lanes16 else nparts):
        lanes[k % 16] = lanes[k % 16] + part[k].astype(f64)
    s = np.zeros(C, f64)
    for l in range(16):
        s = s + lanes[l]
    return s


def moments_emulate(yp, stage1="fp64", mutant=None):
    """ngan_bn_moments: sums of d = y - y[0] and d^2 per chunk (fp64; stage1 = "fp32": chan_reduce_stage1<0>, what the entry point
    launched before), the chunks added in fp64, M2 = s1 - s0 d"""
    npix, C = yp.shape
    chunk = red_chunk(npix, C)[0]
    dt = f32 if stage1 == "fp32" else f64
    dev = yp - yp[0] if dt is f32 else yp.astype(f64) - yp[0].astype(f64)
    drop = mutant == "drop_ragged"
    s0 = sum_parts(partials(dev, None, chunk, dt, drop), mutant == "drop_lanes16")
    s1 = sum_parts(partials(dev, dev, chunk, dt, drop), mutant == "drop_lanes16")
    dd = s0 / float(npix)
    return np.concatenate([[float(npix)], yp[0].astype(f64) + dd, np.maximum(s1 - s0 * dd, 0.0)])


def merge_emulate(recs, gamma, beta, eps, momentum, run_mean, run_var, mutant=None, rank=0):
    """bn_merge_fold_kernel on (world, 1 + 2C) records.  mutants: "no_d2" (the d^2 n nb / (n + nb) term dropped), "equal_means" (the
    means averaged with equal weights), "local_unbiased" (running_var's unbiased factor from rank `rank`'s own count)"""
    C = (recs.shape[1] - 1) // 2
    n, mu, m2 = recs[0, 0], recs[0, 1:1 + C].copy(), recs[0, 1 + C:].copy()
    for r in range(1, recs.shape[0]):
        nb = recs[r, 0]
        nn = n + nb
        dlt = recs[r, 1:1 + C] - mu
        mu = mu + dlt * (1.0 / (r + 1) if mutant == "equal_means" else nb / nn)
        m2 = m2 + recs[r, 1 + C:] + (0.0 if mutant == "no_d2" else dlt * dlt * (n * nb / nn))
        n = nn
    var = m2 / n
    rstd = (1.0 / np.sqrt(var + float(f32(eps)))).astype(f32)
    muf = mu.astype(f32)
    scale = (gamma * rstd).astype(f32)
    out = dict(mean=muf, rstd=rstd, scale=scale, shift=(beta - (muf * scale).astype(f32)).astype(f32), n_total=np.array([n]))
    if run_mean is not None:
        unb = m2 / (n - 1.0) if n > 1.0 else var
        if mutant == "local_unbiased":
            nl = recs[rank, 0]
            unb = var * (nl / (nl - 1.0)) if nl > 1.0 else var
        m = float(f32(momentum))
        out["running_mean"] = ((1.0 - m) * run_mean.astype(f64) + m * mu).astype(f32)
        out["running_var"] = ((1.0 - m) * run_var.astype(f64) + m * unb).astype(f32)
    return out


def _gz_xhat(yp, gp, st, act):
    """fp32 gz and xhat as chan_reduce_stage1<1> and bn_act_bwd_apply form them"""
    z = W._fma(np.broadcast_to(st["scale"], yp.shape), yp, np.broadcast_to(st["shift"], yp.shape))
    gz = np.where(z > 0, gp, gp * f32(SLOPE)).astype(f32) if act else gp
    return gz, ((yp - st["mean"]) * st["rstd"]).astype(f32)


def bwd_partial_emulate(yp, gp, st, act, mutant=None, eps=1e-5):
    """ngan_bn_act_bwd_partial: fp32 sums per chunk, the chunks in fp64.  mutant "local_xhat": xhat from this part's own statistics"""
    npix, C = yp.shape
    chunk = red_chunk(npix, C)[0]
    if mutant == "local_xhat":
        y64 = yp.astype(f64)
        own = y64.mean(0)
        st = dict(st, mean=own.astype(f32), rstd=(1.0 / np.sqrt(((y64 - own) ** 2).mean(0) + float(f32(eps)))).astype(f32))
    gz, xh = _gz_xhat(yp, gp, st, act)
    drop = mutant == "drop_ragged"
    return np.concatenate([sum_parts(partials(gz, None, chunk, f32, drop), mutant == "drop_lanes16"),
                           sum_parts(partials(gz, xh, chunk, f32, drop), mutant == "drop_lanes16")])


def bwd_merged_emulate(yp, gp, st, gamma, act, recs, rank, n_total, mutant=None):
    """ngan_bn_act_bwd_merged on (world, 2C) records.  mutants: "local_count" (the coefficients over this part's count),
    "dgamma_total" (dgamma / dbeta written as the total, not the own share)"""
    C = yp.shape[1]
    s = np.zeros(2 * C, f64)
    for r in range(recs.shape[0]):
        s = s + recs[r]
    n = float(yp.shape[0]) if mutant == "local_count" else float(n_total)
    k1 = (gamma * st["rstd"]).astype(f32)
    m0, m1 = (s[:C] / n).astype(f32), (s[C:] / n).astype(f32)
    gz, xh = _gz_xhat(yp, gp, st, act)
    own = s if mutant == "dgamma_total" else recs[rank]
    return {"gy": (k1 * ((gz - m0) - (xh * m1).astype(f32))).astype(f32), "dgamma": own[C:].astype(f32), "dbeta": own[:C].astype(f32)}


class Emulated:
    """the four launches in numpy, with the interface the GPU module implements over the kernels"""

    def __init__(self, mutant=None, stage1="fp64"):
        self.mutant, self.stage1 = mutant, stage1

    def moments(self, yp):
        return moments_emulate(yp, self.stage1, self.mutant)

    def merge(self, recs, d, o, rank=0):
        rm, rv = (d["run_mean"], d["run_var"]) if o["track"] else (None, None)
        out = merge_emulate(recs, d["gamma"], d["beta"], o["eps"], o["momentum"], rm, rv, self.mutant, rank)
        out["num_batches_tracked"] = np.array([1.0 if o["track"] else 0.0])
        return out

    def apply(self, y, scale, shift, act):
        return W.xf_emulate(y, (scale, shift, act))

    def bwd_partial(self, yp, gp, st, act, eps):
        return bwd_partial_emulate(yp, gp, st, act, self.mutant, eps)

    def bwd_merged(self, yp, gp, st, gamma, act, recs, rank, n_total):
        return bwd_merged_emulate(yp, gp, st, gamma, act, recs, rank, n_total, self.mutant)


# ---- the chains: every output of the launches, each against the fp64 reference of exactly its inputs -------------------------------
def forward_chain(case, impl, act=1, merge_rank=0):
    """per-part records -> merge -> stored activation.  Yields (output name, got, (ref, absref, n_round)); the merge is rank
    `merge_rank`'s (every rank merges the same gathered records)"""
    C, parts = case
    d, o = inputs(case), options(case)
    recs = []
    for sl in slices(parts):
        rec = np.asarray(impl.moments(d["y"][sl]), f64)
        ref = part_moments_ref(d["y"][sl])
        yield "moments/count", rec[:1], ref["count"]
        yield "moments/mean", rec[1:1 + C], ref["mean"]
        yield "moments/M2", rec[1 + C:], ref["M2"]
        recs.append(rec)
    got = impl.merge(np.stack(recs), d, o, merge_rank)
    refs = merge_refs(d, o)
    for k in refs:
        yield f"merge/{k}", got[k], refs[k]
    yield "bn_act_apply/a", impl.apply(d["y"], got["scale"], got["shift"], act), W.bn_apply_refs(d["y"], got["scale"], got["shift"], act)["a"]


def backward_chain(case, impl, act):
    """per-part backward records on the fixed statistics -> every rank's merged launch: its slice of gy, its shares; then gy
    reassembled and the shares added up against the whole tensor's gradients"""
    C, parts = case
    d, o = inputs(case), options(case)
    st = fixed_stats(d, o)
    whole, per = bwd_refs(d, st, act, parts)
    sls = slices(parts)
    recs = []
    for sl, ref in zip(sls, per):
        rec = np.asarray(impl.bwd_partial(d["y"][sl], d["g"][sl], st, act, o["eps"]), f64)
        yield "bwd_partial/S0", rec[:C], ref["S0"]
        yield "bwd_partial/S1", rec[C:], ref["S1"]
        recs.append(rec)
    recs = np.stack(recs)
    n_total = float(sum(parts))
    gys, dgs, dbs = [], [], []
    gy_ref, gy_abs, gy_n = whole["gy"]
    for r, (sl, ref) in enumerate(zip(sls, per)):
        got = impl.bwd_merged(d["y"][sl], d["g"][sl], st, d["gamma"], act, recs, r, n_total)
        got = {k: np.asarray(v) for k, v in got.items()}
        yield "bwd_merged/gy", got["gy"], (gy_ref[sl], gy_abs[sl], gy_n)
        yield "bwd_merged/dgamma", got["dgamma"], ref["S1"]
        yield "bwd_merged/dbeta", got["dbeta"], ref["S0"]
        gys.append(got["gy"])
        dgs.append(got["dgamma"].astype(f64))
        dbs.append(got["dbeta"].astype(f64))
    yield "bwd_merged/gy_whole", np.concatenate(gys), whole["gy"]
    yield "bwd_merged/dgamma_sum", sum(dgs), whole["dgamma"]
    yield "bwd_merged/dbeta_sum", sum(dbs), whole["dbeta"]


def ratio_at(got, ref, absref, n_round, c=C_ACC):
    return W.ratio_at(got, ref, absref, n_round, c)
