"""The WGAN kernels of csrc/stride2.hip (4x4 stride-2 convolutions, BatchNorm, channel reductions, stem): inputs, fp64 references with
their absolute-value twins, the per-element bound, fp32 emulations and their deliberately wrong variants.  Shared by
tests/test_gpu_wgan_kernels.py (the kernels against the references) and tests/test_wgan_bounds_cpu.py (the emulations against the
references: it settles the constants on the CPU before any kernel is looked at, and shows that the bound can fail).

Bound, per element:   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref,   C_ACC = 8   (as tests/wide_f32_cases.py)
  absref   the operator's formula with absolute values propagated through it: conv(|a|, |w|) + |bias| for the convolutions (a = the
           transformed input), the backward formula on |gz|, |xhat| and the sums of absolute values for the BatchNorm backward.  The
           variance is mean((y - mean)^2), a sum of squares of the centred values: it is its own twin, and so are rstd and scale.
  n_round  the fp32 roundings applied to the element AFTER its last addition or subtraction, that one's own included; the roundings
           before it act on the terms of that sum and are carried by the accumulation term.
n_round per output, read from csrc/stride2.hip:
  s2 conv y          acc + bias (the MFMA chain ends in an addition either way)                                                  1
          y, tanh    tanhf of it: the device library's tanh is within 2 ulp (|tanh'| <= 1 carries the argument's error)          2
  dgrad dx           the same kernel without bias                                                                                1
  s2 wgrad dW        the splits summed in order                                                                                  1
  chan_sum           chunk partials summed in order                                                                              1
  bn_stats mean      sum, division by n (the kernel: y[0] + s0 / n, one rounding after its last addition)                        2
           rstd      1 / sqrtf(var + eps): addition, sqrt, reciprocal                                                            3
           scale     gamma * rstd: one more product                                                                              4
           shift     beta - mean * scale                                                                                         1
           running_mean / running_var   (1 - m) * run + m * new                                                                  1
  bn_fold_eval scale gamma / sqrtf(var + eps): addition, sqrt, division                                                          3
           shift     beta - mean * scale                                                                                         1
  bn_act_apply       act(fmaf(scale, y, shift)): the fma, the slope product                                                      2
  bn_act_bwd dbeta / dgamma   sums                                                                                               1
           gy        k1 * (gz - m0 - xhat * m1): the subtraction, the product, k1 = gamma * rstd rounded                         3
           gy, no BatchNorm   g * slope                                                                                          1
  tanh_bwd           g * (1 - t t): the subtraction, the product  (absref |g| (1 + t t))                                         2
  stem y             butterfly sum + bias                                                                                        1
  stem gW / gb       fma chain / sum over the batch                                                                              1

LeakyReLU: every reference takes the kernel's own sign pattern, recomputed from the operator's inputs as the kernel computes it,
sign(fmaf(scale, y, shift)) (exact in fp64: the product of two fp32 numbers is exact and the sum keeps its sign), so no case has to
keep z off the kink.  Without an affine part the pattern is sign(y).

Statistics: the bound of rstd (and of scale, shift and running_var through it) follows from the operation: a centred two-pass
evaluation in fp32 meets it with a factor two (tests/test_wgan_bounds_cpu.py).  RAISED lists the (output, case) whose emulated worst
err / bound exceeds 0.5 with C_ACC = 8, with the next power of two that brings it to 0.5 or below and the emulated ratio there."""
import numpy as np
import torch

import fp64_conv as R

SLOPE = 0.2
C_ACC = 8.0
# (output, case id) -> (raised C_ACC, emulated worst err / bound at that constant)
RAISED = {
    # 17 pixels per chunk, then 965 chunk partials added in order: 0.940 / 0.794 / 1.253 / 1.471 with C_ACC = 8
    ("bn_stats/rstd", "C1024-npix16400"): (32.0, 0.346), ("bn_stats/scale", "C1024-npix16400"): (32.0, 0.318),
    ("bn_stats/shift", "C1024-npix16400"): (32.0, 0.369), ("bn_stats/running_var", "C1024-npix16400"): (32.0, 0.433),
    # shift = beta - mean * scale carries the errors of both factors: 0.527 / 0.503 / 0.515 with C_ACC = 8
    ("bn_stats/shift", "C129-npix128"): (16.0, 0.293), ("bn_stats/shift", "C256-npix65"): (16.0, 0.280),
    ("bn_stats/shift", "C300-npix55"): (16.0, 0.286),
    # 80 products rounded one by one in the emulation: 0.565 with C_ACC = 8
    ("s2_up/y", "up-g45-C20-M65-act-bias"): (16.0, 0.292),
}

f32, f64 = np.float32, np.float64


def c_acc(name, case_id):
    return float(RAISED.get((name, case_id), (C_ACC, None))[0])


def ratio_at(got, ref, absref, n_round, c=C_ACC):
    """(worst err / bound over the elements, its flat index); NaN counts as infinitely wrong"""
    got = np.asarray(got, dtype=f64)
    ref, absref = np.asarray(ref, dtype=f64), np.asarray(absref, dtype=f64)
    assert got.shape == ref.shape == absref.shape, (got.shape, ref.shape, absref.shape)
    bound = n_round * 2.0 ** -23 * np.abs(ref) + c * 2.0 ** -24 * absref + 1e-30
    r = np.abs(got - ref) / bound
    r = np.where(np.isnan(r), np.inf, r).reshape(-1)
    if r.size == 0:
        return 0.0, 0
    i = int(r.argmax())
    return float(r[i]), i


def ratio(got, ref, absref, n_round, c=C_ACC):
    return ratio_at(got, ref, absref, n_round, c)[0]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f64))


def _n(t):
    return t.numpy()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).numpy().astype(f32)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g).numpy().astype(f32)


def _fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


# ---- on-load transform -------------------------------------------------------------------------------------------------------------
XF_KINDS = ("none", "act", "affine", "affine_act")


def make_xf(kind, g, C):
    """(scale, shift, act) of a transform kind; scale in +-[0.5, 1.5), shift of order 1 (padding transformed by mistake would show)"""
    if kind == "none":
        return None
    act = int(kind.endswith("act"))
    if kind == "act":
        return (None, None, act)
    sign = np.where(_rand(g, C) < 0.3, f32(-1), f32(1))
    return ((_rand(g, C) + f32(0.5)) * sign, _randn(g, C) + np.where(_rand(g, C) < 0.5, f32(-1), f32(1)), act)


def xf_mask(x, xf):
    """act' per element (fp64), from the kernel's own sign pattern"""
    if xf is None or not xf[2]:
        return np.ones(x.shape, f64)
    z = x.astype(f64) if xf[0] is None else x.astype(f64) * xf[0].astype(f64) + xf[1].astype(f64)
    return np.where(z > 0, 1.0, SLOPE)


def xf_ref(x, xf):
    """the transformed input a in fp64, with the kernel's sign pattern; the convolutions' twins take |a|"""
    x64 = x.astype(f64)
    if xf is None:
        return x64
    z = x64 if xf[0] is None else x64 * xf[0].astype(f64) + xf[1].astype(f64)
    return z * xf_mask(x, xf)


def xf_emulate(x, xf):
    if xf is None:
        return x
    z = x if xf[0] is None else _fma(np.broadcast_to(xf[0], x.shape), x, np.broadcast_to(xf[1], x.shape))
    return np.where(z > 0, z, f32(SLOPE) * z).astype(f32) if xf[2] else z


# ---- the stride-2 convolutions -----------------------------------------------------------------------------------------------------
GRIDS = {"g45": (3, 3, 5), "g1": (1, 1, 1), "narrow": (2, 8, 2), "strip": (1, 2, 40)}       # (B, Hq, Wq): the grid a kernel enumerates
# (grid, C, M, transform, bias).  MT = 1 / 2 / 4 for M <= 16 / <= 32 / > 32; VEC for C % 4 == 0.  Every C in {1, 3, 4, 12, 20, 48} and
# every M in {1, 3, 17, 33, 65, 100}, every MT on the VEC and on the scalar path, every transform with and without bias.
_CONV = [
    ("g45", 1, 1, "none", True), ("g45", 3, 17, "act", True), ("g45", 1, 33, "affine", False), ("g45", 4, 3, "affine_act", True),
    ("g45", 12, 17, "affine_act", False), ("g45", 20, 65, "act", True), ("g45", 48, 100, "affine", True), ("g45", 12, 33, "none", True),
    ("g1", 3, 3, "affine_act", True), ("g1", 20, 33, "affine", False), ("g1", 1, 1, "act", True),
    ("narrow", 3, 65, "affine_act", True), ("narrow", 12, 1, "none", False), ("narrow", 4, 100, "act", True),
    ("strip", 1, 17, "affine_act", True), ("strip", 48, 3, "affine_act", False), ("strip", 20, 17, "none", True), ("strip", 3, 1, "affine", True),
]
CONV_CASES = [(("up" if up else "down"),) + c for up in (0, 1) for c in _CONV]


def conv_id(case):
    d, grid, C, M, kind, bias = case
    return f"{d}-{grid}-C{C}-M{M}-{kind}-{'bias' if bias else 'nobias'}"


def conv_inputs(case):
    """x (the kernel's input, channels-last), w (torch layout), bias, xf, g (gradient w.r.t. the output), tanh"""
    d, grid, C, M, kind, use_bias = case
    up = d == "up"
    B, Hq, Wq = GRIDS[grid]
    g = _gen(1 + CONV_CASES.index(case))
    hin, win = (Hq, Wq) if up else (2 * Hq, 2 * Wq)
    hout, wout = (2 * Hq, 2 * Wq) if up else (Hq, Wq)
    return dict(up=up, tanh=up and M <= 3, x=_randn(g, B, hin, win, C), w=_randn(g, *((C, M, 4, 4) if up else (M, C, 4, 4))),
                bias=_randn(g, M) if use_bias else None, xf=make_xf(kind, g, C), g=_randn(g, B, hout, wout, M))


def conv_refs(d):
    """{output: (ref, absref, n_round)} of a conv case: y, dx (the opposite pass on g), dw, db"""
    up = d["up"]
    a = _t(xf_ref(d["x"], d["xf"]))
    w, g = _t(d["w"]), _t(d["g"])
    b = None if d["bias"] is None else _t(d["bias"])
    fwd, bwd = (R.s2_up, R.s2_down) if up else (R.s2_down, R.s2_up)
    y, ya = _n(fwd(a, w, b)), _n(fwd(a.abs(), w.abs(), None if b is None else b.abs()))
    out = {"y": (np.tanh(y), ya, 2) if d["tanh"] else (y, ya, 1),
           "dx": (_n(bwd(g, w)), _n(bwd(g.abs(), w.abs())), 1)}
    half, full = (a, g) if up else (g, a)
    out["dw"] = (_n(R.s2_wgrad(half, full)), _n(R.s2_wgrad(half.abs(), full.abs())), 1)
    M = g.shape[-1]
    out["db"] = (_n(g.reshape(-1, M).sum(0)), _n(g.abs().reshape(-1, M).sum(0)), 1)
    return out


def _pad1(x):
    return np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))


def s2_emulate(x, w, bias, xf, up, tanh=False, mutant=None):
    """fp32, one accumulator per output element, sequential over (tap, channel), products rounded before they are added.
    mutant: "hw_swap" (H and W exchanged in the pixel decode), "pad_first" (zero padding before the on-load transform), "drop_chan"
    (the last channel of a partly filled 16-channel group), "mask_m" (the output channel mask one short)"""
    B, H, Wd, C = x.shape
    if mutant == "hw_swap":
        y = s2_emulate(x.reshape(B, Wd, H, C), w, bias, xf, up, tanh)
        return y.reshape(B, 2 * H, 2 * Wd, -1) if up else y.reshape(B, H // 2, Wd // 2, -1)
    ap = xf_emulate(_pad1(x), xf) if mutant == "pad_first" else _pad1(xf_emulate(x, xf))
    Ce = C - 1 if (mutant == "drop_chan" and C % 16) else C
    M = w.shape[1] if up else w.shape[0]
    if up:        # padded input row i' = i + 1 feeds output rows o = 2 i' - 3 + ky: an output takes two taps per axis, rows -1 .. H
        yp = np.zeros((B, 2 * (H + 2) + 2, 2 * (Wd + 2) + 2, M), f32)
        for ky in range(4):
            for kx in range(4):
                v = yp[:, ky:ky + 2 * (H + 2):2, kx:kx + 2 * (Wd + 2):2, :]
                for c in range(Ce):
                    v += ap[..., c:c + 1] * w[c, :, ky, kx]
        acc = yp[:, 3:3 + 2 * H, 3:3 + 2 * Wd, :]
    else:
        ho, wo = H // 2, Wd // 2
        acc = np.zeros((B, ho, wo, M), f32)
        for ky in range(4):
            for kx in range(4):
                t = ap[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2, :]
                for c in range(Ce):
                    acc = acc + t[..., c:c + 1] * w[:, c, ky, kx]
    y = acc + bias if bias is not None else acc.copy()
    if tanh:
        y = np.tanh(y.astype(f64)).astype(f32)
    if mutant == "mask_m":
        y[..., M - 1] = 0
    return y.astype(f32)


def wgrad_plan(B, Hh, Wh, CH, CF):
    """(nsplit, kper, workspace floats) of csrc/stride2.hip's wgrad_plan"""
    HB, FB = -(-CH // 16), -(-CF // 16)
    K = B * Hh * Wh
    ns = max(1, min(-(-4096 // (HB * FB)), -(-K // 128), 1024))
    kper = -(-(-(-K // ns)) // 4) * 4
    nsplit = max(1, -(-K // kper))
    return nsplit, kper, nsplit * HB * 16 * FB * 16 * 16


def wgrad_emulate(half, full, half_xf=None, full_xf=None, mutant=None):
    """fp32: each k-split sequential over its pixels, then the splits in order.  mutant "drop_split": the last split is left out"""
    ha, fa = xf_emulate(half, half_xf), _pad1(xf_emulate(full, full_xf))
    B, Hh, Wh, CH = half.shape
    CF = full.shape[3]
    K = B * Hh * Wh
    nsplit, kper, _ = wgrad_plan(B, Hh, Wh, CH, CF)
    h2 = ha.reshape(K, CH)
    taps = np.stack([fa[:, ky:ky + 2 * Hh:2, kx:kx + 2 * Wh:2, :].reshape(K, CF) for ky in range(4) for kx in range(4)], 2)   # (K, CF, 16)
    total = np.zeros((CH, CF, 16), f32)
    for s in range(nsplit - 1 if mutant == "drop_split" else nsplit):
        acc = np.zeros((CH, CF, 16), f32)
        for k in range(s * kper, min(K, (s + 1) * kper)):
            acc = acc + h2[k][:, None, None] * taps[k][None]
        total = total + acc
    return total.reshape(CH, CF, 4, 4)


def conv_emulate(d, mutant=None):
    up = d["up"]
    conv_mut = mutant if mutant in ("hw_swap", "pad_first", "drop_chan", "mask_m") else None
    out = {"y": s2_emulate(d["x"], d["w"], d["bias"], d["xf"], up, d["tanh"], conv_mut),
           "dx": s2_emulate(d["g"], d["w"], None, None, not up, False, "hw_swap" if mutant == "hw_swap" else None)}
    out["dw"] = (wgrad_emulate(d["x"], d["g"], half_xf=d["xf"], mutant=mutant) if up
                 else wgrad_emulate(d["g"], d["x"], full_xf=d["xf"], mutant=mutant))
    M = d["g"].shape[-1]
    out["db"] = chan_sum_emulate(d["g"].reshape(-1, M))
    return out


# (K as (B, Hh, Wh), CH, CF, which side carries a transform, its kind): K = 1, 45 and 297 (three splits of 100, 100, 97)
WGRAD_GRIDS = {1: (1, 1, 1), 45: (3, 3, 5), 297: (3, 9, 11)}
WGRAD_CASES = [(K, ch, cf, side, kind)
               for i, (K, (ch, cf)) in enumerate((K, hc) for K in (1, 45, 297) for hc in ((1, 17), (17, 3), (20, 33), (48, 16)))
               for side, kind in [(("half", "full", "neither")[i % 3], ("affine_act", "act", "affine")[(i // 3) % 3])]]
# every side at K = 297 on the ragged (20, 33) tile
WGRAD_CASES += [(297, 20, 33, "half", "act"), (297, 20, 33, "full", "affine_act"), (45, 17, 3, "full", "affine")]


def wgrad_id(case):
    K, ch, cf, side, kind = case
    return f"K{K}-CH{ch}-CF{cf}-{side}-{kind if side != 'neither' else 'none'}"


def wgrad_inputs(case):
    K, ch, cf, side, kind = case
    B, Hh, Wh = WGRAD_GRIDS[K]
    g = _gen(500 + WGRAD_CASES.index(case))
    d = dict(half=_randn(g, B, Hh, Wh, ch), full=_randn(g, B, 2 * Hh, 2 * Wh, cf), half_xf=None, full_xf=None)
    if side == "half":
        d["half_xf"] = make_xf(kind, g, ch)
    elif side == "full":
        d["full_xf"] = make_xf(kind, g, cf)
    return d


def wgrad_refs(d):
    h, f = _t(xf_ref(d["half"], d["half_xf"])), _t(xf_ref(d["full"], d["full_xf"]))
    return {"dw": (_n(R.s2_wgrad(h, f)), _n(R.s2_wgrad(h.abs(), f.abs())), 1)}


# ---- channel reductions and BatchNorm --------------------------------------------------------------------------------------------
def red_plan(npix, C):
    """(chunk, nparts) of csrc/stride2.hip's red_chunk"""
    chunk = max(1, -(-16384 // C))
    nparts = -(-npix // chunk)
    if nparts > 1024:
        chunk = -(-npix // 1024)
        nparts = -(-npix // chunk)
    return chunk, nparts


def chunked_sum(v, chunk):
    """fp32 column sums of v (npix, C) in the partition of chan_reduce_stage1: a chunk of pixels per workgroup, inside it L = 256 // C
    pixel lanes per channel (one above 256 channels), each sequential over its pixels i, i + L, ...; then the lanes in order, then the
    chunks in order"""
    npix, C = v.shape
    nparts = -(-npix // chunk)
    L = 256 // C if C <= 256 else 1
    steps = -(-chunk // L)
    p = np.zeros((nparts, steps * L, C), f32)
    full = npix // chunk
    p[:full, :chunk] = v[:full * chunk].reshape(full, chunk, C)
    if full < nparts:
        p[full, :npix - full * chunk] = v[full * chunk:]
    p = p.reshape(nparts, steps, L, C)
    lanes = np.zeros((nparts, L, C), f32)
    for i in range(steps):
        lanes = lanes + p[:, i]
    part = np.zeros((nparts, C), f32)
    for l in range(L):
        part = part + lanes[:, l]
    s = np.zeros(C, f32)
    for k in range(nparts):
        s = s + part[k]
    return s


def chan_sum_emulate(g, mutant=None):
    s = chunked_sum(g, red_plan(*g.shape)[0])
    if mutant == "skip_pass":
        s[256 * ((g.shape[1] - 1) // 256):] = 0
    return s


RED_C = [1, 3, 5, 100, 129, 256, 257, 300, 513]
BWD_MODES = ("bn_act", "bn_noact", "act_only")


def red_npix(C):
    """below the lane count, a few, one chunk of red_chunk exactly, one pixel into a second chunk"""
    chunk = max(1, -(-16384 // C))
    return [1, 2, 7, chunk, chunk + 1]


# (C, index into red_npix(C)); the options cycle with the running index so that every value of each meets every C or npix class
RED_CASES = [(C, j) for C in RED_C for j in range(5)]
BIG_CASE = (1024, 16400)        # np > 1024: red_chunk re-chunks to 17 pixels per workgroup, 965 workgroups


def red_id(case):
    C, j = case
    return f"C{C}-npix{red_npix(C)[j]}"


def red_options(case):
    i = RED_CASES.index(case) if case in RED_CASES else 7
    return dict(momentum=(0.1, 0.37)[i % 2], eps=(1e-5, 1e-3)[(i // 2) % 2], track=(i % 3) != 2, bwd=BWD_MODES[i % 3],
                want_affine=(i % 4) != 3)


def red_inputs(case, npix=None):
    """y (npix, C) with mean / sigma = 0, 3, 1000 by channel (c % 3), sigma in [0.5, 2); channel 1 constant; pixel 0 of channels 3, 4, 5
    (one per mean / sigma class; of channel 0 where C = 3, of the only channel in every third single-channel case) 6 sigma from the
    channel mean, the pivot of a one-pass variance about the first pixel; g, gamma, beta and running buffers"""
    C = case[0]
    npix = red_npix(C)[case[1]] if npix is None else npix
    idx = RED_CASES.index(case) if case in RED_CASES else 7
    g = _gen(9000 + 31 * C + npix)
    sigma = (_rand(g, C) * f32(1.5) + f32(0.5)).astype(f32)
    mean = (np.array([0.0, 3.0, 1000.0], f32)[np.arange(C) % 3] * sigma).astype(f32)
    y = (_randn(g, npix, C) * sigma + mean).astype(f32)
    six = [c for c in (3, 4, 5) if c < C] or ([0] if C == 3 or (C == 1 and idx % 3 == 2) else [])
    const = [1] if C > 1 else ([0] if idx % 3 == 1 else [])
    for c in six:
        y[0, c] = mean[c] + f32(6) * sigma[c]
    for c in const:
        y[:, c] = f32(3.1) * sigma[c]
    return dict(y=y, g=_randn(g, npix, C), gamma=(_randn(g, C) * f32(0.1) + f32(1)).astype(f32), beta=(_randn(g, C) * f32(0.1)).astype(f32),
                run_mean=_randn(g, C), run_var=_rand(g, C) + f32(0.5), six=six, const=const)


def bn_stats_refs(y, gamma, beta, eps, momentum, run_mean, run_var):
    """{output: (ref, absref, n_round)}; the running buffers only when given; eps and momentum as the fp32 numbers the kernel is passed"""
    eps, momentum = float(f32(eps)), float(f32(momentum))
    args = (_t(y), _t(gamma), _t(beta), eps, momentum, None if run_mean is None else _t(run_mean), None if run_var is None else _t(run_var))
    s, a = R.bn_stats(*args), R.bn_stats_abs(*args)
    n = {"mean": 2, "rstd": 3, "scale": 4, "shift": 1, "running_mean": 1, "running_var": 1}
    return {k: (_n(s[k]), _n(a[k]), n[k]) for k in n if k in s}


def _finish_stats(mean, var, npix, gamma, beta, eps, momentum, run_mean, run_var, mutant=None):
    n = f32(npix)
    rstd = (f32(1) / np.sqrt(var + f32(eps))).astype(f32)
    scale = gamma * rstd
    out = dict(mean=mean, rstd=rstd, scale=scale, shift=beta - mean * scale)
    if run_mean is not None:
        unb = var * (n / (n - f32(1))) if (npix > 1 and mutant != "biased_running") else var
        m = f32(momentum)
        out["running_mean"] = (f32(1) - m) * run_mean + m * mean
        out["running_var"] = (f32(1) - m) * run_var + m * unb
    if mutant == "skip_pass":
        for v in out.values():
            v[256 * ((len(mean) - 1) // 256):] = 0
    return {k: v.astype(f32) for k, v in out.items()}


def bn_stats_emulate(y, gamma, beta, eps, momentum, run_mean, run_var, mutant=None):
    """the operation in fp32, centred two-pass in its corrected form (Chan, Golub, LeVeque 1983): a first mean m0, then the deviations
    from it, whose mean corrects m0 and whose mean square, less the square of that correction, is the variance; each a chunked sum"""
    npix, C = y.shape
    chunk = red_plan(npix, C)[0]
    m0 = chunked_sum(y, chunk) / f32(npix)
    dev = y - m0
    corr = chunked_sum(dev, chunk) / f32(npix)
    mean = m0 + corr
    var = np.maximum(chunked_sum(dev * dev, chunk) / f32(npix) - corr * corr, f32(0))
    return _finish_stats(mean, var, npix, gamma, beta, eps, momentum, run_mean, run_var, mutant)


def bn_stats_emulate_onepass(y, gamma, beta, eps, momentum, run_mean, run_var):
    """one pass about the pivot y[0, c]: var = s1 / n - (s0 / n)^2 of the shifted values (bn_stats_finish before this module existed)"""
    npix, C = y.shape
    chunk = red_plan(npix, C)[0]
    d = y - y[0]
    s0, s1 = chunked_sum(d, chunk), chunked_sum(d * d, chunk)
    dd = s0 / f32(npix)
    var = np.maximum(s1 / f32(npix) - dd * dd, f32(0))
    return _finish_stats(y[0] + dd, var, npix, gamma, beta, eps, momentum, run_mean, run_var)


def bn_apply_refs(y, scale, shift, act):
    xf = (scale, shift, act)
    m = xf_mask(y, xf)
    y64 = y.astype(f64)
    if scale is None:
        return {"a": (y64 * m, np.abs(y64) * m, 2)}
    s, h = scale.astype(f64), shift.astype(f64)
    return {"a": ((y64 * s + h) * m, (np.abs(y64) * np.abs(s) + np.abs(h)) * m, 2)}


def bn_bwd_refs(mode, y, g, scale, shift, mean, rstd, gamma):
    """{gy, dgamma, dbeta}; the statistics (scale, shift, mean, rstd) are the operator's fp32 inputs"""
    if mode == "act_only":
        r = _n(R.act_backward(_t(y), _t(g), SLOPE))
        return {"gy": (r, np.abs(r), 1)}
    mask = _t(xf_mask(y, (scale, shift, int(mode == "bn_act"))))
    gy, dg, db = R.bn_act_backward(_t(y), _t(g), _t(gamma), None, _t(mean), _t(rstd), SLOPE, mask=mask)
    gya, dga, dba = R.bn_act_backward_abs(_t(y), _t(g), _t(gamma), _t(mean), _t(rstd), mask)
    return {"gy": (_n(gy), _n(gya), 3), "dgamma": (_n(dg), _n(dga), 1), "dbeta": (_n(db), _n(dba), 1)}


def bn_bwd_emulate(mode, y, g, scale, shift, mean, rstd, gamma):
    if mode == "act_only":
        return {"gy": np.where(y > 0, g, g * f32(SLOPE)).astype(f32)}
    npix, C = y.shape
    chunk = red_plan(npix, C)[0]
    gz = g
    if mode == "bn_act":
        z = _fma(np.broadcast_to(scale, y.shape), y, np.broadcast_to(shift, y.shape))
        gz = np.where(z > 0, g, g * f32(SLOPE)).astype(f32)
    xh = (y - mean) * rstd
    s0, s1 = chunked_sum(gz, chunk), chunked_sum(gz * xh, chunk)
    n = f32(npix)
    return {"gy": ((gamma * rstd) * (gz - s0 / n - xh * (s1 / n))).astype(f32), "dgamma": s1, "dbeta": s0}


def bn_apply_emulate(y, scale, shift, act):
    return {"a": xf_emulate(y, (scale, shift, act))}


class Emulated:
    """the reductions in fp32 on the CPU, with the interface the GPU module implements over the kernels (red_chain's `impl`)"""

    def __init__(self, mutant=None, onepass=False):
        self.mutant, self.onepass = mutant, onepass

    def stats(self, y, gamma, beta, eps, momentum, run_mean, run_var):
        if self.onepass:
            return bn_stats_emulate_onepass(y, gamma, beta, eps, momentum, run_mean, run_var)
        return bn_stats_emulate(y, gamma, beta, eps, momentum, run_mean, run_var, self.mutant)

    def apply(self, y, scale, shift, act):
        return bn_apply_emulate(y, scale, shift, act)["a"]

    def bwd(self, mode, y, g, scale, shift, mean, rstd, gamma, want_affine):
        return bn_bwd_emulate(mode, y, g, scale, shift, mean, rstd, gamma)

    def chan_sum(self, g):
        return chan_sum_emulate(g, self.mutant)


def red_chain(d, o, impl, stats_only=False):
    """statistics (two consecutive calls when the running buffers are tracked: the second starts from what the first wrote) -> stored
    activation -> backward -> plain channel sum, each through `impl` on the fp32 outputs of the step before it, each against its own
    fp64 reference of exactly those inputs.  Yields (output name, got, (ref, absref, n_round))."""
    y, gamma, beta = d["y"], d["gamma"], d["beta"]
    rm, rv = (d["run_mean"], d["run_var"]) if o["track"] else (None, None)
    for _ in range(2 if o["track"] else 1):
        s = impl.stats(y, gamma, beta, o["eps"], o["momentum"], rm, rv)
        refs = bn_stats_refs(y, gamma, beta, o["eps"], o["momentum"], rm, rv)
        for k in refs:
            yield f"bn_stats/{k}", s[k], refs[k]
        if o["track"]:
            rm, rv = s["running_mean"], s["running_var"]
    if stats_only:
        return
    mode = o["bwd"]
    act = int(mode != "bn_noact")
    yield "bn_act_apply/a", impl.apply(y, s["scale"], s["shift"], act), bn_apply_refs(y, s["scale"], s["shift"], act)["a"]
    got = impl.bwd(mode, y, d["g"], s["scale"], s["shift"], s["mean"], s["rstd"], gamma, o["want_affine"])
    refs = bn_bwd_refs(mode, y, d["g"], s["scale"], s["shift"], s["mean"], s["rstd"], gamma)
    for k in got:
        yield f"bn_act_bwd_{mode}/{k}", got[k], refs[k]
    g64 = d["g"].astype(f64)
    yield "chan_sum/out", impl.chan_sum(d["g"]), (g64.sum(0), np.abs(g64).sum(0), 1)


FOLD_C = [1, 257]


def fold_inputs(C):
    g = _gen(70 + C)
    return dict(gamma=_randn(g, C), beta=_randn(g, C), run_mean=_randn(g, C) * f32(3), run_var=_rand(g, C) * f32(2) + f32(1e-3), eps=1e-5)


def fold_refs(d):
    args = (_t(d["gamma"]), _t(d["beta"]), _t(d["run_mean"]), _t(d["run_var"]), float(f32(d["eps"])))
    (s, h), (sa, ha) = R.bn_fold_eval(*args), R.bn_fold_eval_abs(*args)
    return {"scale": (_n(s), _n(sa), 3), "shift": (_n(h), _n(ha), 1)}


def fold_emulate(d):
    s = (d["gamma"] / np.sqrt(d["run_var"] + f32(d["eps"]))).astype(f32)
    return {"scale": s, "shift": (d["beta"] - d["run_mean"] * s).astype(f32)}


# ---- pointwise: tanh backward and the stored activation ----------------------------------------------------------------------------
POINT_N = [1, 255, 257]
APPLY_SHAPES = {1: (1, 1), 255: (85, 3), 257: (257, 1)}       # (npix, C) with npix C = n
APPLY_KINDS = {1: "act", 255: "affine_act", 257: "affine"}


def tanh_bwd_inputs(n):
    g = _gen(40 + n)
    return dict(t=np.tanh(_randn(g, n) * f32(1.5)).astype(f32), g=_randn(g, n))


def tanh_bwd_refs(d):
    t, g = d["t"].astype(f64), d["g"].astype(f64)
    return {"o": (g * (1 - t * t), np.abs(g) * (1 + t * t), 2)}


def tanh_bwd_emulate(d):
    return {"o": (d["g"] * (f32(1) - d["t"] * d["t"])).astype(f32)}


def apply_inputs(n):
    npix, C = APPLY_SHAPES[n]
    g = _gen(60 + n)
    return dict(y=_randn(g, npix, C), xf=make_xf(APPLY_KINDS[n], g, C))


# ---- stem --------------------------------------------------------------------------------------------------------------------------
# (K, B, S, C, which gradients): K in {1, 63, 64, 65, 130} (under, at and over the 64 lanes, two strides), B in {1, 3, 65} (65: past the
# 64 rows the kernel's comment speaks of), (S, C) = (9, 5): 45 rows, a ragged last workgroup of the forward
STEM_CASES = [(1, 1, 1, 1, "both"), (63, 3, 9, 5, "gw"), (64, 65, 16, 16, "gb"), (65, 3, 16, 16, "both"), (130, 65, 9, 5, "both"),
              (130, 1, 16, 16, "gw"), (1, 65, 9, 5, "gb"), (65, 1, 1, 1, "both"), (63, 65, 1, 1, "gw"), (64, 3, 9, 5, "gb")]


def stem_id(case):
    K, B, S, C, which = case
    return f"K{K}-B{B}-S{S}-C{C}-{which}"


def stem_inputs(case):
    K, B, S, C, _ = case
    g = _gen(300 + STEM_CASES.index(case))
    return dict(z=_randn(g, B, K), w=_randn(g, C * S, K), bias=_randn(g, C * S), g=_randn(g, B, S, C), S=S, C=C)


def stem_refs(d):
    z, w, b, g = _t(d["z"]), _t(d["w"]), _t(d["bias"]), _t(d["g"])
    S, C = d["S"], d["C"]
    gw, gb = R.stem_grads(z, g, S, C)
    gwa, gba = R.stem_grads(z.abs(), g.abs(), S, C)
    return {"y": (_n(R.stem(z, w, b, S, C)), _n(R.stem(z.abs(), w.abs(), b.abs(), S, C)), 1), "gw": (_n(gw), _n(gwa), 1), "gb": (_n(gb), _n(gba), 1)}


def stem_emulate(d, mutant=None):
    """fp32, sequential over k (forward) and over the batch (gradients).  mutant "gb_rows": gb summed over B - 1 rows"""
    z, w, g, S, C = d["z"], d["w"], d["g"], d["S"], d["C"]
    B, K = z.shape
    acc = np.zeros((B, C * S), f32)
    for k in range(K):
        acc = acc + z[:, k:k + 1] * w[None, :, k]
    y = (acc + d["bias"]).reshape(B, C, S).transpose(0, 2, 1)
    g2 = g.transpose(0, 2, 1).reshape(B, C * S)
    gw, gb = np.zeros((C * S, K), f32), np.zeros(C * S, f32)
    for b in range(B):
        gw = gw + g2[b][:, None] * z[b][None, :]
        if not (mutant == "gb_rows" and b == B - 1):
            gb = gb + g2[b]
    return {"y": np.ascontiguousarray(y), "gw": gw, "gb": gb}
