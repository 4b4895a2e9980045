"""Cases, fp64 oracle, kernel emulation and error bounds of the pairwise similarity loss (include/nganx.h; csrc/simloss.hip), shared
by tests/test_simloss_bounds_cpu.py (which settles the bounds on the CPU) and tests/test_gpu_simloss.py (which holds the kernels to them).

Oracle (`oracle`): the reference's similarity_loss expression (loss_functions.py:185-205: rows divided by their norms, the two cosine
matrices by matmul, the squared difference summed and divided by B (B - 1)) in fp64 under autograd, with the centring written out
(x - mean(x) before anything else) and the diagonal masked exactly.  Gradients are autograd's.  It centres BEFORE it multiplies, so its
own error has no cancellation in it and stays at a few N 2^-53 relative: below every bound here.  The Gram matrix alone is compared
against an extended-precision (np.longdouble) restatement, `gram_exact`.

Emulation (`emulate`): the kernels in their own operation order -- the Gram sums per pixel group, group by group, the slabs by lane and butterfly
(simloss_bits.h gram_plan, restated in `gram_plan`), the head's fp64 lines one rounding each with its 64-lane butterflies, the mix's
fp32 fma chain (an fma is restated as the fp64 sum of the exact product and the accumulator rounded to fp32: a double rounding that
can differ from the kernel by one fp32 ulp, inside the bound).  `defect=` names one of six wrong kernels.

Bounds (`bounds`), u = 2^-53, v = 2^-24, first order in u (second-order terms are below 1e-6 of the first for every case here):
  G raw       N u sum_p |x_i x_j|: a sum of N exact products, added one by one in some order -- (N - 1) u in the standard bound.
  G centred   + the cancellation of G - N m_i m_j: the sums carry N u sum|x| each, so m carries (N + 1) u mean|x|, the product N m_i m_j
              N (N + 1) u (|m_i| a_j + |m_j| a_i) + 3 u N |m_i m_j| (three roundings: m_i m_j, times N, the subtraction).  With a
              1e-3 amplitude on a -1 background this is 1e6 times the centred norm's own rounding: the stated cancellation.
  S, T        bG_ij / (n_i n_j) + |S_ij| (bG_ii / G_ii + bG_jj / G_jj) / 2 + 3 u |S_ij| (product, square root, quotient).
  L           v |L| (the one fp32 rounding) + w sum 2 |d_ij| (bS_ij + bT_ij) + (B + 70) u |L| (the row butterflies are 6 levels, the
              rows B terms, the squares, the weight and the product a handful more).
  M, r        carried the same way: bA = 2 w (bS + bT) + 3 u |A|; bM_ij = 2 bA_ij / (n_i n_j) + |M_ij| (rel_i + rel_j) / 2 + 4 u |M_ij|;
              bM_ii = 2 sum_j (bA_ij |S_ij| + |A_ij| bS_ij) / G_ii + |M_ii| (rel_i + 10 u); br_i = sum_j (bM_ij |m_j| + |M_ij| bm_j)
              + 8 u sum_j |M_ij m_j|, rel_i = bG_ii / G_ii.
  gradient    c v (|addend| + |upstream| (sum_j |M_ij| |x_j[p]| + |r_i|)) + |upstream| (sum_j bM_ij |x_j[p]| + br_i) with c = B + 5:
              B fmas, the roundings of M and r to fp32 (one each, against terms of the same sum), the subtraction, the product
              with upstream and the addition of the addend on the store.
Every fp64 term is doubled where the comparison is against the fp64 oracle, for the oracle's own rounding.
"""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import multiotsu_ref  # noqa: E402

U64, U32 = 2.0 ** -53, 2.0 ** -24
BATCHES = (2, 3, 5, 8, 16, 64)
FAMILIES = ("noise", "micrograph", "identical", "negated", "cancel")
DEFECTS = ("diagonal_kept", "no_mix_diagonal", "no_shift", "fp32_centring", "b_squared", "not_symmetrised")
LATENT = 64


def latents(b, dim=LATENT, seed=0):
    """(b, dim) fp32 from the product's sample_latent_vec (normal draws clamped to [-5, 5], projected on the unit sphere)"""
    from __graft_entry__ import load_package
    return load_package().utils.sample_latent_vec((b, dim), seed=1000 + 7 * b + seed).numpy().astype(np.float32)


@functools.lru_cache(maxsize=None)
def _fields(n_fields, size):
    return np.stack([multiotsu_ref.micrograph(40 + k, size).astype(np.float32) / 127.5 - 1.0 for k in range(n_fields)])


def images(family, b, n, seed=0):
    """(b, n) fp32 rows of one family"""
    rng = np.random.default_rng(1234 + 31 * b + seed)
    x = rng.uniform(-1.0, 1.0, (b, n)).astype(np.float32)
    if family == "noise":
        return x
    if family == "micrograph":      # the synthetic micrograph fields scaled to [-1, 1]; rows beyond the distinct fields get a little noise
        size = int(round(n ** 0.5))
        if size * size != n:
            raise ValueError("micrograph rows are square images")
        f = _fields(min(b, 8), size).reshape(-1, n)
        return (f[np.arange(b) % f.shape[0]] + 0.05 * x * (np.arange(b)[:, None] >= f.shape[0])).astype(np.float32)
    if family == "identical":       # S_01 = 1
        x[1] = x[0]
        return x
    if family == "negated":         # S_01 = -1
        x[1] = -x[0]
        return x
    if family == "cancel":          # a 1e-3 amplitude on a -1 background: the centring cancellation
        x[0] = (-1.0 + 1e-3 * x[0]).astype(np.float32)
        return x
    raise ValueError(family)


def gram_plan(b, n):
    """simloss_bits.h gram_plan: (groups, chunk, slabs)"""
    lanes = 1
    while 4 * lanes < b:
        lanes *= 2
    groups = 256 // (lanes * lanes)
    tile = 256 if groups > 64 else 64
    per = (n + 1023) // 1024
    per = (per + tile - 1) // tile * tile
    chunk = max(256, per)
    return groups, chunk, (n + chunk - 1) // chunk


def _seq_sum(a):
    """sum over axis 0, one term after the other"""
    return np.cumsum(a, axis=0)[-1]


def _slab_sum(parts):
    """the reduce launch: lane l adds the slabs l, l + 64, ... ascending from 0.0, then the 64-lane butterfly; parts: (slabs, ...)"""
    pad = (-parts.shape[0]) % 64
    parts = np.concatenate([parts, np.zeros((pad,) + parts.shape[1:])]).reshape((-1, 64) + parts.shape[1:])      # [step][lane]
    lanes = _seq_sum(np.concatenate([np.zeros((1,) + parts.shape[1:]), parts]))                                   # (64, ...)
    return _lane_sum(np.moveaxis(lanes, 0, -1))


def gram_emu(x):
    """(gram, sums) as nganx_pair_gram adds them"""
    b, n = x.shape
    groups, chunk, slabs = gram_plan(b, n)
    x64 = x.astype(np.float64)
    parts_g, parts_s = [], []
    for s in range(slabs):
        blk = x64[:, s * chunk:min(n, (s + 1) * chunk)]
        pad = (-blk.shape[1]) % groups
        blk = np.pad(blk, ((0, 0), (0, pad))).reshape(b, -1, groups)           # [row][step][group]: pixel = step * groups + group
        prod = np.einsum("ilg,jlg->lgij", blk, blk)                              # exact products
        parts_g.append(_seq_sum(_seq_sum(prod)))                                 # steps ascending, then groups ascending
        parts_s.append(_seq_sum(_seq_sum(np.transpose(blk, (1, 2, 0)))))
    return _slab_sum(np.stack(parts_g)), _slab_sum(np.stack(parts_s))


def gram_exact(x, center):
    """the centred Gram matrix in extended precision, rounded to fp64"""
    xl = x.astype(np.longdouble)
    if center:
        xl = xl - xl.mean(axis=1, keepdims=True)
    return (xl @ xl.T).astype(np.float64)


def _lane_sum(v):
    """the head's butterfly over 64 lanes; v: (..., 64)"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., 0]


def _pad64(a):
    return np.pad(a, [(0, 0)] * (a.ndim - 1) + [(0, 64 - a.shape[-1])])


def head_emu(gx, sx, gz, lam, n, center, defect=None):
    """nganx_simloss_head line by line -> dict(L fp32, S fp64, M fp32, r fp32)"""
    b = gx.shape[0]
    lam = float(np.float32(lam))
    mean = sx / float(n) if center else np.zeros(b)
    if defect == "fp32_centring":       # the mean taken after the product sum, in fp32
        m32 = mean.astype(np.float32)
        gc = (gx.astype(np.float32) - (np.float32(n) * m32[:, None]) * m32[None, :]).astype(np.float64)
    else:
        gc = gx - float(n) * (mean[:, None] * mean[None, :])
    dx, dz = np.diag(gc).copy(), np.diag(gz).copy()
    w = lam / (float(b) * float(b if defect == "b_squared" else b - 1))
    eye = np.eye(b, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = gc / np.sqrt(dx[:, None] * dx[None, :])
        t = gz / np.sqrt(dz[:, None] * dz[None, :])
        d = t - s if defect == "diagonal_kept" else np.where(eye, 0.0, t - s)
        a = -2.0 * (w * d)
        nn = np.sqrt(dx)[:, None] * np.sqrt(dx)[None, :]
        m_off = ((1.0 if defect == "not_symmetrised" else 2.0) * a) / nn
        c = a * s
        row_c = _lane_sum(_pad64(c))
        row_d2 = _lane_sum(_pad64(d * d))
        m_diag = ((-1.0 if defect == "not_symmetrised" else -2.0) * row_c) / dx
        if defect == "diagonal_kept":       # no special case for j == i anywhere: the generic formula stands on the diagonal
            m = m_off
        elif defect == "no_mix_diagonal":
            m = np.where(eye, 0.0, m_off)
        else:
            m = np.where(eye, m_diag[:, None], m_off)
        r = _lane_sum(_pad64(m * mean[None, :]))
        if defect == "no_shift":
            r = np.zeros(b)
        total = 0.0
        for i in range(b):
            total = total + row_d2[i]
    return {"L": np.float32(w * total), "S": s, "M": m.astype(np.float32), "r": r.astype(np.float32)}


def mix_emu(x, m, r, upstream=1.0, addend=None):
    """nganx_pair_mix: fp32 fmas over j ascending, the subtraction, the product, the addition"""
    b = x.shape[0]
    up = np.float32(upstream)
    out = np.empty_like(x)
    with np.errstate(invalid="ignore"):
        for i in range(b):
            acc = np.zeros(x.shape[1], dtype=np.float32)
            for j in range(b):
                acc = (np.float64(m[i, j]) * x[j].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
            val = up * (acc - r[i])
            out[i] = val if addend is None else addend[i] + val
    return out


def emulate(x, z, lam, center, upstream=1.0, addend=None, defect=None):
    gx, sx = gram_emu(x)
    gz, _ = gram_emu(z)
    mean = sx / float(x.shape[1]) if center else np.zeros(x.shape[0])
    out = head_emu(gx, sx, gz, lam, x.shape[1], center, defect)
    out["G"] = gx - float(x.shape[1]) * (mean[:, None] * mean[None, :])
    out["Gz"] = gz
    out["grad"] = mix_emu(x, out["M"], out["r"], upstream, addend)
    return out


def oracle(x, z, lam, center, upstream=1.0, addend=None):
    """the reference's expression in fp64 under autograd -> dict(L, S, grad); grad includes upstream and the addend"""
    xt = torch.tensor(x.astype(np.float64), requires_grad=True)
    zt = torch.tensor(z.astype(np.float64))
    b = xt.shape[0]
    xc = xt - xt.mean(dim=1, keepdim=True) if center else xt
    im = xc / xc.norm(2, dim=1, keepdim=True)
    zz = zt / zt.norm(2, dim=1, keepdim=True)
    s = im @ im.t()
    off = 1.0 - torch.eye(b, dtype=torch.float64)
    loss = float(np.float32(lam)) * (torch.pow(zz @ zz.t() - s, 2) * off).sum() / (b * (b - 1))
    grad, = torch.autograd.grad(loss, xt)
    g = float(np.float32(upstream)) * grad.numpy()
    if addend is not None:
        g = addend.astype(np.float64) + g
    return {"L": float(loss.detach()), "S": s.detach().numpy(), "grad": g}


def bounds(x, z, lam, center, upstream=1.0, addend=None):
    """dict(G, Gz, S, L, grad): the bounds of the module docstring, evaluated at the exact (fp64) quantities"""
    b, n = x.shape
    lam, up = float(np.float32(lam)), abs(float(np.float32(upstream)))
    ax = np.abs(x.astype(np.float64))

    def gram_bound(rows, centre):
        a = np.abs(rows.astype(np.float64))
        k = rows.shape[1]
        bg = k * U64 * (a @ a.T)
        m = rows.astype(np.float64).mean(axis=1) if centre else np.zeros(rows.shape[0])
        bm = (k + 1) * U64 * a.mean(axis=1) if centre else np.zeros(rows.shape[0])
        if centre:
            am = np.abs(m)
            bg = bg + k * (am[:, None] * bm[None, :] + am[None, :] * bm[:, None]) + 3 * U64 * k * am[:, None] * am[None, :]
        return bg, m, bm

    bgx, mean, bmean = gram_bound(x, center)
    bgz, _, _ = gram_bound(z, False)
    gx, gz = gram_exact(x, center), gram_exact(z, False)
    bgx, bgz = bgx + U64 * np.abs(gx), bgz + U64 * np.abs(gz)

    def cos_bound(g, bg):
        dg = np.diag(g)
        nn = np.sqrt(dg[:, None] * dg[None, :])
        s = g / nn
        rel = np.diag(bg) / dg
        return s, bg / nn + np.abs(s) * (rel[:, None] + rel[None, :]) / 2 + 3 * U64 * np.abs(s), rel, nn

    s, bs, rel, nn = cos_bound(gx, bgx)
    t, bt, _, _ = cos_bound(gz, bgz)
    off = ~np.eye(b, dtype=bool)
    w = lam / (b * (b - 1))
    d = np.where(off, t - s, 0.0)
    loss = w * (d * d).sum()
    carried_l = w * (2 * np.abs(d) * (bs + bt) * off).sum() + (b + 70) * U64 * abs(loss)
    a = -2.0 * w * d
    ba = (2 * w * (bs + bt) + 3 * U64 * np.abs(a)) * off
    m = 2 * a / nn
    bm = 2 * ba / nn + np.abs(m) * (rel[:, None] + rel[None, :]) / 2 + 4 * U64 * np.abs(m)
    dg = np.diag(gx)
    m_diag = -2 * (a * s).sum(axis=1) / dg
    bm_diag = 2 * (ba * np.abs(s) + np.abs(a) * bs).sum(axis=1) / dg + np.abs(m_diag) * (rel + 10 * U64)
    m[~off], bm[~off] = m_diag, bm_diag
    r = m @ mean
    br = bm @ np.abs(mean) + np.abs(m) @ bmean + 8 * U64 * (np.abs(m) @ np.abs(mean))
    c = b + 5
    spread = np.abs(m) @ ax + np.abs(r)[:, None]
    grad = c * U32 * ((0.0 if addend is None else np.abs(addend.astype(np.float64))) + up * spread) + 2 * up * (bm @ ax + br[:, None])
    return {"G": bgx, "Gz": bgz, "S": 2 * bs, "L": U32 * abs(loss) + 2 * carried_l, "grad": grad,
            "M": U32 * np.abs(m) + 2 * bm, "r": U32 * np.abs(r) + 2 * br, "M_exact": m, "r_exact": r}


def ratio(got, ref, bound):
    """max over ALL elements of |got - ref| / bound; inf where a value is not finite or misses a zero bound"""
    got, ref, bound = (np.asarray(v, dtype=np.float64) for v in (got, ref, bound))
    got, ref, bound = np.broadcast_arrays(got, ref, bound)
    err = np.abs(got - ref)
    if not np.isfinite(err).all():
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    return float(np.max(q)) if q.size else 0.0


def ratios(out, x, z, lam, center, upstream=1.0, addend=None):
    """{output: err / bound} of a kernel's or the emulation's outputs `out` (dict with G (centred), Gz, S, L, grad, and M, r when
    present) against the oracle and the extended-precision Gram matrices"""
    ref, bnd = oracle(x, z, lam, center, upstream, addend), bounds(x, z, lam, center, upstream, addend)
    res = {"G": ratio(out["G"], gram_exact(x, center), bnd["G"]), "Gz": ratio(out["Gz"], gram_exact(z, False), bnd["Gz"]),
           "S": ratio(out["S"], ref["S"], bnd["S"]), "L": ratio(out["L"], ref["L"], bnd["L"]),
           "grad": ratio(out["grad"], ref["grad"], bnd["grad"])}
    if "M" in out:
        res["M"] = ratio(out["M"], bnd["M_exact"], bnd["M"])
        res["r"] = ratio(out["r"], bnd["r_exact"], bnd["r"])
    return res
