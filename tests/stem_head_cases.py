"""The generator stem, the critic head (csrc/linear.hip) and the scalar heads of the losses (the last section of csrc/pointwise.hip)
at every dispatch branch: inputs, fp64 references with their absolute-value twins, the per-element bound and fp32 emulations in the
kernels' own summation order.  Shared by tests/test_gpu_stem_head.py (the kernels against the references) and
tests/test_stem_head_bounds_cpu.py (the emulations against the references: the constants are settled on the CPU, before any kernel
is looked at).  `ratio`, `draws` and C_ACC are those of tests/wide_f32_cases.py.

Bound, per element:   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref,   C_ACC = 8
  absref   the operator's formula with absolute values propagated through it
  n_round  the fp32 roundings applied to the element AFTER its last addition (each relative to |ref|); the rounding of a last
           addition itself counts as one.  A bf16 store adds 2^-8 |ref| (one round-to-nearest of an 8-bit significand): BF16_STORE
           roundings of 2^-23.
n_round per output, from the kernel source:
  linear_fwd   y   v / r, v = lrelu(acc), r = sqrt(ss / C + eps): slope product 1; ss / C and + eps reach y through the root, halved:
                   together 1; sqrtf 1; reciprocal 1; product with it 1                                                          5
                   absref: va / r for v's own error plus |y| mean_c(|v| va) / r^2 for the error that the C dot products leave in
                   r (first-order propagation of dr = mean_c(v dv) / r), va = m scale sum_k |z| |W|
               rn  ss / C and + eps (halved by the root: together 1), sqrtf 1; absref sqrt(mean va^2 + eps)                        2
  linear_wgrad     acc * scale (MFMA form, and the row-streaming form's first 16 samples) or fma(acc, scale, old)                 1
                   accumulate = 1: the addition of the buffer, one more                                                          2
  linear_dgrad     acc * scale                                                                                                   1
  final_dot_fwd    t * scale + bias: the last addition                                                                           1
  final_dot_dx     (scale * go[b]) * W: two products, no sum                                                                     2
  final_dot_dw gW  s * scale 1, with accumulate bit 0 the addition 2;  gb: the last addition 1, with accumulate bit 1 2
  wloss_head       mean_real / mean_fake: sum / n 1;  loss: the last addition 1
  wloss_head_bwd   (gl (-1 + 2 drift s) + gr) / n: the last addition, the division                                                2
  gp_head          lambda * s / B: two roundings.  norms are in [0.5, 1.5), so norms - 1 is exact (Sterbenz) and the terms
                   (norms - 1)^2 are positive: absref = ref                                                                      2
  gp_coef          g 2 lambda (norm - 1) / (B norm): g * 2 and norm - 1 exact; * lambda, * (norm - 1), B * norm, the division       4
  sample_l2norm    sqrtf of a sum of squares (positive terms: absref = ref; the root halves the sum's error)                     1
  scale_rows 1;  xhat e real + (1 - e) fake: the last addition 1 (1 - e rounds: a term's rounding);  axpby fma(cb, b, ca a) 1, b null: 1
  latent_normalize clamp(z) * (1 / sqrtf(ss)): sqrtf, reciprocal, product                                                        3
  lerp 1, fade_bwd 2: tests/wide_f32_cases.py
For the elementwise kernels without a sum (final_dot_dx, gp_coef, scale_rows, axpby with b null, fade_bwd) absref = |ref| and the
bound is n_round 2^-23 |ref| but for the constant's 2^-21 |ref|.

The rounding inside v_mfma_f32_16x16x4_f32 (four products added to the accumulator) is not documented: the MFMA emulations come in
two forms, the group of four summed exactly and rounded once ("exact") and summed one fma after the other in fp32 ("seq"), and both
are held to the bound.

RAISED lists the outputs whose emulated worst err / bound exceeds 0.5 with C_ACC = 8, with the next power of two that brings it to
0.5 or below and the emulated ratio at that constant; tests/test_stem_head_bounds_cpu.py pins both.  One entry: the stem's stored weight gradient."""
import functools

import numpy as np
import torch

import wide_f32_cases as W
from wide_f32_cases import C_ACC, draws, ratio  # noqa: F401  (re-exported: the GPU test and the CPU test take them from here)

f32, f64 = np.float32, np.float64
SLOPE, EPS = W.SLOPE, W.EPS
BF16_STORE = 2 ** 15            # 2^-8 |ref| in units of 2^-23 |ref|
# output name -> (raised C_ACC, emulated worst err / bound at that constant)
RAISED = {
    # 0.587 with C_ACC = 8 (row-streaming form, B = 16, K = 528, 180 rows; the MFMA form summed one fma after the other reaches 0.581
    # at B = 37, K = 496, 4096 rows): sums of at most 37 terms, where a single rounding of a partial sum is a large share of absref, and
    # up to four million outputs per case to find the worst among
    "linear_wgrad/gW": (16.0, 0.322),
}


def c_acc(name):
    return float(RAISED.get(name, (C_ACC, None))[0])


def r32(x):
    """a host scalar as the C ABI passes it: rounded to fp32"""
    return float(f32(x))


def seed_of(tag, *shape):
    s = tag
    for v in shape:
        s = (s * 131 + int(v)) % (2 ** 31 - 1)
    return s


def bf16(a):
    """round-to-nearest-even to bf16, returned as fp32"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


def plus(ref, buf):
    """reference of an accumulating form that starts from `buf`: one more rounding, the addition"""
    r, a, n = ref
    return r + buf.astype(f64), a + np.abs(buf.astype(f64)), n + 1


def stored(ref, extra):
    r, a, n = ref
    return r, a, n + extra


# ---- case lists: the smallest shapes that reach each branch ------------------------------------------------------------------------
BMAX = 37
# ngan_linear_lrelu_pn_fwd: K = 16 (tail loop only), 256 (one unrolled group), 272 (group + tail), 512; C = 4 (< 16), 20 (ragged tile),
# 64 (one tile per wave), 80 (a fifth tile on wave 0); B = 1, a full chunk, one row into the second, three chunks with a ragged last
STEM_FWD = [(B, K, S, C) for K in (16, 256, 272, 512) for C, S in ((4, 1), (20, 9), (64, 16), (80, 4)) for B in (1, 16, 17, 37)]
STEM_FWD_RAISED_LDS = [(5, 64, 16, 1024), (3, 512, 1, 1024)]       # 70.6 KB and 98.9 KB of dynamic LDS
# ngan_linear_wgrad, MFMA form (K % 16 == 0, K <= 512): NT = 8 with nt = 1 and 8, NT = 32 with nt = 9, 31 and 32; rows 9 (one
# partial wave), 180 (ragged last block), 4096; B = 1, 3 (one ragged group of 4 samples), 4, 37
WGRAD_MFMA = [(B, K, S, C) for K in (16, 128, 144, 496, 512) for C, S in ((1, 9), (20, 9), (64, 64)) for B in (1, 3, 4, 37)]
# row-streaming form: K4 = 5 (K % 16 != 0), 65 (two waves per row, the second mostly idle), 132 and 192 (three), 256 (four, rstep 1);
# rows 180 (rows_per_block 4), 4096 (16), 4100 (16, ragged last block); B across the 16-sample register chunk
WGRAD_ROWS = [(B, K, S, C) for K in (20, 260, 528, 768, 1024) for C, S in ((20, 9), (64, 64), (205, 20)) for B in (1, 16, 17, 37)]
WGRAD_ACC_REFUSED = [528, 20]
DGRAD = [(B, K, S, C) for K in (16, 256, 272, 1024) for B in (1, 5) for S, C in ((9, 20), (16, 64))]
# ngan_final_dot_fwd (S2, C): LDS without tail (S2 % 4 != 0: the scalar transposition; 12, 16, 256: the 16-byte one), (64, 512): raised
# LDS at n = 32768 exactly, (64, 528): the tail loop, (256, 152): the smallest without LDS, (256, 512): preset 0007
HEAD_SHAPES = [(9, 20), (12, 20), (16, 32), (256, 128), (64, 512), (64, 528), (256, 152), (256, 512)]
HEAD_FWD = [(B, S2, C) for S2, C in HEAD_SHAPES for B in (1, 5)]
HEAD_DX = [(2, S2, C) for S2, C in HEAD_SHAPES] + [(9, 256, 512)]       # 9 * 131072 > 4096 * 256: the grid-stride second trip
HEAD_DW = [(B, S2, C) for S2, C in ((9, 20), (256, 128), (256, 152)) for B in (1, 2, 5)]
WLOSS = [(1, 0), (24, 24), (64, 64), (65, 0), (256, 256), (257, 300), (600, 600)]
DRIFTS = [0.0, 0.001]
GP_B = [1, 6, 64, 257, 600]
L2NORM = [(3, 4), (3, 36), (1, 37), (2, 65536), (2, 65540), (1, 262145)]
ROWS_N = [1, 255, 65536, 70000]
ROWS_B = [1, 3]
LATENT_DIMS = [1, 16, 63, 64, 65, 512, 1000]
LATENT_ROWS = [1, 7]
LATENT_CLAMP = 5.0
AXPBY_N = [1, 257, 1100000]
LERP_N = [1, 1100000]
LAMBDA = 10.0
CA, CB = 0.7, -1.3


def head_uses_lds(S2, C):
    return S2 * (C + 1) * 4 <= 150 * 1024


# ---- fp32 emulation helpers ----------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _tree64(v):
    """group_sum<64>: butterfly over the last axis (64 lanes), lane 0's value"""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def _lanes(x, n):
    """a thread-strided loop `for (i = tid; i < len; i += n)`: (trips, n), zero padded (adding 0 is exact)"""
    x = np.asarray(x, f32)
    pad = (-x.shape[-1]) % n
    if pad:
        x = np.concatenate([x, np.zeros(x.shape[:-1] + (pad,), f32)], -1)
    return x.reshape(x.shape[:-1] + (-1, n))


def _block_sum_256(v):
    """block_sum_256: v (256,) per-thread values"""
    r = _tree64(v.reshape(4, 64))
    return (r[0] + r[1]) + (r[2] + r[3])


def _rows_of(gc):
    """gc (B, S, C) -> (B, C*S): the weight's row order c*S + p"""
    return np.ascontiguousarray(gc.transpose(0, 2, 1).reshape(gc.shape[0], -1))


# ---- generator stem -------------------------------------------------------------------------------------------------------------
STEM_SCALE = 0.0613


@functools.lru_cache(maxsize=4)
def stem_inputs(K, S, C):
    """z (BMAX, K), w (C*S, K), gc (BMAX, S, C), buf (C*S, K): a case with B samples takes the first B rows"""
    return draws(seed_of(11, K, S, C), z=(BMAX, K), w=(C * S, K), gc=(BMAX, S, C), buf=(C * S, K))


def linear_fwd_emulate(z, w, S, C, scale, mode):
    """csrc/linear.hip linear_fwd_kernel: z * scale first; per k-step s and component x / y / z / w one MFMA over the four lane quads
    (k = 16 s + 4 q + j, q = 0..3); LeakyReLU; the sum of squares as an fma chain per 16-lane part and a 16-lane butterfly"""
    B, K = z.shape
    zs = z * f32(scale)
    acc = np.zeros((B, C * S), f32)
    for s in range(K // 16):
        for j in range(4):
            ks = 16 * s + 4 * np.arange(4) + j
            if mode == "exact":
                acc = (acc.astype(f64) + zs[:, ks].astype(f64) @ w[:, ks].astype(f64).T).astype(f32)
            else:
                for k in ks:
                    acc = _fma(zs[:, k:k + 1], w[None, :, k], acc)
    v = acc.reshape(B, C, S).transpose(0, 2, 1)                      # (B, S, C)
    v = np.where(v > 0, v, f32(SLOPE) * v).astype(f32)
    parts = _lanes(v, 16)                                            # (B, S, trips, 16)
    ss = np.zeros(parts.shape[:2] + (16,), f32)
    for t in range(parts.shape[2]):
        ss = _fma(parts[:, :, t], parts[:, :, t], ss)
    idx = np.arange(16)
    for o in (8, 4, 2, 1):
        ss = ss + ss[..., idx ^ o]
    r = np.sqrt(ss[..., 0] / f32(C) + f32(EPS)).astype(f32)
    return {"y": v * (f32(1) / r)[..., None], "rn": r}


def linear_fwd_ref(z, w, S, C, scale, y_stored):
    """{output: (ref, absref, n_round)}; the LeakyReLU pattern is the stored output's"""
    B = z.shape[0]
    sc = r32(scale)
    z64, w64 = z.astype(f64), w.astype(f64)
    u = (sc * z64 @ w64.T).reshape(B, C, S).transpose(0, 2, 1)
    ua = (sc * np.abs(z64) @ np.abs(w64).T).reshape(B, C, S).transpose(0, 2, 1)
    m = W.mask_of(y_stored)
    v, va = u * m, ua * m
    r = np.sqrt((v * v).mean(2, keepdims=True) + EPS)
    ra = np.sqrt((va * va).mean(2, keepdims=True) + EPS)
    y = v / r
    ya = va / r + np.abs(y) * (np.abs(v) * va).mean(2, keepdims=True) / (r * r)
    return {"y": (y, ya, 5), "rn": (r[..., 0], ra[..., 0], 2)}


def linear_wgrad_mfma_emulate(z, gc, scale, mode, buf=None):
    """linear_wgrad_mfma_kernel: one MFMA per group of 4 samples (zero padded), acc * scale, + the buffer with accumulate"""
    B, K = z.shape
    g = _rows_of(gc)
    acc = np.zeros((g.shape[1], K), f32)
    for b0 in range(0, B, 4):
        bs = slice(b0, min(b0 + 4, B))
        if mode == "exact":
            acc = (acc.astype(f64) + g[bs].astype(f64).T @ z[bs].astype(f64)).astype(f32)
        else:
            for b in range(bs.start, bs.stop):
                acc = _fma(g[b][:, None], z[b][None, :], acc)
    out = acc * f32(scale)
    return {"gW": out + buf if buf is not None else out}


def linear_wgrad_rows_emulate(z, gc, scale):
    """linear_wgrad_kernel: fma chains over register chunks of 16 samples, fp32 read-modify-write across the chunks"""
    B, K = z.shape
    g = _rows_of(gc)
    out = None
    for b0 in range(0, B, 16):
        acc = np.zeros((g.shape[1], K), f32)
        for b in range(b0, min(b0 + 16, B)):
            acc = _fma(z[b][None, :], g[b][:, None], acc)
        out = acc * f32(scale) if b0 == 0 else _fma(acc, f32(scale), out)
    return {"gW": out}


def linear_wgrad_ref(z, gc, scale):
    g = _rows_of(gc).astype(f64)
    sc = r32(scale)
    return {"gW": (sc * g.T @ z.astype(f64), sc * np.abs(g).T @ np.abs(z.astype(f64)), 1)}


def linear_dgrad_emulate(gc, w, scale):
    """linear_dgrad_kernel: one sequential fma chain over the weight rows (c outer, p inner)"""
    g = _rows_of(gc)
    acc = np.zeros((g.shape[0], w.shape[1]), f32)
    for j in range(w.shape[0]):
        acc = _fma(g[:, j:j + 1], w[j][None, :], acc)
    return {"gz": acc * f32(scale)}


def linear_dgrad_ref(gc, w, scale):
    g = _rows_of(gc).astype(f64)
    sc = r32(scale)
    return {"gz": (sc * g @ w.astype(f64), sc * np.abs(g) @ np.abs(w.astype(f64)), 1)}


# ---- critic head ------------------------------------------------------------------------------------------------------------------
HEAD_SCALE = 0.0221
HEAD_BMAX = 9


@functools.lru_cache(maxsize=4)
def head_inputs(S2, C):
    """y (HEAD_BMAX, S2, C), w (C, S2), bias (1,), go (HEAD_BMAX,), bufw (C, S2), bufb (1,)"""
    return draws(seed_of(13, S2, C), y=(HEAD_BMAX, S2, C), w=(C, S2), bias=(1,), go=(HEAD_BMAX,), bufw=(C, S2), bufb=(1,))


def final_dot_fwd_emulate(y, w, bias, scale):
    """final_dot_fwd_kernel: 1024 threads, element i = tid + 1024 u.  LDS path: u < 32 into accumulator u & 3, the tail into a[0],
    s = (a0 + a1) + (a2 + a3); without LDS one accumulator.  Then the 64-lane butterfly, the 16 waves in order, t * scale + bias"""
    B, S2, C = y.shape
    yl = _lanes(y.reshape(B, -1), 1024)                               # (B, trips, 1024)
    wl = _lanes(np.ascontiguousarray(w.T).reshape(-1), 1024)          # (p, c) order, as the activations
    trips = yl.shape[1]
    if head_uses_lds(S2, C):
        a = np.zeros((4, B, 1024), f32)
        for u in range(trips):
            i = u & 3 if u < 32 else 0
            a[i] = _fma(yl[:, u], wl[u][None, :], a[i])
        s = (a[0] + a[1]) + (a[2] + a[3])
    else:
        s = np.zeros((B, 1024), f32)
        for u in range(trips):
            s = _fma(yl[:, u], wl[u][None, :], s)
    red = _tree64(s.reshape(B, 16, 64))
    t = np.zeros(B, f32)
    for i in range(16):
        t = t + red[:, i]
    out = t * f32(scale)
    return {"out": out + bias[0] if bias is not None else out}


def final_dot_fwd_ref(y, w, bias, scale):
    sc = r32(scale)
    y64 = y.astype(f64).reshape(y.shape[0], -1)
    w64 = np.ascontiguousarray(w.T).astype(f64).reshape(-1)
    b = float(bias[0]) if bias is not None else 0.0
    return {"out": (sc * y64 @ w64 + b, sc * np.abs(y64) @ np.abs(w64) + abs(b), 1)}


def final_dot_dx_emulate(go, w, scale):
    return {"gy": (f32(scale) * go)[:, None, None] * np.ascontiguousarray(w.T)[None]}


def final_dot_dx_ref(go, w, scale):
    r = r32(scale) * go.astype(f64)[:, None, None] * np.ascontiguousarray(w.T).astype(f64)[None]
    return {"gy": (r, np.abs(r), 2)}


def final_dot_dw_emulate(y, go, scale, bufw=None, bufb=None):
    """final_dot_dw_kernel: two fma chains over the even and the odd samples, s0 + s1, * scale; gb: the samples in order"""
    B = y.shape[0]
    s = [np.zeros(y.shape[1:], f32), np.zeros(y.shape[1:], f32)]
    sb = f32(0)
    for b in range(B):
        s[b & 1] = _fma(go[b], y[b], s[b & 1])
        sb = f32(sb + go[b])
    gw = ((s[0] + s[1]) * f32(scale)).T
    return {"gW": gw + bufw if bufw is not None else gw, "gb": np.array([sb + bufb[0] if bufb is not None else sb], f32)}


def final_dot_dw_ref(y, go, scale):
    sc = r32(scale)
    g64, y64 = go.astype(f64), y.astype(f64)
    return {"gW": (sc * np.einsum("b,bpc->cp", g64, y64), sc * np.einsum("b,bpc->cp", np.abs(g64), np.abs(y64)), 1),
            "gb": (np.array([g64.sum()]), np.array([np.abs(g64).sum()]), 1)}


# ---- scalar heads of the losses ---------------------------------------------------------------------------------------------------
def wloss_inputs(n_real, n_fake):
    return draws(seed_of(17, n_real, n_fake), scores=(n_real + n_fake,), g=(3,))


def wloss_head_emulate(scores, n_real, n_fake, drift):
    """wloss_head_kernel: per-thread sums with stride 256, block_sum_256 each"""
    real, fake = _lanes(scores[:n_real], 256), _lanes(scores[n_real:], 256)
    sr, sq, sf = np.zeros(256, f32), np.zeros(256, f32), np.zeros(256, f32)
    for t in range(real.shape[0]):
        sr = sr + real[t]
        sq = _fma(real[t], real[t], sq)
    for t in range(fake.shape[0] if n_fake else 0):
        sf = sf + fake[t]
    sr, sq, sf = _block_sum_256(sr), _block_sum_256(sq), _block_sum_256(sf)
    mr = sr / f32(n_real)
    mf = sf / f32(n_fake) if n_fake else f32(0)
    loss = -mr + mf + (f32(drift) * sq / f32(n_real) if drift > 0 else f32(0))
    return {"loss": np.array([loss], f32), "mean_real": np.array([mr], f32), "mean_fake": np.array([mf], f32)}


def wloss_head_ref(scores, n_real, n_fake, drift):
    s = scores.astype(f64)
    d = r32(drift)
    real, fake = s[:n_real], s[n_real:]
    mr, mra = real.mean(), np.abs(real).mean()
    mf, mfa = (fake.mean(), np.abs(fake).mean()) if n_fake else (0.0, 0.0)
    q = d * (real * real).mean()
    one = lambda v: np.array([v])
    return {"loss": (one(-mr + mf + q), one(mra + mfa + q), 1), "mean_real": (one(mr), one(mra), 1), "mean_fake": (one(mf), one(mfa), 1)}


def wloss_head_bwd_emulate(scores, n_real, n_fake, drift, gl, gr, gf):
    gl, gr, gf = (f32(0) if v is None else f32(v) for v in (gl, gr, gf))
    real = (gl * (f32(-1) + f32(2) * f32(drift) * scores[:n_real]) + gr) / f32(n_real)
    fake = np.full(n_fake, (gl + gf) / f32(max(n_fake, 1)), f32)
    return {"gs": np.concatenate([real, fake]).astype(f32)}


def wloss_head_bwd_ref(scores, n_real, n_fake, drift, gl, gr, gf):
    gl, gr, gf = (0.0 if v is None else float(v) for v in (gl, gr, gf))
    d = r32(drift)
    s = scores.astype(f64)[:n_real]
    real, reala = (gl * (-1 + 2 * d * s) + gr) / n_real, (abs(gl) * (1 + 2 * d * np.abs(s)) + abs(gr)) / n_real
    fake, fakea = np.full(n_fake, (gl + gf) / max(n_fake, 1)), np.full(n_fake, (abs(gl) + abs(gf)) / max(n_fake, 1))
    return {"gs": (np.concatenate([real, fake]), np.concatenate([reala, fakea]), 2)}


def gp_inputs(B):
    return draws(seed_of(19, B), norms_pos=(B,), g=(1,))


def gp_head_emulate(norms, lam):
    d = _lanes(norms - f32(1), 256)              # the padding's zeros add nothing
    s = np.zeros(256, f32)
    for t in range(d.shape[0]):
        s = _fma(d[t], d[t], s)
    return {"out": np.array([f32(lam) * _block_sum_256(s) / f32(len(norms))], f32)}


def gp_head_ref(norms, lam):
    r = np.array([r32(lam) * ((norms.astype(f64) - 1) ** 2).mean()])
    return {"out": (r, r, 2)}


def gp_coef_emulate(norms, lam, g):
    return {"coef": f32(g) * f32(2) * f32(lam) * (norms - f32(1)) / (f32(len(norms)) * norms)}


def gp_coef_ref(norms, lam, g):
    n = norms.astype(f64)
    r = float(g) * 2 * r32(lam) * (n - 1) / (len(n) * n)
    return {"coef": (r, np.abs(r), 4)}


def l2norm_inputs(B, n):
    return draws(seed_of(23, B, n), g=(B, n))


def sample_l2norm_emulate(g):
    """sample_sumsq_kernel + sample_l2norm_finish_kernel: nchunk blocks of 256 threads, 16-byte loads into 4 fma chains, the tail
    (n % 4) on block 0, wave butterflies and (r0 + r1) + (r2 + r3); then 64 lanes over the chunks, a butterfly and the root"""
    B, n = g.shape
    n4 = n // 4
    nchunk = min(max((n4 + 255) // 256, 1), 64)
    q = _lanes(g[:, :n4 * 4].reshape(B, n4, 4).transpose(0, 2, 1), nchunk * 256)       # (B, 4, trips, nchunk * 256)
    a = np.zeros((B, 4, nchunk * 256), f32)
    for t in range(q.shape[2]):
        a = _fma(q[:, :, t], q[:, :, t], a)
    s = ((a[:, 0] + a[:, 1]) + (a[:, 2] + a[:, 3])).reshape(B, nchunk, 256)
    tail = _lanes(g[:, n4 * 4:], 256) if n % 4 else np.zeros((B, 0, 256), f32)
    for t in range(tail.shape[1]):
        s[:, 0] = _fma(tail[:, t], tail[:, t], s[:, 0])
    r = _tree64(s.reshape(B, nchunk, 4, 64))
    part = (r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])          # (B, nchunk)
    lanes = _lanes(part, 64)
    f = np.zeros((B, 64), f32)
    for t in range(lanes.shape[1]):
        f = f + lanes[:, t]
    return {"norms": np.sqrt(_tree64(f)).astype(f32)}


def sample_l2norm_ref(g):
    r = np.sqrt((g.astype(f64) ** 2).sum(1))
    return {"norms": (r, r, 1)}


def rows_inputs(B, n):
    return draws(seed_of(29, B, n), g=(B, n), real=(B, n), fake=(B, n), coef=(B,), eps=(B,))


def scale_rows_emulate(g, coef):
    return {"out": coef[:, None] * g}


def scale_rows_ref(g, coef):
    r = coef.astype(f64)[:, None] * g.astype(f64)
    return {"out": (r, np.abs(r), 1)}


def xhat_emulate(real, fake, eps):
    e = eps[:, None]
    return {"out": e * real + (f32(1) - e) * fake}


def xhat_ref(real, fake, eps):
    e, r, f = eps.astype(f64)[:, None], real.astype(f64), fake.astype(f64)
    return {"out": (e * r + (1 - e) * f, np.abs(e) * np.abs(r) + (1 + np.abs(e)) * np.abs(f), 1)}


def latent_inputs(rows, dim):
    d = draws(seed_of(31, rows, dim), z=(rows, dim))
    d["z"] = (d["z"] * f32(3)).astype(f32)           # so that the clamp at 5 acts
    return d


def latent_normalize_emulate(z, c):
    v = np.clip(z, f32(-c), f32(c))
    lanes = _lanes(v, 64)
    ss = np.zeros((z.shape[0], 64), f32)
    for t in range(lanes.shape[1]):
        ss = _fma(lanes[:, t], lanes[:, t], ss)
    inv = f32(1) / np.sqrt(_tree64(ss)).astype(f32)
    return {"z": v * inv[:, None]}


def latent_normalize_ref(z, c):
    v = np.clip(z.astype(f64), -c, c)
    r = v / np.sqrt((v * v).sum(1, keepdims=True))
    return {"z": (r, np.abs(r), 3)}


def ew_inputs(n):
    return draws(seed_of(37, n), a=(n,), b=(n,))


def axpby_emulate(a, b, ca, cb):
    t = f32(ca) * a
    return {"out": _fma(f32(cb), b, t) if b is not None else t}


def axpby_ref(a, b, ca, cb):
    t = r32(ca) * a.astype(f64)
    if b is None:
        return {"out": (t, np.abs(t), 1)}
    u = r32(cb) * b.astype(f64)
    return {"out": (t + u, np.abs(t) + np.abs(u), 1)}
