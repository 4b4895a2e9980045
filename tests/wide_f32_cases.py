"""The fp32 per-pixel operators at the compatibility widths: inputs, fp64 references with their absolute-value twins, the
per-element bound, and an fp32 emulation in the summation order of csrc/wide.hip.  Shared by tests/test_gpu_wide_f32.py (the
kernels against the references) and tests/test_wide_f32_bounds_cpu.py (the emulation against the references: it settles the
constants of the bound on the CPU, before any kernel is looked at).

Bound, per element:   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref,   C_ACC = 8
  absref   the operator's whole formula with absolute values propagated through it, per-pixel sums included (no factor C)
  n_round  the fp32 roundings applied to the element's value AFTER its last addition or subtraction (each is relative to |ref|).  The
           roundings before it act on the terms of that sum; they are relative to the terms, whose magnitudes add up to absref, and
           are carried by the accumulation term together with the error of the sums.
n_round per operator, from csrc/wide.hip (pixelnorm.hip / pointwise.hip compute the same expressions):
  pn_fwd           y = lrelu(c + b) * (1 / sqrt(ss / C + eps)): slope product, sqrt, reciprocal, scaling                     4
  pn_bwd / bwd2    ((g - y s) inv_r + kk y) m: subtraction, reciprocal, product with inv_r, mask product                     4
                   with gr: the addition of kk y as well                                                                    5
  pn_bwdbwd ggy    (m h - y t) inv_r: mask product, subtraction, reciprocal, product                                         4
            gy_out -(s h' + t g) inv_r: addition, reciprocal, product                                                        3
            gr_out -C (u - s t) inv_r inv_r: subtraction, product with C, reciprocal, two products                           5
  channel_sum      s * scale                                                                                                1
  to_image_fwd     tanhf of the dot product: the device library's tanh is within 2 ulp                                      2
  to_image_bwd gx  fma chain over the colours of w q, q = g (1 - t t) (absref: |g| (1 + t t)): product with g, the last fma  2
               gw  a sum over pixels; the roundings of q are per term                                                       1
  to_image_bwd_pnbwd gc  (o - y sdot) inv_r m: subtraction, reciprocal, two products                                         4
  from_image_dx / dw / db   fma chains; 0.25 s is exact                                                                     1
  up2_adjoint      fma chains over the taps                                                                                 1
  up2_adjoint_pnbwd  the adjoint (stored, a term of the subtraction) then pn_bwd                                            4
  pool2_fwd 0.25 ((a + b) + (c + d)): 1;  pool2_adjoint 0.25 g: 1;  lerp fma(alpha, b - a, a): 1;  fade_bwd (1 - alpha) g: 2

RAISED lists the (operator output, C) whose emulated worst err / bound exceeds 0.5 with C_ACC = 8, with the next power of two that
brings it to 0.5 or below and the emulated ratio at that constant; tests/test_wide_f32_bounds_cpu.py pins both."""
import numpy as np
import torch

from fp64_conv import pool2, resample_adjoint

SLOPE = 0.2
EPS = 1e-8
WIDTHS = [4, 8, 48, 96, 192, 256, 320, 512, 1024]       # 4 / 8 / 256: the lane-group kernels' boundary widths; the rest: csrc/wide.hip
PIXELS = [96, 256, 257, 1000]                           # one block, one full block, one pixel into the second, three full + ragged
SHAPES = {96: (2, 6, 8), 256: (1, 16, 16), 257: (1, 257, 1), 1000: (2, 20, 25)}      # (B, H, W) of the image-shaped operators
C_ACC = 8.0
# (output, C) -> (raised C_ACC, emulated worst err / bound at that constant)
RAISED = {("pn_fwd_bias/y", 1024): (16.0, 0.355)}      # 0.533 with C_ACC = 8: the error of the 1024-term sum of squares reaches every y through r

f32, f64 = np.float32, np.float64


def c_acc(name, C):
    return float(RAISED.get((name, C), (C_ACC, None))[0])


def ratio(got, ref, absref, n_round, c=C_ACC):
    """worst err / bound over the elements"""
    got = np.asarray(got, dtype=f64)
    bound = n_round * 2.0 ** -23 * np.abs(ref) + c * 2.0 ** -24 * absref + 1e-30
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    return float((np.abs(got - ref) / bound).max())


def is_wide(C):
    """True where the entry points dispatch to csrc/wide.hip (pixelnorm.hip: lpp_ok, pointwise.hip: pow2_quads)"""
    q = C // 4
    return not (q <= 64 and (q & (q - 1)) == 0)


def draws(seed, **shapes):
    """name -> fp32 array; a name ending in '_pos' is uniform in [0.5, 1.5) (norms), every other standard normal"""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for k, shp in shapes.items():
        t = torch.rand(*shp, generator=gen) + 0.5 if k.endswith("_pos") else torch.randn(*shp, generator=gen)
        out[k] = t.numpy().astype(f32)
    return out


def mask_of(y):
    return np.where(np.asarray(y, dtype=f64) > 0, 1.0, SLOPE)


# (_fma, _m32, _q32, _adj_w, _pooled_img32 and _pool_adjoint_img are shared with tests/lane_group_cases.py, which imports them: keep their meaning)
# ---- fp32 emulation helpers: the order of csrc/wide.hip -------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def _dot4(a, b):
    """per-pixel sum over the channels: one sequential accumulator, four channels per step (f4dot)"""
    s = np.zeros(a.shape[0], f32)
    for k in range(0, a.shape[1], 4):
        s = s + (((a[:, k] * b[:, k] + a[:, k + 1] * b[:, k + 1]) + a[:, k + 2] * b[:, k + 2]) + a[:, k + 3] * b[:, k + 3])
    return s


def _m32(y):
    return np.where(y > 0, f32(1), f32(SLOPE)).astype(f32)


# ---- LeakyReLU -> PixelNorm ------------------------------------------------------------------------------------------------------
def pn_inputs(C, P):
    d = draws(1000 * C + P, c=(P, C), b=(C,), gy=(P, C), gy2=(P, C), y=(P, C), h=(P, C), rn_pos=(P,), gr=(P,))
    d["b"] = (d["b"] * f32(0.3)).astype(f32)
    return d


def pn_fwd_emulate(c, b):
    v = c + b[None, :] if b is not None else c
    v = np.where(v > 0, v, f32(SLOPE) * v).astype(f32)
    r = np.sqrt(_dot4(v, v) / f32(c.shape[1]) + f32(EPS)).astype(f32)
    inv = f32(1) / r
    return {"y": v * inv[:, None], "rn": r}


def pn_fwd_ref(c, b, y_stored):
    """{output: (ref, absref, n_round)}; the LeakyReLU pattern is the stored output's"""
    c64 = c.astype(f64)
    b64 = b.astype(f64)[None, :] if b is not None else 0.0
    m = mask_of(y_stored)
    a = (c64 + b64) * m
    r = np.sqrt((a * a).mean(1, keepdims=True) + EPS)
    aabs = (np.abs(c64) + np.abs(b64)) * m
    return {"y": (a / r, aabs / r, 4), "rn": (r[:, 0], r[:, 0], 4)}


def pn_bwd_emulate(gy, gy2, gr, y, rn):
    C = y.shape[1]
    g = gy + gy2 if gy2 is not None else gy
    inv_c, inv_r = f32(1) / f32(C), f32(1) / rn
    s = _dot4(g, y) * inv_c
    kk = gr * inv_c if gr is not None else np.zeros_like(rn)
    return {"gc": ((g - y * s[:, None]) * inv_r[:, None] + kk[:, None] * y) * _m32(y)}


def pn_bwd_ref(gy, gy2, gr, y, rn):
    C = y.shape[1]
    g = gy.astype(f64) + (gy2.astype(f64) if gy2 is not None else 0.0)
    ga = np.abs(gy.astype(f64)) + (np.abs(gy2.astype(f64)) if gy2 is not None else 0.0)
    y64, r, m = y.astype(f64), rn.astype(f64)[:, None], mask_of(y)
    kk = gr.astype(f64)[:, None] / C if gr is not None else 0.0
    s = (g * y64).mean(1, keepdims=True)
    sa = (ga * np.abs(y64)).mean(1, keepdims=True)
    ref = ((g - y64 * s) / r + kk * y64) * m
    absref = ((ga + np.abs(y64) * sa) / r + np.abs(kk) * np.abs(y64)) * m
    return {"gc": (ref, absref, 5 if gr is not None else 4)}


def pn_bwdbwd_emulate(h, gy, y, rn):
    C = y.shape[1]
    hp = h * _m32(y)
    inv_c, inv_r = f32(1) / f32(C), (f32(1) / rn)
    s, t, u = _dot4(gy, y) * inv_c, _dot4(hp, y) * inv_c, _dot4(hp, gy) * inv_c
    ir = inv_r[:, None]
    return {"ggy": (hp - y * t[:, None]) * ir, "gy_out": -(s[:, None] * hp + t[:, None] * gy) * ir,
            "gr_out": -f32(C) * (u - s * t) * inv_r * inv_r}


def pn_bwdbwd_ref(h, gy, y, rn):
    C = y.shape[1]
    g, y64, r = gy.astype(f64), y.astype(f64), rn.astype(f64)[:, None]
    hp = h.astype(f64) * mask_of(y)
    s, t, u = (g * y64).mean(1, keepdims=True), (hp * y64).mean(1, keepdims=True), (hp * g).mean(1, keepdims=True)
    sa = (np.abs(g) * np.abs(y64)).mean(1, keepdims=True)
    ta = (np.abs(hp) * np.abs(y64)).mean(1, keepdims=True)
    ua = (np.abs(hp) * np.abs(g)).mean(1, keepdims=True)
    return {"ggy": ((hp - y64 * t) / r, (np.abs(hp) + np.abs(y64) * ta) / r, 4),
            "gy_out": (-(s * hp + t * g) / r, (sa * np.abs(hp) + ta * np.abs(g)) / r, 3),
            "gr_out": ((-C * (u - s * t) / r ** 2)[:, 0], (C * (ua + sa * ta) / r ** 2)[:, 0], 5)}


# ---- channel sums and the image edges ---------------------------------------------------------------------------------------------
def edge_inputs(C, P, ncol):
    B, H, W = SHAPES[P]
    d = draws(7000 * C + 10 * P + ncol, g=(P, C), buf=(C,), x=(P, C), wimg=(ncol, C), gt=(P, ncol), rn_pos=(P,), bufw=(ncol, C),
              gimg=(P, C), wf=(C, ncol), img=(B, H, W, ncol), img2=(B, 2 * H, 2 * W, ncol), bufwf=(C, ncol), bufb=(C,))
    d["wimg"] = (d["wimg"] / f32(np.sqrt(C))).astype(f32)
    d["t"] = np.tanh(d["x"].astype(f64) @ d["wimg"].astype(f64).T).astype(f32)       # the forward's output, an input of the backward
    return d


CHANNEL_SUM_SCALE = 0.5


def channel_sum_emulate(g):
    # (csrc/wide.hip sums the pixels in runs of 1024 -- wide_pixel_sum; up to 1024 pixels, i.e. for every case of PIXELS, that is this
    # one sequential accumulator, bit for bit.  tests/test_gpu_large_offsets.py runs the reductions at 4.5e7 pixels.)
    s = np.zeros(g.shape[1], f32)
    for p in range(g.shape[0]):
        s = s + g[p]
    return {"out": s * f32(CHANNEL_SUM_SCALE)}


def channel_sum_ref(g):
    g64 = g.astype(f64)
    return {"out": (CHANNEL_SUM_SCALE * g64.sum(0), CHANNEL_SUM_SCALE * np.abs(g64).sum(0), 1)}


def to_image_fwd_emulate(x, w):
    return {"t": np.stack([np.tanh(_dot4(x, np.broadcast_to(w[k], x.shape))) for k in range(w.shape[0])], 1).astype(f32)}


def to_image_fwd_ref(x, w):
    d = x.astype(f64) @ w.astype(f64).T
    return {"t": (np.tanh(d), np.abs(x.astype(f64)) @ np.abs(w.astype(f64)).T, 2)}      # |tanh'| <= 1


def _q32(gt, t):
    return gt * (f32(1) - t * t)


def to_image_bwd_emulate(gt, t, x, w, rn):
    P, C = x.shape
    q = _q32(gt, t)
    o = np.zeros((P, C), f32)
    for k in range(w.shape[0]):
        o = _fma(np.broadcast_to(w[k][None, :], (P, C)), np.broadcast_to(q[:, k:k + 1], (P, C)), o)
    gw = np.zeros(w.shape, f32)
    for p in range(P):
        gw = _fma(np.broadcast_to(x[p][None, :], gw.shape), np.broadcast_to(q[p][:, None], gw.shape), gw)
    if rn is not None:
        sdot = _dot4(o, x) * (f32(1) / f32(C))
        o = (o - x * sdot[:, None]) * (f32(1) / rn)[:, None] * _m32(x)
    return {"gx": o, "gw": gw}


def to_image_bwd_ref(gt, t, x, w, rn):
    C = x.shape[1]
    q = gt.astype(f64) * (1 - t.astype(f64) ** 2)
    x64, w64 = x.astype(f64), w.astype(f64)
    qa = np.abs(gt.astype(f64)) * (1 + t.astype(f64) ** 2)          # 1 - t t is a subtraction: both its terms count
    o, oa = q @ w64, qa @ np.abs(w64)
    out = {"gw": (q.T @ x64, qa.T @ np.abs(x64), 1)}
    if rn is None:
        out["gx"] = (o, oa, 2)
        return out
    m, r = mask_of(x), rn.astype(f64)[:, None]
    s, sa = (o * x64).mean(1, keepdims=True), (oa * np.abs(x64)).mean(1, keepdims=True)
    out["gx"] = ((o - x64 * s) / r * m, (oa + np.abs(x64) * sa) / r * m, 4)
    return out


def _pool_adjoint_img(v, B, H, W):
    v = v.reshape(B, H, W, -1)
    return 0.25 * v.repeat(2, axis=1).repeat(2, axis=2)


def from_image_dx_emulate(g, wf, shape, pool):
    B, H, W = shape
    P, C = g.shape
    s = np.zeros((P, wf.shape[1]), f32)
    for c in range(C):
        s = _fma(np.broadcast_to(g[:, c:c + 1], s.shape), np.broadcast_to(wf[c][None, :], s.shape), s)
    return {"gx": _pool_adjoint_img(s, B, H, W).astype(f32) if pool else s.reshape(B, H, W, -1)}


def from_image_dx_ref(g, wf, shape, pool):
    B, H, W = shape
    r, ra = g.astype(f64) @ wf.astype(f64), np.abs(g.astype(f64)) @ np.abs(wf.astype(f64))
    if pool:
        return {"gx": (_pool_adjoint_img(r, B, H, W), _pool_adjoint_img(ra, B, H, W), 1)}
    return {"gx": (r.reshape(B, H, W, -1), ra.reshape(B, H, W, -1), 1)}


def _pooled_img32(img):
    return f32(0.25) * ((img[:, 0::2, 0::2] + img[:, 0::2, 1::2]) + (img[:, 1::2, 0::2] + img[:, 1::2, 1::2]))


def from_image_dw_emulate(img, g, pool):
    xi = (_pooled_img32(img) if pool else img).reshape(g.shape[0], -1)
    C, ncol = g.shape[1], xi.shape[1]
    acc, sb = np.zeros((C, ncol), f32), np.zeros(C, f32)
    for p in range(g.shape[0]):
        sb = sb + g[p]
        acc = _fma(np.broadcast_to(g[p][:, None], acc.shape), np.broadcast_to(xi[p][None, :], acc.shape), acc)
    return {"gw": acc, "gb": sb}


def from_image_dw_ref(img, g, pool):
    i64 = img.astype(f64)
    xi, xa = i64, np.abs(i64)
    if pool:
        xi, xa = pool2(torch.from_numpy(xi)).numpy(), pool2(torch.from_numpy(xa)).numpy()
    g64 = g.astype(f64)
    xi, xa = xi.reshape(g.shape[0], -1), xa.reshape(g.shape[0], -1)
    return {"gw": (g64.T @ xi, np.abs(g64).T @ xa, 1), "gb": (g64.sum(0), np.abs(g64).sum(0), 1)}


# ---- resampling and the fade-in arithmetic ----------------------------------------------------------------------------------------
def resample_inputs(C, P):
    B, h, w = SHAPES[P]
    return draws(3000 * C + P, g=(B, 2 * h, 2 * w, C), y=(B, h, w, C), rn_pos=(B, h, w), lo=(B, h, w, C), a=(B, h, w, C), b=(B, h, w, C))


def _adj_w(i, R, n):
    if R < 0 or R > 2 * n - 1:
        return 0.0
    d = R - 2 * i
    if d in (-1, 2):
        return 0.25
    if d == 0:
        return 1.0 if i == 0 else 0.75
    return 1.0 if i == n - 1 else 0.75


def up2_adjoint_emulate(g):
    """rows of taps summed with fmas, then the rows (up2_adjoint_vec_kernel)"""
    B, h2, w2, C = g.shape
    h, w = h2 // 2, w2 // 2
    out = np.zeros((B, h, w, C), f32)
    for Y in range(h):
        for X in range(w):
            s = np.zeros((B, C), f32)
            for dy in range(-1, 3):
                wy = _adj_w(Y, 2 * Y + dy, h)
                if wy == 0.0:
                    continue
                row = np.zeros((B, C), f32)
                for dx in range(-1, 3):
                    wx = _adj_w(X, 2 * X + dx, w)
                    if wx != 0.0:
                        row = _fma(g[:, 2 * Y + dy, 2 * X + dx, :], np.full((B, C), wx, f32), row)
                s = _fma(row, np.full((B, C), wy, f32), s)
            out[:, Y, X, :] = s
    return {"gx": out}


def up2_adjoint_ref(g):
    g64 = torch.from_numpy(g.astype(f64))
    return {"gx": (resample_adjoint(g64, 2).numpy(), resample_adjoint(g64.abs(), 2).numpy(), 1)}


def up2_adjoint_pnbwd_emulate(g, y, rn):
    C = y.shape[-1]
    adj = up2_adjoint_emulate(g)["gx"].reshape(-1, C)
    return {"out": pn_bwd_emulate(adj, None, None, y.reshape(-1, C), rn.reshape(-1))["gc"].reshape(y.shape)}


def up2_adjoint_pnbwd_ref(g, y, rn):
    C = y.shape[-1]
    adj, adj_abs, _ = up2_adjoint_ref(g)["gx"]
    y64, r, m = y.astype(f64), rn.astype(f64)[..., None], mask_of(y)
    s, sa = (adj * y64).mean(-1, keepdims=True), (adj_abs * np.abs(y64)).mean(-1, keepdims=True)
    return {"out": ((adj - y64 * s) / r * m, (adj_abs + np.abs(y64) * sa) / r * m, 4)}


def pool2_emulate(x):
    return {"y": _pooled_img32(x)}


def pool2_ref(x):
    x64 = torch.from_numpy(x.astype(f64))
    return {"y": (pool2(x64).numpy(), pool2(x64.abs()).numpy(), 1)}


def pool2_adjoint_emulate(gy):
    return {"gx": (f32(0.25) * gy).repeat(2, axis=1).repeat(2, axis=2)}


def pool2_adjoint_ref(gy):
    r = 0.25 * gy.astype(f64).repeat(2, axis=1).repeat(2, axis=2)
    return {"gx": (r, np.abs(r), 1)}


ALPHA = 0.3


def lerp_emulate(a, b):
    al = np.full(a.shape, ALPHA, f32)
    return {"out": _fma(al, b - a, a)}


def lerp_ref(a, b):
    al = float(f32(ALPHA))
    a64, b64 = a.astype(f64), b.astype(f64)
    return {"out": (a64 + al * (b64 - a64), np.abs(a64) + al * (np.abs(b64) + np.abs(a64)), 1)}


def fade_bwd_emulate(g):
    al = f32(ALPHA)
    return {"ga": (f32(1) - al) * g, "gb": al * g}


def fade_bwd_ref(g):
    al = float(f32(ALPHA))
    g64 = g.astype(f64)
    return {"ga": ((1 - al) * g64, np.abs((1 - al) * g64), 2), "gb": (al * g64, np.abs(al * g64), 2)}


# ---- convolution cases of tests/test_gpu_wide_f32.py (tests/test_wide_f32_bounds_cpu.py runs torch's fp32 on the same) -------------
CONV_WIDE = [
    # B, H, W, Cin, Cout, resample, bias.  Every chunk-list shape of ops._n_chunks over the output channels ...
    (2, 8, 8, 32, 256, 0, True),        # (128, 128)
    (2, 8, 8, 16, 240, 0, False),       # (128, 64, 32, 16)
    (2, 8, 8, 64, 320, 0, True),        # (128, 128, 64)
    (2, 8, 8, 32, 144, 0, False),       # (128, 16)
    (2, 4, 4, 64, 512, 0, True), (2, 4, 4, 32, 1024, 0, False),
    # ... every contraction width with a tuned Cout (the input gradient is chunked over Cin) ...
    (2, 8, 8, 48, 16, 0, False), (2, 16, 16, 96, 64, 0, True), (1, 32, 32, 192, 16, 0, False), (4, 4, 4, 256, 128, 0, False),
    (1, 12, 20, 320, 32, 0, True), (2, 8, 8, 512, 64, 0, False), (4, 4, 4, 1024, 128, 0, True),
    # ... both wide: the presets' layers ...
    (2, 16, 16, 256, 256, 0, True), (2, 8, 8, 512, 512, 0, False), (4, 4, 4, 1024, 512, 0, True),
    # ... pooled and bilinear input on layers chunked over Cout, over Cin (the chunked _run_dgrad's own branches) and over both ...
    (2, 8, 8, 64, 256, 1, False), (2, 8, 8, 64, 256, 2, True), (2, 8, 8, 256, 64, 1, False), (2, 8, 8, 320, 32, 2, False),
    (2, 8, 8, 256, 256, 1, False), (1, 16, 16, 256, 144, 2, False),
    # ... ragged tile edges on chunked layers
    (1, 12, 20, 48, 240, 0, True), (1, 12, 20, 256, 64, 0, False),
]
CONV_RAW_WIDE = [(2, 8, 8, 48, 240, 0, True), (1, 8, 8, 256, 96, 1, False), (1, 8, 8, 320, 256, 2, False)]
# chunking is copies only: (B, H, W, Cin, Cout, resample) for the bit-equality tests
CHUNK_EQUAL = [(2, 8, 8, 240, 240, 0), (2, 8, 8, 256, 320, 1), (1, 12, 20, 320, 144, 2)]
WGRAD_WIDE = [
    # B, H, W, Cin, Cout, resample
    (2, 8, 8, 48, 16, 0), (2, 8, 8, 48, 16, 1), (2, 8, 8, 48, 16, 2), (2, 12, 20, 16, 48, 0), (2, 8, 8, 16, 48, 1), (2, 16, 16, 96, 192, 0),
    (1, 8, 8, 96, 192, 2), (2, 8, 8, 256, 256, 0), (1, 8, 8, 256, 256, 1), (2, 8, 8, 320, 32, 0), (1, 8, 8, 320, 32, 2), (2, 8, 8, 512, 128, 0),
    (1, 4, 4, 512, 128, 1), (2, 4, 4, 1024, 512, 0), (1, 4, 4, 1024, 512, 2),
]
# models._conv_any_width: B, H, W, Cin, Cout, resample, LeakyReLU -> PixelNorm
PAD_CASES = [(2, 8, 12, ci, co, res, act) for ci, co in ((8, 8), (16, 8), (8, 16), (24, 40), (12, 20)) for res in (0, 1, 2) for act in (True, False)]


def conv_tensors(case):
    """the operands of a conv case (B, H, W, Cin, Cout, resample, bias) as run_both takes them, its resample code and equalised-LR scale"""
    B, H, Wd, Cin, Cout, res, use_bias = case
    torch.manual_seed(hash(case) % 1000)
    hin, win = (2 * H, 2 * Wd) if res == 1 else ((H // 2, Wd // 2) if res == 2 else (H, Wd))
    t = {"x": torch.randn(B, Cin, hin, win), "w": torch.randn(Cout, Cin, 3, 3)}
    if use_bias:
        t["b"] = torch.randn(Cout) * 0.5
    return t, res, 1.3868 / np.sqrt(9 * Cin)
