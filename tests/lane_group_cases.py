"""The per-pixel operators at the lane-group widths (csrc/pixelnorm.hip, csrc/pointwise.hip: C in 4 ... 256 with C / 4 a power of
two -- every width of the default configurations and of the benchmark), in both activation storage types: case lists, the fp64
references that tests/wide_f32_cases.py does not have, the per-element bounds, and an fp32 / bf16 emulation in the lane-group
kernels' own summation order.  Shared by tests/test_gpu_lane_group.py (the kernels against the references) and
tests/test_lane_group_bounds_cpu.py (the emulation against the references: it settles the constants on the CPU before any kernel is
looked at, and shows that wrong emulations miss the bounds).  No test in here, and nothing of the package is imported.

References: fp64 with absolute-value twins, imported from tests/wide_f32_cases.py (whose docstring holds the n_round table of the
operators both files share); each returns {output: (ref, absref, n_round)}.  Added here, n_round re-derived from the kernel text:
  up2_fwd            top = fma(x01, wx1, x00 wx0), bot likewise, y = fma(bot, wy1, top wy0): the roundings of top, bot and top wy0 act on
                     terms of the last fma's sum (the accumulation term carries them); one rounding after that addition          1
  from_image_fwd     o = bias, then o = fma(w[c][k], v_k, o) over the colours; v_k is the image value or 0.25 ((a + b) + (c + d)) of
                     the pooled one (a term: its two roundings are relative to the term); one rounding after the last fma      1
  pn_fwd, no bias    y = lrelu(c) * (1 / sqrt(ss / C + eps)): slope product, sqrt, reciprocal, scaling -- as with the bias, whose
                     addition is the last ADDITION of the chain and comes before all four (wide_f32_cases.pn_fwd_ref, b = None)  4

Bounds, per element (derived; nothing here was fitted to a kernel's result):
  an fp32 output, in either storage type   |got - ref| <= e32 = n_round 2^-23 |ref| + C_ACC 2^-24 absref,   C_ACC = 8
  a bf16 output                            |got - ref| <= 2^-8 |ref| + (1 + 2^-8) e32
The second is one round-to-nearest-even rounding (unit roundoff 2^-8) of an fp32 value v within e32 of the reference:
|rne(v) - ref| <= 2^-8 |v| + |v - ref| <= 2^-8 (|ref| + e32) + e32.  A store that truncates is off by up to 2^-7 |v| and misses it.  In the
bf16 storage type the operands are bf16-representable fp32 arrays (rounded once through torch's bfloat16, nearest even), the fp64
reference is evaluated on those rounded operands, and the outputs include/ngan.h declares `ngan_bf16*` are rounded once; norms,
gr_out, channel sums, images, parameter and image gradients stay fp32.  LeakyReLU masks are those of the stored y.

Emulation order (class Emulator): V quads per lane and LPP lanes per pixel as the dispatch picks them -- fp32: V = 1, LPP = C / 4; bf16:
V = 2, LPP = C / 8 where C % 8 == 0 (PN_DISPATCH; `wide_access` of to_image_bwd and from_image_fwd), else as fp32; the other bf16
kernels of pointwise.hip keep one quad per lane.  A lane adds f4dot over its V quads, then the butterfly of group_sum<LPP>
(v += shfl_xor(v, o) for o = LPP / 2 ... 1).  Parameter gradients and channel sums follow their kernels: a thread accumulates its
pixels with stride gridDim * 256 / Q (two per trip where V = 2), block_quad_sum adds the 256 / Q threads of a channel quad in
ascending order, reduce_partials_kernel adds the blocks (lane l takes parts l, l + 64, ... in four accumulators while four fit, the
rest into the first; (s0 + s1) + (s2 + s3); butterfly over 64 lanes).  from_image_dw_kernel: one block per image row, a thread walks
the columns with stride 256 / Q.  up2_adjoint_strip_kernel: four horizontal taps per high-resolution row (a product, then three
fmas, clamped indices with zero weights), then the same over the four rows.

RAISED lists the (output, C) whose emulated fp32 worst err / bound exceeds 0.5 at C_ACC = 8, with the next power of two that
brings it to 0.5 or below and the emulated ratio there; tests/test_lane_group_bounds_cpu.py pins both."""
import numpy as np
import torch

import fp64_conv
import wide_f32_cases as W
from wide_f32_cases import (ALPHA, C_ACC, CHANNEL_SUM_SCALE, EPS, SLOPE, channel_sum_ref, draws, f32, f64, fade_bwd_ref,     # noqa: F401
                            from_image_dw_ref, from_image_dx_ref, lerp_ref, mask_of, pn_bwd_ref, pn_bwdbwd_ref, pn_fwd_ref,
                            pool2_adjoint_ref, pool2_ref, ratio, to_image_bwd_ref, to_image_fwd_ref, up2_adjoint_pnbwd_ref,
                            up2_adjoint_ref)
# (the helpers below are shared on purpose: see the note above them in tests/wide_f32_cases.py)
from wide_f32_cases import _adj_w, _fma, _m32, _pool_adjoint_img, _pooled_img32, _q32

LANE_WIDTHS = [4, 8, 16, 32, 64, 128, 256]              # 1, 2, 4, 8, 16, 32, 64 lanes per pixel in fp32; 1, 1, 2, ... 32 in bf16
LANE_PIXELS = [1, 3, 96, 256, 257, 1000]                # 1 and 3: less than one lane group's share of a block; the rest: W.PIXELS
# (B, H, W) of the image-shaped operators, and the low-resolution grid of the resampling ones: (2, 6, 8) is not square, (1, 1, 1) and
# (1, 1, 3) have h = 1 (every vertical tap clamped), (1, 257, 1) has w = 1
SHAPES = {1: (1, 1, 1), 3: (1, 1, 3), **W.SHAPES}
STORAGES = ["float", "bf16"]
# (output, C) -> (raised C_ACC, emulated fp32 worst err / bound at that constant)
RAISED = {}


def c_acc(name, C):
    return float(RAISED.get((name, C), (C_ACC, None))[0])


def lanes(C, storage):
    """(V, LPP) of the pixelnorm.hip instances, to_image_bwd_kernel and from_image_fwd_kernel"""
    V = 2 if storage == "bf16" and C % 8 == 0 else 1
    return V, C // (4 * V)


def rbf(a):
    """round to bf16 (nearest even, torch's conversion) and back: a bf16-representable fp32 array"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).to(torch.bfloat16).float().numpy()


def trunc_bf16(a):
    """the wrong store: the low 16 bits dropped"""
    return (np.ascontiguousarray(a, dtype=f32).view(np.uint32) & np.uint32(0xffff0000)).view(f32)


def ratio_bf16(got, ref, absref, n_round, c=C_ACC):
    """worst err / bound over the elements of a bf16 output"""
    got = np.asarray(got, dtype=f64)
    e32 = n_round * 2.0 ** -23 * np.abs(ref) + c * 2.0 ** -24 * absref
    bound = 2.0 ** -8 * np.abs(ref) + (1 + 2.0 ** -8) * e32 + 1e-30
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    return float((np.abs(got - ref) / bound).max())


def worst(name, C, got, ref, bf16_out):
    r, a, n = ref
    return (ratio_bf16 if bf16_out else ratio)(got, r, a, n, c_acc(name, C))


def plus(ref, buf):
    """reference of an accumulating form that starts from `buf`: the addition is the element's last, so n_round stays"""
    r, a, n = ref
    return r + buf.astype(f64), a + np.abs(buf.astype(f64)), n


# ---- inputs: those of tests/wide_f32_cases.py at these shapes; activations bf16-representable in the bf16 storage type --------------
def _act(d, storage, names):
    if storage == "bf16":
        for k in names:
            d[k] = rbf(d[k])
    return d


def pn_inputs(C, P, storage):
    d = draws(1000 * C + P, c=(P, C), b=(C,), gy=(P, C), gy2=(P, C), y=(P, C), h=(P, C), rn_pos=(P,), gr=(P,))
    d["b"] = (d["b"] * f32(0.3)).astype(f32)
    d["c"][0] *= f32(2.0 ** -13)                 # pixel 0: mean square ~ 8e-9, next to eps = 1e-8 (without the bias)
    return _act(d, storage, ("c", "gy", "gy2", "y", "h"))


def edge_inputs(C, P, ncol, storage):
    B, H, Wd = SHAPES[P]
    d = draws(7000 * C + 10 * P + ncol, g=(P, C), buf=(C,), x=(P, C), wimg=(ncol, C), gt=(P, ncol), rn_pos=(P,), bufw=(ncol, C),
              gimg=(P, C), wf=(C, ncol), img=(B, H, Wd, ncol), img2=(B, 2 * H, 2 * Wd, ncol), bufwf=(C, ncol), bufb=(C,), bimg=(C,))
    d["wimg"] = (d["wimg"] / f32(np.sqrt(C))).astype(f32)
    _act(d, storage, ("g", "x", "gimg"))
    d["t"] = np.tanh(d["x"].astype(f64) @ d["wimg"].astype(f64).T).astype(f32)       # the forward's output, an input of the backward
    return d


def resample_inputs(C, P, storage):
    B, h, w = SHAPES[P]
    d = draws(3000 * C + P, g=(B, 2 * h, 2 * w, C), y=(B, h, w, C), rn_pos=(B, h, w), lo=(B, h, w, C), a=(B, h, w, C), b=(B, h, w, C))
    return _act(d, storage, ("g", "y", "lo", "a", "b"))


# ---- references tests/wide_f32_cases.py does not have --------------------------------------------------------------------------------
def up2_fwd_ref(x):
    x64 = torch.from_numpy(x.astype(f64))
    return {"y": (fp64_conv.up2(x64).numpy(), fp64_conv.up2(x64.abs()).numpy(), 1)}


def from_image_fwd_ref(img, wf, bias, pool):
    i64 = torch.from_numpy(img.astype(f64))
    xi, xa = (fp64_conv.pool2(i64), fp64_conv.pool2(i64.abs())) if pool else (i64, i64.abs())
    w64, b64 = wf.astype(f64), bias.astype(f64)
    return {"y": (xi.numpy() @ w64.T + b64, xa.numpy() @ np.abs(w64).T + np.abs(b64), 1)}


# ---- the emulation ------------------------------------------------------------------------------------------------------------------
def _f4dot(a, b):
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3]


def group_sum(d):
    """butterfly over the last axis (a power of two of lanes): v += shfl_xor(v, o), o = L / 2 ... 1; every lane ends with the same sum"""
    L = d.shape[-1]
    idx = np.arange(L)
    o = L // 2
    while o:
        d = d + d[..., idx ^ o]
        o >>= 1
    return d[..., 0]


def pixel_dot(a, b, V, quads=None):
    """per-pixel sum over the channels of a b: LPP = C / (4 V) lanes, each f4dot over its V quads, then group_sum<LPP>"""
    P, C = a.shape
    L = C // (4 * V)
    a4, b4 = a.reshape(P, L, V, 4), np.broadcast_to(b, a.shape).reshape(P, L, V, 4)
    d = _f4dot(a4[:, :, 0], b4[:, :, 0])
    for i in range(1, V if quads is None else quads):
        d = d + _f4dot(a4[:, :, i], b4[:, :, i])
    return group_sum(d)


def stream_blocks(npix, Q):
    return min((npix * Q + 255) // 256, 1024)


def strided_partials(a, b, nblk, PPB, U):
    """per-block partial sums (nblk, M) over the pixels of acc = a[p] + acc (b None) or fma(a[p], b[p], acc): thread (block, phase)
    takes pixels block PPB + phase + i nblk PPB, U of them per loop trip; then block_quad_sum over the phases in ascending order"""
    P, M = a.shape
    acc = np.zeros((nblk, PPB, M), f32)
    stride = nblk * PPB
    base = np.arange(nblk)[:, None] * PPB + np.arange(PPB)[None, :]
    while (base < P).any():
        for u in range(U):
            pix = base + u * stride
            ok = (base < P) & (pix < P)
            if ok.any():
                acc[ok] = acc[ok] + a[pix[ok]] if b is None else _fma(a[pix[ok]], b[pix[ok]], acc[ok])
        base = base + U * stride
    s = np.zeros((nblk, M), f32)
    for p in range(PPB):
        s = s + acc[:, p]
    return s


def reduce_partials(parts, scale, buf=None):
    """reduce_partials_kernel: one wave per output over the rows of parts (nparts, M)"""
    n, M = parts.shape
    s = np.zeros((4, 64, M), f32)
    j = np.arange(64)
    while True:
        main = j + 192 < n
        if not main.any():
            break
        for q in range(4):
            s[q][main] = s[q][main] + parts[(j + 64 * q)[main]]
        j = np.where(main, j + 256, j)
    while True:
        tail = j < n
        if not tail.any():
            break
        s[0][tail] = s[0][tail] + parts[j[tail]]
        j = np.where(tail, j + 64, j)
    v = group_sum(((s[0] + s[1]) + (s[2] + s[3])).T) * f32(scale)
    return v if buf is None else buf + v


def _clamped_taps(n):
    """up2_adjoint_strip_kernel: for low-resolution index i the four high-resolution taps 2 i - 1 ... 2 i + 2, clamped, with their weights"""
    idx = np.array([[min(max(2 * i + k - 1, 0), 2 * n - 1) for i in range(n)] for k in range(4)])
    wgt = np.array([[_adj_w(i, 2 * i + k - 1, n) for i in range(n)] for k in range(4)], dtype=f32)
    return idx, wgt


class Emulator:
    """the operators in numpy fp32 in the lane-group kernels' order; `wrong` names one deliberate fault (tests/test_lane_group_bounds_cpu.py)"""

    def __init__(self, storage, wrong=None):
        self.storage, self.wrong = storage, wrong

    def store(self, a):
        """an output that include/ngan.h declares ngan_bf16* in the bf16 storage type"""
        a = np.ascontiguousarray(a, dtype=f32)
        if self.storage != "bf16":
            return a
        return trunc_bf16(a) if self.wrong == "truncating_store" else rbf(a)

    def _store_quads(self, a, V):
        if self.wrong == "quads_swapped_on_store" and V == 2:
            P, C = a.shape
            a = a.reshape(P, C // 8, 2, 4)[:, :, ::-1].reshape(P, C)
        return self.store(a)

    def _inv_c(self, C, LPP):
        return f32(1) / f32(4 * LPP if self.wrong == "inv_c_from_lane_count" else C)

    # -- pixelnorm.hip
    def pn_fwd(self, c, b):
        C = c.shape[1]
        V, _ = lanes(C, self.storage)
        lrelu = lambda v: np.where(v > 0, v, f32(SLOPE) * v).astype(f32)
        if b is not None and self.wrong == "bias_after_lrelu":
            v = lrelu(c) + b[None, :]
        else:
            v = lrelu(c + b[None, :] if b is not None else c)
        ms = pixel_dot(v, v, V) / f32(C)
        r = np.sqrt(ms + f32(EPS)).astype(f32)
        rn = np.sqrt(ms).astype(f32) if self.wrong == "rn_before_eps" else r
        return {"y": self._store_quads(v * (f32(1) / r)[:, None], V), "rn": rn}

    def pn_bwd(self, gy, gy2, gr, y, rn):
        C = y.shape[1]
        V, LPP = lanes(C, self.storage)
        g = gy + gy2 if gy2 is not None and self.wrong != "gy2_dropped" else gy
        inv_c, inv_r = self._inv_c(C, LPP), f32(1) / rn
        s = pixel_dot(g, y, V, 1 if self.wrong == "second_quad_left_out" else None) * inv_c
        kk = gr * inv_c if gr is not None and self.wrong != "gr_dropped" else np.zeros_like(rn)
        return {"gc": self._store_quads(((g - y * s[:, None]) * inv_r[:, None] + kk[:, None] * y) * _m32(y), V)}

    def pn_bwdbwd(self, h, gy, y, rn):
        C = y.shape[1]
        V, LPP = lanes(C, self.storage)
        hp = h * _m32(y)
        inv_c, inv_r = self._inv_c(C, LPP), f32(1) / rn
        s, t, u = pixel_dot(gy, y, V) * inv_c, pixel_dot(hp, y, V) * inv_c, pixel_dot(hp, gy, V) * inv_c
        ir = inv_r[:, None]
        return {"ggy": self._store_quads((hp - y * t[:, None]) * ir, V), "gy_out": self._store_quads(-(s[:, None] * hp + t[:, None] * gy) * ir, V),
                "gr_out": -f32(C) * (u - s * t) * inv_r * inv_r}

    # -- pointwise.hip
    def channel_sum(self, g, entry, buf):
        """entry: 'plain' (ngan_channel_sum), 'acc' (ngan_channel_sum_acc; accumulate = buf is not None)"""
        P, C = g.shape
        Q = C // 4
        parts = strided_partials(g, None, stream_blocks(P, Q), 256 // Q, 1)
        return {"out": reduce_partials(parts, CHANNEL_SUM_SCALE, buf)}

    def from_image_fwd(self, img, wf, bias, shape, pool):
        xi = _pooled_img32(img) if pool else img
        C = wf.shape[0]
        o = np.broadcast_to(bias, xi.shape[:3] + (C,)).astype(f32)
        for k in range(wf.shape[1]):
            o = _fma(np.broadcast_to(wf[:, k], o.shape), np.broadcast_to(xi[..., k:k + 1], o.shape), o)
        return {"y": self.store(o)}

    def from_image_dx(self, g, wf, shape, pool):
        B, H, Wd = shape
        s = np.stack([pixel_dot(g, wf[:, k][None, :], 1) for k in range(wf.shape[1])], 1)
        return {"gx": _pool_adjoint_img(s, B, H, Wd).astype(f32) if pool else s.reshape(B, H, Wd, -1)}

    def from_image_dw(self, img, g, shape, pool, entry, bufs):
        """bufs: (gw start or None, gb start or None): accumulate bit 0 is gw +=, bit 1 is gb +="""
        B, H, Wd = shape
        C = g.shape[1]
        xi = (_pooled_img32(img) if pool else img).reshape(B * H, Wd, -1)
        ncol, Q = xi.shape[2], C // 4
        PPB = 256 // Q
        assert B * H < 2048                                       # one image row per block
        g3 = g.reshape(B * H, Wd, C)
        acc = np.zeros((B * H, PPB, ncol + 1, C), f32)
        for x0 in range(0, Wd, PPB):
            n = min(PPB, Wd - x0)
            gv = g3[:, x0:x0 + n]
            acc[:, :n, ncol] = acc[:, :n, ncol] + gv
            for k in range(ncol):
                acc[:, :n, k] = _fma(gv, np.broadcast_to(xi[:, x0:x0 + n, k:k + 1], gv.shape), acc[:, :n, k])
        s = np.zeros((B * H, ncol + 1, C), f32)
        for p in range(PPB):
            s = s + acc[:, p]
        slab = np.concatenate([s[:, :ncol].transpose(0, 2, 1).reshape(B * H, C * ncol), s[:, ncol]], 1)        # [c Ncol + k], then the bias sums
        start = None
        if bufs[0] is not None or bufs[1] is not None:             # (adding a zero start is exact)
            start = np.concatenate([np.zeros(C * ncol, f32) if bufs[0] is None else bufs[0].reshape(-1), np.zeros(C, f32) if bufs[1] is None else bufs[1]])
        out = reduce_partials(slab, 1.0, start)
        return {"gw": out[:C * ncol].reshape(C, ncol), "gb": out[C * ncol:]}

    def to_image_fwd(self, x, w):
        return {"t": np.stack([np.tanh(pixel_dot(x, w[k][None, :], 1)) for k in range(w.shape[0])], 1).astype(f32)}

    def to_image_bwd(self, gt, t, x, w, rn, entry, buf):
        """entry: 'bwd', 'pnbwd', 'pnbwd_acc' (accumulate = buf is not None)"""
        P, C = x.shape
        ncol = w.shape[0]
        V, Q = lanes(C, self.storage)
        q = _q32(gt, t)
        o = np.zeros((P, C), f32)
        for k in range(ncol):
            o = _fma(np.broadcast_to(w[k][None, :], (P, C)), np.broadcast_to(q[:, k:k + 1], (P, C)), o)
        parts = strided_partials(np.tile(x, (1, ncol)), np.repeat(q, C, axis=1), stream_blocks(P, C // 4), 256 // Q, V)
        gw = reduce_partials(parts, 1.0, None if buf is None else buf.reshape(-1)).reshape(ncol, C)
        if rn is not None:
            sdot = pixel_dot(o, x, V) * (f32(1) / f32(C))
            o = (o - x * sdot[:, None]) * (f32(1) / rn)[:, None] * _m32(x)
        return {"gx": self.store(o), "gw": gw}

    def up2_fwd(self, x):
        def taps(n):
            d = np.arange(2 * n)
            i, odd = d >> 1, (d & 1).astype(bool)
            return (np.where(odd, i, np.maximum(i - 1, 0)), np.where(odd, np.minimum(i + 1, n - 1), i),
                    np.where(odd, f32(0.75), f32(0.25)).astype(f32), np.where(odd, f32(0.25), f32(0.75)).astype(f32))
        _, h, w, _ = x.shape
        y0, y1, wy0, wy1 = taps(h)
        x0, x1, wx0, wx1 = taps(w)
        wx0, wx1, wy0, wy1 = wx0[None, None, :, None], wx1[None, None, :, None], wy0[None, :, None, None], wy1[None, :, None, None]
        r0, r1 = x[:, y0], x[:, y1]
        top = _fma(r0[:, :, x1], np.broadcast_to(wx1, r0[:, :, x1].shape), r0[:, :, x0] * wx0)
        bot = _fma(r1[:, :, x1], np.broadcast_to(wx1, top.shape), r1[:, :, x0] * wx0)
        return {"y": self.store(_fma(bot, np.broadcast_to(wy1, top.shape), top * wy0))}

    def _adjoint32(self, g):
        B, h2, w2, C = g.shape
        h, w = h2 // 2, w2 // 2
        rx, wx = _clamped_taps(w)
        ry, wy = _clamped_taps(h)
        if self.wrong == "adjoint_border_row0":
            wy[1, 0] = 0.75                       # up2_adj_w(0, 0, h): the interior weight (the tap above stays out of range)
        bc = lambda v, shape, axis: np.broadcast_to(v.reshape([-1 if a == axis else 1 for a in range(4)]), shape)
        hr = g[:, :, rx[0]] * wx[0][None, None, :, None]                                   # every high-resolution row, combined horizontally
        for k in range(1, 4):
            hr = _fma(g[:, :, rx[k]], bc(wx[k], hr.shape, 2), hr)
        s = hr[:, ry[0]] * wy[0][None, :, None, None]
        for k in range(1, 4):
            s = _fma(hr[:, ry[k]], bc(wy[k], s.shape, 1), s)
        return s

    def up2_adjoint(self, g):
        return {"gx": self.store(self._adjoint32(g))}

    def up2_adjoint_pnbwd(self, g, y, rn):
        C = y.shape[-1]
        s, yy = self._adjoint32(g).reshape(-1, C), y.reshape(-1, C)
        dot = pixel_dot(s, yy, 1) * (f32(1) / f32(C))
        return {"out": self.store(((s - yy * dot[:, None]) * (f32(1) / rn.reshape(-1))[:, None] * _m32(yy)).reshape(y.shape))}

    def pool2_fwd(self, x):
        return {"y": self.store(_pooled_img32(x))}

    def pool2_adjoint(self, gy):
        return {"gx": self.store((f32(0.25) * gy).repeat(2, axis=1).repeat(2, axis=2))}

    def lerp(self, a, b):
        return {"out": self.store(_fma(np.full(a.shape, ALPHA, f32), b - a, a))}

    def fade_bwd(self, g):
        al = f32(ALPHA)
        ga, gb = (f32(1) - al) * g, al * g
        if self.wrong == "fade_alpha_swapped":
            ga, gb = gb, ga
        return {"ga": self.store(ga), "gb": self.store(gb)}


# ---- the operators of one case: (output name, value, (ref, absref, n_round), the output is bf16 in the bf16 storage type) -------------
# `impl` is an Emulator or the kernel caller of tests/test_gpu_lane_group.py: the same methods on numpy fp32 arrays
def pixelnorm_operators(impl, C, P, storage):
    bf = storage == "bf16"
    d = pn_inputs(C, P, storage)
    for tag, b in (("pn_fwd", None), ("pn_fwd_bias", d["b"])):
        got = impl.pn_fwd(d["c"], b)
        ref = pn_fwd_ref(d["c"], b, got["y"])
        yield f"{tag}/y", got["y"], ref["y"], bf
        yield f"{tag}/rn", got["rn"], ref["rn"], False
    for tag, gy2, gr in (("pn_bwd", None, None), ("pn_bwd_gr", None, d["gr"]), ("pn_bwd2", d["gy2"], None), ("pn_bwd2_gr", d["gy2"], d["gr"])):
        got = impl.pn_bwd(d["gy"], gy2, gr, d["y"], d["rn_pos"])
        yield f"{tag}/gc", got["gc"], pn_bwd_ref(d["gy"], gy2, gr, d["y"], d["rn_pos"])["gc"], bf
    got, ref = impl.pn_bwdbwd(d["h"], d["gy"], d["y"], d["rn_pos"]), pn_bwdbwd_ref(d["h"], d["gy"], d["y"], d["rn_pos"])
    yield "pn_bwdbwd/ggy", got["ggy"], ref["ggy"], bf
    yield "pn_bwdbwd/gy_out", got["gy_out"], ref["gy_out"], bf
    yield "pn_bwdbwd/gr_out", got["gr_out"], ref["gr_out"], False


def edge_operators(impl, C, P, storage):
    bf = storage == "bf16"
    shape = SHAPES[P]
    for ncol in (1, 3):
        e = edge_inputs(C, P, ncol, storage)
        if ncol == 1:
            ref = channel_sum_ref(e["g"])["out"]
            yield "channel_sum/out", impl.channel_sum(e["g"], "plain", None)["out"], ref, False
            yield "channel_sum/out", impl.channel_sum(e["g"], "acc", None)["out"], ref, False
            yield "channel_sum/out", impl.channel_sum(e["g"], "acc", e["buf"])["out"], plus(ref, e["buf"]), False
        yield f"to_image_fwd{ncol}/t", impl.to_image_fwd(e["x"], e["wimg"])["t"], to_image_fwd_ref(e["x"], e["wimg"])["t"], False
        for tag, entry, rn, buf in (("to_image_bwd", "bwd", None, None), ("to_image_bwd_pnbwd", "pnbwd", e["rn_pos"], None),
                                    ("to_image_bwd_pnbwd", "pnbwd_acc", e["rn_pos"], None), ("to_image_bwd_pnbwd", "pnbwd_acc", e["rn_pos"], e["bufw"])):
            got, ref = impl.to_image_bwd(e["gt"], e["t"], e["x"], e["wimg"], rn, entry, buf), to_image_bwd_ref(e["gt"], e["t"], e["x"], e["wimg"], rn)
            yield f"{tag}{ncol}/gx", got["gx"], ref["gx"], bf
            yield f"{tag}{ncol}/gw", got["gw"], ref["gw"] if buf is None else plus(ref["gw"], buf), False
        for pool in (0, 1):
            img = e["img2"] if pool else e["img"]
            yield (f"from_image_fwd{ncol}_pool{pool}/y", impl.from_image_fwd(img, e["wf"], e["bimg"], shape, pool)["y"],
                   from_image_fwd_ref(img, e["wf"], e["bimg"], pool)["y"], bf)
            yield (f"from_image_dx{ncol}_pool{pool}/gx", impl.from_image_dx(e["gimg"], e["wf"], shape, pool)["gx"],
                   from_image_dx_ref(e["gimg"], e["wf"], shape, pool)["gx"], False)
            ref = from_image_dw_ref(img, e["gimg"], pool)
            for entry, code in (("plain", 0), ("acc", 0), ("acc", 1), ("acc", 2), ("acc", 3)):          # every accumulate code: a swap of the bits fails
                bufs = (e["bufwf"] if code & 1 else None, e["bufb"] if code & 2 else None)
                got = impl.from_image_dw(img, e["gimg"], shape, pool, entry, bufs)
                yield f"from_image_dw{ncol}_pool{pool}/gw", got["gw"], ref["gw"] if bufs[0] is None else plus(ref["gw"], bufs[0]), False
                yield f"from_image_dw{ncol}_pool{pool}/gb", got["gb"], ref["gb"] if bufs[1] is None else plus(ref["gb"], bufs[1]), False


def resample_operators(impl, C, P, storage):
    bf = storage == "bf16"
    r = resample_inputs(C, P, storage)
    yield "up2_fwd/y", impl.up2_fwd(r["lo"])["y"], up2_fwd_ref(r["lo"])["y"], bf
    yield "up2_adjoint/gx", impl.up2_adjoint(r["g"])["gx"], up2_adjoint_ref(r["g"])["gx"], bf
    yield "up2_adjoint_pnbwd/out", impl.up2_adjoint_pnbwd(r["g"], r["y"], r["rn_pos"])["out"], up2_adjoint_pnbwd_ref(r["g"], r["y"], r["rn_pos"])["out"], bf
    yield "pool2_fwd/y", impl.pool2_fwd(r["g"])["y"], pool2_ref(r["g"])["y"], bf
    yield "pool2_adjoint/gx", impl.pool2_adjoint(r["lo"])["gx"], pool2_adjoint_ref(r["lo"])["gx"], bf
    yield "lerp/out", impl.lerp(r["a"], r["b"])["out"], lerp_ref(r["a"], r["b"])["out"], bf
    got, ref = impl.fade_bwd(r["a"]), fade_bwd_ref(r["a"])
    yield "fade_bwd/ga", got["ga"], ref["ga"], bf
    yield "fade_bwd/gb", got["gb"], ref["gb"], bf


GROUPS = {"pixelnorm": pixelnorm_operators, "edges": edge_operators, "resampling": resample_operators}
