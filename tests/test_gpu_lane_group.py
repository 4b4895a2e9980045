"""The lane-group per-pixel kernels (csrc/pixelnorm.hip, csrc/pointwise.hip) per element against fp64, in both activation storage
types, at every width they take: C in {4, 8, 16, 32, 64, 128, 256} -- the widths of every default configuration and of the benchmark
-- on 1, 3, 96, 256, 257 and 1000 pixels.  tests/test_gpu_wide_f32.py reaches these kernels only at C = 4, 8 and 256 in fp32, and the
bf16 instances (two quads per lane through one 16-byte access wherever C % 8 == 0, so half the lanes per pixel) were compared only
with their fp32 twins at C = 32.

Through the C ABI (`_C.call`, which raises on a non-zero return code), per element
    an fp32 output, either storage type   |got - ref| <= e32 = n_round 2^-23 |ref| + 8 2^-24 absref
    a bf16 output                         |got - ref| <= 2^-8 |ref| + (1 + 2^-8) e32
with the references, absref, n_round and inputs of tests/lane_group_cases.py; in the bf16 storage type the reference is fp64 on the
bf16-rounded operands.  The bf16 bound is one nearest-even rounding of a value within e32 of the reference: half the 2^-7 used so far,
which a truncating store misses.  Both bounds were settled on the CPU (tests/test_lane_group_bounds_cpu.py: emulated fp32 ratios
<= 0.30, bf16 <= 1, no raised constant; ten kinds of wrong emulation miss them), never against a kernel.

Every output buffer lies between two guard regions and starts as NaN: after the call the guards are bit-unchanged and no NaN is
left inside, so an element no thread wrote, or one written outside the tensor, fails.  The accumulating entry points are run with
accumulate = 0 into NaN and with every accumulate code (1, 2 and 3 of ngan_from_image_dw_acc) into known non-zero buffers, against ref + buffer.  The (float, C, P) with C in
{4, 8, 256} and P in {96, 256, 257, 1000} are left to tests/test_gpu_wide_f32.py, which runs them on the same bound; everything else of
LANE_WIDTHS x LANE_PIXELS x {float, bf16} is run here.

measured on MI355X (a record, not a bound: worst err / bound per operator output over all widths and pixel counts; 1 is the bound):
see DESIGN.md, "The lane-group kernels per element"."""
import math

import numpy as np
import pytest
import torch

import lane_group_cases as L
import wide_f32_cases as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
GUARD = 64              # elements on either side of an output: 128 / 256 bytes, so the tensor stays 16-byte aligned
CASES = [(s, C, P) for s in L.STORAGES for C in L.LANE_WIDTHS for P in L.LANE_PIXELS
         if not (s == "float" and C in (4, 8, 256) and P in W.PIXELS)]


def dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


class Kernels:
    """the methods of lane_group_cases.Emulator on the entry points of include/ngan.h: numpy fp32 in, numpy fp32 out"""

    def __init__(self, call, storage, C):
        self.call, self.bf = call, storage == "bf16"
        self.prefix = "ngan_bf16_" if self.bf else "ngan_"
        self.ws = torch.empty(1024 * C * 4, device=DEV)
        self.alpha = torch.tensor([L.ALPHA], device=DEV)
        self.pending = []

    def act(self, a):
        """an activation operand: bf16-representable by construction, so the conversion is exact"""
        t = dv(a)
        if self.bf and t is not None:
            assert torch.equal(t.to(BF).float(), t)
            t = t.to(BF)
        return t

    def out(self, shape, act, start=None):
        n = math.prod(shape)
        flat = torch.full((n + 2 * GUARD,), float("nan"), dtype=BF if act and self.bf else torch.float32, device=DEV)
        view = flat[GUARD:GUARD + n].view(*shape)
        if start is not None:
            view.copy_(dv(start))
        assert view.data_ptr() % 16 == 0
        self.pending.append((flat, n))
        return view

    def run(self, op, *args):
        self.call(self.prefix + op, *args)
        for flat, n in self.pending:
            bits = flat.view(torch.int16 if flat.dtype == BF else torch.int32)
            nan = torch.full((1,), float("nan"), dtype=flat.dtype, device=DEV).view(bits.dtype)
            assert bool((bits[:GUARD] == nan).all()) and bool((bits[GUARD + n:] == nan).all()), (op, "a guard region was written")
            assert not bool(torch.isnan(flat[GUARD:GUARD + n]).any()), (op, "an element was left unwritten")
        self.pending = []

    @staticmethod
    def host(**views):
        return {k: v.float().cpu().numpy() for k, v in views.items()}

    def pn_fwd(self, c, b):
        P, C = c.shape
        y, rn = self.out((P, C), True), self.out((P,), False)
        self.run("lrelu_pixelnorm_fwd", self.act(c), dv(b), y, rn, P, C, L.SLOPE, L.EPS)
        return self.host(y=y, rn=rn)

    def pn_bwd(self, gy, gy2, gr, y, rn):
        P, C = y.shape
        gc = self.out((P, C), True)
        if gy2 is None:
            self.run("lrelu_pixelnorm_bwd", self.act(gy), dv(gr), self.act(y), dv(rn), gc, P, C, L.SLOPE)
        else:
            self.run("lrelu_pixelnorm_bwd2", self.act(gy), self.act(gy2), dv(gr), self.act(y), dv(rn), gc, P, C, L.SLOPE)
        return self.host(gc=gc)

    def pn_bwdbwd(self, h, gy, y, rn):
        P, C = y.shape
        ggy, gy_out, gr_out = self.out((P, C), True), self.out((P, C), True), self.out((P,), False)
        self.run("lrelu_pixelnorm_bwdbwd", self.act(h), self.act(gy), self.act(y), dv(rn), ggy, gy_out, gr_out, P, C, L.SLOPE)
        return self.host(ggy=ggy, gy_out=gy_out, gr_out=gr_out)

    def channel_sum(self, g, entry, buf):
        P, C = g.shape
        out = self.out((C,), False, buf)
        if entry == "plain":
            self.run("channel_sum", self.act(g), out, self.ws, P, C, L.CHANNEL_SUM_SCALE)
        else:
            self.run("channel_sum_acc", self.act(g), out, self.ws, P, C, L.CHANNEL_SUM_SCALE, 0 if buf is None else 1)
        return self.host(out=out)

    def from_image_fwd(self, img, wf, bias, shape, pool):
        B, H, Wd = shape
        C, ncol = wf.shape
        y = self.out((B, H, Wd, C), True)
        self.run("from_image_fwd", dv(img), dv(wf), dv(bias), y, B, H, Wd, ncol, C, pool)
        return self.host(y=y)

    def from_image_dx(self, g, wf, shape, pool):
        B, H, Wd = shape
        C, ncol = wf.shape
        gx = self.out((B, 2 * H, 2 * Wd, ncol) if pool else (B, H, Wd, ncol), False)
        self.run("from_image_dx", self.act(g), dv(wf), gx, B, H, Wd, ncol, C, pool)
        return self.host(gx=gx)

    def from_image_dw(self, img, g, shape, pool, entry, bufs):
        B, H, Wd = shape
        C, ncol = g.shape[1], img.shape[3]
        gw, gb = self.out((C, ncol), False, bufs[0]), self.out((C,), False, bufs[1])
        code = (bufs[0] is not None) + 2 * (bufs[1] is not None)
        if entry == "plain":
            assert code == 0
            self.run("from_image_dw", dv(img), self.act(g), gw, gb, self.ws, B, H, Wd, ncol, C, pool)
        else:
            self.run("from_image_dw_acc", dv(img), self.act(g), gw, gb, self.ws, B, H, Wd, ncol, C, pool, code)
        return self.host(gw=gw, gb=gb)

    def to_image_fwd(self, x, w):
        P, C = x.shape
        t = self.out((P, w.shape[0]), False)
        self.run("to_image_fwd", self.act(x), dv(w), t, P, C, w.shape[0])
        return self.host(t=t)

    def to_image_bwd(self, gt, t, x, w, rn, entry, buf):
        P, C = x.shape
        ncol = w.shape[0]
        gx, gw = self.out((P, C), True), self.out((ncol, C), False, buf)
        if entry == "bwd":
            self.run("to_image_bwd", dv(gt), dv(t), self.act(x), dv(w), gx, gw, self.ws, P, C, ncol)
        elif entry == "pnbwd":
            self.run("to_image_bwd_pnbwd", dv(gt), dv(t), self.act(x), dv(rn), dv(w), gx, gw, self.ws, P, C, ncol, L.SLOPE)
        else:
            self.run("to_image_bwd_pnbwd_acc", dv(gt), dv(t), self.act(x), dv(rn), dv(w), gx, gw, self.ws, P, C, ncol, L.SLOPE, 0 if buf is None else 1)
        return self.host(gx=gx, gw=gw)

    def _resample(self, op, x, up, key):
        B, h, w, C = x.shape
        lo = (h, w) if up else (h // 2, w // 2)                    # the entry points take the low-resolution grid
        o = self.out((B, 2 * h, 2 * w, C) if up else (B, h // 2, w // 2, C), True)
        self.run(op, self.act(x), o, B, lo[0], lo[1], C)
        return self.host(**{key: o})

    def up2_fwd(self, x):
        return self._resample("up2_fwd", x, True, "y")

    def up2_adjoint(self, g):
        return self._resample("up2_adjoint", g, False, "gx")

    def pool2_fwd(self, x):
        return self._resample("pool2_fwd", x, False, "y")

    def pool2_adjoint(self, gy):
        return self._resample("pool2_adjoint", gy, True, "gx")

    def up2_adjoint_pnbwd(self, g, y, rn):
        B, h, w, C = y.shape
        o = self.out((B, h, w, C), True)
        self.run("up2_adjoint_pnbwd", self.act(g), self.act(y), dv(rn), o, B, h, w, C, L.SLOPE)
        return self.host(out=o)

    def lerp(self, a, b):
        o = self.out(a.shape, True)
        self.run("lerp", self.act(a), self.act(b), self.alpha, o, o.numel())
        return self.host(out=o)

    def fade_bwd(self, g):
        ga, gb = self.out(g.shape, True), self.out(g.shape, True)
        self.run("fade_bwd", self.act(g), self.alpha, ga, gb, ga.numel())
        return self.host(ga=ga, gb=gb)


def run_group(ngan, group, storage, C, P):
    """every output of the group's operators against its bound; all figures are printed before anything is asserted"""
    worst = {}
    for name, got, ref, bf in L.GROUPS[group](Kernels(ngan._C.call, storage, C), C, P, storage):
        v = L.worst(name, C, got, ref, bf)
        prev = worst.get(name)
        worst[name] = v if prev is None or not prev >= v else prev                    # (a NaN ratio stays)
    for name, v in worst.items():
        print(f"STAT lane_group {storage} {name} C={C} P={P}: {v:.3f}")
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert worst and not bad, (storage, C, P, bad)


@pytest.mark.parametrize("storage,C,P", CASES)
def test_pixelnorm_operators_against_fp64(ngan, storage, C, P):
    """ngan_[bf16_]lrelu_pixelnorm_fwd (with / without bias; pixel 0 has a mean square next to eps), _bwd (with / without gr), _bwd2
    (with / without gr), _bwdbwd"""
    run_group(ngan, "pixelnorm", storage, C, P)


@pytest.mark.parametrize("storage,C,P", CASES)
def test_channel_sum_and_image_edges_against_fp64(ngan, storage, C, P):
    """ngan_[bf16_]channel_sum / _acc, to_image_fwd / _bwd / _bwd_pnbwd / _bwd_pnbwd_acc, from_image_fwd / _dx / _dw / _dw_acc (plain and
    pooled), Ncol 1 and 3; the _acc forms with accumulate = 0 and with every bit set into a non-zero buffer"""
    run_group(ngan, "edges", storage, C, P)


@pytest.mark.parametrize("storage,C,P", CASES)
def test_resampling_and_fade_against_fp64(ngan, storage, C, P):
    """ngan_[bf16_]up2_fwd, up2_adjoint, up2_adjoint_pnbwd, pool2_fwd, pool2_adjoint, lerp, fade_bwd; the low-resolution grid takes
    lane_group_cases.SHAPES (1 x 1, 1 x 3, 6 x 8, 16 x 16, 257 x 1, 20 x 25)"""
    run_group(ngan, "resampling", storage, C, P)
