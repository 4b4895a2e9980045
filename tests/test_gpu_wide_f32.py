"""The exact-fp32 storage type at the compatibility widths -- every channel count outside the tuned 16 / 32 / 64 / 128 -- kernel by
kernel against fp64.  tests/test_gpu_bf16_wide.py pins the same paths for the bf16 instantiations; in fp32 they were reached only
through whole nets.

1. per-pixel operators through the C ABI at C in wide_f32_cases.WIDTHS (4 / 8 / 256: the lane-group kernels' boundary widths, the
   rest: csrc/wide.hip) and pixel counts that cross the 256-thread block seam (96, 256, 257, 1000).  Per element
       |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref,   C_ACC = 8
   with absref the operator's formula on absolute values and n_round derived per operator in tests/wide_f32_cases.py.  The constants
   were settled on the CPU against an fp32 emulation in the kernels' summation order (tests/test_wide_f32_bounds_cpu.py: every
   emulated ratio <= 0.5; one raise, pn_fwd with bias at C = 1024 -> C_ACC 16), never against a kernel.  Every output buffer starts
   as NaN, so an element no thread wrote fails the comparison.
2. convolutions at non-tuned widths through ops.ConvLReLUPN / ops.Conv and run_both (forward, first order, d/dW |dL/dx|^2) in both
   fp32 arithmetic modes at run_both's default tolerances, every chunk list of ops._n_chunks; and chunking is copies only: the
   chunked result is bit-equal to the chunks launched by hand.
3. weight gradients at non-tuned widths in the f32, bf16x3 and bf16 modes against tests/fp64_conv.py.
4. models._conv_any_width (zero padding to multiples of 16) against the UNPADDED fp64 operator.

measured on MI355X (a record, not a bound: worst err / bound per operator over all widths, pixel counts, Ncol and pooling; 1 is the
bound): pn_fwd y 0.49 rn 0.39, with bias y 0.47 rn 0.44; pn_bwd 0.22, with gr 0.21; pn_bwd2 0.25, with gr 0.24; pn_bwdbwd ggy 0.22
gy_out 0.27 gr_out 0.18; channel_sum 0.42; to_image_fwd 0.22; to_image_bwd gx 0.28 gw 0.34; to_image_bwd_pnbwd gx 0.27 gw 0.34;
from_image_dx 0.43; from_image_dw gw 0.43 gb 0.31; up2_adjoint 0.30; up2_adjoint_pnbwd 0.26; pool2_fwd 0.19; pool2_adjoint 0 (exact);
lerp 0.17; fade_bwd 0.08.  The kernels sit where the emulation does (<= 0.5): no kernel needed a fix and no constant moved."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp64_conv
import wide_f32_cases as W
from test_gpu_ops import DEV, SLOPE, grad_close, lrelu_like, nchw, nhwc, pn_ref, resample_ref, run_both

pytestmark = pytest.mark.gpu
EPS = W.EPS


def dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nans(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def host(t):
    return t.detach().cpu().numpy()


class Checker:
    """collects err / bound of every output of one test and asserts at the end, so that one run shows every figure"""

    def __init__(self, C, P):
        self.C, self.P, self.bad = C, P, []

    def __call__(self, name, got, ref):
        r, a, n = ref
        worst = W.ratio(host(got) if isinstance(got, torch.Tensor) else got, r, a, n, W.c_acc(name, self.C))
        print(f"STAT wide_f32 {name} C={self.C} P={self.P}: {worst:.3f}")
        if not worst <= 1.0:
            self.bad.append((name, worst))

    def done(self):
        assert not self.bad, (self.C, self.P, self.bad)


def plus(ref, buf):
    """reference of an accumulating form that starts from `buf`"""
    r, a, n = ref
    return r + buf.astype(np.float64), a + np.abs(buf.astype(np.float64)), n


# ---- 1. per-pixel operators ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", W.PIXELS)
@pytest.mark.parametrize("C", W.WIDTHS)
def test_pixelnorm_operators_f32_against_fp64(ngan, C, P):
    """ngan_lrelu_pixelnorm_fwd (with / without bias, out of place / in place as ops._run_conv's chunked path calls it), _bwd (with /
    without gr, out of place / in place as ops._run_dgrad calls it), _bwd2 (gy + gy2, with / without gr), _bwdbwd"""
    call = ngan._C.call
    d = W.pn_inputs(C, P)
    ck = Checker(C, P)
    for tag, b in (("pn_fwd", None), ("pn_fwd_bias", d["b"])):
        y, rn = nans(P, C), nans(P)
        call("ngan_lrelu_pixelnorm_fwd", dv(d["c"]), dv(b), y, rn, P, C, SLOPE, EPS)
        ref = W.pn_fwd_ref(d["c"], b, host(y))
        ck(f"{tag}/y", y, ref["y"])
        ck(f"{tag}/rn", rn, ref["rn"])
        y2, rn2 = dv(d["c"]), nans(P)
        call("ngan_lrelu_pixelnorm_fwd", y2, dv(b), y2, rn2, P, C, SLOPE, EPS)           # in place
        assert torch.equal(y2, y) and torch.equal(rn2, rn), (tag, "in place differs from out of place")
    y, rn = dv(d["y"]), dv(d["rn_pos"])
    for tag, gy2, gr in (("pn_bwd", None, None), ("pn_bwd_gr", None, d["gr"]), ("pn_bwd2", d["gy2"], None), ("pn_bwd2_gr", d["gy2"], d["gr"])):
        gc = nans(P, C)
        if gy2 is None:
            call("ngan_lrelu_pixelnorm_bwd", dv(d["gy"]), dv(gr), y, rn, gc, P, C, SLOPE)
        else:
            call("ngan_lrelu_pixelnorm_bwd2", dv(d["gy"]), dv(gy2), dv(gr), y, rn, gc, P, C, SLOPE)
        ck(f"{tag}/gc", gc, W.pn_bwd_ref(d["gy"], gy2, gr, d["y"], d["rn_pos"])["gc"])
        if gy2 is None:
            g2 = dv(d["gy"])
            call("ngan_lrelu_pixelnorm_bwd", g2, dv(gr), y, rn, g2, P, C, SLOPE)           # in place
            assert torch.equal(g2, gc), (tag, "in place differs from out of place")
    ggy, gyo, gro = nans(P, C), nans(P, C), nans(P)
    call("ngan_lrelu_pixelnorm_bwdbwd", dv(d["h"]), dv(d["gy"]), y, rn, ggy, gyo, gro, P, C, SLOPE)
    ref = W.pn_bwdbwd_ref(d["h"], d["gy"], d["y"], d["rn_pos"])
    ck("pn_bwdbwd/ggy", ggy, ref["ggy"])
    ck("pn_bwdbwd/gy_out", gyo, ref["gy_out"])
    ck("pn_bwdbwd/gr_out", gro, ref["gr_out"])
    ck.done()


def acc_refused(call, C, *args):
    """the accumulating forms exist in the lane-group kernels only: csrc/wide.hip refuses them (include/ngan.h)"""
    assert W.is_wide(C)
    with pytest.raises(RuntimeError, match="accumulate is not available"):
        call(*args)


@pytest.mark.parametrize("P", W.PIXELS)
@pytest.mark.parametrize("C", W.WIDTHS)
def test_channel_sum_and_image_edges_f32_against_fp64(ngan, C, P):
    """ngan_channel_sum / _acc, ngan_to_image_fwd / _bwd / _bwd_pnbwd / _bwd_pnbwd_acc, ngan_from_image_dx / _dw / _dw_acc (plain and
    pooled), Ncol 1 and 3.  The _acc forms add into a non-zero buffer at the lane-group widths and are refused at csrc/wide.hip's."""
    call = ngan._C.call
    B, H, Wd = W.SHAPES[P]
    ck = Checker(C, P)
    ws = torch.empty(1024 * C * 4, device=DEV)
    for ncol in (1, 3):
        e = W.edge_inputs(C, P, ncol)
        if ncol == 1:
            ref = W.channel_sum_ref(e["g"])["out"]
            out = nans(C)
            call("ngan_channel_sum", dv(e["g"]), out, ws, P, C, W.CHANNEL_SUM_SCALE)
            ck("channel_sum/out", out, ref)
            out = nans(C)
            call("ngan_channel_sum_acc", dv(e["g"]), out, ws, P, C, W.CHANNEL_SUM_SCALE, 0)
            ck("channel_sum/out", out, ref)
            out = dv(e["buf"])
            if W.is_wide(C):
                acc_refused(call, C, "ngan_channel_sum_acc", dv(e["g"]), out, ws, P, C, W.CHANNEL_SUM_SCALE, 1)
            else:
                call("ngan_channel_sum_acc", dv(e["g"]), out, ws, P, C, W.CHANNEL_SUM_SCALE, 1)
                ck("channel_sum/out", out, plus(ref, e["buf"]))
        x, wimg, gt, t_in, rn = dv(e["x"]), dv(e["wimg"]), dv(e["gt"]), dv(e["t"]), dv(e["rn_pos"])
        t = nans(P, ncol)
        call("ngan_to_image_fwd", x, wimg, t, P, C, ncol)
        ck(f"to_image_fwd{ncol}/t", t, W.to_image_fwd_ref(e["x"], e["wimg"])["t"])
        ref = W.to_image_bwd_ref(e["gt"], e["t"], e["x"], e["wimg"], None)
        gx, gw = nans(P, C), nans(ncol, C)
        call("ngan_to_image_bwd", gt, t_in, x, wimg, gx, gw, ws, P, C, ncol)
        ck(f"to_image_bwd{ncol}/gx", gx, ref["gx"])
        ck(f"to_image_bwd{ncol}/gw", gw, ref["gw"])
        ref = W.to_image_bwd_ref(e["gt"], e["t"], e["x"], e["wimg"], e["rn_pos"])
        gx, gw = nans(P, C), nans(ncol, C)
        call("ngan_to_image_bwd_pnbwd", gt, t_in, x, rn, wimg, gx, gw, ws, P, C, ncol, SLOPE)
        ck(f"to_image_bwd_pnbwd{ncol}/gx", gx, ref["gx"])
        ck(f"to_image_bwd_pnbwd{ncol}/gw", gw, ref["gw"])
        gx, gw = nans(P, C), nans(ncol, C)
        call("ngan_to_image_bwd_pnbwd_acc", gt, t_in, x, rn, wimg, gx, gw, ws, P, C, ncol, SLOPE, 0)
        ck(f"to_image_bwd_pnbwd{ncol}/gx", gx, ref["gx"])
        ck(f"to_image_bwd_pnbwd{ncol}/gw", gw, ref["gw"])
        gx, gw = nans(P, C), dv(e["bufw"])
        if W.is_wide(C):
            acc_refused(call, C, "ngan_to_image_bwd_pnbwd_acc", gt, t_in, x, rn, wimg, gx, gw, ws, P, C, ncol, SLOPE, 1)
        else:
            call("ngan_to_image_bwd_pnbwd_acc", gt, t_in, x, rn, wimg, gx, gw, ws, P, C, ncol, SLOPE, 1)
            ck(f"to_image_bwd_pnbwd{ncol}/gx", gx, ref["gx"])
            ck(f"to_image_bwd_pnbwd{ncol}/gw", gw, plus(ref["gw"], e["bufw"]))
        gimg, wf = dv(e["gimg"]), dv(e["wf"])
        for pool in (0, 1):
            gxi = nans(B, 2 * H, 2 * Wd, ncol) if pool else nans(B, H, Wd, ncol)
            call("ngan_from_image_dx", gimg, wf, gxi, B, H, Wd, ncol, C, pool)
            ck(f"from_image_dx{ncol}_pool{pool}/gx", gxi, W.from_image_dx_ref(e["gimg"], e["wf"], (B, H, Wd), pool)["gx"])
            img = e["img2"] if pool else e["img"]
            ref = W.from_image_dw_ref(img, e["gimg"], pool)
            gwf, gbf = nans(C, ncol), nans(C)
            call("ngan_from_image_dw", dv(img), gimg, gwf, gbf, ws, B, H, Wd, ncol, C, pool)
            ck(f"from_image_dw{ncol}_pool{pool}/gw", gwf, ref["gw"])
            ck(f"from_image_dw{ncol}_pool{pool}/gb", gbf, ref["gb"])
            gwf, gbf = nans(C, ncol), nans(C)
            call("ngan_from_image_dw_acc", dv(img), gimg, gwf, gbf, ws, B, H, Wd, ncol, C, pool, 0)
            ck(f"from_image_dw{ncol}_pool{pool}/gw", gwf, ref["gw"])
            ck(f"from_image_dw{ncol}_pool{pool}/gb", gbf, ref["gb"])
            gwf, gbf = dv(e["bufwf"]), dv(e["bufb"])
            if W.is_wide(C):
                acc_refused(call, C, "ngan_from_image_dw_acc", dv(img), gimg, gwf, gbf, ws, B, H, Wd, ncol, C, pool, 3)
            else:
                call("ngan_from_image_dw_acc", dv(img), gimg, gwf, gbf, ws, B, H, Wd, ncol, C, pool, 3)
                ck(f"from_image_dw{ncol}_pool{pool}/gw", gwf, plus(ref["gw"], e["bufwf"]))
                ck(f"from_image_dw{ncol}_pool{pool}/gb", gbf, plus(ref["gb"], e["bufb"]))
    ck.done()


@pytest.mark.parametrize("P", W.PIXELS)
@pytest.mark.parametrize("C", W.WIDTHS)
def test_resampling_and_fade_f32_against_fp64(ngan, C, P):
    """ngan_up2_adjoint, ngan_up2_adjoint_pnbwd (at csrc/wide.hip's widths: two launches, the adjoint, then wide_pn_bwd<float> in
    place), ngan_pool2_fwd / _adjoint, ngan_lerp, ngan_fade_bwd"""
    call = ngan._C.call
    B, h, w = W.SHAPES[P]
    r = W.resample_inputs(C, P)
    ck = Checker(C, P)
    gx = nans(B, h, w, C)
    call("ngan_up2_adjoint", dv(r["g"]), gx, B, h, w, C)
    ck("up2_adjoint/gx", gx, W.up2_adjoint_ref(r["g"])["gx"])
    out = nans(B, h, w, C)
    call("ngan_up2_adjoint_pnbwd", dv(r["g"]), dv(r["y"]), dv(r["rn_pos"]), out, B, h, w, C, SLOPE)
    ck("up2_adjoint_pnbwd/out", out, W.up2_adjoint_pnbwd_ref(r["g"], r["y"], r["rn_pos"])["out"])
    y = nans(B, h, w, C)
    call("ngan_pool2_fwd", dv(r["g"]), y, B, h, w, C)
    ck("pool2_fwd/y", y, W.pool2_ref(r["g"])["y"])
    gx = nans(B, 2 * h, 2 * w, C)
    call("ngan_pool2_adjoint", dv(r["lo"]), gx, B, h, w, C)
    ck("pool2_adjoint/gx", gx, W.pool2_adjoint_ref(r["lo"])["gx"])
    alpha = torch.tensor([W.ALPHA], device=DEV)
    out = nans(B, h, w, C)
    call("ngan_lerp", dv(r["a"]), dv(r["b"]), alpha, out, out.numel())
    ck("lerp/out", out, W.lerp_ref(r["a"], r["b"])["out"])
    ga, gb = nans(B, h, w, C), nans(B, h, w, C)
    call("ngan_fade_bwd", dv(r["a"]), alpha, ga, gb, ga.numel())
    ref = W.fade_bwd_ref(r["a"])
    ck("fade_bwd/ga", ga, ref["ga"])
    ck("fade_bwd/gb", gb, ref["gb"])
    ck.done()


# ---- 2. convolutions at non-tuned widths -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.CONV_WIDE)
def test_wide_conv_lrelu_pn_all_orders(ngan, case, conv_precision):
    """ops.ConvLReLUPN where the output channels (ops._run_conv), the input gradient's channels (ops._run_dgrad) or both run as
    chunks, and the contraction is wider than the tuned kernels': forward, first order, d/dW |dL/dx|^2 against fp64 with the
    kernel's own LeakyReLU pattern (as test_gpu_ops.py::test_conv_lrelu_pn_all_orders), run_both's default tolerances"""
    ops = ngan.ops
    t, res, scale = W.conv_tensors(case)

    def f_hip(d):
        y, _ = ops.ConvLReLUPN.apply(nhwc(d["x"]), d["w"], d.get("b"), res, scale, SLOPE)
        return nchw(y)

    with torch.no_grad():
        pattern = f_hip({k: v.to(DEV) for k, v in t.items()})

    def f_ref(d):
        return pn_ref(lrelu_like(F.conv2d(scale * resample_ref(d["x"], res), d["w"], d.get("b"), padding=1), pattern))

    run_both(f_hip, f_ref, t, [k for k in t if k != "x"], x_name="x")


@pytest.mark.parametrize("case", W.CONV_RAW_WIDE)
def test_wide_conv_raw_all_orders(ngan, case, conv_precision):
    """ops.Conv (no epilogue) on chunked layers, as test_gpu_ops.py::test_conv_raw_all_orders"""
    ops = ngan.ops
    t, res, scale = W.conv_tensors(case)
    run_both(lambda d: torch.tanh(nchw(ops.Conv.apply(nhwc(d["x"]), d["w"], d.get("b"), res, scale))),
             lambda d: torch.tanh(F.conv2d(scale * resample_ref(d["x"], res), d["w"], d.get("b"), padding=1)),
             t, [k for k in t if k != "x"], x_name="x")


@pytest.mark.parametrize("case", W.CHUNK_EQUAL)
def test_chunking_is_copies_only(ngan, case, conv_precision):
    """ops._run_conv / ops._run_dgrad with more than one chunk are bit-equal to each chunk's launch made by hand on the sliced weight
    and concatenated (+ the unfused per-pixel launch); the chunked input gradient with a PNLink is bit-equal to the unlinked one
    followed by ngan_lrelu_pixelnorm_bwd"""
    ops, call = ngan.ops, ngan._C.call
    B, H, Wd, Cin, Cout, res = case
    torch.manual_seed(sum(case))
    hin, win = (2 * H, 2 * Wd) if res == 1 else ((H // 2, Wd // 2) if res == 2 else (H, Wd))
    x = torch.randn(B, hin, win, Cin, device=DEV)
    w = torch.randn(Cout, Cin, 3, 3, device=DEV)
    bias = torch.randn(Cout, device=DEV)
    scale = 1.3868 / np.sqrt(9 * Cin)
    out_chunks, in_chunks = ops._n_chunks(Cout), ops._n_chunks(Cin)
    assert len(out_chunks) > 1 and len(in_chunks) > 1
    assert [n for _, n in out_chunks] == {240: [128, 64, 32, 16], 320: [128, 128, 64], 144: [128, 16]}[Cout]
    y, rn = ops._run_conv(x, w, bias, res, scale, 1, SLOPE)
    parts = [ops._run_conv(x, w[c0:c0 + n].contiguous(), bias[c0:c0 + n].contiguous(), res, scale, 0, 0.0)[0] for c0, n in out_chunks]
    plain = torch.cat(parts, dim=3).contiguous()
    assert torch.equal(ops._run_conv(x, w, bias, res, scale, 0, 0.0)[0], plain)
    y2, rn2 = torch.empty_like(plain), torch.empty_like(rn)
    call("ngan_lrelu_pixelnorm_fwd", plain, None, y2, rn2, B * H * Wd, Cout, SLOPE, EPS)
    assert torch.equal(y, y2) and torch.equal(rn, rn2)
    # input gradient: chunks over Cin
    g = torch.randn(B, H, Wd, Cout, device=DEV)
    gx = ops._run_dgrad(g, w, res, scale)
    assert tuple(gx.shape) == tuple(x.shape)
    parts = [ops._run_dgrad(g, w[:, c0:c0 + n].contiguous(), 1 if res == 1 else 0, scale) for c0, n in in_chunks]
    full = torch.cat(parts, dim=3).contiguous()
    if res == 2:
        by_hand = torch.empty_like(gx)
        call("ngan_up2_adjoint", full, by_hand, B, H // 2, Wd // 2, Cin)
    else:
        by_hand = full
    assert torch.equal(gx, by_hand)
    link = ops.PNLink()
    link.y, link.rn, link.slope = torch.randn_like(x), torch.rand(B, hin, win, device=DEV) + 0.5, SLOPE
    linked = ops._run_dgrad(g, w, res, scale, link=link)
    unfused = torch.empty_like(gx)
    call("ngan_lrelu_pixelnorm_bwd", gx, None, link.y, link.rn, unfused, B * hin * win, Cin, SLOPE)
    assert torch.equal(linked, unfused)


# ---- 3. weight gradients at non-tuned widths ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("case", W.WGRAD_WIDE)
def test_wide_weight_gradient_against_fp64(ngan, case, mode):
    """ngan_conv3x3_wgrad (precision 0 and 1) and ngan_bf16_conv3x3_wgrad through ops._run_wgrad, written and accumulated into a
    non-zero gradient, against fp64_conv.conv3x3_wgrad.  f32 / bf16x3: grad_close at 2e-4 (test_gpu_ops.py's first-order bound);
    bf16: 1e-4 relative L2 on bf16-rounded operands (test_gpu_bf16.py::test_bf16_weight_gradient_against_fp64)"""
    ops = ngan.ops
    B, H, Wd, Cin, Cout, res = case
    torch.manual_seed(sum(case) + 3)
    hin, win = (2 * H, 2 * Wd) if res == 1 else ((H // 2, Wd // 2) if res == 2 else (H, Wd))
    x, g = torch.randn(B, hin, win, Cin), torch.randn(B, H, Wd, Cout)
    scale = 0.37
    ops.set_conv_precision(mode)
    try:
        if mode == "bf16":
            x, g = x.to(torch.bfloat16), g.to(torch.bfloat16)
        xr = fp64_conv.resample(x.double(), res)
        if mode == "bf16":      # the staging rounds the blended value once (test_gpu_bf16.py: resample_ref)
            xr = xr.float().to(torch.bfloat16).double()
        ref = fp64_conv.conv3x3_wgrad(xr, g.double(), scale, 0)
        got = ops._run_wgrad(x.to(DEV), g.to(DEV), res, scale)
        start = torch.randn(Cout, Cin, 3, 3)
        acc = start.to(DEV)
        ops._run_wgrad(x.to(DEV), g.to(DEV), res, scale, accumulate_into=acc)
    finally:
        ops.set_conv_precision("f32")
    assert got.dtype == torch.float32 and acc.dtype == torch.float32
    for what, a, b in (("written", got, ref), ("accumulated", acc, ref + start.double())):
        if mode == "bf16":
            err = float((a.double().cpu() - b).norm() / b.norm())
            assert err < 1e-4, (what, err)
        else:
            ok, info = grad_close(a, b, 2e-4)
            assert ok, (what, info)


# ---- 4. the zero-padding path -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.PAD_CASES)
def test_conv_any_width_against_the_unpadded_operator(ngan, case, conv_precision):
    """models._conv_any_width for widths that are not multiples of 16: the fp64 reference is the UNPADDED operator, so PixelNorm's
    mean is over the layer's real channel count"""
    B, H, Wd, Cin, Cout, res, act = case
    t, res, scale = W.conv_tensors((B, H, Wd, Cin, Cout, res, True))

    def f_hip(d):
        m = types.SimpleNamespace(weight=d["w"], bias=d["b"], scale_value=scale)
        return (nchw(ngan.models._conv_any_width(nhwc(d["x"]), m, res, SLOPE)) if act
                else torch.tanh(nchw(ngan.models._conv_any_width(nhwc(d["x"]), m, res, None))))

    pattern = None
    if act:
        with torch.no_grad():
            pattern = f_hip({k: v.to(DEV) for k, v in t.items()})
        assert tuple(pattern.shape[:2]) == (B, Cout)

    def f_ref(d):
        c = F.conv2d(scale * resample_ref(d["x"], res), d["w"], d["b"], padding=1)
        return pn_ref(lrelu_like(c, pattern)) if act else torch.tanh(c)

    run_both(f_hip, f_ref, t, ["w", "b"], x_name="x")


def test_conv_any_width_refuses_widths_that_are_not_multiples_of_4(ngan):
    m = types.SimpleNamespace(weight=torch.randn(6, 8, 3, 3, device=DEV), bias=None, scale_value=0.1)
    with pytest.raises(NotImplementedError, match="multiples of 4"):
        ngan.models._conv_any_width(torch.randn(1, 4, 4, 8, device=DEV), m, 0, SLOPE)
