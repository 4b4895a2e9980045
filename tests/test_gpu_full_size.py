"""The 512^2-stage layers at their full training sizes, every pass element by element against an fp64 reference evaluated on the GPU
(tests/fp64_conv.py: shifted slices and fp64 matrix products, checked against torch's own fp64 operators by test_fp64_conv_cpu.py).
The error statistics are reduced on the device; nothing large is copied to the host.

Covered: the 3x3 layers of test_gpu_ops.FULL_SIZE_LAYERS in the f32 and bf16x3 modes and in the bf16 storage mode -- forward plain and
with the LeakyReLU -> PixelNorm epilogue (and its pooled side output where the kernel offers one), input gradient plain and with the
producer's PixelNorm backward (epilogue 2), weight gradient stored, accumulated and through the deferred slab reduction with three
contributions -- and the WGAN stride-2 layers and BatchNorm at the full WGAN configuration (batch 8, 512^2).

Bounds, stated before any full-size run (relative L2 = |got - ref| / |ref|, max = max|got - ref| / max|ref|):
  exact fp32 ("f32")        forward, input gradient: relative L2 <= 1e-6, max <= 2e-5 (test_winograd_kernels_against_fp64's bounds, which
                            the same kernel families meet at <= 256^2); weight gradient: relative L2 <= 1e-5, max <= 1e-4 (fp32
                            accumulation over up to 8.4 M pixels in fixed-order slabs: an estimate, not a measurement)
  split-bf16 ("bf16x3")     every pass: max <= 2e-4 (the kernel-level bound of the split-bf16 kernels)
  bf16 storage ("bf16")     test_gpu_bf16.py's criteria on the bf16-rounded operands (inputs as stored, weights as the packing kernel
                            rounds them, a resampled input rounded once): a bf16 output is the bf16 neighbour of the fp64 value
                            (<= 2^-7 relative + 2e-5 of the maximum, 3e-5 for the input gradient, 1e-4 behind the PixelNorm backward),
                            the fp32 norm to 2e-5, a weight gradient to 1e-4 relative L2
  stride 2 / BatchNorm      max <= TOL = 5e-5 (test_gpu_wgan.py); BatchNorm statistics and the folded transform 1e-5, running mean
                            1e-6, running variance 1e-5, BatchNorm backward 1e-4 (test_gpu_wgan.py's bounds)
LeakyReLU's kink: the references apply LeakyReLU themselves, so every pre-activation is kept away from zero -- a +-12 bias per output
channel in front of the PixelNorm epilogue (as test_winograd_kernels_against_fp64), a +-2 BatchNorm shift with a small scale in front of
the BatchNorm backward -- and the tests assert that it is.
"""
import numpy as np
import pytest
import torch

import fp64_conv as R
from test_gpu_ops import FULL_SIZE_LAYERS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOPE = 0.2
BF = torch.bfloat16
BOUNDS = {  # mode -> pass kind -> (relative L2, max of max|ref|); None: not bounded
    "f32": {"act": (1e-6, 2e-5), "wgrad": (1e-5, 1e-4)},
    "bf16x3": {"act": (None, 2e-4), "wgrad": (None, 2e-4)},
}
BF16_WGRAD_L2 = 1e-4
S2_TOL = 5e-5


def layer_id(layer):
    B, H, W, K, N, res = layer
    return f"{B}x{H}x{W}_{K}to{N}_r{res}"


def in_hw(H, W, res):
    return (2 * H, 2 * W) if res == 1 else ((H // 2, W // 2) if res == 2 else (H, W))


def rbf(t):
    return t.to(BF).double()


def errors(got, ref):
    """(relative L2, max of max|ref|), reduced on the device"""
    d = got.double() - ref
    return float(d.norm() / ref.norm()), float(d.abs().max() / ref.abs().max())


def check(tag, got, ref, bound):
    assert tuple(got.shape) == tuple(ref.shape), (tag, tuple(got.shape), tuple(ref.shape))
    assert not bool(torch.isnan(got).any()), (tag, "NaN: an element was never written")
    l2, mx = errors(got, ref)
    print(f"STAT {tag}: rel_l2 {l2:.3e} max {mx:.3e} (bound {bound})")
    assert (bound[0] is None or l2 <= bound[0]) and mx <= bound[1], (tag, l2, mx, bound)


def check_bf16(tag, got, want, extra):
    """got (bf16) is the bf16 neighbour of want (fp64): |got - want| <= 2^-7 |want| + (extra + 1e-6) max|want| (test_gpu_bf16.bf16_close)"""
    assert got.dtype == BF and tuple(got.shape) == tuple(want.shape), (tag, got.dtype, tuple(got.shape))
    err = (got.double() - want).abs()
    amax = want.abs().max()
    nbad = int((err > 2.0 ** -7 * want.abs() + (extra + 1e-6) * amax).sum())
    print(f"STAT {tag}: max {float(err.max() / amax):.3e} beyond the bf16 neighbour: {nbad} (extra {extra})")
    assert nbad == 0, (tag, nbad)


def _gen(layer, salt):
    return torch.Generator(device=DEV).manual_seed(sum(layer) * 7 + salt)


def _randn(gen, *shape):
    return torch.randn(*shape, device=DEV, generator=gen)


def _signed_bias(gen, n, amp, noise=0.5):
    """+-amp per channel (half the channels negative: both LeakyReLU slopes), plus a little noise"""
    sign = torch.tensor([1.0 if (c // 2) % 2 == 0 else -1.0 for c in range(n)], device=DEV)
    return amp * sign + noise * _randn(gen, n)


def _in_operand(x, res, mode):
    """what the fp64 reference convolves: the input itself, or (bf16 mode) its resampled copy rounded once as the staging does"""
    if mode != "bf16":
        return x.double(), res
    return (rbf(R.resample(x.double(), res).float()) if res else x.double()), 0


def _weights(w, scale, mode):
    return (rbf((w * scale).float()), 1.0) if mode == "bf16" else (w.double(), scale)


def _forward(ngan, layer, mode):
    ops, C = ngan.ops, ngan._C
    B, H, W, K, N, res = layer
    gen = _gen(layer, 1)
    hin, win = in_hw(H, W, res)
    x = _randn(gen, B, hin, win, K)
    if mode == "bf16":
        x = x.to(BF)
    w = _randn(gen, N, K, 3, 3)
    bias = _randn(gen, N)
    scale = 1.3868 / np.sqrt(9 * K)
    xin, rin = _in_operand(x, res, mode)
    wq, sq = _weights(w, scale, mode)
    tag = f"{mode} {layer_id(layer)}"
    # plain
    y, _ = ops._run_conv(x, w, bias, res, scale, 0, 0.0)
    ref = R.conv3x3(xin, wq, sq, rin, bias.double())
    if mode == "bf16":
        check_bf16(f"{tag} fwd", y, ref, 2e-5)
    else:
        check(f"{tag} fwd", y, ref, BOUNDS[mode]["act"])
    del y, ref
    # LeakyReLU -> PixelNorm epilogue, the pooled side output where the kernel writes one
    b12 = _signed_bias(gen, N, 12.0)
    y1, rn = ops._run_conv(x, w, b12, res, scale, 1, SLOPE, pool_out=True)
    c = R.conv3x3(xin, wq, sq, rin, b12.double())
    assert float(c.abs().min()) > 1.0                       # every pre-activation is far from the kink
    yr, rr = R.lrelu_pixelnorm(c, SLOPE)
    del c
    if mode == "bf16":
        check_bf16(f"{tag} fwd_lrelu_pn", y1, yr, 2e-5)
        check(f"{tag} fwd_rnorm", rn, rr, (None, 2e-5))
        return
    check(f"{tag} fwd_lrelu_pn", y1, yr, BOUNDS[mode]["act"])
    check(f"{tag} fwd_rnorm", rn, rr, BOUNDS[mode]["act"])
    r_eff = 0 if (res == 1 and mode == "f32") else res     # ops._pool_first: exact fp32 pools a pooled input first
    prec = C.conv3x3_algorithm(B, H, W, K, N, r_eff, ops.PRECISIONS[mode])
    side = ops._pooled_side(y1)
    assert (side is not None) == C.conv3x3_pooled_output(B, H, W, K, N, r_eff, prec)
    if side is not None:
        assert torch.equal(side, ops._pooled(y1)), "the pooled side output is not bit-identical to ngan_pool2_fwd of the output"
        check(f"{tag} fwd_pooled_side", side, R.pool2(yr), BOUNDS[mode]["act"])


def _dgrad(ngan, layer, mode):
    ops = ngan.ops
    B, H, W, K, N, res = layer
    gen = _gen(layer, 2)
    hin, win = in_hw(H, W, res)
    g = _randn(gen, B, H, W, N)
    w = _randn(gen, N, K, 3, 3)
    ay = _randn(gen, B, hin, win, K)                       # stands for the producer's output (y, rnorm)
    arn = torch.rand(B, hin, win, device=DEV, generator=gen) + 0.5
    if mode == "bf16":
        g, ay = g.to(BF), ay.to(BF)
    scale = 1.3868 / np.sqrt(9 * K)
    wq, sq = _weights(w, scale, mode)
    tag = f"{mode} {layer_id(layer)}"
    gx = ops._run_dgrad(g, w, res, scale)
    if mode == "bf16":
        full = R.conv3x3_dgrad(g.double(), wq, sq, 0)
        if res == 2:
            # two launches with a bf16 intermediate: the conv at the output's resolution, stored, then the bilinear adjoint.  The
            # intermediate is rounded from an fp32 sum in the kernel and from the fp64 value here; where the two straddle a bf16
            # rounding midpoint they take different neighbours, and one ulp of the intermediate (2^-8 of it) reaches the adjoint's output
            # with weight up to 9/16 -- more than the criterion allows for an output element much smaller than its neighbourhood (at
            # 32 x 512^2: a few hundred of 33 M elements).  So each stage is pinned on its own: the intermediate (the same launch
            # _run_dgrad makes) against the fp64 conv, and the result against the fp64 adjoint of that intermediate.
            gfull = torch.empty((B, H, W, K), device=DEV, dtype=BF)
            ngan._C.call("ngan_bf16_conv3x3_fwd", g, ops._packed(w, 1, scale, 5), None, gfull, None, None, None, None, B, H, W, N, K,
                         0, ops.EPI_NONE, 0, 0.0, 0.0)
            check_bf16(f"{tag} dgrad_intermediate", gfull, full, 3e-5)
            full = gfull.double()
        ref = R.resample_adjoint(full, res)
        del full
        check_bf16(f"{tag} dgrad", gx, ref, 3e-5)
    else:
        ref = R.conv3x3_dgrad(g.double(), wq, sq, res)
        check(f"{tag} dgrad", gx, ref, BOUNDS[mode]["act"])
    del gx
    link = ops.PNLink()
    link.y, link.rn, link.slope = ay, arn, SLOPE
    gl = ops._run_dgrad(g, w, res, scale, link=link)       # what ConvLReLUPN.backward runs with an input link (_conv_backward_tail)
    want = R.pixelnorm_bwd(ref, ay.double(), arn.double(), SLOPE)
    del ref
    if mode == "bf16":
        check_bf16(f"{tag} dgrad_pn_bwd", gl, want, 1e-4)
    else:
        check(f"{tag} dgrad_pn_bwd", gl, want, BOUNDS[mode]["act"])


def _wgrad(ngan, layer, mode):
    ops = ngan.ops
    B, H, W, K, N, res = layer
    gen = _gen(layer, 3)
    hin, win = in_hw(H, W, res)
    scale = 1.3868 / np.sqrt(9 * K)
    tag = f"{mode} {layer_id(layer)}"

    def operands():
        x, g = _randn(gen, B, hin, win, K), _randn(gen, B, H, W, N)
        return (x.to(BF), g.to(BF)) if mode == "bf16" else (x, g)

    def reference(x, g, s):
        xin, rin = _in_operand(x, res, mode)
        return R.conv3x3_wgrad(xin, g.double(), s, rin)

    def judge(name, got, ref):
        if mode == "bf16":
            l2, mx = errors(got, ref)
            print(f"STAT {tag} {name}: rel_l2 {l2:.3e} max {mx:.3e} (bound {BF16_WGRAD_L2} relative L2)")
            assert got.dtype == torch.float32 and l2 <= BF16_WGRAD_L2, (name, l2)
        else:
            check(f"{tag} {name}", got, ref, BOUNDS[mode]["wgrad"])

    x, g = operands()
    ref = reference(x, g, scale)
    judge("wgrad", ops._run_wgrad(x, g, res, scale), ref)
    acc0 = 0.5 * float(ref.std()) * _randn(gen, N, K, 3, 3)   # an existing gradient of the same scale
    acc = acc0.clone()
    out = ops._run_wgrad(x, g, res, scale, accumulate_into=acc)
    assert out.data_ptr() == acc.data_ptr()
    judge("wgrad_accumulate", acc, acc0.double() + ref)
    # deferred slab reduction: three contributions to one gradient, arriving as roles 1, 0, 0 (flush_wgrad sums them as 0, 0, 1)
    (x2, g2), (x3, g3) = operands(), operands()
    contributions = [(x, g, scale, 1), (x2, g2, 0.5 * scale, 0), (x3, g3, 2.0 * scale, 0)]
    acc = acc0.clone()
    with ops.deferred_wgrad():
        for xi, gi, si, role in contributions:
            ops._run_wgrad(xi, gi, res, si, accumulate_into=acc, role=role)
    want = acc0.double() + ref + reference(x2, g2, 0.5 * scale) + reference(x3, g3, 2.0 * scale)
    judge("wgrad_deferred", acc, want)


class _bf16_mode:
    def __init__(self, ops):
        self.ops = ops

    def __enter__(self):
        self.ops.set_conv_precision("bf16")

    def __exit__(self, *exc):
        self.ops.set_conv_precision("f32")
        return False


LAYER_IDS = [layer_id(layer) for layer in FULL_SIZE_LAYERS]


@pytest.mark.parametrize("layer", FULL_SIZE_LAYERS, ids=LAYER_IDS)
def test_full_size_forward_against_fp64(ngan, layer, conv_precision):
    _forward(ngan, layer, conv_precision)


@pytest.mark.parametrize("layer", FULL_SIZE_LAYERS, ids=LAYER_IDS)
def test_full_size_input_gradient_against_fp64(ngan, layer, conv_precision):
    _dgrad(ngan, layer, conv_precision)


@pytest.mark.parametrize("layer", FULL_SIZE_LAYERS, ids=LAYER_IDS)
def test_full_size_weight_gradient_against_fp64(ngan, layer, conv_precision):
    _wgrad(ngan, layer, conv_precision)


@pytest.mark.parametrize("layer", FULL_SIZE_LAYERS, ids=LAYER_IDS)
def test_full_size_bf16_forward_against_fp64(ngan, layer):
    with _bf16_mode(ngan.ops):
        _forward(ngan, layer, "bf16")


@pytest.mark.parametrize("layer", FULL_SIZE_LAYERS, ids=LAYER_IDS)
def test_full_size_bf16_input_gradient_against_fp64(ngan, layer):
    with _bf16_mode(ngan.ops):
        _dgrad(ngan, layer, "bf16")


@pytest.mark.parametrize("layer", FULL_SIZE_LAYERS, ids=LAYER_IDS)
def test_full_size_bf16_weight_gradient_against_fp64(ngan, layer):
    with _bf16_mode(ngan.ops):
        _wgrad(ngan, layer, "bf16")


# ---- WGAN stride-2 layers at the full configuration (tools/make_golden_wgan.py FULL: batch 8, 512^2, dw [16, 16, 32, 32, 64, 128],
# gw [128, 64, 32, 32, 16, 16]) ----------------------------------------------------------------------------------------------------
S2_LAYERS = [  # name, B, H, W of the input, C in, M out, up (ConvTranspose2d), BatchNorm -> LeakyReLU on load, Tanh
    ("D_conv_1to16_512", 8, 512, 512, 1, 16, False, False, False),        # C % 4 != 0: the scalar path at its largest pixel count
    ("D_conv_16to16_256_bn", 8, 256, 256, 16, 16, False, True, False),
    ("G_convT_16to16_128_bn", 8, 128, 128, 16, 16, True, True, False),
    ("G_convT_16to1_256_bn_tanh", 8, 256, 256, 16, 1, True, True, True),
]


@pytest.mark.parametrize("layer", S2_LAYERS, ids=[s[0] for s in S2_LAYERS])
def test_full_size_stride2_layer_against_fp64(ngan, layer):
    from neuron_gan_amd import wgan_ops as W
    name, B, H, Wd, C, M, up, xf, tanh = layer
    gen = torch.Generator(device=DEV).manual_seed(B + H + C + M)
    x = _randn(gen, B, H, Wd, C)
    wshape = (C, M, 4, 4) if up else (M, C, 4, 4)
    w = 0.1 * _randn(gen, *wshape)
    bias = _randn(gen, M)
    xform, a = None, x.double()
    if xf:
        sc = torch.rand(C, device=DEV, generator=gen) + 0.5
        sh = 0.3 * _randn(gen, C)
        xform = (sc, sh, 1, SLOPE)
        a = R.act_on_load(a, sc.double(), sh.double(), 1, SLOPE)
    bound = (None, S2_TOL)
    y = W.conv(x, w, bias, up, xform, tanh)
    ref = R.s2_up(a, w.double(), bias.double()) if up else R.s2_down(a, w.double(), bias.double())
    if tanh:
        ref = torch.tanh(ref)
    check(f"{name} fwd", y, ref, bound)
    go = _randn(gen, *ref.shape)
    gy, gref = go, go.double()
    if tanh:
        gy = torch.empty_like(go)
        ngan._C.call("ngan_tanh_bwd", y, go, gy, go.numel())
        gref = gref * (1 - ref * ref)
    del ref
    ga = W.dgrad(gy, w, up)
    check(f"{name} dgrad", ga, R.s2_down(gref, w.double()) if up else R.s2_up(gref, w.double()), bound)
    del ga
    dw = W.wgrad(x, gy, wshape, half_xf=xform) if up else W.wgrad(gy, x, wshape, full_xf=xform)
    check(f"{name} wgrad", dw, R.s2_wgrad(a, gref) if up else R.s2_wgrad(gref, a), bound)
    check(f"{name} bias_grad", W.chan_sum(gy), gref.sum(dim=(0, 1, 2)), bound)


@pytest.mark.parametrize("shape", [(8, 256, 256, 16), (8, 128, 128, 32)])
def test_full_size_batchnorm_against_fp64(ngan, shape):
    from neuron_gan_amd import wgan_ops as W
    B, H, Wd, C = shape
    gen = torch.Generator(device=DEV).manual_seed(C + H)
    y = 2.0 * _randn(gen, B, H, Wd, C) + 3.0
    bn = torch.nn.BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(0.15 + 0.02 * _randn(gen, C))     # small scale, +-2 shift: BN(y) stays away from LeakyReLU's kink
        bn.bias.copy_(_signed_bias(gen, C, 2.0, noise=0.1))
        bn.running_mean.copy_(0.1 * _randn(gen, C))
        bn.running_var.copy_(torch.rand(C, device=DEV, generator=gen) + 0.5)
    gam, bet = bn.weight.detach().double(), bn.bias.detach().double()
    s = R.bn_stats(y.double(), gam, bet, bn.eps, bn.momentum, bn.running_mean.double().clone(), bn.running_var.double().clone())
    spec = W.BNSpec(bn)
    scale, shift, mean, rstd = spec.fold(y, bn.weight, bn.bias)
    for k, got in (("mean", mean), ("rstd", rstd), ("scale", scale), ("shift", shift)):
        check(f"bn {shape} {k}", got, s[k], (None, 1e-5))
    check(f"bn {shape} running_mean", bn.running_mean, s["running_mean"], (None, 1e-6))
    check(f"bn {shape} running_var", bn.running_var, s["running_var"], (None, 1e-5))
    assert int(bn.num_batches_tracked) == 1
    z = y.double() * s["scale"] + s["shift"]
    assert float(z.abs().min()) > 1e-3                      # off the kink: the backward's slope pattern is unambiguous
    act = torch.empty_like(y)
    ngan._C.call("ngan_bn_act_apply", y, scale, shift, 1, SLOPE, y.numel() // C, C, act)
    check(f"bn {shape} act", act, R.act_on_load(y.double(), s["scale"], s["shift"], 1, SLOPE), (None, S2_TOL))

    class Ctx:
        pass
    ctx = Ctx()
    ctx.bn, ctx.act, ctx.slope = spec, True, SLOPE
    go = _randn(gen, B, H, Wd, C)
    gy, dg, db = W._bn_act_backward(ctx, y, go, scale, shift, mean, rstd, bn.weight, True)
    rgy, rdg, rdb = R.bn_act_backward(y.double(), go.double(), gam, bet, s["mean"], s["rstd"], SLOPE)
    check(f"bn {shape} bwd_gy", gy, rgy, (None, 1e-4))
    check(f"bn {shape} bwd_dgamma", dg, rdg, (None, S2_TOL))
    check(f"bn {shape} bwd_dbeta", db, rdb, (None, S2_TOL))
