"""The "bf16" mode (precision code 5) at every channel width the reference's constructors accept: contraction widths other than
16 / 32 / 64 / 128 in the 3x3 conv (csrc/conv3x3_bf16_wide.hip: 128-channel slices of one fp32 accumulation) and the per-pixel
operators at channel counts outside the lane-group kernels' range (csrc/wide.hip over the storage type).  The reference's presets
0004 - 0008 have 256-, 512- and 1024-channel blocks (the reference's configs/config.py:87-98).

* kernel level, through the C ABI: against fp64 evaluated on the bf16-rounded operands.  Per element
      |got - ref| <= 2^-7 |ref| + C_ACC 2^-24 sum|products|,   C_ACC = 8
  -- one bf16 rounding of the store plus the fp32 accumulation term of a contraction whose terms may cancel (sum|products| is the
  same fp64 contraction on |operands|).  Operators with no contraction get the same bound with sum|products| = |ref| scaled by the
  channel count of their per-pixel sums.  (tests/test_gpu_bf16_conv.py pins the wide conv instances per element with fp32-tight bounds.)
* model level, against the CPU oracle, at tolerances derived BEFORE any GPU run from the CPU emulation of this mode
  (tests/lowprec_budget.py, "bf16mode") on the six width sets below: 1.5 x the largest emulated deviation over the sets, or the
  existing small-net bounds of tests/test_gpu_bf16.py where those are larger.  tests/test_bf16_wide_budget_cpu.py re-derives the
  emulated deviations and pins that the bounds cover them.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOPE = 0.2
BF = torch.bfloat16
C_ACC = 8.0

# the non-default width sets of tests/test_gpu_models.py::test_losses_and_gradients_match_oracle_on_the_fly (n_colors, res, alpha, widths)
WIDE_SETS = [(1, 16, 0.5, ([32, 8], [8, 32])), (1, 32, 1.0, ([16, 8, 8], [8, 8, 16])),
             (1, 32, 1.0, ([256, 128, 64], [64, 128, 256])), (1, 16, 0.5, ([256, 128], [128, 256])),
             (1, 16, 1.0, ([1024, 512], [256, 512])), (1, 16, 0.5, ([96, 48], [48, 96]))]

# model-level tolerances.  Emulated bf16-mode deviation from the fp32 oracle, largest over WIDE_SETS (tests/lowprec_budget.py,
# recomputed by tests/test_bf16_wide_budget_cpu.py): scalars / largest scalar 1.3e-3, |grad D| 2.3e-2, parameter gradients 1.9e-1
# relative L2 per net (G of ([96, 48], [48, 96])).  x 1.5 = 2.0e-3 / 3.5e-2 / 2.9e-1: tests/test_gpu_bf16.py's TOL_SCALAR 5e-2,
# TOL_NORM 6e-2 and TOL_GRAD 3e-1 are larger and stand.
TOL_SCALAR, TOL_NORM, TOL_GRAD = 5e-2, 6e-2, 3e-1

# the generator / critic widths of the reference's presets (configs/config.py:87-89 and 96-98)
PRESET_0004 = ([1024, 512, 256, 128, 64, 32, 16, 8], [16, 32, 64, 128, 128, 128, 128])
PRESET_0008 = ([512, 256, 128, 64], [64, 128, 256, 512])


@pytest.fixture
def bf16_mode(ngan):
    ngan.ops.set_conv_precision("bf16")
    yield ngan
    ngan.ops.set_conv_precision("f32")


def rbf(t):
    return t.to(BF).to(t.dtype)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def acc_close(got_bf16, ref64, absref64, c=C_ACC):
    """|got - ref| <= 2^-7 |ref| + c 2^-24 absref elementwise (absref: sum of |products| of the contraction)"""
    got = got_bf16.detach().double().cpu()
    err = (got - ref64).abs()
    bound = 2.0 ** -7 * ref64.abs() + c * 2.0 ** -24 * absref64 + 1e-30
    return not bool((err > bound).any()), float((err / bound).max())


def resample_ref(x, code):
    if code == 1:
        return rbf(F.avg_pool2d(x, 2).float()).double()
    if code == 2:
        return rbf(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=None).float()).double()
    return x


# ---- 1. conv forward / input gradient against fp64 ------------------------------------------------------------------------------
CONV = [
    # B, H, W, K, N, resample
    (2, 8, 8, 48, 16, 0), (4, 16, 16, 96, 64, 0), (2, 32, 32, 192, 16, 0), (8, 4, 4, 256, 128, 0), (2, 8, 8, 512, 64, 0),
    (4, 4, 4, 1024, 128, 0), (2, 16, 16, 48, 128, 1), (2, 8, 8, 256, 64, 1), (4, 4, 4, 1024, 16, 1), (2, 16, 16, 96, 16, 2),
    (2, 8, 8, 512, 128, 2), (4, 32, 32, 192, 64, 2), (2, 12, 20, 320, 32, 0),
]


@pytest.mark.parametrize("case", CONV)
def test_wide_conv_forward_against_fp64(bf16_mode, case):
    """ngan_bf16_conv3x3_fwd at contraction widths the tuned instances do not take: epilogue 0 and 1 (LeakyReLU -> PixelNorm with
    its fp32 norm)"""
    ops = bf16_mode.ops
    B, H, W, K, N, res = case
    torch.manual_seed(K + 7 * N + res)
    hin, win = (2 * H, 2 * W) if res == 1 else ((H // 2, W // 2) if res == 2 else (H, W))
    x = rbf(torch.randn(B, K, hin, win))
    w = torch.randn(N, K, 3, 3)
    bias = torch.randn(N) * 0.5
    scale = 1.3868 / np.sqrt(9 * K)
    wq = rbf((w * scale).float()).double()
    xr = resample_ref(x.double(), res)
    c_ref = F.conv2d(xr, wq, bias.double(), padding=1)
    c_abs = F.conv2d(xr.abs(), wq.abs(), bias.double().abs(), padding=1)
    xd = nhwc(x).to(DEV).to(BF)
    y0, _ = ops._run_conv(xd, w.to(DEV), bias.to(DEV), res, scale, 0, 0.0)
    assert y0.dtype == BF and tuple(y0.shape) == (B, H, W, N)
    ok, worst = acc_close(nchw(y0), c_ref, c_abs)
    assert ok, ("plain", worst)
    y1, rn = ops._run_conv(xd, w.to(DEV), bias.to(DEV), res, scale, 1, SLOPE)
    mask = (nchw(y1).double().cpu() > 0).double()          # the kernel's own activation pattern (ties at rounding level)
    lr = mask + SLOPE * (1 - mask)
    a = c_ref * lr
    r_ref = torch.sqrt(torch.mean(a * a, dim=1, keepdim=True) + 1e-8)
    # the norm is fp32 over N channels of fp32 sums: relative to r, the accumulation term of the channel sums plus fp32 rounding
    rel_acc = float((C_ACC * 2.0 ** -24 * c_abs * lr.abs()).max() / r_ref.min())
    assert float(((rn.double().cpu() - r_ref[:, 0]).abs() / r_ref[:, 0]).max()) < 2e-5 + rel_acc
    ok, worst = acc_close(nchw(y1), a / r_ref, (c_abs * lr) / r_ref)
    assert ok, ("lrelu_pn", worst)


DGRAD = [
    # B, H, W (conv resolution), Cout (= contraction), Cin (= outputs), pool-adjoint store
    (2, 8, 8, 48, 16, 0), (4, 16, 16, 96, 128, 0), (2, 8, 8, 192, 64, 0), (8, 4, 4, 256, 128, 0), (2, 8, 8, 512, 16, 0),
    (4, 4, 4, 1024, 64, 0), (2, 8, 8, 256, 32, 1), (4, 4, 4, 512, 128, 1), (2, 16, 16, 96, 64, 1),
]


@pytest.mark.parametrize("case", DGRAD)
def test_wide_input_gradient_against_fp64(bf16_mode, case):
    """the input-gradient call (flipped packed weights) with K = the layer's Cout: plain, with the producer's LeakyReLU -> PixelNorm
    backward (epilogue 2), and with the avg-pool adjoint store (out_mode 1), through the C ABI"""
    ngan = bf16_mode
    ops, C = ngan.ops, ngan._C
    B, H, W, K, N, pool = case
    torch.manual_seed(3 * K + N + pool)
    g = rbf(torch.randn(B, K, H, W))
    w = torch.randn(K, N, 3, 3)                 # forward weight (Cout = K, Cin = N)
    scale = 1.3868 / np.sqrt(9 * N)
    wq = rbf((w * scale).float()).double()
    gx_ref = F.conv_transpose2d(g.double(), wq, padding=1)
    gx_abs = F.conv_transpose2d(g.double().abs(), wq.abs(), padding=1)
    if pool:
        gx_ref = gx_ref.repeat_interleave(2, 2).repeat_interleave(2, 3) * 0.25
        gx_abs = gx_abs.repeat_interleave(2, 2).repeat_interleave(2, 3) * 0.25
    oh, ow = (2 * H, 2 * W) if pool else (H, W)
    gd = nhwc(g).to(DEV).to(BF)
    packed = ops._packed(w.to(DEV), 1, scale, 5)
    for epi in (0, 2):
        ay = rbf(torch.randn(B, N, oh, ow))
        arn = torch.rand(B, oh, ow) + 0.5
        gx = torch.empty((B, oh, ow, N), device=DEV, dtype=BF)
        ayd, arnd = nhwc(ay).to(DEV).to(BF), arn.to(DEV)
        C.call("ngan_bf16_conv3x3_fwd", gd, packed, None, gx, None, ayd if epi else None, arnd if epi else None, None,
               B, H, W, K, N, 0, epi, pool, SLOPE, 0.0)
        if epi == 0:
            ok, worst = acc_close(nchw(gx), gx_ref, gx_abs)
            assert ok, ("plain", worst)
            continue
        yy = ay.double()
        m = torch.where(yy > 0, torch.ones_like(yy), torch.full_like(yy, SLOPE))
        s = (gx_ref * yy).sum(1, keepdim=True) / N
        ref = (gx_ref - yy * s) / arn.double()[:, None] * m
        s_abs = (gx_abs * yy.abs()).sum(1, keepdim=True) / N
        absref = (gx_abs + yy.abs() * s_abs) / arn.double()[:, None] * m
        ok, worst = acc_close(nchw(gx), ref, absref)
        assert ok, ("pn_bwd", worst)


# ---- 2. wide per-pixel operators against fp64 formulas ---------------------------------------------------------------------------
WIDE_C = [48, 96, 192, 512, 1024]


def _pp_bound(ref, C):
    """per-pixel operators: one rounding + fp32 sums over C channels (C_ACC 2^-24 C |ref|)"""
    return ref.abs() * (2.0 ** -7 + C_ACC * 2.0 ** -24 * C)


def _check(got, ref, absref, what):
    got = got.detach().double().cpu()
    err = (got - ref).abs()
    bound = 2.0 ** -7 * ref.abs() + C_ACC * 2.0 ** -24 * absref + 1e-30
    assert not bool((err > bound).any()), (what, float((err / bound).max()))


@pytest.mark.parametrize("C", WIDE_C)
def test_wide_pixelnorm_operators_against_fp64(bf16_mode, C):
    """ngan_bf16_lrelu_pixelnorm_fwd / bwd / bwd2 / bwdbwd at channel counts of csrc/wide.hip"""
    _wide_pixelnorm_operators(bf16_mode, C, 96)


@pytest.mark.parametrize("P", [257, 1000])
@pytest.mark.parametrize("C", WIDE_C)
def test_wide_pixelnorm_operators_across_blocks_against_fp64(bf16_mode, C, P):
    """the same with more pixels than one 256-thread block of csrc/wide.hip's one-thread-per-pixel kernels: one pixel into the second
    block, and three full blocks with a ragged fourth (same bounds)"""
    _wide_pixelnorm_operators(bf16_mode, C, P)


def _wide_pixelnorm_operators(ngan, C, P):
    Cc = ngan._C
    torch.manual_seed(C)
    c = rbf(torch.randn(P, C))
    bias = torch.randn(C) * 0.3
    y = torch.empty(P, C, device=DEV, dtype=BF)
    rn = torch.empty(P, device=DEV)
    Cc.call("ngan_bf16_lrelu_pixelnorm_fwd", c.to(DEV).to(BF), bias.to(DEV), y, rn, P, C, SLOPE, 1e-8)
    a = c.double() + bias.double()
    m = torch.where(a > 0, torch.ones_like(a), torch.full_like(a, SLOPE))
    a = a * m
    r = torch.sqrt((a * a).mean(1, keepdim=True) + 1e-8)
    assert float(((rn.double().cpu() - r[:, 0]).abs() / r[:, 0]).max()) < 1e-5
    _check(y, a / r, (c.double().abs() + bias.double().abs()) * m / r * (1 + C_ACC), "fwd")
    # backward: y, rn as the forward stored them (bf16 y, fp32 rn)
    yb = y.double().cpu()
    rb = rn.double().cpu()[:, None]
    mk = torch.where(yb > 0, torch.ones_like(yb), torch.full_like(yb, SLOPE))
    gy, gy2 = rbf(torch.randn(P, C)), rbf(torch.randn(P, C))
    gr = torch.randn(P)
    gc = torch.empty(P, C, device=DEV, dtype=BF)
    Cc.call("ngan_bf16_lrelu_pixelnorm_bwd", gy.to(DEV).to(BF), gr.to(DEV), y, rn, gc, P, C, SLOPE)
    g = gy.double()
    s = (g * yb).sum(1, keepdim=True) / C
    kk = gr.double()[:, None] / C
    ref = ((g - yb * s) / rb + kk * yb) * mk
    absref = ((g.abs() + yb.abs() * (g.abs() * yb.abs()).sum(1, keepdim=True) / C) / rb + kk.abs() * yb.abs()) * mk.abs() * C
    _check(gc, ref, absref, "bwd")
    Cc.call("ngan_bf16_lrelu_pixelnorm_bwd2", gy.to(DEV).to(BF), gy2.to(DEV).to(BF), None, y, rn, gc, P, C, SLOPE)
    g = gy.double() + gy2.double()
    s = (g * yb).sum(1, keepdim=True) / C
    ref = (g - yb * s) / rb * mk
    absref = (g.abs() + yb.abs() * (g.abs() * yb.abs()).sum(1, keepdim=True) / C) / rb * mk.abs() * C
    _check(gc, ref, absref, "bwd2")
    # double backward
    h = rbf(torch.randn(P, C))
    ggy = torch.empty(P, C, device=DEV, dtype=BF)
    gyo = torch.empty(P, C, device=DEV, dtype=BF)
    gro = torch.empty(P, device=DEV)
    Cc.call("ngan_bf16_lrelu_pixelnorm_bwdbwd", h.to(DEV).to(BF), gy.to(DEV).to(BF), y, rn, ggy, gyo, gro, P, C, SLOPE)
    g = gy.double()
    hp = h.double() * mk
    s, t, u = (g * yb).sum(1, keepdim=True) / C, (hp * yb).sum(1, keepdim=True) / C, (hp * g).sum(1, keepdim=True) / C
    sa = (g.abs() * yb.abs()).sum(1, keepdim=True) / C
    ta = (hp.abs() * yb.abs()).sum(1, keepdim=True) / C
    ua = (hp.abs() * g.abs()).sum(1, keepdim=True) / C
    _check(ggy, (hp - yb * t) / rb, (hp.abs() + yb.abs() * ta) / rb * C, "bwdbwd ggy")
    _check(gyo, -(s * hp + t * g) / rb, (sa * hp.abs() + ta * g.abs()) / rb * C, "bwdbwd gy")
    gr_ref = -C * (u - s * t) / rb ** 2
    gr_abs = C * (ua + sa * ta) / rb ** 2
    err = (gro.double().cpu()[:, None] - gr_ref).abs()
    assert bool((err <= 1e-5 * gr_ref.abs() + C_ACC * 2.0 ** -24 * C * gr_abs + 1e-30).all()), "bwdbwd gr"


@pytest.mark.parametrize("C", WIDE_C)
def test_wide_channel_sum_and_image_edges_against_fp64(bf16_mode, C):
    """ngan_bf16_channel_sum, to_image_fwd / bwd (+ the PixelNorm-backward variant), from_image_dx / dw at csrc/wide.hip's widths"""
    _wide_channel_sum_and_image_edges(bf16_mode, C, 2, 8, 8)


@pytest.mark.parametrize("C", WIDE_C)
def test_wide_channel_sum_and_image_edges_across_blocks_against_fp64(bf16_mode, C):
    """the same on 2 x 20 x 25 = 1000 pixels: three full 256-thread blocks and a ragged fourth (same bounds)"""
    _wide_channel_sum_and_image_edges(bf16_mode, C, 2, 20, 25)


def _wide_channel_sum_and_image_edges(ngan, C, B, H, W):
    Cc = ngan._C
    torch.manual_seed(5 * C)
    Ncol = 1
    P = B * H * W
    g = rbf(torch.randn(P, C))
    out = torch.empty(C, device=DEV)
    ws = torch.empty(1 << 20, device=DEV)
    Cc.call("ngan_bf16_channel_sum", g.to(DEV).to(BF), out, ws, P, C, 0.5)
    ref = 0.5 * g.double().sum(0)
    assert bool(((out.double().cpu() - ref).abs() <= C_ACC * 2.0 ** -24 * P * 0.5 * g.double().abs().sum(0) + 1e-30).all()), "channel_sum"
    # ToImage: t = tanh(x . w) per pixel
    x = rbf(torch.randn(P, C) * 0.2)
    wimg = torch.randn(Ncol, C) / np.sqrt(C)
    t = torch.empty(P, Ncol, device=DEV)
    xd = x.to(DEV).to(BF)
    Cc.call("ngan_bf16_to_image_fwd", xd, wimg.to(DEV), t, P, C, Ncol)
    d = x.double() @ wimg.double().T
    dabs = x.double().abs() @ wimg.double().abs().T
    assert bool(((t.double().cpu() - torch.tanh(d)).abs() <= C_ACC * 2.0 ** -24 * dabs + 1e-6).all()), "to_image_fwd"
    gt = torch.randn(P, Ncol)
    gx = torch.empty(P, C, device=DEV, dtype=BF)
    gw = torch.empty(Ncol, C, device=DEV)
    Cc.call("ngan_bf16_to_image_bwd", gt.to(DEV), t, xd, wimg.to(DEV), gx, gw, ws, P, C, Ncol)
    tt = t.double().cpu()
    q = gt.double() * (1 - tt * tt)
    _check(gx, q @ wimg.double(), q.abs() @ wimg.double().abs(), "to_image_bwd gx")
    gw_ref = q.T @ x.double()
    gw_abs = q.abs().T @ x.double().abs()
    assert bool(((gw.double().cpu() - gw_ref).abs() <= C_ACC * 2.0 ** -24 * P * gw_abs + 1e-30).all()), "to_image_bwd gw"
    # with the LeakyReLU -> PixelNorm backward of the producer (x = its output y, rn its norm)
    rn = torch.rand(P) + 0.5
    Cc.call("ngan_bf16_to_image_bwd_pnbwd", gt.to(DEV), t, xd, rn.to(DEV), wimg.to(DEV), gx, gw, ws, P, C, Ncol, SLOPE)
    o = q @ wimg.double()
    oa = q.abs() @ wimg.double().abs()
    yb = x.double()
    mk = torch.where(yb > 0, torch.ones_like(yb), torch.full_like(yb, SLOPE))
    s = (o * yb).sum(1, keepdim=True) / C
    sa = (oa * yb.abs()).sum(1, keepdim=True) / C
    rr = rn.double()[:, None]
    _check(gx, (o - yb * s) / rr * mk, (oa + yb.abs() * sa) / rr * mk * C, "to_image_bwd_pnbwd gx")
    # FromImage: dx (fp32 image gradient) and dw / db from a bf16 gradient, plain and pooled
    for pool in (0, 1):
        gimg = rbf(torch.randn(P, C))
        wf = torch.randn(C, Ncol)
        gxi = torch.empty((B, 2 * H, 2 * W, Ncol) if pool else (B, H, W, Ncol), device=DEV)
        Cc.call("ngan_bf16_from_image_dx", gimg.to(DEV).to(BF), wf.to(DEV), gxi, B, H, W, Ncol, C, pool)
        r = (gimg.double() @ wf.double()).reshape(B, H, W, Ncol)
        ra = (gimg.double().abs() @ wf.double().abs()).reshape(B, H, W, Ncol)
        if pool:
            r = 0.25 * r.repeat_interleave(2, 1).repeat_interleave(2, 2)
            ra = 0.25 * ra.repeat_interleave(2, 1).repeat_interleave(2, 2)
        assert bool(((gxi.double().cpu() - r).abs() <= C_ACC * 2.0 ** -24 * C * ra + 1e-30).all()), ("from_image_dx", pool)
        img = torch.randn(B, 2 * H, 2 * W, Ncol) if pool else torch.randn(B, H, W, Ncol)
        gwf = torch.empty(C, Ncol, device=DEV)
        gbf = torch.empty(C, device=DEV)
        Cc.call("ngan_bf16_from_image_dw", img.to(DEV), gimg.to(DEV).to(BF), gwf, gbf, ws, B, H, W, Ncol, C, pool)
        xi = img.double()
        if pool:
            xi = F.avg_pool2d(xi.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        xi = xi.reshape(P, Ncol)
        wref, wabs = gimg.double().T @ xi, gimg.double().abs().T @ xi.abs()
        assert bool(((gwf.double().cpu() - wref).abs() <= C_ACC * 2.0 ** -24 * P * wabs + 1e-6 * wabs).all()), ("from_image_dw", pool)
        bref, babs = gimg.double().sum(0), gimg.double().abs().sum(0)
        assert bool(((gbf.double().cpu() - bref).abs() <= C_ACC * 2.0 ** -24 * P * babs + 1e-30).all()), ("from_image_db", pool)


@pytest.mark.parametrize("C", WIDE_C)
def test_wide_up2_adjoint_pixelnorm_backward_against_fp64(bf16_mode, C):
    """ngan_bf16_up2_adjoint_pnbwd at wide C: the bilinear x2 adjoint and the PixelNorm backward of the low-resolution producer in one
    pass -- the adjoint is not rounded to bf16 in between (the reference below keeps it in fp64; a rounded intermediate would miss
    the bound by the 2^-7 of that rounding, amplified through the per-pixel sum)"""
    ngan = bf16_mode
    Cc = ngan._C
    torch.manual_seed(11 * C)
    B, h, w = 2, 4, 6
    g = rbf(torch.randn(B, C, 2 * h, 2 * w))
    y = rbf(torch.randn(B, C, h, w))
    rn = torch.rand(B, h, w) + 0.5
    o = torch.empty(B, h, w, C, device=DEV, dtype=BF)
    Cc.call("ngan_bf16_up2_adjoint_pnbwd", nhwc(g).to(DEV).to(BF), nhwc(y).to(DEV).to(BF), rn.to(DEV), o, B, h, w, C, SLOPE)
    gd = g.double().requires_grad_(True)
    lo = torch.zeros(B, C, h, w, dtype=torch.float64, requires_grad=True)
    up = F.interpolate(lo, scale_factor=2, mode="bilinear", align_corners=False)
    adj, = torch.autograd.grad((up * gd).sum(), lo)
    lo2 = torch.zeros(B, C, h, w, dtype=torch.float64, requires_grad=True)
    adj_abs, = torch.autograd.grad((F.interpolate(lo2, scale_factor=2, mode="bilinear", align_corners=False) * g.double().abs()).sum(), lo2)
    yy = y.double()
    mk = torch.where(yy > 0, torch.ones_like(yy), torch.full_like(yy, SLOPE))
    s = (adj * yy).sum(1, keepdim=True) / C
    sa = (adj_abs * yy.abs()).sum(1, keepdim=True) / C
    r = rn.double()[:, None]
    ref = (adj - yy * s) / r * mk
    absref = (adj_abs + yy.abs() * sa) / r * mk * C
    _check(nchw(o), ref, absref, "up2_adjoint_pnbwd")


# ---- 3. model level against the CPU oracle ---------------------------------------------------------------------------------------
def wide_case(ngan, n_colors, res, alpha, widths):
    """the nets, oracle parameters and draws of test_losses_and_gradients_match_oracle_on_the_fly for one width set (CPU tensors)"""
    from oracle import pggan_oracle as O
    torch.manual_seed(11 + n_colors + res)
    gw, dw = widths
    G = ngan.models.Generator_PG(gw, image_size_init=8, latent_dim=64, N_colors=n_colors)
    D = ngan.models.Discriminator_PG(dw, image_size_init=8, N_colors=n_colors)
    G.set_resolution(res, alpha)
    D.set_resolution(res, alpha)
    pg = O.as_leaf_params({k: v.detach().clone() for k, v in G.state_dict().items()})
    pd = O.as_leaf_params({k: v.detach().clone() for k, v in D.state_dict().items()})
    spec = O.NetSpec(image_size_init=8, slope=0.2, alpha=alpha)
    b = 4
    x = torch.rand(b, n_colors, res, res) * 2 - 1
    z1, z2, z3 = (O.sample_latent_vec((b, 64)) for _ in range(3))
    eps = torch.rand(b, 1, 1, 1)
    return G, D, pg, pd, spec, x, z1, z2, eps, z3


def rel_l2(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("n_colors,res,alpha,widths", WIDE_SETS)
def test_wide_nets_against_the_oracle_at_the_modes_tolerance(bf16_mode, n_colors, res, alpha, widths):
    """critic loss + gradient penalty + generator loss in the bf16 mode against the fp32 CPU oracle on the same weights and draws:
    scalars, the penalty's per-sample |grad D|, and the relative L2 of each net's parameter gradients"""
    from oracle import pggan_oracle as O
    ngan = bf16_mode
    G, D, pg, pd, spec, x, z1, z2, eps, z3 = wide_case(ngan, n_colors, res, alpha, widths)
    G.to(DEV)
    D.to(DEV)
    d_loss, s_r, s_f = O.d_w_loss(pg, spec, pd, spec, x, z1, 0.001)
    gp, norms = O.grad_penalty(pg, spec, pd, spec, x, z2, eps, 10.0, return_norms=True)
    (d_loss + gp).backward()
    LF = ngan.loss_functions
    Dl, Gp, Gl = LF.D_W_loss(G, D, 0.001), LF.D_grad_pen_loss(G, D, 10.0), LF.G_W_loss(G, D)
    xd = x.to(DEV)
    d2, sr2, sf2 = Dl(xd, z=z1.to(DEV))
    gp2 = Gp(xd, z=z2.to(DEV), epsilon=eps.to(DEV))
    (d2 + gp2).backward()
    names = [k for k, p in D.named_parameters() if p.grad is not None]
    assert names
    got_d = torch.cat([dict(D.named_parameters())[k].grad.detach().cpu().reshape(-1) for k in names])
    want_d = torch.cat([pd[k].grad.reshape(-1) for k in names])
    assert rel_l2(got_d, want_d) < TOL_GRAD, ("D", rel_l2(got_d, want_d))
    assert M_rel(Gp.last_grad_norms.cpu(), norms.detach()) < TOL_NORM, M_rel(Gp.last_grad_norms.cpu(), norms.detach())
    for p in G.parameters():
        p.grad = None
    for v in pg.values():
        v.grad = None
    g_ref = O.g_w_loss(pg, spec, pd, spec, z3)
    g_ref.backward()
    g2, _ = Gl(xd, z=z3.to(DEV))
    g2.backward()
    got = np.array([float(d2.detach()), float(sr2.detach()), float(sf2.detach()), float(gp2.detach()), float(g2.detach())])
    want = np.array([float(d_loss.detach()), float(s_r.detach()), float(s_f.detach()), float(gp.detach()), float(g_ref.detach())])
    assert float(np.abs(got - want).max()) < TOL_SCALAR * float(np.abs(want).max()), (got, want)
    names = [k for k, p in G.named_parameters() if p.grad is not None]
    got_g = torch.cat([dict(G.named_parameters())[k].grad.detach().cpu().reshape(-1) for k in names])
    want_g = torch.cat([pg[k].grad.reshape(-1) for k in names])
    assert rel_l2(got_g, want_g) < TOL_GRAD, ("G", rel_l2(got_g, want_g))


def M_rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(((a - b).abs() / b.abs()).max())


# ---- 4. the step driver -------------------------------------------------------------------------------------------------------
def test_wide_nets_through_the_step_driver_in_bf16(bf16_mode):
    """the nets of tests/test_gpu_train.py::test_wide_nets_through_the_step_driver in the bf16 mode: captured-graph replay equals eager
    bit for bit, the statistics are finite, parameters and Adam state stay fp32"""
    ngan = bf16_mode

    def make():
        torch.manual_seed(21)
        G = ngan.models.Generator_PG([256, 128], image_size_init=8, latent_dim=32)
        D = ngan.models.Discriminator_PG([128, 256], image_size_init=8)
        G.set_resolution(16, 0.5)
        D.set_resolution(16, 0.5)
        return ngan.train.PGGANTrainer(G.to(DEV), D.to(DEV), learning_rate=1e-3)
    gen = torch.Generator().manual_seed(5)

    def draw(b):
        z = [torch.randn(b, 32, generator=gen) for _ in range(3)]
        z = [(v / v.norm(dim=1, keepdim=True)).to(DEV) for v in z]
        return dict(real=(torch.rand(b, 1, 16, 16, generator=gen) * 2 - 1).to(DEV), z_d=z[0], z_gp=z[1],
                    eps=torch.rand(b, 1, 1, 1, generator=gen).to(DEV), z_g=z[2])
    seq = [draw(4) for _ in range(3)]
    eager, tr = make(), make()
    static = {k: seq[0][k].clone() for k in ("z_d", "z_gp", "eps", "z_g")}
    tr.capture(seq[0]["real"], draws=static)
    for s in seq:
        stats = eager.train_iteration(s["real"], s["z_d"], s["z_gp"], s["eps"], s["z_g"])
        for k, v in static.items():
            v.copy_(s[k])
        tr.replay(s["real"])
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in stats.values())
    for f in (tr.flat_g, tr.flat_d, eager.flat_g, eager.flat_d):
        assert f.flat.dtype == torch.float32 and f.exp_avg.dtype == torch.float32 and f.exp_avg_sq.dtype == torch.float32
    for name, p, pe in zip(tr.flat_g.names + tr.flat_d.names, tr.flat_g.params + tr.flat_d.params, eager.flat_g.params + eager.flat_d.params):
        assert p.dtype == torch.float32
        assert torch.equal(p, pe), f"{name}: {float((p - pe).abs().max())}"


# ---- 5. the reference's wide presets --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["0004", "0008"])
def test_preset_widths_one_iteration_in_bf16(ngan, preset):
    """one PGGANTrainer.train_iteration with a preset's generator and critic widths at 32 x 32, batch 4: finite in the bf16 mode, and
    its losses within the model-level scalar tolerance of the same iteration in f32 on the same weights and draws"""
    gw, dw = PRESET_0004 if preset == "0004" else PRESET_0008
    gen = torch.Generator().manual_seed(17)
    z = [torch.randn(4, 64, generator=gen) for _ in range(3)]
    z = [(v / v.norm(dim=1, keepdim=True)).to(DEV) for v in z]
    real = (torch.rand(4, 1, 32, 32, generator=gen) * 2 - 1).to(DEV)
    eps = torch.rand(4, 1, 1, 1, generator=gen).to(DEV)
    out = {}
    try:
        for mode in ("f32", "bf16"):
            ngan.ops.set_conv_precision(mode)
            torch.manual_seed(23)
            G = ngan.models.Generator_PG(gw, image_size_init=4, latent_dim=64)
            D = ngan.models.Discriminator_PG(dw, image_size_init=4)
            G.set_resolution(32, 1.0)
            D.set_resolution(32, 1.0)
            tr = ngan.train.PGGANTrainer(G.to(DEV), D.to(DEV), learning_rate=1e-4)
            stats = tr.train_iteration(real, z[0], z[1], eps, z[2])
            torch.cuda.synchronize()
            out[mode] = {k: float(v) for k, v in stats.items()}
    finally:
        ngan.ops.set_conv_precision("f32")
    assert all(np.isfinite(v) for v in out["bf16"].values()), out["bf16"]
    keys = [k for k in out["f32"] if k in ("D_loss", "G_loss", "D_grad_pen", "score_real", "score_fake")]
    assert keys, out["f32"]
    ref = max(abs(out["f32"][k]) for k in keys)
    dev = max(abs(out["bf16"][k] - out["f32"][k]) for k in keys)
    assert dev < TOL_SCALAR * ref, (dev, ref, out)
