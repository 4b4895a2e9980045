"""tests/fp64_conv.py (the fp64 reference of tests/test_gpu_full_size.py) against torch's own fp64 operators on the CPU, and the power
of the noise-scaled adjoint-identity statistic (test_gpu_ops.py::test_full_size_layers_satisfy_the_adjoint_identities) against faults
planted in clean torch fp32 results.  No GPU needed."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_conv as R  # noqa: E402

D = torch.float64
TOL = 1e-12


def close(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300)) < TOL


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def resample_torch(x, code):
    if code == 1:
        return F.avg_pool2d(x, 2)
    if code == 2:
        return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    return x


CONV_SHAPES = [  # B, H, W (of the conv's output), K, N, resample: non-square, odd sizes, C = 1 / 3 / 16 / 48
    (2, 5, 7, 3, 16, 0), (1, 9, 4, 1, 3, 0), (3, 6, 10, 16, 48, 1), (2, 4, 6, 48, 16, 1), (1, 10, 14, 3, 1, 2), (2, 6, 8, 16, 16, 2),
    (1, 1, 3, 16, 3, 0),
]


@pytest.mark.parametrize("case", CONV_SHAPES)
def test_conv3x3_triple_matches_torch(case):
    B, H, W, K, N, res = case
    g = torch.Generator().manual_seed(sum(case))
    hin, win = (2 * H, 2 * W) if res == 1 else ((H // 2, W // 2) if res == 2 else (H, W))
    x = torch.randn(B, K, hin, win, generator=g, dtype=D)
    w = torch.randn(N, K, 3, 3, generator=g, dtype=D)
    bias = torch.randn(N, generator=g, dtype=D)
    go = torch.randn(B, N, H, W, generator=g, dtype=D)
    scale = 0.37
    xr = x.clone().requires_grad_()
    xin = resample_torch(xr, res)
    y = F.conv2d(xin, scale * w, bias, padding=1)
    (gx,) = torch.autograd.grad(y, xr, go)
    gw = scale * torch.nn.grad.conv2d_weight(xin.detach(), w.shape, go, padding=1)
    assert close(nchw(R.conv3x3(nhwc(x), w, scale, res, bias)), y.detach())
    assert close(nchw(R.conv3x3_dgrad(nhwc(go), w, scale, res)), gx)
    assert close(R.conv3x3_wgrad(nhwc(x), nhwc(go), scale, res), gw)
    assert close(nchw(R.resample(nhwc(x), res)), xin.detach())


@pytest.mark.parametrize("C", [1, 3, 16])
def test_resample_and_adjoint_match_torch(C):
    g = torch.Generator().manual_seed(C)
    x = torch.randn(2, C, 6, 10, generator=g, dtype=D)
    for code, h in ((1, (3, 5)), (2, (12, 20))):
        xr = x.clone().requires_grad_()
        out = resample_torch(xr, code)
        assert tuple(out.shape[2:]) == h
        v = torch.randn(out.shape, generator=g, dtype=D)
        (ga,) = torch.autograd.grad(out, xr, v)
        assert close(nchw(R.resample(nhwc(x), code)), out.detach())
        assert close(nchw(R.resample_adjoint(nhwc(v), code)), ga)
    assert close(nchw(R.pool2(nhwc(x))), F.avg_pool2d(x, 2))


@pytest.mark.parametrize("C", [3, 16, 48])
def test_pixelnorm_epilogues_match_autograd(C):
    g = torch.Generator().manual_seed(C + 1)
    c = torch.randn(2, 5, 7, C, generator=g, dtype=D).requires_grad_()
    gy = torch.randn(2, 5, 7, C, generator=g, dtype=D)
    a = F.leaky_relu(c, 0.2)
    r = torch.sqrt((a * a).mean(-1, keepdim=True) + 1e-8)
    y = a / r
    (gc,) = torch.autograd.grad(y, c, gy)
    yr, rr = R.lrelu_pixelnorm(c.detach(), 0.2)
    assert close(yr, y.detach()) and close(rr, r[..., 0].detach())
    assert close(R.pixelnorm_bwd(gy, yr, rr, 0.2), gc)


S2_SHAPES = [  # B, H (of the input), W, C, M
    (2, 6, 10, 1, 16), (1, 8, 4, 3, 1), (3, 10, 6, 16, 48), (1, 4, 12, 48, 3),
]


@pytest.mark.parametrize("case", S2_SHAPES)
@pytest.mark.parametrize("up", [False, True])
def test_stride2_triples_match_torch(case, up):
    B, H, W, C, M = case
    g = torch.Generator().manual_seed(sum(case) + up)
    x = torch.randn(B, C, H, W, generator=g, dtype=D)
    w = torch.randn((C, M, 4, 4) if up else (M, C, 4, 4), generator=g, dtype=D)
    bias = torch.randn(M, generator=g, dtype=D)
    scale = torch.rand(C, generator=g, dtype=D) + 0.5
    shift = torch.randn(C, generator=g, dtype=D) * 0.3
    a = F.leaky_relu(x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), 0.2).requires_grad_()
    wr = w.clone().requires_grad_()
    y = F.conv_transpose2d(a, wr, bias, stride=2, padding=1) if up else F.conv2d(a, wr, bias, stride=2, padding=1)
    go = torch.randn(y.shape, generator=g, dtype=D)
    ga, gw = torch.autograd.grad(y, [a, wr], go)
    a_ = R.act_on_load(nhwc(x), scale, shift, 1, 0.2)
    assert close(nchw(a_), a.detach())
    got = R.s2_up(a_, w, bias) if up else R.s2_down(a_, w, bias)
    assert close(nchw(got), y.detach())
    dg = R.s2_down(nhwc(go), w) if up else R.s2_up(nhwc(go), w)       # each pass's input gradient is the other pass
    assert close(nchw(dg), ga)
    dw = R.s2_wgrad(a_, nhwc(go)) if up else R.s2_wgrad(nhwc(go), a_)
    assert close(dw, gw)


@pytest.mark.parametrize("C", [1, 3, 16])
def test_batchnorm_matches_torch(C):
    g = torch.Generator().manual_seed(C + 7)
    y = torch.randn(3, C, 5, 7, generator=g, dtype=D) * 2 + 3
    bn = torch.nn.BatchNorm2d(C).double()
    with torch.no_grad():
        bn.weight.normal_(1.0, 0.1, generator=g)
        bn.bias.normal_(0.0, 0.1, generator=g)
        bn.running_var.uniform_(0.5, 1.5, generator=g)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    yr = y.clone().requires_grad_()
    act = F.leaky_relu(bn(yr), 0.2)
    go = torch.randn(act.shape, generator=g, dtype=D)
    act.backward(go)
    gam, bet = bn.weight.detach(), bn.bias.detach()
    s = R.bn_stats(nhwc(y), gam, bet, bn.eps, bn.momentum, rm0, rv0)
    assert close(s["running_mean"], bn.running_mean) and close(s["running_var"], bn.running_var)
    assert close(nchw(R.act_on_load(nhwc(y), s["scale"], s["shift"], 1, 0.2)), act.detach())
    gy, dgam, dbet = R.bn_act_backward(nhwc(y), nhwc(go), gam, bet, s["mean"], s["rstd"], 0.2)
    assert close(nchw(gy), yr.grad) and close(dgam, bn.weight.grad) and close(dbet, bn.bias.grad)


@pytest.mark.parametrize("case", [(3, 7, 2, 3, 5), (1, 1, 1, 1, 1), (4, 10, 5, 2, 3)])       # B, K, h, w, C: non-square position grids
def test_stem_and_its_gradients_match_torch(case):
    B, K, h, w, C = case
    S = h * w
    g = torch.Generator().manual_seed(sum(case))
    lin = torch.nn.Linear(K, C * S).double()
    z = torch.randn(B, K, generator=g, dtype=D)
    y = lin(z).view(B, C, h, w)
    go = torch.randn(y.shape, generator=g, dtype=D)
    gw, gb = torch.autograd.grad(y, [lin.weight, lin.bias], go)
    wt, b = lin.weight.detach(), lin.bias.detach()
    got = R.stem(z, wt, b, S, C)
    assert close(nchw(got.view(B, h, w, C)), y.detach())
    g_nhwc = nhwc(go).reshape(B, S, C)
    rw, rb = R.stem_grads(z, g_nhwc, S, C)
    assert close(rw, gw) and close(rb, gb)
    # the twins: the same operators on absolute values bound the originals
    assert bool((R.stem(z.abs(), wt.abs(), b.abs(), S, C) >= got.abs()).all())
    aw, ab = R.stem_grads(z.abs(), g_nhwc.abs(), S, C)
    assert bool((aw >= rw.abs()).all()) and bool((ab >= rb.abs()).all())


@pytest.mark.parametrize("C", [1, 5])
def test_batchnorm_eval_fold_matches_torch(C):
    g = torch.Generator().manual_seed(C + 21)
    bn = torch.nn.BatchNorm2d(C, eps=1e-3).double().eval()
    with torch.no_grad():
        bn.weight.normal_(1.0, 0.5, generator=g)
        bn.bias.normal_(0.0, 0.5, generator=g)
        bn.running_mean.normal_(0.0, 2.0, generator=g)
        bn.running_var.uniform_(0.01, 2.0, generator=g)
    x = torch.randn(2, C, 3, 7, generator=g, dtype=D)
    args = (bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps)
    scale, shift = R.bn_fold_eval(*args)
    assert close(nchw(nhwc(x) * scale + shift), bn(x).detach())
    sa, ha = R.bn_fold_eval_abs(*args)
    assert bool((sa >= scale.abs()).all()) and bool((ha >= shift.abs()).all())


@pytest.mark.parametrize("act", [True, False])
def test_batchnorm_backward_variants_match_torch(act):
    """with and without the activation, with a given act' mask, and the absolute-value twins; 3 x 5 x 7 pixels"""
    C = 5
    g = torch.Generator().manual_seed(31 + act)
    y = torch.randn(3, C, 5, 7, generator=g, dtype=D) * 2 + 3
    bn = torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.37).double()
    with torch.no_grad():
        bn.weight.normal_(1.0, 0.1, generator=g)
        bn.bias.normal_(0.0, 0.1, generator=g)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    yr = y.clone().requires_grad_()
    z = bn(yr)
    out = F.leaky_relu(z, 0.2) if act else z
    go = torch.randn(out.shape, generator=g, dtype=D)
    out.backward(go)
    gam, bet = bn.weight.detach(), bn.bias.detach()
    s = R.bn_stats(nhwc(y), gam, bet, bn.eps, bn.momentum, rm0, rv0)
    assert close(s["running_mean"], bn.running_mean) and close(s["running_var"], bn.running_var)
    gy, dgam, dbet = R.bn_act_backward(nhwc(y), nhwc(go), gam, bet, s["mean"], s["rstd"], 0.2, act=act)
    assert close(nchw(gy), yr.grad) and close(dgam, bn.weight.grad) and close(dbet, bn.bias.grad)
    zl = nhwc(z.detach())
    mask = torch.where(zl > 0, torch.ones_like(zl), torch.full_like(zl, 0.2)) if act else torch.ones_like(zl)
    gy2, dgam2, dbet2 = R.bn_act_backward(nhwc(y), nhwc(go), gam, None, s["mean"], s["rstd"], 0.2, mask=mask)
    assert close(gy2, gy) and close(dgam2, dgam) and close(dbet2, dbet)
    ta = R.bn_act_backward_abs(nhwc(y), nhwc(go), gam, s["mean"], s["rstd"], mask)
    assert all(bool((t >= v.abs()).all()) for t, v in zip(ta, (gy, dgam, dbet)))
    a = R.bn_stats_abs(nhwc(y), gam, bet, bn.eps, bn.momentum, rm0, rv0)
    assert all(bool((a[k] >= s[k].abs() * (1 - 1e-15)).all()) for k in s)


def test_activation_backward_and_single_pixel_statistics():
    g = torch.Generator().manual_seed(41)
    y = torch.randn(2, 3, 5, 4, generator=g, dtype=D).requires_grad_()      # channels-last (B, H, W, C)
    go = torch.randn(y.shape, generator=g, dtype=D)
    (gy,) = torch.autograd.grad(F.leaky_relu(y, 0.2), y, go)
    assert close(R.act_backward(y.detach(), go, 0.2), gy)
    # one pixel per channel: torch refuses the batch; the variance is 0 and the running variance takes it as it is
    one = torch.randn(1, 1, 1, 4, generator=g, dtype=D)
    s = R.bn_stats(one, torch.ones(4, dtype=D), torch.zeros(4, dtype=D), 1e-5, 0.1, torch.zeros(4, dtype=D), torch.ones(4, dtype=D))
    assert close(s["mean"], one.reshape(4)) and float(s["var"].abs().max()) == 0.0
    assert close(s["running_var"], torch.full((4,), 0.9, dtype=D))


# ---- the adjoint-identity statistic has power ---------------------------------------------------------------------------------
def _fp32_triple(x, w, g, scale, pad_mode="zeros"):
    """clean torch fp32 results of a 3x3 layer on NCHW operands (pad_mode "circular": the wrap-around fault in all three)"""
    if pad_mode == "zeros":
        y = F.conv2d(x, scale * w, padding=1)
    else:
        y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="circular"), scale * w)
    gx = torch.nn.grad.conv2d_input(x.shape, scale * w, g, padding=1)
    gw = scale * torch.nn.grad.conv2d_weight(x, w.shape, g, padding=1)
    return y, gx, gw


def _margins(x, w, y, g, gx, gw, eps=2e-5):
    return R.identity_margins(nhwc(x), w, nhwc(y), nhwc(g), nhwc(gx), gw, eps)


def test_identity_statistic_flags_planted_faults():
    """4 x 128^2, 16 -> 16 in torch fp32 (the first full-size layer at a reduced size), eps = 2e-5 (the exact-fp32 bound).  A clean result
    must pass by a wide margin; each planted fault (one output tensor altered on the host, as a wrong tile offset, border or split
    boundary would alter it) must fail (margin > 1)."""
    g_ = torch.Generator().manual_seed(11)
    B, H, W, C = 4, 128, 128, 16
    x = torch.randn(B, C, H, W, generator=g_)
    w = torch.randn(C, C, 3, 3, generator=g_)
    g = torch.randn(B, C, H, W, generator=g_)
    scale = 1.0 / 12.0
    y, gx, gw = _fp32_triple(x, w, g, scale)
    clean = _margins(x, w, y, g, gx, gw)
    assert max(clean) < 0.1, clean
    faults = {}
    y1 = y.clone()
    y1[:, :, -8:, :] = 0                                               # last 8-row tile strip of every image never written
    faults["strip_unwritten"] = _margins(x, w, y1, g, gx, gw)[0]
    yc, _, _ = _fp32_triple(x, w, g, scale, "circular")               # wrap-around instead of zero padding on all four borders
    faults["wrap_around"] = _margins(x, w, yc, g, gx, gw)[0]
    gs = torch.zeros_like(g)
    gs[1, :, 40:48, :] = g[1, :, 40:48, :]                            # wgrad: one 8-row strip of one image summed twice
    gw3 = gw + scale * torch.nn.grad.conv2d_weight(x, w.shape, gs, padding=1)
    faults["wgrad_strip_twice"] = _margins(x, w, y, g, gx, gw3)[1]
    y4 = y.clone()
    y4[-1] *= 0.5                                                      # last image of the batch scaled by 0.5
    faults["last_image_half"] = _margins(x, w, y4, g, gx, gw)[0]
    gx5 = gx.clone()
    gx5[:, :, :, 0] = 0                                                # input gradient: left border column dropped
    faults["dgrad_border_dropped"] = _margins(x, w, y, g, gx5, gw)[0]
    print("identity margins |diff|/tau: clean", clean, "faults", faults)
    for name, m in faults.items():
        assert m > 1.0, (name, m)


@pytest.mark.parametrize("res", [1, 2])
def test_identity_statistic_passes_clean_resampled_layers(res):
    """the same statistic on clean fp32 results of pooled and bilinear layers (the adjoint of the resampling included)"""
    g_ = torch.Generator().manual_seed(res)
    B, H, W, K, N = 4, 64, 64, 16, 32
    hin, win = (2 * H, 2 * W) if res == 1 else (H // 2, W // 2)
    x = torch.randn(B, K, hin, win, generator=g_)
    w = torch.randn(N, K, 3, 3, generator=g_)
    g = torch.randn(B, N, H, W, generator=g_)
    scale = 1.0 / 12.0
    xr = x.clone().requires_grad_()
    xin = resample_torch(xr, res)
    y = F.conv2d(xin, scale * w, padding=1)
    (gx,) = torch.autograd.grad(y, xr, g)
    gw = scale * torch.nn.grad.conv2d_weight(xin.detach(), w.shape, g, padding=1)
    m = _margins(x, w, y.detach(), g, gx, gw)
    assert max(m) < 0.1, m
