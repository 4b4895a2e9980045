"""The minibatch standard-deviation layer of the PG critic's head (include/ngan_mbstd.h, csrc/mbstd.hip): the fp64
restatements -- the statistic, its two derivative orders in closed form, the field family and the whole mbstd critic in the plain-torch
concat formulation, built from oracle.pggan_oracle's primitives -- numpy-fp32 emulations of the kernels' arithmetic, the cases, the
families and the per-element bound.  Shared by tests/test_mbstd_cpu.py (closed forms against torch.autograd on the concat formulation),
tests/test_mbstd_bounds_cpu.py (the emulations against the references: the constants are settled on the CPU, before any kernel is looked
at) and tests/test_gpu_mbstd.py (the kernels against the references).  `ratio`, `draws`, `seed_of` are those of tests/stem_head_cases.py.

Semantics.  x (B, H, W, C) holds `segments` critic calls of B / segments samples; G_eff = the largest divisor of B / segments that does
not exceed G; sample n belongs to group n // G_eff (contiguous groups; no group spans two segments because G_eff divides the segment).
Per group and feature j of J = H W C:  mu = mean_n x, d = x - mu, sigma = sqrt(mean_n d^2 + 1e-8), s = mean_j sigma.

Bound, per element:   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref,   C_ACC = 8
n_round counts the roundings applied AFTER the element's last addition (that addition's own rounding counts as one); absref carries the
roundings of the terms.  With A_j = mean_n |x[n, j]| (what the error of mu is relative to: d is a difference of values of that size),
cs = sum_n |gs_n| / (G J) (the coefficient's terms taken absolutely), and per feature
    e_d = |d| + A          a value of d with the error of mu in it
    k1  = A / sigma        how the relative error of sigma exceeds the 2^-24 of a well-conditioned one (1 + k1 in all)
  mbstd_fwd     s      the fp64 sum over j divided by J, rounded to fp32                                                           1
                       absref = mean_j (sigma + A): sigma's own chain is relative to sigma, the error of mu reaches sigma at most once
  mbstd_bwd     gx     gs_g / (G J) (the division), * d (d's subtraction is the last addition), / sigma                            4
                       absref = cs e_d / sigma + |gx| k1
  mbstd_bwdbwd  dgs    the fp64 sum of hd / sigma over j, divided by G J, rounded to fp32                                          1
                       absref = 1 / (G J) sum_j (1 + k1) HD / sigma,   HD = sum_n |h_n| e_d[n]
                dx     coef * fma(-d, curv, (h - hbar) / sigma): the fma's addition, the product                                  3
                       absref = cs ((|h| + mean_n |h|) / sigma (1 + k1) + e_d HD / (G sigma^3) (1 + 3 k1))
  stdfield_add  out    fma(scale s, T, c): the addition                                                                            1
                       absref = |c| + |scale s| Tabs,   Tabs = the sum of |w_std| over the taps inside
  stdfield_ds   gs     scale times the fp64 sum of the fp32 products g T, rounded to fp32                                          1
                       absref = |scale| sum |g| Tabs
  stdfield_dw   gw     scale times the fp64 sum of the fp32 products s g, rounded to fp32                                          1
                       absref = |scale| sum |s g| over the pixels whose tap is inside
At a feature where the group's values coincide sigma = 1e-4 and k1 is 1e4 |x|: the bound then says what it must -- one ulp of d over
sigma is an error the fp64 reference does not have.  The kernels sum the group in pairs so that d is exactly 0 for G_eff in {2, 4}
identical samples (family constant_group, used with those sizes only), and the GPU test asserts the exact zeros besides the bound.

RAISED, as in tests/stem_head_cases.py: the outputs whose emulated worst err / bound exceeds 0.5 with C_ACC = 8, with the next power of
two that brings it to 0.5 or below and the emulated ratio at that constant; tests/test_mbstd_bounds_cpu.py pins both.  No entry: the
emulated worst ratios are s 0.06, gx 0.21, dgs 0.02, dx 0.10, out 0.28, gs (field) 0.11, gw 0.14."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import pggan_oracle as O  # noqa: E402
from stem_head_cases import C_ACC, _fma, draws, ratio, seed_of  # noqa: E402,F401  (re-exported)

f32, f64 = np.float32, np.float64
EPS = 1e-8
RAISED = {}

# (B, segments, G): one group; two groups; G_eff = 3; G_eff = 1; groups stop at the segment boundary; one group of eight
GROUPING = [(4, 1, 4), (8, 1, 4), (6, 1, 4), (5, 1, 4), (8, 2, 4), (8, 1, 8)]
GROUPING_SHAPE = (4, 16)          # (H = W, C) of the grouping cases
# H = W: the centre tap alone; all four corner classes (every pixel a corner); the first interior pixel; the head's own size; 16.
# C: one quad; the lane-group widths' 16; 20 (J no multiple of a block's 1024 floats at any H here but 16); 128 (several blocks per group
# from H = 3 on: J = 1152, and 32 blocks at H = 16)
SIZES, WIDTHS = [1, 2, 3, 4, 16], [4, 16, 20, 128]
SHAPE_BATCHES = [(4, 1, 4), (8, 2, 4)]
FAMILIES = ["random", "pixelnormed", "large", "constant_group"]
BLOCK_FEATURES = 1024


def c_acc(name):
    return float(RAISED.get(name, (C_ACC, None))[0])


def group_size(batch, group):
    """the rule ops.mbstd_group_size implements, restated"""
    return max(g for g in range(1, min(batch, group) + 1) if batch % g == 0)


def cases():
    """(B, segments, G, H, C), without repeats"""
    out = [(b, s, g) + GROUPING_SHAPE for b, s, g in GROUPING]
    out += [(b, s, g, h, c) for b, s, g in SHAPE_BATCHES for h in SIZES for c in WIDTHS if (b, s, g, h, c) not in out]
    return out


def families_of(case):
    b, s, g = case[:3]
    return [f for f in FAMILIES if f != "constant_group" or group_size(b // s, g) in (2, 4)]


def inputs(family, case):
    """x, h (B, H, H, C); gs, s (B,); c, g (B, H, H, C); w_std (C, 1, 3, 3); scale.  pixelnormed: every pixel's channel vector has unit
    RMS (what the head sees after a merged block); large: x scaled by 1e3; constant_group: the samples of each group are bit-identical"""
    b, seg, grp, hh, ch = case
    shp = (b, hh, hh, ch)
    d = draws(seed_of(71 + FAMILIES.index(family), *case), x=shp, h=shp, gs=(b,), s_pos=(b,), c=shp, g=shp, w_std=(ch, 1, 3, 3))
    x = d["x"]
    if family == "pixelnormed":
        x = (x / np.sqrt((x.astype(f64) ** 2).mean(-1, keepdims=True))).astype(f32)
    elif family == "large":
        x = (x * f32(1e3)).astype(f32)
    elif family == "constant_group":
        ge = group_size(b // seg, grp)
        x = np.repeat(x[::ge], ge, axis=0).copy()
    d["x"] = np.ascontiguousarray(x)
    d["s"] = d.pop("s_pos")
    d["scale"] = float(f32(O.weight_scale((ch + 1) * 9, 0.2)))
    return d


# ---- the statistic and its derivatives: fp64 closed forms ------------------------------------------------------------------------------------
def _grouped(a, ge):
    a = np.asarray(a, f64)
    return a.reshape(a.shape[0] // ge, ge, -1)


def _stats(x, ge):
    xg = _grouped(x, ge)
    mu = xg.mean(1, keepdims=True)
    d = xg - mu
    sigma = np.sqrt((d * d).mean(1, keepdims=True) + EPS)
    return xg, d, sigma, np.abs(xg).mean(1, keepdims=True)


def _per_sample(v, ge):
    return np.repeat(np.asarray(v, f64).reshape(-1), ge)


def mbstd_fwd_ref(x, segments, group):
    ge = group_size(x.shape[0] // segments, group)
    _, _, sigma, A = _stats(x, ge)
    return {"s": (_per_sample(sigma.mean((1, 2)), ge), _per_sample((sigma + A).mean((1, 2)), ge), 1)}


def mbstd_bwd_ref(gs, x, segments, group):
    ge = group_size(x.shape[0] // segments, group)
    _, d, sigma, A = _stats(x, ge)
    J = d.shape[2]
    gsg = _grouped(gs, ge)
    coef, cs = gsg.sum(1, keepdims=True) / (ge * J), np.abs(gsg).sum(1, keepdims=True) / (ge * J)
    gx = coef * d / sigma
    a = cs * (np.abs(d) + A) / sigma + np.abs(gx) * (A / sigma)
    return {"gx": (gx.reshape(x.shape), a.reshape(x.shape), 4)}


def mbstd_bwdbwd_ref(h, gs, x, segments, group):
    ge = group_size(x.shape[0] // segments, group)
    _, d, sigma, A = _stats(x, ge)
    J = d.shape[2]
    hg, gsg = _grouped(h, ge), _grouped(gs, ge)
    coef, cs = gsg.sum(1, keepdims=True) / (ge * J), np.abs(gsg).sum(1, keepdims=True) / (ge * J)
    hbar, habs = hg.mean(1, keepdims=True), np.abs(hg).mean(1, keepdims=True)
    hd = (hg * d).sum(1, keepdims=True)
    e_d, k1 = np.abs(d) + A, A / sigma
    HD = (np.abs(hg) * e_d).sum(1, keepdims=True)
    dgs = (hd / sigma).sum((1, 2)) / (ge * J)
    dgs_a = ((1 + k1) * HD / sigma).sum((1, 2)) / (ge * J)
    dx = coef * ((hg - hbar) / sigma - d * hd / (ge * sigma ** 3))
    dx_a = cs * ((np.abs(hg) + habs) / sigma * (1 + k1) + e_d * HD / (ge * sigma ** 3) * (1 + 3 * k1))
    return {"dgs": (_per_sample(dgs, ge), _per_sample(dgs_a, ge), 1), "dx": (dx.reshape(x.shape), dx_a.reshape(x.shape), 3)}


# ---- the field family: fp64 --------------------------------------------------------------------------------------------------------
def tap_masks(hh, ww):
    """(3, 3, H, W): 1 where the source pixel of tap (ky, kx) at (y, x) is inside the image"""
    m = np.zeros((3, 3, hh, ww))
    for ky in range(3):
        for kx in range(3):
            ys = [y for y in range(hh) if 0 <= y + ky - 1 < hh]
            xs = [x for x in range(ww) if 0 <= x + kx - 1 < ww]
            m[ky, kx][np.ix_(ys, xs)] = 1.0
    return m


def field_T(w_std, hh, ww):
    """T (H, W, C) and its absolute twin"""
    w = np.asarray(w_std, f64)[:, 0]                  # (C, 3, 3)
    m = tap_masks(hh, ww)
    return np.einsum("cij,ijyx->yxc", w, m), np.einsum("cij,ijyx->yxc", np.abs(w), m)


def stdfield_add_ref(c, s, w_std, scale):
    T, Ta = field_T(w_std, c.shape[1], c.shape[2])
    k = float(scale) * np.asarray(s, f64)[:, None, None, None]
    return {"out": (np.asarray(c, f64) + k * T, np.abs(np.asarray(c, f64)) + np.abs(k) * Ta, 1)}


def stdfield_ds_ref(g, w_std, scale):
    T, Ta = field_T(w_std, g.shape[1], g.shape[2])
    g = np.asarray(g, f64)
    return {"gs": (float(scale) * (g * T).sum((1, 2, 3)), abs(float(scale)) * (np.abs(g) * Ta).sum((1, 2, 3)), 1)}


def stdfield_dw_ref(g, s, scale):
    m = tap_masks(g.shape[1], g.shape[2])
    sg = np.asarray(s, f64)[:, None, None, None] * np.asarray(g, f64)
    gw = float(scale) * np.einsum("nyxc,ijyx->cij", sg, m)
    ga = abs(float(scale)) * np.einsum("nyxc,ijyx->cij", np.abs(sg), m)
    return {"gw": (gw[:, None], ga[:, None], 1)}


# ---- the concat formulation in torch (any dtype; fp64 is the truth) ------------------------------------------------------------------------
def mbstd_torch(x, segments, group):
    """s (B,) of x (B, ...): what the closed forms and the kernels are held to, differentiable by torch.autograd at every order"""
    b = x.shape[0]
    ge = group_size(b // segments, group)
    xg = x.reshape(b // ge, ge, -1)
    sigma = torch.sqrt(((xg - xg.mean(1, keepdim=True)) ** 2).mean(1) + EPS)
    return sigma.mean(1).repeat_interleave(ge)


def concat_head(y, w, w_std, bias, slope, segments, group):
    """the head conv on cat([y, s plane]) (NCHW): Conv2d_normalized(C + 1, C, 3) on the concatenated tensor, pre-activation"""
    s = mbstd_torch(y, segments, group)
    plane = s.reshape(-1, 1, 1, 1).expand(-1, 1, y.shape[2], y.shape[3])
    return O.scaled_conv(torch.cat([y, plane], 1), torch.cat([w, w_std], 1), bias, slope, 1)


def mbstd_discriminator_forward(params, x, spec, group, segments=1):
    """oracle.pggan_oracle.discriminator_forward with the minibatch standard-deviation channel in front of the head conv; params holds
    'layers.<k>.weight_std' beside the default critic's keys"""
    if spec.alpha < 1:
        y_start = O.from_image(O.pool2(x), params["FromIm.conv.weight"], params["FromIm.conv.bias"])
        last = max(O._block_indices(params, "conv_block_list"))
        last_from = max(int(k.split(".")[1]) for k in params if k.startswith("FromIm_list."))
        y_end = O.from_image(x, params[f"FromIm_list.{last_from}.conv.weight"], params[f"FromIm_list.{last_from}.conv.bias"])
        y_end = O.scale_block(y_end, params[f"conv_block_list.{last}.1.weight"], params[f"conv_block_list.{last}.4.weight"], "down", spec.slope)
        y = y_start + spec.alpha * (y_end - y_start)
    else:
        y = O.from_image(x, params["FromIm.conv.weight"], params["FromIm.conv.bias"])
    merged = O._block_indices(params, "layers")
    for i in merged:
        y = O.scale_block(y, params[f"layers.{i}.1.weight"], params[f"layers.{i}.4.weight"], "down", spec.slope)
    k = len(merged)
    c = concat_head(y, params[f"layers.{k}.weight"], params[f"layers.{k}.weight_std"], params[f"layers.{k}.bias"], spec.slope, segments, group)
    y = O.pixel_norm(O.lrelu(c, spec.slope))
    return O.scaled_conv(y, params[f"layers.{k + 3}.weight"], params[f"layers.{k + 3}.bias"], spec.slope, 0).flatten(1)


# ---- numpy fp32 emulations of the kernels' arithmetic (csrc/mbstd_bits.h; the sums over j are fp64 in the kernels: any order) ------------------
def _pair_sum32(v):
    """(ng, G, J) fp32 -> (ng, J): (v0 + v1) + (v2 + v3) .., the odd one last"""
    s = np.zeros((v.shape[0], v.shape[2]), f32)
    n = 0
    while n + 1 < v.shape[1]:
        s = s + (v[:, n] + v[:, n + 1])
        n += 2
    if n < v.shape[1]:
        s = s + v[:, n]
    return s


def _stats32(x, ge):
    xg = np.asarray(x, f32).reshape(x.shape[0] // ge, ge, -1)
    mu = _pair_sum32(xg) / f32(ge)
    d = xg - mu[:, None]
    q = np.zeros_like(mu)
    for n in range(ge):
        q = _fma(d[:, n], d[:, n], q)
    sigma = np.sqrt(q / f32(ge) + f32(EPS)).astype(f32)
    return xg, d, mu, sigma


def _coef32(gs, ge, J):
    g = np.asarray(gs, f32).reshape(-1, ge, 1)
    return _pair_sum32(g)[:, 0] / (f32(ge) * f32(J))


def mbstd_fwd_emulate(x, segments, group):
    ge = group_size(x.shape[0] // segments, group)
    _, _, _, sigma = _stats32(x, ge)
    return {"s": np.repeat((sigma.astype(f64).sum(1) / sigma.shape[1]).astype(f32), ge)}


def mbstd_bwd_emulate(gs, x, segments, group):
    ge = group_size(x.shape[0] // segments, group)
    _, d, _, sigma = _stats32(x, ge)
    coef = _coef32(gs, ge, d.shape[2])
    return {"gx": ((coef[:, None, None] * d).astype(f32) / sigma[:, None]).astype(f32).reshape(x.shape)}


def mbstd_bwdbwd_emulate(h, gs, x, segments, group):
    ge = group_size(x.shape[0] // segments, group)
    _, d, _, sigma = _stats32(x, ge)
    J = d.shape[2]
    coef = _coef32(gs, ge, J)
    hg = np.asarray(h, f32).reshape(d.shape)
    hbar = _pair_sum32(hg) / f32(ge)
    hd = np.zeros_like(hbar)
    for n in range(ge):
        hd = _fma(hg[:, n], d[:, n], hd)
    curv = hd / (f32(ge) * ((sigma * sigma).astype(f32) * sigma).astype(f32))
    a = ((hg - hbar[:, None]) / sigma[:, None]).astype(f32)
    dx = (coef[:, None, None] * _fma(-d, curv[:, None], a)).astype(f32)
    dgs = ((hd / sigma).astype(f32).astype(f64).sum(1) / (float(ge) * float(J))).astype(f32)
    return {"dgs": np.repeat(dgs, ge), "dx": dx.reshape(x.shape)}


def _field_T32(w_std, hh, ww):
    """T (H, W, C) in fp32, the taps added in (ky, kx) order as mbstd::field_taps adds them"""
    w = np.asarray(w_std, f32)[:, 0]
    m = tap_masks(hh, ww)
    t = np.zeros((hh, ww, w.shape[0]), f32)
    for ky in range(3):
        for kx in range(3):
            t = np.where(m[ky, kx][:, :, None] > 0, t + w[None, None, :, ky, kx], t).astype(f32)
    return t


def stdfield_add_emulate(c, s, w_std, scale):
    k = (f32(scale) * np.asarray(s, f32))[:, None, None, None]
    return {"out": _fma(k, _field_T32(w_std, c.shape[1], c.shape[2])[None], np.asarray(c, f32))}


def stdfield_ds_emulate(g, w_std, scale):
    p = (np.asarray(g, f32) * _field_T32(w_std, g.shape[1], g.shape[2])[None]).astype(f32)
    return {"gs": (float(f32(scale)) * p.astype(f64).sum((1, 2, 3))).astype(f32)}


def stdfield_dw_emulate(g, s, scale):
    p = (np.asarray(s, f32)[:, None, None, None] * np.asarray(g, f32)).astype(f32).astype(f64)
    return {"gw": (float(f32(scale)) * np.einsum("nyxc,ijyx->cij", p, tap_masks(g.shape[1], g.shape[2])))[:, None].astype(f32)}


def concat_conv_field(c_in, s, w, w_std, scale):
    """F.conv2d on the concatenated (C + 1)-channel tensor, in the dtype of its arguments (NCHW): what the field form must equal"""
    plane = s.reshape(-1, 1, 1, 1).expand(-1, 1, c_in.shape[2], c_in.shape[3])
    return F.conv2d(scale * torch.cat([c_in, plane], 1), torch.cat([w, w_std], 1), None, padding=1)
