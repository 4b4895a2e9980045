"""Differentiable operators of the WGAN nets (reference models.py:728-790) over the stride-2 kernels of csrc/stride2.hip.

First order only (the WGAN recipe has no gradient penalty, so nothing is differentiated twice).  Tensors are channels-last fp32 on the
GPU.  A layer's BatchNorm2d -> LeakyReLU is applied by its CONSUMER while it loads (`S2Conv`, `BNActHead`), so the producing layer
writes its raw convolution output and the normalised activation is never stored, except once in front of the critic's Linear head.

    Stem       Generator_wgan's Linear, outputs permuted NCHW -> NHWC              (z, W, b) -> y
    S2Conv     [BatchNorm2d ->] [LeakyReLU ->] Conv2d / ConvTranspose2d (k4, s2, p1) [-> Tanh]
    BNActHead  [BatchNorm2d ->] LeakyReLU -> Flatten -> Linear(-> 1)                (the critic's score)

Inside `ops.inputs_only()`, or for parameters with requires_grad False, weight / bias / affine gradients are not computed (the
generator step back-propagates through the critic for its input gradient only).  Every reduction is deterministic: eager runs and
replayed graphs give the same bits.

Inside `synchronised(handle)` (WGANTrainer with sync_batchnorm=True) a training-mode BatchNorm2d normalises with the statistics of
all ranks' inputs to that call, and its backward with the ranks' summed Σgz, Σgz·x̂: one all-gather of a small fp64 record per forward
and one per backward (ngan_bn_moments -> ngan_bn_merge_fold, ngan_bn_act_bwd_partial -> ngan_bn_act_bwd_merged).
"""
import contextlib

import torch
import torch.distributed as dist
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _C, ops


def _empty(n, like):
    return torch.empty(int(n), device=like.device, dtype=torch.float32)


def _check(t, name):
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: the WGAN kernels run in fp32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def pack(weight, m, c, up):
    wp = _empty(_C.lib().ngan_s2_packed_floats(m, c), weight)
    _C.call("ngan_s2_pack", weight.detach(), wp, m, c, int(up))
    return wp


def conv(x, weight, bias, up, xform=None, tanh=False):
    """x (B, H, W, C) -> down: (B, H/2, W/2, M), up: (B, 2H, 2W, M); weight in torch layout (Conv2d [M][C], ConvTranspose2d [C][M]);
    xform = (scale, shift, act, slope) applied to x on load, or None"""
    x = _check(x, "s2 conv")
    b, h, w, c = x.shape
    m = weight.shape[1] if up else weight.shape[0]
    assert (weight.shape[0] if up else weight.shape[1]) == c, (tuple(weight.shape), c)
    wp = pack(weight, m, c, up)
    oh, ow = (2 * h, 2 * w) if up else (h // 2, w // 2)
    y = torch.empty((b, oh, ow, m), device=x.device, dtype=torch.float32)
    scale, shift, act, slope = xform if xform is not None else (None, None, 0, 0.0)
    _C.call("ngan_s2_conv", x, wp, None if bias is None else bias.detach(), scale, shift, int(act), float(slope), y, b, h, w, c, m,
            int(up), int(tanh))
    return y


def dgrad(g, weight, up):
    """input gradient of conv(., weight, up): the adjoint pass with the same weight tensor"""
    g = _check(g, "s2 dgrad")
    b, h, w, m = g.shape
    c = weight.shape[0] if up else weight.shape[1]
    # down layer (weight [M][C]): up pass from M to C channels; up layer (weight [C][M]): down pass from M to C channels
    wp = pack(weight, c, m, not up)
    oh, ow = (h // 2, w // 2) if up else (2 * h, 2 * w)
    gx = torch.empty((b, oh, ow, c), device=g.device, dtype=torch.float32)
    _C.call("ngan_s2_conv", g, wp, None, None, None, 0, 0.0, gx, b, h, w, m, c, int(not up), 0)
    return gx


def wgrad(half, full, w_shape, half_xf=None, full_xf=None):
    """dW[h][f][4][4] = correlation of half (B, Hh, Wh, CH) with full (B, 2Hh, 2Wh, CF) (see include/ngan.h, ngan_s2_wgrad)"""
    half, full = _check(half, "s2 wgrad"), _check(full, "s2 wgrad")
    b, hh, wh, ch = half.shape
    cf = full.shape[3]
    assert full.shape[1] == 2 * hh and full.shape[2] == 2 * wh and tuple(w_shape) == (ch, cf, 4, 4), (half.shape, full.shape, w_shape)
    dw = torch.empty(w_shape, device=half.device, dtype=torch.float32)
    work = _empty(_C.lib().ngan_s2_wgrad_workspace_floats(b, hh, wh, ch, cf), half)
    hs, hsh, ha, _ = half_xf if half_xf is not None else (None, None, 0, 0.0)
    fs, fsh, fa, _ = full_xf if full_xf is not None else (None, None, 0, 0.0)
    slope = (half_xf or full_xf or (None, None, 0, 0.0))[3]
    _C.call("ngan_s2_wgrad", half, full, hs, hsh, int(ha), fs, fsh, int(fa), float(slope), dw, work, b, hh, wh, ch, cf)
    return dw


def chan_sum(g):
    g = _check(g, "chan_sum")
    c = g.shape[-1]
    npix = g.numel() // c
    out = _empty(c, g)
    _C.call("ngan_chan_sum", g, npix, c, out, _empty(_C.lib().ngan_chan_reduce_workspace_floats(npix, c), g))
    return out


class SyncBN:
    """What a synchronised BatchNorm call needs: the process group, its size, this rank's index in it, and `run(fn)`, which issues the
    collectives of fn (the trainer's communication-stream runner)."""

    def __init__(self, group, world, rank, run):
        self.group, self.world, self.rank, self.run = group, int(world), int(rank), run

    def gather(self, rec):
        """all ranks' records, concatenated in rank order"""
        out = torch.empty(self.world * rec.numel(), device=rec.device, dtype=rec.dtype)
        self.run(lambda: dist.all_gather_into_tensor(out, rec, group=self.group))
        return out


_sync = None      # the SyncBN handle of the innermost `synchronised` block; None: per-call batch statistics


@contextlib.contextmanager
def synchronised(handle):
    global _sync
    prev, _sync = _sync, handle
    try:
        yield
    finally:
        _sync = prev


class BNSpec:
    """The BatchNorm2d in front of a consumer: its module (buffers updated in place) and whether it runs on batch statistics.
    `sync` is the SyncBN handle current when the forward built this spec; the backward, which autograd runs on another thread, uses the
    same one."""

    def __init__(self, module):
        self.module = module
        self.sync = _sync
        self.n_total = None       # synchronised: the global pixel count (one double on the device) the backward divides by

    def fold(self, y, gamma, beta):
        """(scale, shift, mean, rstd): the on-load transform; mean / rstd are None in eval mode"""
        bn = self.module
        c = y.shape[-1]
        scale, shift = _empty(c, y), _empty(c, y)
        if bn.training:
            npix = y.numel() // c
            mean, rstd = _empty(c, y), _empty(c, y)
            track = bn.track_running_stats and bn.running_mean is not None
            if bn.momentum is None:
                raise NotImplementedError("BatchNorm2d(momentum=None) (cumulative average) is not supported")
            momentum = bn.momentum
            work = _empty(_C.lib().ngan_chan_reduce_workspace_floats(npix, c), y)
            if self.sync is not None:
                rec = torch.empty(1 + 2 * c, device=y.device, dtype=torch.float64)
                _C.call("ngan_bn_moments", y, npix, c, rec, work)
                recs = self.sync.gather(rec)
                self.n_total = torch.empty(1, device=y.device, dtype=torch.float64)
                _C.call("ngan_bn_merge_fold", recs, self.sync.world, c, gamma.detach(), beta.detach(), mean, rstd, scale, shift,
                        bn.running_mean if track else None, bn.running_var if track else None, bn.num_batches_tracked if track else None,
                        float(momentum), float(bn.eps), self.n_total)
                return scale, shift, mean, rstd
            _C.call("ngan_bn_stats", y, npix, c, gamma.detach(), beta.detach(), mean, rstd, scale, shift,
                    bn.running_mean if track else None, bn.running_var if track else None, bn.num_batches_tracked if track else None,
                    float(momentum), float(bn.eps), work)
            return scale, shift, mean, rstd
        _C.call("ngan_bn_fold_eval", gamma.detach(), beta.detach(), bn.running_mean, bn.running_var, float(bn.eps), scale, shift, c)
        return scale, shift, None, None


def _bn_act_backward(ctx, y, ga, scale, shift, mean, rstd, gamma, want_affine):
    """gradient w.r.t. the raw tensor y of act(BN(y)) given ga w.r.t. the activation; (gy, dgamma, dbeta)"""
    c = y.shape[-1]
    npix = y.numel() // c
    if ctx.bn is None and not ctx.act:
        return ga, None, None
    if ctx.bn is not None and mean is None:
        raise RuntimeError("backward through an eval-mode BatchNorm2d is not supported by the WGAN kernels (training runs in train mode)")
    gy = torch.empty_like(y)
    dgamma = _empty(c, y) if want_affine else None
    dbeta = _empty(c, y) if want_affine else None
    sync = ctx.bn.sync if ctx.bn is not None else None
    if sync is not None:
        ga = _check(ga, "bn backward")
        rec = torch.empty(2 * c, device=y.device, dtype=torch.float64)
        _C.call("ngan_bn_act_bwd_partial", y, ga, scale, shift, mean, rstd, int(ctx.act), float(ctx.slope), npix, c, rec,
                _empty(_C.lib().ngan_chan_reduce_workspace_floats(npix, c), y))
        recs = sync.gather(rec)
        _C.call("ngan_bn_act_bwd_merged", y, ga, scale, shift, mean, rstd, gamma.detach(), int(ctx.act), float(ctx.slope), npix, c, recs,
                sync.world, sync.rank, ctx.bn.n_total, gy, dgamma, dbeta, _empty(3 * c, y))
        return gy, dgamma, dbeta
    work = _empty(_C.lib().ngan_bn_act_bwd_workspace_floats(npix, c), y) if ctx.bn is not None else None
    _C.call("ngan_bn_act_bwd", y, _check(ga, "bn backward"), scale, shift, mean, rstd, gamma.detach() if ctx.bn is not None else None,
            int(ctx.act), float(ctx.slope), npix, c, gy, dgamma, dbeta, work)
    return gy, dgamma, dbeta


class S2Conv(Function):
    """[BatchNorm2d ->] [LeakyReLU ->] Conv2d(k4, s2, p1) (up=False) or ConvTranspose2d(k4, s2, p1) (up=True), + bias [-> Tanh].
    x is the RAW output of the previous layer; gamma / beta are None without BatchNorm."""

    @staticmethod
    def forward(ctx, x, gamma, beta, weight, bias, bn, act, slope, up, tanh):
        x = _check(x, "S2Conv")
        ctx.bn, ctx.act, ctx.slope, ctx.up, ctx.tanh = bn, bool(act), float(slope), bool(up), bool(tanh)
        scale = shift = mean = rstd = None
        if bn is not None:
            scale, shift, mean, rstd = bn.fold(x, gamma, beta)
        xform = (scale, shift, int(act), float(slope)) if (bn is not None or act) else None
        y = conv(x, weight, bias, up, xform, tanh)
        ctx.save_for_backward(x, gamma, weight, y if tanh else None, scale, shift, mean, rstd)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, gamma, weight, t, scale, shift, mean, rstd = ctx.saved_tensors
        g = _check(g, "S2Conv backward")
        if ctx.tanh:
            gp = torch.empty_like(g)
            _C.call("ngan_tanh_bwd", t, g, gp, g.numel())
            g = gp
        params = ops._param_grads_wanted()
        want_w = params and ctx.needs_input_grad[3]
        want_b = params and ctx.has_bias and ctx.needs_input_grad[4]
        want_affine = params and ctx.bn is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        gx = dgamma = dbeta = gw = gb = None
        if want_w:
            xform = (scale, shift, int(ctx.act), ctx.slope) if (ctx.bn is not None or ctx.act) else None
            if ctx.up:     # ConvTranspose2d: half = transformed input, full = output gradient
                gw = wgrad(x, g, tuple(weight.shape), half_xf=xform)
            else:          # Conv2d: half = output gradient, full = transformed input
                gw = wgrad(g, x, tuple(weight.shape), full_xf=xform)
        if want_b:
            gb = chan_sum(g)
        if ctx.needs_input_grad[0] or want_affine:
            ga = dgrad(g, weight, ctx.up)
            gx, dgamma, dbeta = _bn_act_backward(ctx, x, ga, scale, shift, mean, rstd, gamma, want_affine)
            if not ctx.needs_input_grad[0]:
                gx = None
        return gx, dgamma, dbeta, gw, gb, None, None, None, None, None


class BNActHead(Function):
    """[BatchNorm2d ->] LeakyReLU -> Flatten (NCHW order) -> Linear(C*S*S -> 1): the critic's score (B, 1).  The Linear weight
    [1, C*S*S] is read in its NCHW order by ngan_final_dot_* on the channels-last activation."""

    @staticmethod
    def forward(ctx, x, gamma, beta, weight, bias, bn, slope):
        x = _check(x, "BNActHead")
        ctx.bn, ctx.act, ctx.slope = bn, True, float(slope)
        b, h, w, c = x.shape
        scale = shift = mean = rstd = None
        if bn is not None:
            scale, shift, mean, rstd = bn.fold(x, gamma, beta)
        a = torch.empty_like(x)
        _C.call("ngan_bn_act_apply", x, scale, shift, 1, float(slope), b * h * w, c, a)
        out = torch.empty((b, 1), device=x.device, dtype=torch.float32)
        _C.call("ngan_final_dot_fwd", a, weight.detach(), bias.detach(), out, b, h * w, c, 1.0)
        ctx.save_for_backward(x, a, gamma, weight, scale, shift, mean, rstd)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, go):
        x, a, gamma, weight, scale, shift, mean, rstd = ctx.saved_tensors
        go = _check(go, "BNActHead backward")
        b, h, w, c = x.shape
        params = ops._param_grads_wanted()
        want_affine = params and ctx.bn is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        gx = dgamma = dbeta = gw = gb = None
        if params and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4]):
            gw, gb = torch.empty_like(weight), _empty(1, x)
            _C.call("ngan_final_dot_dw", a, go, gw, gb, b, h * w, c, 1.0)
            gw = gw if ctx.needs_input_grad[3] else None
            gb = gb if ctx.needs_input_grad[4] else None
        if ctx.needs_input_grad[0] or want_affine:
            ga = torch.empty_like(x)
            _C.call("ngan_final_dot_dx", go, weight.detach(), ga, b, h * w, c, 1.0)
            gx, dgamma, dbeta = _bn_act_backward(ctx, x, ga, scale, shift, mean, rstd, gamma, want_affine)
            if not ctx.needs_input_grad[0]:
                gx = None
        return gx, dgamma, dbeta, gw, gb, None, None


class Stem(Function):
    """Linear(K -> C*S) with bias, then Unflatten to (C, s, s): written channels-last, (B, s, s, C)"""

    @staticmethod
    def forward(ctx, z, weight, bias, s, c):
        z = _check(z, "Stem")
        b, k = z.shape
        y = torch.empty((b, s, s, c), device=z.device, dtype=torch.float32)
        _C.call("ngan_wgan_stem_fwd", z, weight.detach(), bias.detach(), y, b, k, s * s, c)
        ctx.save_for_backward(z, weight)
        ctx.sc = (s, c)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        z, weight = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("the latent input of Generator_wgan takes no gradient on the HIP path")
        s, c = ctx.sc
        b, k = z.shape
        gw = gb = None
        if ops._param_grads_wanted() and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]):
            gw, gb = torch.empty_like(weight), _empty(weight.shape[0], z)
            _C.call("ngan_wgan_stem_grad", z, _check(g, "Stem backward"), gw, gb, b, k, s * s, c)
            gw = gw if ctx.needs_input_grad[1] else None
            gb = gb if ctx.needs_input_grad[2] else None
        return None, gw, gb, None, None
