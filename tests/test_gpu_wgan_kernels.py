"""The WGAN kernels of csrc/stride2.hip per element against fp64: the stride-2 convolutions with their three gradients, the channel
reductions (BatchNorm statistics, stored activation, BatchNorm backward, bias gradient), the eval-mode fold, the stem and the two
pointwise kernels, on the cases of tests/wgan_cases.py through wgan_ops (conv / dgrad / wgrad / chan_sum / BNSpec.fold /
_bn_act_backward) or the C ABI (stem, bn_fold_eval, tanh_bwd, bn_act_apply).  Per element
    |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref,   C_ACC = 8
with absref, n_round and the raised constants of tests/wgan_cases.py, settled on the CPU by tests/test_wgan_bounds_cpu.py (every
emulated ratio <= 0.5) and never against a kernel.  Every output, and every workspace wgan_ops allocates on the way, lies between two
guards of 64 sentinel floats that must come back intact; outputs start as NaN and none may be left.  num_batches_tracked and the
running buffers of a BatchNorm that does not track are compared exactly.

What each gap of the earlier suite maps to (case ids as pytest prints them):
  local mistakes under a max-norm         every test: the bound is per element, with the absolute-value twin as its floor
  square images only                      down/up-g45-* (3 x 5), -narrow-* (8 x 2), -strip-* (2 x 40); K297-* (9 x 11); the autograd stack (2 x 8)
  C % 4 == 0, C % 16 != 0                 *-C4-*, *-C12-*, *-C20-* (and CF / CH = 20 in K*-CH20-CF33-*)
  M just past a tile                      *-M17-* (MT = 2, one live row), *-M33-* (MT = 4), *-M65-* (second blockIdx.y, one live row)
  CH / CF off the 16 grid                 K*-CH1-CF17-*, K*-CH17-CF3-*, K*-CH20-CF33-*; every conv case's dw
  transforms other than affine + act      *-none-*, *-act-* (scale == nullptr), *-affine-*; K*-half-*, K*-full-*, K*-neither-*
  chan_reduce_stage1 sizes                C257 / C300 / C513 (strided passes, ragged last), C5 / C100 / C129 (idle threads), npix1 / 2 / 7
                                          (below the lane count), npix = chunk + 1, C1024-npix16400 (re-chunking)
  statistics edges                        channels 3..5 (pixel 0 six sigma out), channel 1 (constant), npix1, track off, momentum 0.37,
                                          eps 1e-3: spread over the C*-npix* cases (wgan_cases.red_options / red_inputs)
  entry points without a kernel test      test_stem_*, test_bn_fold_eval, C257-npix64 ... (chan_sum at C > 256), the act_only and
                                          want_affine = False backward modes of test_channel_reductions

The statistics cases forced one kernel change: ngan_bn_stats formed the variance in fp32 from sums shifted by pixel 0,
s1 / n - (s0 / n)^2, which cancels when pixel 0 lies far from the channel mean.  With it
14 of the 45 C*-npix* cases failed (every one with a six-sigma channel and more than a few pixels), worst C5-npix3278 (channel 4: mean / sigma = 3, pixel 0 six sigma out): rstd 12.70, scale 11.12,
shift 16.62 times the bound, running_var 9.25 at C300-npix56, mean 2.85 at C129-npix129 -- where the fp32 emulation of that form puts
them (13.44 / 11.76 / 17.61 / 8.86 / 2.85).  ngan_bn_stats now forms the two sums in fp64 beside the fp32 ones (bn_stats_stage1) and
keeps an fp32 moment only where the fp64 one confirms it (bn_stats_finish: the variance within 2^-22, the mean within 2^-23 of
|mean| + sigma), so ordinary data give the bits they gave before and the six-sigma channels the fp64 moments: the same cases give rstd
0.24, scale 0.24, shift 0.46, running_var 0.44, mean 0.42.  (The fp64 moments everywhere give 0.07 .. 0.32, but move the one-pass results
by an ulp in most channels, which tests/test_gpu_wgan.py::test_matches_wgan_full_fixture's Adam step does not forgive.)

measured on MI355X (a record, not a bound: worst err / bound per operator over its cases): s2_down y 0.50 dx 0.40
dw 0.46 db 0.14; s2_up y 0.49 dx 0.42 dw 0.48 db 0.14; s2_wgrad 0.37; chan_sum 0.32; bn_stats mean 0.42 rstd 0.24 scale 0.24 shift 0.46
running_mean 0.35 running_var 0.44; bn_act_apply 0.16; bn_act_bwd with BatchNorm and activation gy 0.24 dgamma 0.28 dbeta 0.30, without
activation 0.25 / 0.25 / 0.30, activation only 0.12; bn_fold_eval scale 0.12 shift 0.17; tanh_bwd 0.09; stem y 0.15 gw 0.42 gb 0.20.
The convolutions sit where the sequential emulation does (0.50 / 0.47).  The module takes about 5 s."""
import copy
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import wgan_cases as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SLOPE = W.SLOPE
GUARD = 64
SENTINEL = 12345.0


def dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


class Guarded:
    """Device buffers between two guards of GUARD sentinel elements, NaN inside (integers: a sentinel inside as well).  Stands in for
    torch.empty / torch.empty_like inside wgan_ops for the length of a test, so the outputs and workspaces it allocates are guarded too."""

    def __init__(self):
        self.bufs = []

    def alloc(self, shape, dtype=torch.float32):
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape)) if shape else 1
        raw = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV, dtype=dtype)
        body = raw[GUARD:GUARD + n]
        if dtype.is_floating_point:
            body.fill_(float("nan"))
        self.bufs.append((raw, n))
        return body.view(shape)

    def verify(self):
        for raw, n in self.bufs:
            lo, hi = raw[:GUARD], raw[GUARD + n:]
            assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), ("guard overwritten", n)
        self.bufs = []


class _TorchProxy:
    def __init__(self, guarded):
        self._g = guarded

    def __getattr__(self, k):
        return getattr(torch, k)

    def empty(self, *size, device=None, dtype=torch.float32):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = size[0]
        return self._g.alloc(size, dtype)

    def empty_like(self, t):
        return self._g.alloc(t.shape, t.dtype)


@pytest.fixture
def wops(ngan):
    import neuron_gan_amd.wgan_ops as wgan_ops
    return wgan_ops


@pytest.fixture
def guarded(wops, monkeypatch):
    g = Guarded()
    monkeypatch.setattr(wops, "torch", _TorchProxy(g))
    yield g
    g.verify()


class Checker:
    """collects err / bound of every output of one case and asserts at the end, so that one run shows every figure"""

    def __init__(self, cid):
        self.cid, self.bad = cid, []

    def __call__(self, name, got, ref):
        r, a, n = ref
        g = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
        assert not np.isnan(g).any(), (name, self.cid, "an element was never written")
        worst, idx = W.ratio_at(g, r, a, n, W.c_acc(name, self.cid))
        print(f"STAT wgan {name} {self.cid}: {worst:.3f}")
        if not worst <= 1.0:
            self.bad.append((name, round(worst, 3), tuple(int(i) for i in np.unravel_index(idx, r.shape))))

    def done(self):
        assert not self.bad, (self.cid, self.bad)


def dev_xf(xf):
    return None if xf is None else (dv(xf[0]), dv(xf[1]), xf[2], SLOPE)


# ---- the stride-2 convolutions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.CONV_CASES, ids=W.conv_id)
def test_s2_conv_and_its_gradients(wops, guarded, case):
    """forward with the on-load transform, bias and tanh of the case; then, on one output gradient g, the input gradient (the opposite
    pass), the weight gradient (the transform on the side of the layer's input) and the bias gradient"""
    d = W.conv_inputs(case)
    refs = W.conv_refs(d)
    ck = Checker(W.conv_id(case))
    up, xf = d["up"], dev_xf(d["xf"])
    x, w, g = dv(d["x"]), dv(d["w"]), dv(d["g"])
    tag = f"s2_{case[0]}"
    ck(f"{tag}/y", wops.conv(x, w, dv(d["bias"]), up, xf, d["tanh"]), refs["y"])
    ck(f"{tag}/dx", wops.dgrad(g, w, up), refs["dx"])
    dw = wops.wgrad(x, g, tuple(w.shape), half_xf=xf) if up else wops.wgrad(g, x, tuple(w.shape), full_xf=xf)
    ck(f"{tag}/dw", dw, refs["dw"])
    ck(f"{tag}/db", wops.chan_sum(g), refs["db"])
    guarded.verify()
    ck.done()


@pytest.mark.parametrize("case", W.WGRAD_CASES, ids=W.wgrad_id)
def test_s2_wgrad(ngan, wops, guarded, case):
    d = W.wgrad_inputs(case)
    B, Hh, Wh, CH = d["half"].shape
    CF = d["full"].shape[3]
    nsplit, _, floats = W.wgrad_plan(B, Hh, Wh, CH, CF)
    assert nsplit == {1: 1, 45: 1, 297: 3}[case[0]]
    assert ngan._C.lib().ngan_s2_wgrad_workspace_floats(B, Hh, Wh, CH, CF) == floats
    ck = Checker(W.wgrad_id(case))
    dw = wops.wgrad(dv(d["half"]), dv(d["full"]), (CH, CF, 4, 4), half_xf=dev_xf(d["half_xf"]), full_xf=dev_xf(d["full_xf"]))
    ck("s2_wgrad/dw", dw, W.wgrad_refs(d)["dw"])
    guarded.verify()
    ck.done()


# ---- channel reductions and BatchNorm --------------------------------------------------------------------------------------------
class Kernels:
    """wgan_cases.red_chain's `impl` over the kernels: BNSpec.fold on a stock BatchNorm2d, ngan_bn_act_apply, _bn_act_backward, chan_sum"""

    def __init__(self, ngan, wops, guarded, d, o):
        self.ngan, self.wops, self.guarded, self.track = ngan, wops, guarded, o["track"]
        C = d["y"].shape[1]
        self.bn = nn.BatchNorm2d(C, eps=o["eps"], momentum=o["momentum"]).to(DEV)
        with torch.no_grad():
            self.bn.weight.copy_(dv(d["gamma"]))
            self.bn.bias.copy_(dv(d["beta"]))
            self.bn.running_mean.copy_(dv(d["run_mean"]))
            self.bn.running_var.copy_(dv(d["run_var"]))
        self.bn.track_running_stats = self.track       # the buffers stay: a BatchNorm that does not track must leave them alone
        self.start = (self.bn.running_mean.clone(), self.bn.running_var.clone())
        self.spec = None

    def stats(self, y, gamma, beta, eps, momentum, run_mean, run_var):
        self.spec = self.wops.BNSpec(self.bn)
        self.dev = dict(zip(("scale", "shift", "mean", "rstd"), self.spec.fold(dv(y), self.bn.weight, self.bn.bias)))
        out = {k: host(v) for k, v in self.dev.items()}
        if self.track:
            out.update(running_mean=host(self.bn.running_mean), running_var=host(self.bn.running_var))
        return out

    def apply(self, y, scale, shift, act):
        npix, C = y.shape
        a = self.guarded.alloc((npix, C))
        self.ngan._C.call("ngan_bn_act_apply", dv(y), self.dev["scale"], self.dev["shift"], act, SLOPE, npix, C, a)
        return a

    def bwd(self, mode, y, g, scale, shift, mean, rstd, gamma, want_affine):
        s = self.dev
        if mode == "act_only":
            ctx = types.SimpleNamespace(bn=None, act=True, slope=SLOPE)
            gy, dg, db = self.wops._bn_act_backward(ctx, dv(y), dv(g), None, None, None, None, None, False)
            assert dg is None and db is None
            return {"gy": gy}
        ctx = types.SimpleNamespace(bn=self.spec, act=mode == "bn_act", slope=SLOPE)
        gy, dg, db = self.wops._bn_act_backward(ctx, dv(y), dv(g), s["scale"], s["shift"], s["mean"], s["rstd"], self.bn.weight, want_affine)
        if not want_affine:
            assert dg is None and db is None
            return {"gy": gy}
        return {"gy": gy, "dgamma": dg, "dbeta": db}

    def chan_sum(self, g):
        return self.wops.chan_sum(dv(g))

    def check_buffers(self):
        if self.track:
            assert int(self.bn.num_batches_tracked) == 2
        else:
            assert int(self.bn.num_batches_tracked) == 0
            assert torch.equal(self.bn.running_mean, self.start[0]) and torch.equal(self.bn.running_var, self.start[1])


def run_red_chain(ngan, wops, guarded, d, o, cid):
    ck = Checker(cid)
    impl = Kernels(ngan, wops, guarded, d, o)
    for name, got, ref in W.red_chain(d, o, impl):
        ck(name, got, ref)
    impl.check_buffers()
    guarded.verify()
    ck.done()


@pytest.mark.parametrize("case", W.RED_CASES, ids=W.red_id)
def test_channel_reductions(ngan, wops, guarded, case):
    """ngan_bn_stats (twice where the running buffers are tracked) -> ngan_bn_act_apply -> ngan_bn_act_bwd in the case's mode ->
    ngan_chan_sum, each on the fp32 outputs of the one before and against the fp64 reference of exactly those inputs"""
    C, npix = case[0], W.red_npix(case[0])[case[1]]
    chunk, nparts = W.red_plan(npix, C)
    assert ngan._C.lib().ngan_chan_reduce_workspace_floats(npix, C) == 6 * nparts * C
    run_red_chain(ngan, wops, guarded, W.red_inputs(case), W.red_options(case), W.red_id(case))


def test_channel_reductions_rechunked(ngan, wops, guarded):
    """16400 pixels of 1024 channels: 16 pixels per workgroup would make 1025 workgroups, so red_chunk takes 17 and makes 965"""
    C, npix = W.BIG_CASE
    assert W.red_plan(npix, C) == (17, 965) and ngan._C.lib().ngan_chan_reduce_workspace_floats(npix, C) == 6 * 965 * C
    case = (C, None)
    run_red_chain(ngan, wops, guarded, W.red_inputs(case, npix), W.red_options(case), "C%d-npix%d" % W.BIG_CASE)


@pytest.mark.parametrize("C", W.FOLD_C)
def test_bn_fold_eval(ngan, guarded, C):
    d = W.fold_inputs(C)
    scale, shift = guarded.alloc((C,)), guarded.alloc((C,))
    ngan._C.call("ngan_bn_fold_eval", dv(d["gamma"]), dv(d["beta"]), dv(d["run_mean"]), dv(d["run_var"]), d["eps"], scale, shift, C)
    refs = W.fold_refs(d)
    ck = Checker(f"C{C}")
    ck("bn_fold_eval/scale", scale, refs["scale"])
    ck("bn_fold_eval/shift", shift, refs["shift"])
    guarded.verify()
    ck.done()


@pytest.mark.parametrize("n", W.POINT_N)
def test_tanh_bwd_and_bn_act_apply(ngan, guarded, n):
    call = ngan._C.call
    ck = Checker(f"n{n}")
    d = W.tanh_bwd_inputs(n)
    o = guarded.alloc((n,))
    call("ngan_tanh_bwd", dv(d["t"]), dv(d["g"]), o, n)
    ck("tanh_bwd/o", o, W.tanh_bwd_refs(d)["o"])
    d = W.apply_inputs(n)
    scale, shift, act = d["xf"]
    npix, C = d["y"].shape
    a = guarded.alloc((npix, C))
    call("ngan_bn_act_apply", dv(d["y"]), dv(scale), dv(shift), act, SLOPE, npix, C, a)
    ck("bn_act_apply/a", a, W.bn_apply_refs(d["y"], scale, shift, act)["a"])
    guarded.verify()
    ck.done()


# ---- stem ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.STEM_CASES, ids=W.stem_id)
def test_stem_forward_and_gradients(ngan, guarded, case):
    K, B, S, C, which = case
    d = W.stem_inputs(case)
    refs = W.stem_refs(d)
    call = ngan._C.call
    ck = Checker(W.stem_id(case))
    y = guarded.alloc((B, S, C))
    call("ngan_wgan_stem_fwd", dv(d["z"]), dv(d["w"]), dv(d["bias"]), y, B, K, S, C)
    ck("stem/y", y, refs["y"])
    gw = guarded.alloc((C * S, K)) if which in ("gw", "both") else None
    gb = guarded.alloc((C * S,)) if which in ("gb", "both") else None
    call("ngan_wgan_stem_grad", dv(d["z"]), dv(d["g"]), gw, gb, B, K, S, C)
    if gw is not None:
        ck("stem/gw", gw, refs["gw"])
    if gb is not None:
        ck("stem/gb", gb, refs["gb"])
    guarded.verify()
    ck.done()


# ---- autograd level: Stem, S2Conv and BNActHead on a non-square stack against the same stock modules in fp64 -------------------------
K_LAT, C0, C1, C2, S_SIDE, H0, W0 = 10, 5, 4, 6, 4, 2, 8        # the stem's 4 x 4 positions are read as 2 x 8; up to 4 x 16; down to 2 x 8
FLOOR = 5e-5        # the bound the stride-2 kernels meet against fp64 in tests/test_gpu_wgan.py (TOL), relative to the largest value


def build_stack(seed=3):
    g = torch.Generator().manual_seed(seed)
    m = nn.ModuleDict(dict(lin=nn.Linear(K_LAT, C0 * H0 * W0), bn0=nn.BatchNorm2d(C0), ct=nn.ConvTranspose2d(C0, C1, 4, 2, 1), bn1=nn.BatchNorm2d(C1),
                           cv=nn.Conv2d(C1, C2, 4, 2, 1), bn2=nn.BatchNorm2d(C2), head=nn.Linear(C2 * H0 * W0, 1)))
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.2))
        for k in ("bn0", "bn1", "bn2"):
            m[k].weight.add_(1.0)
            m[k].running_mean.copy_(torch.randn(m[k].running_mean.shape, generator=g) * 0.2)
            m[k].running_var.copy_(torch.rand(m[k].running_var.shape, generator=g) + 0.5)
    return m


def stack_ref(m, z, x):
    """stock torch modules, NCHW; x is added to the up layer's output"""
    h = m["lin"](z).view(z.shape[0], C0, H0, W0)
    u = m["ct"](F.leaky_relu(m["bn0"](h), SLOPE))
    d = m["cv"](F.leaky_relu(m["bn1"](u + x), SLOPE))
    return m["head"](F.leaky_relu(m["bn2"](d), SLOPE).flatten(1))


def stack_hip(wops, m, z, x):
    """the same modules' parameters through Stem / S2Conv / BNActHead, channels-last; x (B, 4, 16, C1)"""
    h = wops.Stem.apply(z, m["lin"].weight, m["lin"].bias, S_SIDE, C0).view(z.shape[0], H0, W0, C0)
    u = wops.S2Conv.apply(h, m["bn0"].weight, m["bn0"].bias, m["ct"].weight, m["ct"].bias, wops.BNSpec(m["bn0"]), True, SLOPE, True, False)
    d = wops.S2Conv.apply(u + x, m["bn1"].weight, m["bn1"].bias, m["cv"].weight, m["cv"].bias, wops.BNSpec(m["bn1"]), True, SLOPE, False, False)
    return wops.BNActHead.apply(d, m["bn2"].weight, m["bn2"].bias, m["head"].weight, m["head"].bias, wops.BNSpec(m["bn2"]), SLOPE)


def stack_inputs(B=3):
    g = torch.Generator().manual_seed(17)
    return (torch.randn(B, K_LAT, generator=g, dtype=torch.float64), torch.randn(B, C1, 2 * H0, 2 * W0, generator=g, dtype=torch.float64),
            torch.randn(B, 1, generator=g, dtype=torch.float64))


def within(got, r64, r32, scale, what):
    """|got - fp64| <= max(3 |fp32 - fp64|, FLOOR * scale): three times what the same modules lose in torch's own fp32 on the CPU"""
    err = float((got.detach().double().cpu() - r64).abs().max())
    bound = max(3 * float((r32.double() - r64).abs().max()), FLOOR * scale)
    assert err <= bound, (what, err, bound)


@pytest.mark.parametrize("setting", ["normal", "inputs_only", "frozen"])
def test_autograd_stack_matches_stock_modules(ngan, wops, setting):
    """parameter and input gradients of the stack, normally, inside ops.inputs_only() (no parameter gradient is computed) and with
    the up layer's parameters frozen; then the running buffers the forward left"""
    z, x, coef = stack_inputs()
    base = build_stack()
    if setting == "frozen":
        base["ct"].weight.requires_grad_(False)
        base["ct"].bias.requires_grad_(False)
    m64, m32, mh = copy.deepcopy(base).double(), copy.deepcopy(base), copy.deepcopy(base).to(DEV)
    x64, x32 = x.clone().requires_grad_(), x.float().requires_grad_()
    xh = x.float().permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_()
    o64, o32 = stack_ref(m64, z, x64), stack_ref(m32, z.float(), x32)
    (o64 * coef).sum().backward()
    (o32 * coef.float()).sum().backward()
    with (ngan.ops.inputs_only() if setting == "inputs_only" else torch.enable_grad()):
        oh = stack_hip(wops, mh, z.float().to(DEV), xh)
        (oh * coef.float().to(DEV)).sum().backward()
    torch.cuda.synchronize()
    within(oh, o64.detach(), o32.detach(), float(o64.detach().abs().max()), "forward")
    p64, p32, ph = dict(m64.named_parameters()), dict(m32.named_parameters()), dict(mh.named_parameters())
    gmax = max(float(p.grad.abs().max()) for p in p64.values() if p.grad is not None)
    within(xh.grad.permute(0, 3, 1, 2), x64.grad, x32.grad, float(x64.grad.abs().max()), "input gradient")
    for k, p in ph.items():
        if setting == "inputs_only" or (setting == "frozen" and k.startswith("ct.")):
            assert p.grad is None, (setting, k)
        else:
            within(p.grad, p64[k].grad, p32[k].grad, gmax, k)
    b64, b32 = dict(m64.named_buffers()), dict(m32.named_buffers())
    for k, b in mh.named_buffers():
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(b64[k]) == 1, k
        else:
            within(b, b64[k], b32[k], float(b64[k].abs().max()), k)


def test_autograd_stack_eval_mode(wops):
    """eval mode folds the running statistics (ngan_bn_fold_eval); the backward through it is refused with the documented error"""
    z, x, _ = stack_inputs()
    base = build_stack().eval()
    m64, m32, mh = copy.deepcopy(base).double(), copy.deepcopy(base), copy.deepcopy(base).to(DEV)
    xh = x.float().permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_()
    with torch.no_grad():
        o64, o32 = stack_ref(m64, z, x), stack_ref(m32, z.float(), x.float())
    oh = stack_hip(wops, mh, z.float().to(DEV), xh)
    within(oh, o64, o32, float(o64.abs().max()), "eval forward")
    assert all(int(b) == 0 for k, b in mh.named_buffers() if k.endswith("num_batches_tracked"))
    with pytest.raises(RuntimeError, match="eval-mode BatchNorm2d"):
        oh.sum().backward()
