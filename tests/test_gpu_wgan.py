"""The WGAN nets on the stride-2 kernels (csrc/stride2.hip, wgan_ops.py) against torch fp64 on the CPU.

Kernel level: Conv2d / ConvTranspose2d (k4, s2, p1) forward with the fused bias, BatchNorm-on-load, LeakyReLU and Tanh, both
gradients, the BatchNorm statistics and running buffers, the clipping optimiser steps.  Model level: WGANTrainer iterations against the
reference's loop (train.py:470-506) replayed in fp64 over copies of the same stock torch modules; graph replay against eager; resume.
Bound: the exact-fp32 kernels accumulate in fp32, so each quantity is compared as max|got - ref| <= TOL * max|ref| (+ floor), TOL from
the project's fp32 kernel bound (a few 1e-5 for contractions of up to 16K terms).
"""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import __graft_entry__ as graft

pkg = graft.load_package()
from neuron_gan_amd import models, ops, train, utils  # noqa: E402
from neuron_gan_amd import wgan_ops as W  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 5e-5


def rel_err(got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2)


CONV_CASES = [  # (B, C_in, C_out, H_in) for down; up uses H_in as its (half-size) input
    (1, 1, 8, 4), (3, 3, 16, 8), (2, 8, 1, 16), (5, 16, 3, 6), (4, 32, 64, 8), (2, 64, 32, 4), (1, 128, 128, 4), (2, 512, 16, 2),
    (1, 16, 1024, 2), (1, 1024, 8, 2), (16, 16, 16, 32), (2, 16, 16, 128),
]


@pytest.mark.parametrize("up", [False, True])
@pytest.mark.parametrize("case", CONV_CASES)
def test_s2_conv_fwd_dgrad_wgrad(case, up):
    b, cin, cout, h = case
    if not up and h % 2:
        pytest.skip("odd input")
    g = torch.Generator().manual_seed(hash(case) % 1000 + up)
    x = torch.randn(b, cin, h, h, generator=g, dtype=torch.float64)
    wshape = (cin, cout, 4, 4) if up else (cout, cin, 4, 4)
    w = torch.randn(wshape, generator=g, dtype=torch.float64) * 0.1
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    scale = torch.rand(cin, generator=g, dtype=torch.float64) + 0.5
    shift = torch.randn(cin, generator=g, dtype=torch.float64) * 0.3
    slope = 0.2
    a = F.leaky_relu(x * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), slope)
    a.requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    ref = (F.conv_transpose2d(a, wr, bias, stride=2, padding=1) if up else F.conv2d(a, wr, bias, stride=2, padding=1))
    tanh = up and cout <= 3
    if tanh:
        ref = torch.tanh(ref)
    go = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    ref.backward(go)
    f = lambda t: t.float().to(DEV)
    xform = (f(scale), f(shift), 1, slope)
    y = W.conv(nhwc(f(x)), f(w), f(bias), up, xform, tanh)
    assert rel_err(nchw(y), ref) < TOL, rel_err(nchw(y), ref)
    # input gradient (w.r.t. the activated input) and weight gradient through S2Conv's pieces
    gy = nhwc(f(go))
    if tanh:
        gp = torch.empty_like(gy)
        pkg._C.call("ngan_tanh_bwd", y, gy, gp, gy.numel())
        gy = gp
    ga = W.dgrad(gy, f(w), up)
    assert rel_err(nchw(ga), a.grad) < TOL, rel_err(nchw(ga), a.grad)
    xa = nhwc(f(x))
    dw = W.wgrad(xa, gy, wshape, half_xf=xform) if up else W.wgrad(gy, xa, wshape, full_xf=xform)
    assert rel_err(dw, wr.grad) < TOL, rel_err(dw, wr.grad)
    db = W.chan_sum(gy)
    bref = (go * (1 - ref.detach() ** 2) if tanh else go).sum(dim=(0, 2, 3))
    assert rel_err(db, bref) < TOL


@pytest.mark.parametrize("shape", [(4, 8, 16), (3, 64, 8), (16, 1024, 2), (1, 32, 64), (8, 16, 128)])
def test_bn_stats_running_and_backward(shape):
    b, c, h = shape
    g = torch.Generator().manual_seed(c + h)
    y = (torch.randn(b, c, h, h, generator=g, dtype=torch.float64) * 2 + 3)
    bn_ref = torch.nn.BatchNorm2d(c).double()
    with torch.no_grad():
        bn_ref.weight.normal_(1.0, 0.1, generator=g)
        bn_ref.bias.normal_(0.0, 0.1, generator=g)
        bn_ref.running_var.uniform_(0.5, 1.5, generator=g)
    bn = copy.deepcopy(bn_ref).float().to(DEV)
    yr = y.clone().requires_grad_(True)
    gam = bn_ref.weight
    act_ref = F.leaky_relu(bn_ref(yr), 0.2)
    go = torch.randn(act_ref.shape, generator=g, dtype=torch.float64)
    act_ref.backward(go)
    spec = W.BNSpec(bn)
    yd = nhwc(y.float().to(DEV))
    scale, shift, mean, rstd = spec.fold(yd, bn.weight, bn.bias)
    a = torch.empty_like(yd)
    pkg._C.call("ngan_bn_act_apply", yd, scale, shift, 1, 0.2, yd.numel() // c, c, a)
    assert rel_err(nchw(a), act_ref) < TOL
    assert rel_err(bn.running_mean, bn_ref.running_mean) < 1e-6
    assert rel_err(bn.running_var, bn_ref.running_var) < 1e-5
    assert int(bn.num_batches_tracked) == int(bn_ref.num_batches_tracked) == 1

    class Ctx:
        pass
    ctx = Ctx()
    ctx.bn, ctx.act, ctx.slope = spec, True, 0.2
    gy, dg, dbt = W._bn_act_backward(ctx, yd, nhwc(go.float().to(DEV)), scale, shift, mean, rstd, bn.weight, True)
    assert rel_err(nchw(gy), yr.grad) < 1e-4
    assert rel_err(dg, gam.grad) < TOL and rel_err(dbt, bn_ref.bias.grad) < TOL


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_clip_step_bit_equal(kind):
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 16, 4, 2, 1), torch.nn.BatchNorm2d(16), torch.nn.Linear(16, 1)).to(DEV)
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(0.05)
    nets = [copy.deepcopy(net), copy.deepcopy(net)]
    cls = {"adam": (train.FusedAdam, train.ClippedFusedAdam), "rmsprop": (train.FusedRMSprop, train.ClippedFusedRMSprop)}[kind]
    opts = []
    for n, c in zip(nets, cls):
        fl = train.FlatParams(n, c.STATE)
        fl.set_active(fl.params)
        opts.append((fl, c(fl, 1e-2)))
    opts[1][1].clip = 0.01
    for it in range(3):
        g = torch.randn(opts[0][0].total, device=DEV, generator=torch.Generator(DEV).manual_seed(it))
        for fl, opt in opts:
            fl.grad.copy_(g)
            opt.step()
        opts[0][0].flat.clamp_(-0.01, 0.01)
        torch.cuda.synchronize()
        assert torch.equal(opts[0][0].flat, opts[1][0].flat)
        st = opts[0][1].STATE
        for s in st:
            assert torch.equal(getattr(opts[0][0], s), getattr(opts[1][0], s))


# ------------------------------------------------------------------------------------------------------------------
# model level: the reference's loop in fp64 over deep copies of the same stock modules
# ------------------------------------------------------------------------------------------------------------------
def make_nets(gw, dw, latent, size, colors=1, seed=1):
    torch.manual_seed(seed)
    G = models.Generator_wgan(gw, latent_dim=latent, image_size=size, N_colors=colors)
    D = models.Discriminator_wgan(dw, image_size=size, N_colors=colors)
    G.apply(utils.init_weights)
    D.apply(utils.init_weights)
    return G, D


def ref_iteration(Gl, Dl, optG, optD, real, zs_d, z_g, n_critic, drift=0.001, clip=0.01):
    out = {}
    for i in range(n_critic):
        sr_all = Dl(real)
        s_real = sr_all.mean()
        fake = Gl(zs_d[i]).detach()
        s_fake = Dl(fake).mean()
        loss = -s_real + s_fake + drift * torch.square(sr_all).mean()
        Dl.zero_grad()
        loss.backward()
        optD.step()
        for p in Dl.parameters():
            p.data.clamp_(-clip, clip)
        out.update(D_loss=loss.item(), score_real=s_real.item(), score_fake=s_fake.item())
    gl = -Dl(Gl(z_g)).mean()
    Gl.zero_grad()
    gl.backward()
    optG.step()
    out["G_loss"] = gl.item()
    return out


def ref_opts(Gl, Dl, kind, lr):
    if kind == "adam":
        return torch.optim.Adam(Gl.parameters(), lr=lr, betas=(0.5, 0.999)), torch.optim.Adam(Dl.parameters(), lr=lr, betas=(0.5, 0.999))
    return torch.optim.RMSprop(Gl.parameters(), lr=lr), torch.optim.RMSprop(Dl.parameters(), lr=lr)


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
@pytest.mark.parametrize("cfg", [dict(gw=[32, 16, 8], dw=[8, 16, 32], latent=16, size=64, b=4, n_critic=2, colors=1),
                                 dict(gw=[16, 8], dw=[8, 16], latent=32, size=32, b=3, n_critic=1, colors=3)])
def test_trainer_matches_fp64_reference(kind, cfg):
    """Bound per quantity: max(3 * |ref_fp32 - ref_fp64|, floor), the reference's own loop run in fp32 and in fp64 on the CPU.  Adam's
    first steps move each weight by about lr * sign(g), so a gradient near zero whose sign fp32 rounding flips moves a weight by up
    to 2 lr either way: the fp32 reference shows how much of that a correct fp32 implementation carries.  floor = 1e-5 * max|ref|
    (fp32 accumulation of the contractions).  Scalars: within 1e-3 relative, as on the PGGAN path."""
    G, D = make_nets(cfg["gw"], cfg["dw"], cfg["latent"], cfg["size"], cfg["colors"])
    Gl, Dl = copy.deepcopy(G.layers).double(), copy.deepcopy(D.layers).double()
    G32, D32 = copy.deepcopy(G.layers), copy.deepcopy(D.layers)
    lr = 1e-3 if kind == "adam" else 1e-4
    optG, optD = ref_opts(Gl, Dl, kind, lr)
    optG32, optD32 = ref_opts(G32, D32, kind, lr)
    G.to(DEV)
    D.to(DEV)
    tr = train.WGANTrainer(G, D, learning_rate=lr, optimizer=kind, n_critic=cfg["n_critic"])
    g = torch.Generator().manual_seed(7)
    b = cfg["b"]
    for it in range(2):
        real = torch.rand(b, cfg["colors"], cfg["size"], cfg["size"], generator=g, dtype=torch.float64) * 2 - 1
        zs = [torch.randn(b, cfg["latent"], generator=g, dtype=torch.float64) for _ in range(cfg["n_critic"])]
        zg = torch.randn(b, cfg["latent"], generator=g, dtype=torch.float64)
        want = ref_iteration(Gl, Dl, optG, optD, real, zs, zg, cfg["n_critic"])
        ref_iteration(G32, D32, optG32, optD32, real.float(), [z.float() for z in zs], zg.float(), cfg["n_critic"])
        got = tr.train_iteration(real.float().to(DEV), [z.float().to(DEV) for z in zs], zg.float().to(DEV))
        for k, v in want.items():
            assert abs(float(got[k]) - v) <= 1e-3 * max(abs(v), 1e-2), (it, k, float(got[k]), v)
    torch.cuda.synchronize()
    for net, ref, r32 in ((G, Gl, G32), (D, Dl, D32)):
        sd, rd, sd32 = net.layers.state_dict(), ref.state_dict(), r32.state_dict()
        for k in rd:
            if k.endswith("num_batches_tracked"):
                assert int(sd[k]) == int(rd[k]), k
                continue
            err = float((sd[k].double().cpu() - rd[k]).abs().max())
            bound = max(3 * float((sd32[k].double() - rd[k]).abs().max()), 1e-5 * float(rd[k].abs().max()) + 1e-7)
            assert err <= bound, (k, err, bound)
    # eval-mode sample from the running statistics
    G.eval()
    Gl.eval()
    z = torch.randn(4, cfg["latent"], generator=g, dtype=torch.float64)
    with torch.no_grad():
        s = G(z.float().to(DEV))
        sref = Gl(z)
    G.train()
    assert float((s.double().cpu() - sref).abs().max()) < 1e-3


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_graph_replay_equals_eager(kind):
    cfg = dict(gw=[32, 16, 8], dw=[8, 16, 32], latent=16, size=64, b=5)
    runs = []
    for mode in ("eager", "graph"):
        G, D = make_nets(cfg["gw"], cfg["dw"], cfg["latent"], cfg["size"])
        G.to(DEV)
        D.to(DEV)
        tr = train.WGANTrainer(G, D, learning_rate=1e-3, optimizer=kind, n_critic=2)
        gen = torch.Generator().manual_seed(3)
        static = {"z_d": [torch.zeros(cfg["b"], cfg["latent"], device=DEV) for _ in range(2)],
                  "z_g": torch.zeros(cfg["b"], cfg["latent"], device=DEV)}
        out = []
        for it in range(3):
            real = (torch.rand(cfg["b"], 1, cfg["size"], cfg["size"], generator=gen) * 2 - 1).to(DEV)
            zs = [torch.randn(cfg["b"], cfg["latent"], generator=gen).to(DEV) for _ in range(2)]
            zg = torch.randn(cfg["b"], cfg["latent"], generator=gen).to(DEV)
            if mode == "eager":
                st = tr.train_iteration(real, zs, zg)
            else:
                for s, v in zip(static["z_d"], zs):
                    s.copy_(v)
                static["z_g"].copy_(zg)
                if it == 0:
                    tr.capture(real, draws=static)
                st = tr.replay(real)
            out.append({k: v.clone() for k, v in st.items()})
        torch.cuda.synchronize()
        runs.append((out, tr.flat_g.flat.clone(), tr.flat_d.flat.clone(), [b.clone() for b in tr._bn_buffers()]))
    (o1, g1, d1, b1), (o2, g2, d2, b2) = runs
    for a, b in zip(o1, o2):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert torch.equal(g1, g2) and torch.equal(d1, d2)
    assert all(torch.equal(x, y) for x, y in zip(b1, b2))


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_capture_trains_nothing(kind):
    """capture() warms up on a snapshot: parameters, optimiser state, step counts, the BatchNorm running buffers (num_batches_tracked
    among them) and the device RNG state are afterwards what they were, bit for bit; the first replay() is the first update."""
    cfg = dict(gw=[32, 16, 8], dw=[8, 16, 32], latent=16, size=64, b=5)
    G, D = make_nets(cfg["gw"], cfg["dw"], cfg["latent"], cfg["size"])
    G.to(DEV)
    D.to(DEV)
    tr = train.WGANTrainer(G, D, learning_rate=1e-3, optimizer=kind, n_critic=2, device_latents=True)
    real = (torch.rand(cfg["b"], 1, cfg["size"], cfg["size"], generator=torch.Generator().manual_seed(3)) * 2 - 1).to(DEV)
    state = tr._training_state()
    assert all(any(b is t for t in state) for b in tr._bn_buffers()) and len(tr._bn_buffers()) > 0
    before = [t.clone() for t in state]
    rng = torch.cuda.get_rng_state()
    tr.capture(real, warmup=2)
    torch.cuda.synchronize()
    for i, (a, t) in enumerate(zip(before, tr._training_state())):
        assert torch.equal(a, t), f"capture() changed tensor {i} of _training_state()"
    assert torch.equal(rng, torch.cuda.get_rng_state()), "capture() advanced the device RNG"
    means = [b for net in (G, D) for n, b in net.named_buffers() if n.endswith("running_mean")]
    means_before = [m.clone() for m in means]
    g0, d0 = tr.flat_g.flat.clone(), tr.flat_d.flat.clone()
    tr.replay(real)
    torch.cuda.synchronize()
    assert not torch.equal(g0, tr.flat_g.flat) and not torch.equal(d0, tr.flat_d.flat)
    assert any(not torch.equal(a, m) for a, m in zip(means_before, means))


def test_checkpoint_resume_equals_uninterrupted(tmp_path):
    cfg = dict(gw=[16, 8], dw=[8, 16], latent=16, size=32, b=4)
    gen = torch.Generator().manual_seed(5)
    data = [((torch.rand(cfg["b"], 1, 32, 32, generator=gen) * 2 - 1), [torch.randn(cfg["b"], 16, generator=gen)],
             torch.randn(cfg["b"], 16, generator=gen)) for _ in range(4)]

    def run(iters, tr):
        for real, zs, zg in iters:
            tr.train_iteration(real.to(DEV), [z.to(DEV) for z in zs], zg.to(DEV))

    G, D = make_nets(cfg["gw"], cfg["dw"], cfg["latent"], cfg["size"])
    G.to(DEV)
    D.to(DEV)
    tr = train.WGANTrainer(G, D, learning_rate=1e-3, optimizer="rmsprop")
    run(data, tr)
    full = (tr.flat_g.flat.clone(), tr.flat_d.flat.clone(), [b.clone() for b in tr._bn_buffers()])

    G2, D2 = make_nets(cfg["gw"], cfg["dw"], cfg["latent"], cfg["size"])
    G2.to(DEV)
    D2.to(DEV)
    tr2 = train.WGANTrainer(G2, D2, learning_rate=1e-3, optimizer="rmsprop")
    run(data[:2], tr2)
    fn = str(tmp_path / "ck.pth")
    utils.Checkpointer(G2, D2, 1e-3, fn, N_epochs=4, device=DEV, trainer=tr2).save_state(2)
    G3, D3 = make_nets(cfg["gw"], cfg["dw"], cfg["latent"], cfg["size"], seed=9)
    G3.to(DEV)
    D3.to(DEV)
    tr3 = train.WGANTrainer(G3, D3, learning_rate=1e-3, optimizer="rmsprop")
    utils.Checkpointer(G3, D3, 1e-3, fn, N_epochs=4, device=DEV, trainer=tr3, verbose=False).load_state()
    run(data[2:], tr3)
    torch.cuda.synchronize()
    assert torch.equal(full[0], tr3.flat_g.flat) and torch.equal(full[1], tr3.flat_d.flat)
    assert all(torch.equal(x, y) for x, y in zip(full[2], tr3._bn_buffers()))


def test_epoch_driver_sums_and_checkpoint(tmp_path):
    from types import SimpleNamespace
    G, D = make_nets([16, 8], [8, 16], 16, 32)
    G.to(DEV)
    D.to(DEV)
    tr = train.WGANTrainer(G, D, learning_rate=1e-4, optimizer="adam", device_latents=True)
    ds = train.TensorImageDataset.synthetic(8, 32, 1, device="cpu")
    cfg = SimpleNamespace(N_epochs=3, batch_size=4, checkpointing_period=2, ID="t", adapt_critic=False)
    ck = utils.Checkpointer(G, D, 1e-4, str(tmp_path / "w.pth"), N_epochs=3, device=DEV, trainer=tr, verbose=False)
    hist = train.wgan_train(tr, ds, cfg, checkpoint=ck, epoch_init=1, epoch_final=4, log=lambda *a: None,
                            samples_dir=str(tmp_path))
    assert len(hist) == 3 and all(np.isfinite(list(h.values())).all() for h in hist)
    assert os.path.exists(str(tmp_path / "w.pth"))
    assert ck.Loss_G[0] == pytest.approx(hist[0]["G_loss"])
    assert any(f.endswith(".png") for f in os.listdir(tmp_path))


# ------------------------------------------------------------------------------------------------------------------
# against the fixtures written by tools/make_golden_wgan.py from the reference's own modules
# Bound per tensor: max(3 * dev, FLOOR * max|ref|), dev = max|ref_fp32 - ref_fp64| of the reference's loop replayed in fp32 (stored
# with the fixture).  FLOOR = 5e-5: TOL, the bound every stride-2 kernel meets against fp64 in the kernel tests above.
# ------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOOR = 5e-5


def _tool():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_make_golden_wgan", os.path.join(root, "tools", "make_golden_wgan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bn_fed_biases(G, D):
    """biases of the layers whose output goes straight into a BatchNorm2d: the batch mean cancels them exactly, so their gradient is
    zero in exact arithmetic and what any implementation computes for it is rounding noise; the optimiser then moves them by noise
    (up to about lr per step).  They influence no output: their post-step values are not compared, their gradients are compared on
    the scale of the net's gradients."""
    out = set()
    for tag, net in (("G", G), ("D", D)):
        L = list(net.layers)
        for i, m in enumerate(L):
            nxt = [x for x in L[i + 1:i + 3] if isinstance(x, torch.nn.BatchNorm2d)]
            if getattr(m, "bias", None) is not None and not isinstance(m, torch.nn.BatchNorm2d) and nxt:
                out.add((tag, f"layers.{i}.bias"))
    return out


def _scale_floor(k, ref_amax, grad_amax):
    """FLOOR times max|ref| of the tensor, for gradients times the largest gradient of that net (see bn_fed_biases)"""
    if k.startswith("grad"):
        return FLOOR * grad_amax[k[4]]
    return FLOOR * ref_amax


def _step_slack(k, grad_amax_of, grad_amax, lr, n_updates, eps=1e-8):
    """post-step parameters whose own gradient is near zero (below 1e-4 of the net's largest, or within 1000 eps of zero, where
    Adam's eps = 1e-8 no longer dominates the denominator's sensitivity): Adam / RMSprop divide the gradient by
    its own running magnitude, so a gradient error at the floor's size moves such a parameter by up to about lr per update (capped at
    2 lr by the normalisation); elsewhere the step is insensitive to it and no slack is added"""
    if k.startswith("grad") or k.endswith(("running_mean", "running_var")):
        return 0.0
    net, name = k[0], k[2:]
    ga = grad_amax_of.get(f"grad{net}.{name}")
    if ga is None or ga >= max(1e-4 * grad_amax[net], 1e3 * eps):
        return 0.0
    return lr * n_updates * min(2.0, FLOOR * grad_amax[net] / eps)


def _fed_bias_slack(k, ours, ref_of, skip):
    """running_mean of a BatchNorm fed by a bias of `bn_fed_biases`: the batch mean carries that bias, whose value is noise-driven"""
    if not k.endswith("running_mean"):
        return 0.0
    net, layer = k[0], int(k.split(".")[2])
    bias = f"{net}.layers.{layer - 1}.bias"
    if bias not in skip and layer >= 2 and f"{net}.layers.{layer - 2}.bias" in skip:      # the G stem: Linear, Unflatten, BN
        bias = f"{net}.layers.{layer - 2}.bias"
    if bias not in skip:
        return 0.0
    return float((ours[bias].double().cpu() - ref_of(bias)).abs().max())


def _our_states(tr, G, D):
    out = {}
    for tag, net in (("G", G), ("D", D)):
        for k, v in net.state_dict().items():
            out[f"{tag}.{k}"] = v.detach()
    for tag, net in (("gradD", D), ("gradG", G)):
        for k, p in net.named_parameters():
            out[f"{tag}.{k}"] = p.grad.detach()
    return out


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_matches_wgan_small_fixture(kind):
    fx = np.load(os.path.join(GOLDEN, "wgan_small.npz"))
    cfg = _tool().SMALL
    G, D = make_nets(cfg["gw"], cfg["dw"], cfg["latent"], cfg["size"], cfg["colors"])
    for tag, net in (("init_G", G), ("init_D", D)):
        for k, v in net.state_dict().items():
            assert np.array_equal(v.numpy(), fx[f"{tag}.{k}"]), k
    G.to(DEV)
    D.to(DEV)
    tr = train.WGANTrainer(G, D, learning_rate=cfg["lr"], optimizer=kind, n_critic=cfg["n_critic"])
    for i in range(cfg["iters"]):
        zd = torch.from_numpy(fx[f"z_d.{i}"]).to(DEV)
        got = tr.train_iteration(torch.from_numpy(fx[f"real.{i}"]).to(DEV), list(zd), torch.from_numpy(fx[f"z_g.{i}"]).to(DEV))
        for name in ("score_real", "score_fake", "D_loss", "G_loss"):
            v = float(fx[f"{kind}.scalar64.{name}"][i])
            assert abs(float(got[name]) - v) <= 1e-3 * max(abs(v), 1e-2), (i, name, float(got[name]), v)
    torch.cuda.synchronize()
    ours = _our_states(tr, G, D)
    skip = {f"{t}.{k}" for t, k in bn_fed_biases(G, D)}
    gmax_of = {k: float(np.abs(fx[f"{kind}.{k}"]).max()) for k in ours if k.startswith("grad")}
    grad_amax = {t: max(v for k, v in gmax_of.items() if k.startswith("grad" + t)) for t in "DG"}
    for k, v in ours.items():
        ref = fx[f"{kind}.{k}"]
        if v.dtype == torch.int64:
            assert int(v) == int(ref), k
            continue
        if k in skip:
            continue
        ref = torch.from_numpy(ref).double()
        err = float((v.double().cpu() - ref).abs().max())
        bound = max(3 * float(fx[f"{kind}.dev.{k}"]), _scale_floor(k, float(ref.abs().max()), grad_amax))
        bound += _step_slack(k, gmax_of, grad_amax, cfg["lr"], cfg["iters"] * (cfg["n_critic"] if k[0] == "D" else 1))
        bound += _fed_bias_slack(k, ours, lambda b: torch.from_numpy(fx[f"{kind}.{b}"]).double(), skip)
        assert err <= bound, (k, err, bound)
    G.eval()
    with torch.no_grad():
        s = G(torch.from_numpy(fx["z_eval"]).to(DEV))
    ref = torch.from_numpy(fx[f"{kind}.sample"]).double()
    err = float((s.double().cpu() - ref).abs().max())
    assert err <= max(3 * float(fx[f"{kind}.dev.sample"]), FLOOR * float(ref.abs().max())), err


def test_matches_wgan_full_fixture():
    """the default widths at 512^2, batch 8, one Adam iteration: element pins and checksums of every parameter, buffer and gradient"""
    fx = np.load(os.path.join(GOLDEN, "wgan_full.npz"))
    tool = _tool()
    cfg = tool.FULL
    G, D = make_nets(cfg["gw"], cfg["dw"], cfg["latent"], cfg["size"], cfg["colors"])
    G.to(DEV)
    D.to(DEV)
    tr = train.WGANTrainer(G, D, learning_rate=cfg["lr"], optimizer="adam", n_critic=cfg["n_critic"])
    (real, zs, zg), = tool.inputs_full()
    got = tr.train_iteration(real.to(DEV), [z.to(DEV) for z in zs], zg.to(DEV))
    for name in ("score_real", "score_fake", "D_loss", "G_loss"):
        v = float(fx[f"scalar64.{name}"][0])
        assert abs(float(got[name]) - v) <= 1e-3 * max(abs(v), 1e-2), (name, float(got[name]), v)
    torch.cuda.synchronize()
    ours = _our_states(tr, G, D)
    skip = {f"{t}.{k}" for t, k in bn_fed_biases(G, D)}
    gmax_of = {k: float(fx[f"amax.{k}"]) for k in ours if k.startswith("grad")}
    grad_amax = {t: max(v for k, v in gmax_of.items() if k.startswith("grad" + t)) for t in "DG"}
    for k, v in ours.items():
        if v.dtype == torch.int64:
            assert int(v) == int(fx[f"int.{k}"]), k
            continue
        if k in skip:
            continue
        flat = v.reshape(-1).double().cpu()
        amax = float(fx[f"amax.{k}"])
        bound = max(3 * float(fx[f"dev.{k}"]), _scale_floor(k, amax, grad_amax))
        bound += _step_slack(k, gmax_of, grad_amax, cfg["lr"], 1)
        bound += _fed_bias_slack(k, ours, lambda b: None, set())
        idx = torch.from_numpy(fx[f"idx.{k}"])
        err = float((flat[idx] - torch.from_numpy(fx[f"pin.{k}"])).abs().max())
        assert err <= bound, (k, "pins", err, bound)
        ssum, sabs = fx[f"sum.{k}"]
        dsum, dabs = fx[f"sumdev.{k}"]
        n = flat.numel()     # checksums: independent per-element errors within `bound` add up to about bound * sqrt(n)
        assert abs(float(flat.sum()) - ssum) <= max(3 * dsum, bound * n ** 0.5), (k, "sum")
        assert abs(float(flat.abs().sum()) - sabs) <= max(3 * dabs, bound * n ** 0.5), (k, "sum|.|")


def test_epoch_driver_adapt_critic_and_sums(tmp_path):
    """adapt_critic over several epochs (n_critic from the score series); the series hold per-epoch SUMS of the per-batch values"""
    from types import SimpleNamespace
    G, D = make_nets([16, 8], [8, 16], 16, 32)
    G.to(DEV)
    D.to(DEV)
    tr = train.WGANTrainer(G, D, learning_rate=1e-4, optimizer="rmsprop", n_critic=5, device_latents=True)
    seen, steps = [], []
    inner = tr.step

    def step(real, use_graph=True):
        st = inner(real, use_graph=use_graph)
        seen.append({k: float(v) for k, v in st.items()})
        steps.append(tr.n_critic)
        return st
    tr.step = step
    ds = train.TensorImageDataset.synthetic(12, 32, 1, device="cpu")
    cfg = SimpleNamespace(N_epochs=4, batch_size=4, checkpointing_period=2, ID="t", adapt_critic=True)
    ck = utils.Checkpointer(G, D, 1e-4, str(tmp_path / "w.pth"), N_epochs=4, device=DEV, trainer=tr, verbose=False)
    hist = train.wgan_train(tr, ds, cfg, checkpoint=ck, epoch_init=1, epoch_final=5, log=lambda *a: None, samples_dir=str(tmp_path))
    assert len(hist) == 4 and len(seen) == 12
    for e in range(4):
        for k in ("score_real", "score_fake", "D_loss", "G_loss"):
            want = sum(s[k] for s in seen[3 * e:3 * e + 3])
            assert hist[e][k] == pytest.approx(want, rel=1e-5, abs=1e-6), (e, k)
    assert ck.Loss_real[3] == pytest.approx(hist[3]["score_real"]) and ck.Loss_G[3] == pytest.approx(hist[3]["G_loss"])
    for e in range(4):    # the critic-step count of each epoch follows the series of the epochs before it
        want = train.wgan_critic_steps([h["score_real"] for h in hist[:e]], [h["score_fake"] for h in hist[:e]], 5)
        assert steps[3 * e:3 * e + 3] == [want] * 3, (e, steps)
    assert tr.n_critic == 5
    assert any(f.endswith(".png") for f in os.listdir(tmp_path))
