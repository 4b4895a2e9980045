"""RMSprop on the GPU (the reference's RMSprop switch, train.py:220-225: optim.RMSprop(params, lr) with torch's defaults alpha 0.99,
eps 1e-8): the flat multi-tensor kernel and the stem's gradient-free epilogue against torch.optim.RMSprop, the fused and stored stem
paths, one training iteration against the oracle, graph replay, checkpoint resume and the epoch driver."""
import types

import numpy as np
import pytest
import torch

from conftest import load_golden, split_state
from oracle import pggan_oracle as O

import test_gpu_models as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP = 2.0 ** -23          # fp32 unit roundoff x 2: one ulp of a number in [1, 2)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_flat_rmsprop_against_torch_rmsprop(ngan, gscale):
    """FusedRMSprop (ngan_rmsprop_step over the flat buffers) next to torch.optim.RMSprop(foreach=False) on copies of the same GPU
    tensors: five steps, tensor 1 without a gradient for the first two (torch skips `.grad is None` tensors), sizes that are not
    multiples of the 4096-element chunk, gradient scales from 1e-2 to 10; grad_scale 0.5 against torch fed 0.5 * g.

    Bound: the kernel evaluates torch's formula in fp32 in torch's order -- sqrt(v) + eps, g / that, times lr, subtracted from p --
    except that alpha*v + (1-alpha)*g*g is one fused multiply-add where torch rounds alpha*v first: at most one ulp of v per step,
    so five steps differ by <= 5 ulp of v.  That difference reaches p through sqrt(v) as a relative 1e-7 of a step (<= 10 lr = 2e-2:
    ~2e-9, far below one ulp of p ~ 0.3), and can shift p's rounding by one ulp per step: <= 5 ulp of p.  Asserted: 8 ulp of each
    tensor's max-norm, for p and for square_avg."""
    torch.manual_seed(17)
    net = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, device=DEV) * 0.3) for n in (5000, 37, 4096, 12289)])
    ref = [torch.nn.Parameter(p.detach().clone()) for p in net]
    lr = 2e-3
    opt = torch.optim.RMSprop(ref, lr=lr, foreach=False)
    flat = ngan.train.FlatParams(net, ngan.train.FusedRMSprop.STATE)
    fr = ngan.train.FusedRMSprop(flat, lr)
    fr.set_grad_scale(gscale)
    for it in range(5):
        late = it < 2                                      # tensor 1 joins at the third step
        flat.set_active([p for i, p in enumerate(flat.params) if not (late and i == 1)])
        flat.zero_grad()
        for i, (p, r) in enumerate(zip(flat.params, ref)):
            if late and i == 1:
                r.grad = None
                continue
            g = torch.randn_like(p) * (10.0 ** (i - 2))    # gradient scales from 1e-2 to 10
            p.grad.copy_(g)
            r.grad = g * gscale
        fr.step()
        opt.step()
    torch.cuda.synchronize()
    assert flat.seg_step.cpu().tolist() == [5.0, 3.0, 5.0, 5.0]
    for i, (p, r, o) in enumerate(zip(flat.params, ref, flat.offsets)):
        v, vr = flat.square_avg[o:o + p.numel()], opt.state[r]["square_avg"]
        assert int(opt.state[r]["step"]) == flat.seg_step.cpu().tolist()[i]
        dp, dv = float((p.detach() - r.detach()).abs().max()), float((v - vr).abs().max())
        assert dp <= 8 * ULP * float(r.detach().abs().max()), (i, dp)
        assert dv <= 8 * ULP * float(vr.abs().max()), (i, dv)


# the last: nt = 9 < NT on the NT = 32 instantiation (the `t < nt` guards of the epilogue), rows not a multiple of 64
STEM_CASES = [(16, 512, 256, 128, 1.0), (24, 64, 16, 32, 0.5), (7, 48, 9, 20, 1.0), (5, 144, 9, 20, 1.0)]


@pytest.mark.parametrize("act", ["f32", "bf16"])
@pytest.mark.parametrize("B,K,S2,C,gscale", STEM_CASES)
def test_stem_rmsprop_epilogue(ngan, B, K, S2, C, gscale, act):
    """ngan_linear_wgrad_rmsprop: RMSprop applied to the stem weight in the epilogue of its gradient's factor product, three steps.
    (a) bit-equal to ngan_linear_wgrad (the stored gradient, same MFMA kernel and accumulation order) followed by ngan_rmsprop_step;
    (b) against torch.optim.RMSprop fed the fp64 gradient  scale * gscale * sum_b gc[b] (x) z[b]  of the same (bf16-rounded) gc.

    Bounds of (b): the first step moves every weight by lr * g / sqrt(0.01 g^2) = 10 lr sign(g) whatever |g| is, and later steps by at
    most 10 lr too (v >= 0.01 g^2).  The fp32 gradient differs from the fp64 one by ~1e-7 of the tensor's scale; an element whose
    gradient is at that level may take the other sign and move up to 20 lr the wrong way per step -- bounded by the arithmetic, so
    the worst element is checked only against 20.2 lr per step.  What is asserted is their share: elements off by more than 0.02 of a
    first step (0.2 lr) below 2e-4 (the Adam epilogue test's rule, its step being lr), and the mean difference below 1e-3 lr per step.
    square_avg = 0.01 g^2 + ...: a relative 1e-7 in g is 2e-7 in v; 1e-5 of the tensor's max as in the Adam test."""
    C_ = ngan._C
    torch.manual_seed(12)
    rows = C * S2
    w = torch.randn(rows, K) * 0.1
    p1, p2 = w.clone().to(DEV), w.clone().to(DEV)
    v1, v2 = torch.zeros_like(p1), torch.zeros_like(p1)
    g2 = torch.empty_like(p1)
    lr, alpha, eps, scale = 1e-3, 0.99, 1e-8, 0.0613
    hyper = torch.tensor([lr, alpha, eps, gscale, 1.0 - alpha], dtype=torch.float32, device=DEV)
    n = rows * K
    chunks = list(range(0, n, 4096))
    seg_off = torch.zeros(1, dtype=torch.int64, device=DEV)
    seg_len = torch.tensor([n], dtype=torch.int64, device=DEV)
    seg_active = torch.ones(1, dtype=torch.int32, device=DEV)
    seg_step = torch.zeros(1, dtype=torch.float32, device=DEV)
    chunk_seg = torch.zeros(len(chunks), dtype=torch.int32, device=DEV)
    chunk_off = torch.tensor(chunks, dtype=torch.int64, device=DEV)
    ref = torch.nn.Parameter(w.double())
    opt = torch.optim.RMSprop([ref], lr=lr, alpha=alpha, eps=eps)
    bf = act == "bf16"
    for it in range(3):
        z = torch.randn(B, K)
        gc = torch.randn(B, S2, C)
        if bf:
            gc = gc.bfloat16()
        ref.grad = scale * gscale * torch.einsum("bpc,bk->cpk", gc.double(), z.double()).reshape(rows, K)
        opt.step()
        zd, gcd = z.to(DEV), gc.to(DEV)
        C_.call(ngan.ops._k("ngan_linear_wgrad_rmsprop", gcd), zd, gcd, p1, v1, hyper, hyper.numel(), B, K, S2, C, scale)
        C_.call(ngan.ops._k("ngan_linear_wgrad", gcd), zd, gcd, g2, B, K, S2, C, scale)
        C_.call("ngan_rmsprop_step", p2, g2, v2, seg_off, seg_len, seg_active, seg_step, 1, chunk_seg, chunk_off, len(chunks),
                hyper, hyper.numel())
        torch.cuda.synchronize()
        assert torch.equal(p1, p2) and torch.equal(v1, v2), it                                   # (a)
        diff = (p1.cpu().double() - ref.detach()).abs()                                          # (b)
        assert float((diff > 0.2 * lr).double().mean()) < 2e-4, (it, float((diff > 0.2 * lr).double().mean()))
        assert float(diff.mean()) < 1e-3 * lr * (it + 1), (it, float(diff.mean()))
        assert float(diff.max()) < 20.2 * lr * (it + 1), it
    assert float(seg_step) == 3.0
    assert rel(v1.cpu(), opt.state[ref]["square_avg"]) < 1e-5


def small_trainer(ngan, fix, **kw):
    G, D = T.build_small(ngan, fix)
    return G, D, ngan.train.PGGANTrainer(G, D, optimizer="rmsprop", **kw)


def test_fused_and_stored_stem_paths_agree(ngan):
    """fused_stem=True (the stem's RMSprop in the factor product's epilogue, no stored gradient) and fused_stem=False (stored gradient,
    flat RMSprop launch) over three eager iterations on the same draws: same kernels' arithmetic, so the same bits."""
    fix = load_golden("small_res8_warm")
    t = lambda k: torch.from_numpy(fix[k]).to(DEV)
    out = []
    for fused in (True, False):
        G, D, tr = small_trainer(ngan, fix, learning_rate=1e-3, fused_stem=fused)
        assert tr.fused_stem == fused
        for _ in range(3):
            tr.train_iteration(t("real"), z_d=t("z_d"), z_gp=t("z_gp"), eps=t("eps"), z_g=t("z_g"))
        if fused:
            assert float(tr.stem.weight.grad.abs().max()) == 0.0              # never stored
        torch.cuda.synchronize()
        out.append([x.detach().cpu().clone() for x in (tr.flat_g.flat, tr.flat_g.square_avg, tr.flat_d.flat, tr.flat_d.square_avg,
                                                       tr.flat_g.seg_step)])
    for i, (a, b) in enumerate(zip(*out)):
        assert torch.equal(a, b), i


def rmsprop_close(got, want, lr):
    """the adam_close rule for RMSprop: its first step moves each weight by ~10 lr sign(g); allow a few sign flips where |g| is at
    rounding level -- the share of elements whose update differs by more than a tenth of a step (lr) stays below 2e-3"""
    bad = np.mean(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) > 0.1 * (10 * lr))
    return bad < 2e-3


@pytest.mark.parametrize("name", T.SMALL)
def test_one_iteration_against_the_oracle(ngan, name, conv_precision):
    """One iteration through the trainer with optimizer="rmsprop" against oracle.train_step on fp64 leaves with torch.optim.RMSprop,
    then a second iteration on draws of a seeded generator (the oracle continuing from its own RMSprop state).

    Bounds: post-step parameters by rmsprop_close; square_avg within 1e-2 of each tensor's max -- the gradients are pinned at 2e-3 of
    their max-norm (test_small_nets_match_reference) and v = 0.01 g^2 after one step, so its error is at most 2 * 2e-3 of max v; the
    second iteration's scalars within 5e-3 (rtol, atol 5e-5), the second-iteration bound of test_full_width_second_iteration, for
    its reason: the first step moves every weight by a sign-like amount, so rounding-level gradient elements move differently."""
    fix = load_golden(name)
    res, alpha, init, latent, batch, lr = fix["meta"]
    lr, batch, latent = float(lr), int(batch), int(latent)
    G, D, tr = small_trainer(ngan, fix, learning_rate=lr)
    pg = O.as_leaf_params(split_state(fix, "G/"), torch.float64)
    pd = O.as_leaf_params(split_state(fix, "D/"), torch.float64)
    spec = O.NetSpec(image_size_init=int(init), slope=0.2, alpha=float(alpha))
    og = torch.optim.RMSprop([p for p in pg.values() if p.requires_grad], lr=lr)
    od = torch.optim.RMSprop([p for p in pd.values() if p.requires_grad], lr=lr)
    d64 = lambda k: torch.from_numpy(fix[k]).double()
    O.train_step(pg, spec, pd, spec, og, od, d64("real"), d64("z_d"), d64("z_gp"), d64("eps"), d64("z_g"))
    t = lambda k: torch.from_numpy(fix[k]).to(DEV)
    tr.train_iteration(t("real"), z_d=t("z_d"), z_gp=t("z_gp"), eps=t("eps"), z_g=t("z_g"))
    torch.cuda.synchronize()
    checked = 0
    for net, leaves, flat, opt in ((G, pg, tr.flat_g, og), (D, pd, tr.flat_d, od)):
        names = {id(p): n for n, p in net.named_parameters()}
        for p, o, a in zip(flat.params, flat.offsets, flat.active_host):
            leaf = leaves.get(names[id(p)])
            if not a or leaf is None or leaf.grad is None:
                continue
            key = names[id(p)]
            assert rmsprop_close(p.detach().cpu().numpy(), leaf.detach().numpy(), lr), (key, "parameter")
            v = flat.square_avg[o:o + p.numel()].view(p.shape).cpu()
            assert rel(v, opt.state[leaf]["square_avg"]) < 1e-2, (key, rel(v, opt.state[leaf]["square_avg"]))
            checked += 1
    assert checked >= 8
    gen = torch.Generator().manual_seed(2024)
    z_d, z_gp, z_g = (O.sample_latent_vec((batch, latent), generator=gen) for _ in range(3))
    eps = torch.rand(batch, 1, 1, 1, generator=gen)
    want = O.train_step(pg, spec, pd, spec, og, od, d64("real"), z_d.double(), z_gp.double(), eps.double(), z_g.double())
    got = tr.train_iteration(t("real"), z_d=z_d.to(DEV), z_gp=z_gp.to(DEV), eps=eps.to(DEV), z_g=z_g.to(DEV))
    g = np.array([float(got[k]) for k in ("D_loss", "score_real", "score_fake", "D_grad_pen", "G_loss")])
    w = np.array([want[k] for k in ("D_loss", "score_real", "score_fake", "GP", "G_loss")])
    assert np.allclose(g, w, rtol=5e-3, atol=5e-5), (g, w)


def make_32(ngan, optimizer="rmsprop"):
    torch.manual_seed(21)
    G = ngan.models.Generator_PG([32, 16, 16], image_size_init=8, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 16, 32], image_size_init=8)
    G.set_resolution(32, 1.0)
    D.set_resolution(32, 1.0)
    return ngan.train.PGGANTrainer(G.to(DEV), D.to(DEV), learning_rate=1e-3, optimizer=optimizer)


def draws_32(seed, n=3, b=4):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        z = [torch.randn(b, 32, generator=gen) for _ in range(3)]
        z = [(v / v.norm(dim=1, keepdim=True)).to(DEV) for v in z]
        out.append(dict(real=(torch.rand(b, 1, 32, 32, generator=gen) * 2 - 1).to(DEV), z_d=z[0], z_gp=z[1],
                        eps=torch.rand(b, 1, 1, 1, generator=gen).to(DEV), z_g=z[2]))
    return out


def assert_same_training_state(tr, eager):
    for (name, a, b) in [("G", tr.flat_g.flat, eager.flat_g.flat), ("D", tr.flat_d.flat, eager.flat_d.flat),
                         ("G square_avg", tr.flat_g.square_avg, eager.flat_g.square_avg),
                         ("D square_avg", tr.flat_d.square_avg, eager.flat_d.square_avg),
                         ("G step", tr.flat_g.seg_step, eager.flat_g.seg_step), ("D step", tr.flat_d.seg_step, eager.flat_d.seg_step)]:
        assert torch.equal(a, b), f"{name}: {float((a - b).abs().max())}"


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_graph_replay_equals_eager(ngan, mode):
    """A captured RMSprop iteration (the hyper-parameters are device floats, the step counts advance on the device) replayed three times
    on the eager trajectory's draws: parameters, square_avg and step counts bit-equal.  (force_exchange, the three-segment capture,
    needs a process group: test_gpu_rmsprop_dist.py.)"""
    seq = draws_32(5)
    try:
        ngan.ops.set_conv_precision(mode)
        eager, tr = make_32(ngan), make_32(ngan)
        static = {k: seq[0][k].clone() for k in ("z_d", "z_gp", "eps", "z_g")}
        tr.capture(seq[0]["real"], draws=static)
        assert float(tr.flat_g.seg_step.sum()) == 0.0 and float(tr.flat_g.square_avg.abs().max()) == 0.0    # capturing is not training
        for s in seq:
            eager.train_iteration(s["real"], s["z_d"], s["z_gp"], s["eps"], s["z_g"])
            for k, v in static.items():
                v.copy_(s[k])
            tr.replay(s["real"])
        torch.cuda.synchronize()
        assert_same_training_state(tr, eager)
        assert int(tr.flat_g.seg_step[0]) == 3
    finally:
        ngan.ops.set_conv_precision("f32")


def test_checkpoint_resume_continues_the_trajectory(ngan, tmp_path, capsys):
    """Four uninterrupted eager iterations == two, a Checkpointer save, a fresh trainer's load_state(), two more (bit for bit).  An
    Adam checkpoint resumed into a RMSprop trainer loads the networks, starts the optimiser from zero and says so."""
    utils = ngan.utils
    seq = draws_32(8, n=4)
    run = lambda tr, ss: [tr.train_iteration(s["real"], s["z_d"], s["z_gp"], s["eps"], s["z_g"]) for s in ss]
    whole = make_32(ngan)
    run(whole, seq)
    first = make_32(ngan)
    run(first, seq[:2])
    f = str(tmp_path / "GenDisc_r001.pth")
    utils.Checkpointer(first.G, first.D, 1e-3, f, N_epochs=10, verbose=False, device=torch.device(DEV), trainer=first).save_state(2)
    saved = utils.load_checkpoint_dict(f)
    assert saved["optimizer_state"]["kind"] == "rmsprop" and "square_avg" in saved["optimizer_state"]["G"]
    second = make_32(ngan)
    ck = utils.Checkpointer(second.G, second.D, 1e-3, f, N_epochs=10, verbose=False, device=torch.device(DEV), trainer=second)
    ck.load_state()
    assert ck.epoch == 2
    run(second, seq[2:])
    torch.cuda.synchronize()
    assert_same_training_state(second, whole)
    # an Adam checkpoint (written by a default trainer) resumed with RMSprop
    adam = make_32(ngan, "adam")
    run(adam, seq[:1])
    fa = str(tmp_path / "GenDisc_a001.pth")
    utils.Checkpointer(adam.G, adam.D, 1e-3, fa, N_epochs=10, verbose=False, device=torch.device(DEV), trainer=adam).save_state(1)
    rms = make_32(ngan)
    run(rms, seq[:1])                                   # non-zero state that the resume must clear
    capsys.readouterr()
    utils.Checkpointer(rms.G, rms.D, 1e-3, fa, N_epochs=10, verbose=False, device=torch.device(DEV), trainer=rms).load_state()
    out = capsys.readouterr().out
    assert "adam state" in out and "rmsprop optimiser starts fresh" in out and len(out.strip().splitlines()) == 1
    for a, b in zip(rms.G.state_dict().values(), adam.G.state_dict().values()):
        assert torch.equal(a, b)
    for flat in (rms.flat_g, rms.flat_d):
        assert float(flat.square_avg.abs().max()) == 0.0 and float(flat.seg_step.abs().max()) == 0.0


def test_epoch_driver_with_growth(ngan, tmp_path):
    """pggan_train over a RMSprop trainer across two growth events (graph capture on): finite series, and the checkpoint's optimiser
    state says rmsprop, with fewer steps for the blocks that joined late."""
    models, train, utils = ngan.models, ngan.train, ngan.utils
    cfg = types.SimpleNamespace(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[3, 6], N_epochs=9,
                                alpha_step=0.5, learning_rate=1e-4, checkpointing_period=4, ID="r002")
    torch.manual_seed(5)
    G = models.Generator_PG([32, 16, 16], image_size_init=4, latent_dim=32).to(DEV)
    D = models.Discriminator_PG([16, 16, 32], image_size_init=4).to(DEV)
    data = train.TensorImageDataset.synthetic(8, 16, device=DEV)
    tr = train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, alpha_step=cfg.alpha_step, device_latents=True, optimizer="rmsprop")
    f = str(tmp_path / "GenDisc_r002.pth")
    ck = utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=torch.device(DEV), trainer=tr,
                            extra_checkpoint_period=1e3)
    series = train.pggan_train(tr, data, cfg, checkpoint=ck, epoch_final=cfg.N_epochs + 1, log=lambda *_: None)
    assert all(len(v) == 9 and np.isfinite(v).all() for v in series.values())
    assert G.image_size == 16 and G.alpha_value() >= 1
    saved = utils.load_checkpoint_dict(f)
    st = saved["optimizer_state"]
    assert saved["epoch"] == 8 and st["kind"] == "rmsprop" and "exp_avg" not in st["G"]
    steps = dict(zip(st["D"]["names"], st["D"]["step"].tolist()))
    assert steps["layers.0.weight"] > steps["conv_block_list.1.1.weight"] > steps["conv_block_list.0.1.weight"] > 0
    assert all(np.isfinite(v.numpy()).all() for v in st["G"]["square_avg"].values())
