"""The minibatch standard-deviation layer on the GPU (include/ngan_mbstd.h, ops.MinibatchStd / StdField*, Discriminator_PG(mbstd_group=)):
every entry point through the C ABI, per element, against the fp64 restatements of tests/mbstd_cases.py within that file's bound (its
constants are settled on the CPU by tests/test_mbstd_bounds_cpu.py); bit reproducibility and the independence of the groups; the mbstd
critic against the fp64 concat oracle with the measure and the bounds tests/test_gpu_models.py applies to the default critic; and the
trainer: captured against eager, the epoch driver with a growth step, resume, and the switch left off."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import mbstd_cases as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ws(ngan, case):
    b, seg, grp, hh, ch = case
    ge = M.group_size(b // seg, grp)
    n = ngan._C.mbstd_workspace_doubles(b, hh, hh, ch, ge)
    assert n == (b // ge) * -(-(hh * hh * ch) // M.BLOCK_FEATURES)
    return torch.empty(n, device=DEV, dtype=torch.float64), ge


def run_stat(ngan, case, x, gs, h):
    """the three statistic entry points on device tensors -> {name: numpy}"""
    b, seg, grp, hh, ch = case
    w, ge = ws(ngan, case)
    s, dgs = (torch.full((b,), float("nan"), device=DEV) for _ in range(2))
    gx, dx = (torch.full_like(x, float("nan")) for _ in range(2))
    call = ngan._C.call
    call("ngan_mbstd_fwd", x, s, w, b, hh, hh, ch, seg, ge)
    call("ngan_mbstd_bwd", gs, x, gx, b, hh, hh, ch, seg, ge)
    call("ngan_mbstd_bwdbwd", h, gs, x, dgs, dx, w, b, hh, hh, ch, seg, ge)
    return {"mbstd_fwd/s": s, "mbstd_bwd/gx": gx, "mbstd_bwdbwd/dgs": dgs, "mbstd_bwdbwd/dx": dx}


def run_field(ngan, case, d):
    b, _, _, hh, ch = case
    c, g, s, w_std = dev(d["c"]), dev(d["g"]), dev(d["s"]), dev(d["w_std"])
    out = torch.full_like(c, float("nan"))
    gs = torch.full((b,), float("nan"), device=DEV)
    gw = torch.full((ch, 1, 3, 3), float("nan"), device=DEV)
    call = ngan._C.call
    call("ngan_stdfield_add", c, s, w_std, out, b, hh, hh, ch, d["scale"])
    call("ngan_stdfield_ds", g, w_std, gs, b, hh, hh, ch, d["scale"])
    call("ngan_stdfield_dw", g, s, gw, b, hh, hh, ch, d["scale"])
    alone = torch.full_like(c, float("nan"))
    call("ngan_stdfield_add", None, s, w_std, alone, b, hh, hh, ch, d["scale"])        # c = NULL: the field alone
    return {"stdfield_add/out": out, "stdfield_ds/gs": gs, "stdfield_dw/gw": gw}, (out, alone, c)


@pytest.mark.parametrize("case", M.cases(), ids=lambda c: "B{}s{}G{}-H{}C{}".format(*c))
def test_entry_points_against_fp64(ngan, case):
    _, seg, grp, _, _ = case
    worst = {}
    for family in M.families_of(case):
        d = M.inputs(family, case)
        got = {k: v.cpu().numpy() for k, v in run_stat(ngan, case, dev(d["x"]), dev(d["gs"]), dev(d["h"])).items()}
        ref = {"mbstd_fwd/s": M.mbstd_fwd_ref(d["x"], seg, grp)["s"], "mbstd_bwd/gx": M.mbstd_bwd_ref(d["gs"], d["x"], seg, grp)["gx"]}
        ref.update({"mbstd_bwdbwd/" + k: v for k, v in M.mbstd_bwdbwd_ref(d["h"], d["gs"], d["x"], seg, grp).items()})
        if family == "random":
            f, (out, alone, c) = run_field(ngan, case, d)
            got.update({k: v.cpu().numpy() for k, v in f.items()})
            ref["stdfield_add/out"] = M.stdfield_add_ref(d["c"], d["s"], d["w_std"], d["scale"])["out"]
            ref["stdfield_ds/gs"] = M.stdfield_ds_ref(d["g"], d["w_std"], d["scale"])["gs"]
            ref["stdfield_dw/gw"] = M.stdfield_dw_ref(d["g"], d["s"], d["scale"])["gw"]
            zero = M.stdfield_add_ref(np.zeros_like(d["c"]), d["s"], d["w_std"], d["scale"])["out"]
            assert M.ratio(alone.cpu().numpy(), *zero, M.c_acc("stdfield_add/out")) <= 1.0
        assert set(got) == set(ref)
        for k, (r, a, n) in ref.items():
            assert np.isfinite(got[k]).all(), (family, k)
            q = M.ratio(got[k].reshape(r.shape), r, a, n, M.c_acc(k))
            worst[k] = max(worst.get(k, 0.0), q)
            print(f"STAT {k} {family} case={case}: err/bound {q:.3f}")
            assert q <= 1.0, (family, k, q)
        ge = M.group_size(case[0] // seg, grp)
        if family == "constant_group":          # d = 0 exactly under the pair sum: exact zeros, exact sqrt(eps)
            assert not got["mbstd_bwd/gx"].any() and (got["mbstd_fwd/s"] == np.sqrt(np.float32(1e-8))).all()
        if ge == 1:                             # the statistic is the constant sqrt(eps) and its gradient is zero
            assert not got["mbstd_bwd/gx"].any() and (got["mbstd_fwd/s"] == np.sqrt(np.float32(1e-8))).all()


@pytest.mark.parametrize("case", [(8, 1, 4, 4, 16), (8, 2, 4, 16, 128), (6, 1, 4, 3, 20)], ids=str)
def test_bit_reproducible_and_groups_independent(ngan, case):
    b, seg, grp, hh, ch = case
    d = M.inputs("random", case)
    x, gs, h = dev(d["x"]), dev(d["gs"]), dev(d["h"])
    first = run_stat(ngan, case, x, gs, h)
    again = run_stat(ngan, case, x, gs, h)
    for k in first:
        assert torch.equal(first[k], again[k]), k
    f1, _ = run_field(ngan, case, d)
    f2, _ = run_field(ngan, case, d)
    for k in f1:
        assert torch.equal(f1[k], f2[k]), k
    # other inputs in every group but the first: the first group's outputs keep their bits
    ge = M.group_size(b // seg, grp)
    o = M.inputs("large", case)
    x2, gs2, h2 = x.clone(), gs.clone(), h.clone()
    x2[ge:], gs2[ge:], h2[ge:] = dev(o["x"])[ge:], dev(o["gs"])[ge:], dev(o["h"])[ge:]
    other = run_stat(ngan, case, x2, gs2, h2)
    for k in first:
        assert torch.equal(first[k][:ge], other[k][:ge]), k
        assert not torch.equal(first[k][ge:], other[k][ge:]), k


def test_host_side_checks(ngan):
    lib, call = ngan._C.lib(), ngan._C.call
    x = torch.zeros(8, 2, 2, 4, device=DEV)
    s = torch.zeros(8, device=DEV)
    w = torch.zeros(8, device=DEV, dtype=torch.float64)
    for args, word in (((8, 2, 2, 4, 3, 2), "segments"), ((8, 2, 2, 4, 2, 3), "G_eff"), ((8, 2, 2, 6, 1, 4), "C=6"), ((0, 2, 2, 4, 1, 1), "B=0")):
        with pytest.raises(RuntimeError, match=word):
            call("ngan_mbstd_fwd", x, s, w, *args)
    with pytest.raises(RuntimeError, match="16-byte"):
        call("ngan_mbstd_fwd", x.reshape(-1)[1:33].reshape(2, 2, 2, 4), s, w, 2, 2, 2, 4, 1, 2)
    assert lib.ngan_mbstd_workspace_doubles(8, 2, 2, 4, 3) == 0
    assert {"ngan_mbstd_fwd", "ngan_mbstd_bwd", "ngan_mbstd_bwdbwd", "ngan_stdfield_add", "ngan_stdfield_ds", "ngan_stdfield_dw",
            "ngan_mbstd_workspace_doubles"} <= set(ngan._C.exported_symbols())


def test_operators_close_under_double_backward(ngan):
    """ops.MinibatchStd -> StdFieldAdd through torch.autograd at both orders against the fp64 concat formulation, with the kernels'
    bounds scaled by nothing: the operators add no arithmetic of their own, so the per-element bounds of the entry points apply to the
    pieces; here the composed result is held to 1e-5 of its max-norm (fp32 through three operators), and third order is refused"""
    ops = ngan.ops
    case = (8, 2, 4, 4, 16)
    d = M.inputs("random", case)
    x = dev(d["x"]).requires_grad_()
    w_std = dev(d["w_std"]).requires_grad_()
    c = dev(d["c"])
    with ops.mbstd_segments(2):
        assert ops.mbstd_segment_count() == 2
        out = ops.StdFieldAdd.apply(c, ops.MinibatchStd.apply(x, ops.mbstd_segment_count(), 4), w_std, d["scale"])
    assert ops.mbstd_segment_count() == 1
    g = dev(d["g"])
    (gx,) = torch.autograd.grad(out, x, g, create_graph=True)
    # a random cotangent on gx: sum(gx^2) would not do -- over a group it is gs_g^2 / (G J^2) sum_j (1 - eps / sigma_j^2), constant in x
    # but for eps, and its x-derivative is pure cancellation
    pen = (gx * dev(d["h"])).sum()
    dx, dw = torch.autograd.grad(pen, (x, w_std))
    # fp64 twin
    x64, w64 = (torch.tensor(d[k].astype(np.float64), requires_grad=True) for k in ("x", "w_std"))
    s64 = M.mbstd_torch(x64, 2, 4)
    T = torch.einsum("cij,ijyx->yxc", w64[:, 0], torch.tensor(M.tap_masks(4, 4)))
    out64 = torch.tensor(d["c"].astype(np.float64)) + d["scale"] * s64[:, None, None, None] * T
    (gx64,) = torch.autograd.grad(out64, x64, torch.tensor(d["g"].astype(np.float64)), create_graph=True)
    dx64, dw64 = torch.autograd.grad((gx64 * torch.tensor(d["h"].astype(np.float64))).sum(), (x64, w64))
    for name, a, r in (("out", out, out64), ("gx", gx, gx64), ("dx", dx, dx64), ("dw", dw, dw64)):
        err = float((a.detach().cpu().double() - r.detach()).abs().max() / r.detach().abs().max())
        print(f"STAT operators {name}: {err:.2e} of the max-norm")
        assert err < 1e-5, (name, err)
    (gx3,) = torch.autograd.grad(ops.MinibatchStd.apply(x, 1, 4), x, dev(d["gs"]), create_graph=True)
    with pytest.raises(NotImplementedError, match="third-order"):
        torch.autograd.grad((gx3 * gx3).sum(), x, create_graph=True)
    with ops.inputs_only():           # the penalty's first pass wants no critic weight gradients
        assert torch.autograd.grad(ops.StdFieldAdd.apply(c, ops.MinibatchStd.apply(x, 1, 4), w_std, d["scale"]), (x, w_std), g,
                                   allow_unused=True)[1] is None
    with pytest.raises(NotImplementedError, match="bf16"):
        ops.MinibatchStd.apply(x.detach().to(torch.bfloat16), 1, 4)


# ---- the critic ---------------------------------------------------------------------------------------------------------------------
def rel(a, b):
    """the measure of tests/test_gpu_models.py"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def model_quantities(ngan, widths, res, alpha, group, seed=3):
    """(got, want): scores, D_loss and its two means, penalty, |grad D|, the critic's gradients of D_loss + penalty and the generator's
    gradients through the critic -- the HIP path in exact fp32, and the fp64 concat oracle (the reference's separate critic calls)"""
    O, LF = M.O, ngan.loss_functions
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG(widths[::-1], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG(widths, image_size_init=4, mbstd_group=group)
    if res != 4:
        G.set_resolution(res, alpha)
        D.set_resolution(res, alpha)
    pg = O.as_leaf_params({k: v.detach().clone() for k, v in G.state_dict().items()}, torch.float64)
    pd = O.as_leaf_params({k: v.detach().clone() for k, v in D.state_dict().items()}, torch.float64)
    spec = O.NetSpec(image_size_init=4, slope=0.2, alpha=alpha)
    b = 4
    x = torch.rand(b, 1, res, res) * 2 - 1
    z1, z2, z3 = (O.sample_latent_vec((b, 32)) for _ in range(3))
    eps = torch.rand(b, 1, 1, 1)
    x64, e64 = x.double(), eps.double()
    Dw = (lambda p, im: M.mbstd_discriminator_forward(p, im, spec, group)) if group else (lambda p, im: O.discriminator_forward(p, im, spec))
    want = {}
    s_real = Dw(pd, x64)
    with torch.no_grad():
        fake = O.generator_forward(pg, z1.double(), spec)
        x_tilde = O.generator_forward(pg, z2.double(), spec)
    s_fake = Dw(pd, fake)
    d_loss = -s_real.mean() + s_fake.mean() + 0.001 * (s_real ** 2).mean()
    x_hat = (e64 * x64 + (1 - e64) * x_tilde).requires_grad_()
    (gr,) = torch.autograd.grad(Dw(pd, x_hat).sum(), x_hat, create_graph=True)
    norms = gr.norm(2, dim=(1, 2, 3))
    gp = 10.0 * ((norms - 1) ** 2).mean()
    (d_loss + gp).backward()
    want.update(scores=s_real.detach().numpy(), scal=np.array([float(d_loss), float(s_real.mean()), float(s_fake.mean()), float(gp)]),
                norms=norms.detach().numpy(), dgrads={k: v.grad.numpy().copy() for k, v in pd.items() if v.grad is not None})
    g_loss = -Dw(pd, O.generator_forward(pg, z3.double(), spec)).mean()
    O.zero_grads(pg)
    g_loss.backward()
    want.update(g_loss=float(g_loss), ggrads={k: v.grad.numpy().copy() for k, v in pg.items() if v.grad is not None})
    # HIP
    ngan.ops.set_conv_precision("f32")
    G.to(DEV)
    D.to(DEV)
    xd = x.to(DEV)
    got = {}
    with torch.no_grad():
        got["scores"] = D(xd).cpu().numpy()
    d2, sr2, sf2 = LF.D_W_loss(G, D, 0.001, check_nan=False)(xd, z=z1.to(DEV))
    pen = LF.D_grad_pen_loss(G, D, 10.0)
    gp2 = pen(xd, z=z2.to(DEV), epsilon=eps.to(DEV))
    (d2 + gp2).backward()
    got.update(scal=np.array([float(d2), float(sr2), float(sf2), float(gp2)]), norms=pen.last_grad_norms.cpu().numpy(),
               dgrads={k: p.grad.detach().cpu().numpy().copy() for k, p in D.named_parameters() if p.grad is not None})
    G.zero_grad()
    g2, _ = LF.G_W_loss(G, D, check_nan=False)(xd, z=z3.to(DEV))
    g2.backward()
    got.update(g_loss=float(g2), ggrads={k: p.grad.detach().cpu().numpy().copy() for k, p in G.named_parameters() if p.grad is not None})
    return got, want


def check_model(got, want, tag):
    """tests/test_gpu_models.py's bounds for the default critic: scores and |grad D| 1e-3, the scalars rtol 1e-3 / atol 2e-5, every
    parameter gradient 2e-3 of its max-norm (with that file's absolute slack on a one-element gradient)"""
    q = {"scores": rel(got["scores"], want["scores"]), "norms": rel(got["norms"], want["norms"])}
    print(f"STAT model {tag}: scores {q['scores']:.2e} |grad D| {q['norms']:.2e} scalars {got['scal']} / {want['scal']}")
    assert q["scores"] < 1e-3 and q["norms"] < 1e-3, (tag, q)
    assert np.allclose(got["scal"], want["scal"], rtol=1e-3, atol=2e-5), (tag, got["scal"], want["scal"])
    assert abs(got["g_loss"] - want["g_loss"]) < 1e-3 * abs(want["g_loss"]) + 2e-5
    for side in ("dgrads", "ggrads"):
        assert set(got[side]) == set(want[side]), (tag, side, set(got[side]) ^ set(want[side]))
        for k, v in want[side].items():
            g = got[side][k]
            if v.size == 1 and abs(float(g.ravel()[0]) - float(v.ravel()[0])) < 5e-7:
                continue
            r = rel(g, v)
            print(f"STAT model {tag} {side} {k}: {r:.2e}")
            assert r < 2e-3, (tag, side, k, r)


@pytest.mark.parametrize("state", [("stable", 4, 1.0), ("transition", 8, 0.5), ("merged", 8, 1.0)], ids=lambda s: s[0])
def test_critic_against_the_fp64_concat_oracle(ngan, state):
    name, res, alpha = state
    got, want = model_quantities(ngan, [16, 16], res, alpha, 4)
    assert any(k.endswith("weight_std") for k in want["dgrads"])
    check_model(got, want, name)


def test_compatibility_width_critic(ngan):
    got, want = model_quantities(ngan, [8, 8], 8, 1.0, 4)
    check_model(got, want, "widths 8")


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------
def make_trainer(ngan, group=None, seed=11, **kw):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([32, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 32], image_size_init=4, **({} if group is None else {"mbstd_group": group}))
    G.set_resolution(8, 0.5)
    D.set_resolution(8, 0.5)
    return ngan.train.PGGANTrainer(G.to(DEV), D.to(DEV), learning_rate=1e-3, grad_pen_lambda=10.0, **kw)


def draw(gen, b, res=8):
    z = [torch.randn(b, 32, generator=gen) for _ in range(3)]
    z = [(v / v.norm(dim=1, keepdim=True)).to(DEV) for v in z]
    return dict(real=(torch.rand(b, 1, res, res, generator=gen) * 2 - 1).to(DEV), z_d=z[0], z_gp=z[1],
                eps=torch.rand(b, 1, 1, 1, generator=gen).to(DEV), z_g=z[2])


@pytest.mark.parametrize("kw", [{}, {"objective": "lsgan"}, {"optimizer": "rmsprop", "ema_beta": 0.99}, {"diffaug": "color,translation,cutout"}],
                         ids=["wgan-gp", "lsgan", "rmsprop-ema", "diffaug"])
def test_captured_iteration_equals_eager(ngan, kw):
    """the criterion of tests/test_gpu_train.py: the replayed trajectory equals the eager one bit for bit"""
    gen = torch.Generator().manual_seed(5)
    seq = [draw(gen, 4) for _ in range(3)]
    eager, tr = make_trainer(ngan, 4, **kw), make_trainer(ngan, 4, **kw)
    static = {k: seq[0][k].clone() for k in ("z_d", "z_gp", "eps", "z_g")}
    tr.capture(seq[0]["real"], draws=static)
    for s in seq:
        stats = eager.train_iteration(s["real"], s["z_d"], s["z_gp"], s["eps"], s["z_g"])
        for k, v in static.items():
            v.copy_(s[k])
        tr.replay(s["real"])
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in stats.values())
    assert "layers.0.weight_std" in tr.flat_d.names
    for name, p, pe in zip(tr.flat_g.names + tr.flat_d.names, tr.flat_g.params + tr.flat_d.params, eager.flat_g.params + eager.flat_d.params):
        assert torch.equal(p, pe), f"{name}: {float((p - pe).abs().max())}"


def test_switch_off_is_the_trainer_without_the_argument(ngan):
    gen = torch.Generator().manual_seed(6)
    s = draw(gen, 4)
    plain, off, on = make_trainer(ngan), make_trainer(ngan, 0), make_trainer(ngan, 4)
    for tr in (plain, off, on):
        tr.train_iteration(s["real"], s["z_d"], s["z_gp"], s["eps"], s["z_g"])
    torch.cuda.synchronize()
    assert plain.flat_d.names == off.flat_d.names and plain.flat_d.total == off.flat_d.total
    for name, p, q in zip(plain.flat_g.names + plain.flat_d.names, plain.flat_g.params + plain.flat_d.params, off.flat_g.params + off.flat_d.params):
        assert torch.equal(p, q), name
    assert any(not torch.equal(p, q) for p, q in zip(plain.flat_g.params, on.flat_g.params))        # and on, it acts


def test_epoch_driver_grows_checkpoints_and_resumes_bit_identically(ngan, tmp_path):
    """four epochs at batch 4 with one growth step: finite, checkpointed; the same run resumed from its epoch-2 checkpoint (mid fade-in)
    continues with the bits of the uninterrupted one"""
    import shutil
    import test_gpu_epoch_dist as E
    models, train, utils = ngan.models, ngan.train, ngan.utils
    cfg = types.SimpleNamespace(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[2], N_epochs=4,
                                alpha_step=0.5, learning_rate=1e-3, checkpointing_period=2, ID="m001")

    def fresh(f):
        torch.manual_seed(5)
        G = models.Generator_PG([32, 16], image_size_init=4, latent_dim=32).to(DEV)
        D = models.Discriminator_PG([16, 32], image_size_init=4, mbstd_group=4).to(DEV)
        tr = train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, alpha_step=cfg.alpha_step, grad_pen_lambda=10.0, device_latents=True)
        ck = utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=torch.device(DEV), trainer=tr,
                                extra_checkpoint_period=1e3)
        return G, D, tr, ck

    data = train.TensorImageDataset.synthetic(8, 8, device=DEV)
    f, f2 = str(tmp_path / "GenDisc_m001.pth"), str(tmp_path / "GenDisc_m002.pth")
    kept = {}

    def at_epoch_3(epoch, trainer):
        if epoch == 3:          # the epoch-2 checkpoint before epoch 4 overwrites it, and the host generator the batch order is drawn from
            shutil.copy(f, f2)
            kept["rng"] = torch.get_rng_state()

    G, D, tr, ck = fresh(f)
    torch.manual_seed(77)
    series = train.pggan_train(tr, data, cfg, checkpoint=ck, log=lambda *_: None, on_epoch=at_epoch_3, draws=E.pg_draws(32))
    assert all(len(v) == 4 and np.isfinite(v).all() for v in series.values())
    assert D.image_size == 8 and D.alpha_value() >= 1 and "layers.1.weight_std" in D.state_dict()
    saved, mid = utils.load_checkpoint_dict(f), utils.load_checkpoint_dict(f2)
    assert saved["epoch"] == 4 and mid["epoch"] == 2 and "layers.1.weight_std" in saved["Discriminator_state"]
    assert saved["Discriminator_attrs"]["mbstd_group"] == 4 and "layers.0.weight_std" in saved["optimizer_state"]["D"]["names"]
    back = models.Discriminator_PG.from_state_dict(f, verbose=False)
    assert back.mbstd_group == 4 and back.image_size == 8
    # resume from the epoch-2 file into fresh nets, as train._train_main does
    G2, D2, tr2, ck2 = fresh(f2)
    ck2.load_state()
    assert ck2.epoch == 2 and D2.image_size == mid["Discriminator_attrs"]["image_size"]
    lr0 = train.lr_schedule(2, cfg.learning_rate, cfg.transit_sch, cfg.N_epochs)
    if lr0 is not None:
        tr2.set_lr(lr0)
    torch.set_rng_state(kept["rng"])
    train.pggan_train(tr2, data, cfg, checkpoint=ck2, epoch_init=3, log=lambda *_: None, draws=E.pg_draws(32))
    torch.cuda.synchronize()
    for (k, a), b in zip(list(D.state_dict().items()) + list(G.state_dict().items()), list(D2.state_dict().values()) + list(G2.state_dict().values())):
        assert torch.equal(a, b), k


# ---- data parallel ----------------------------------------------------------------------------------------------------------------------
def _dp_nets(ngan):
    torch.manual_seed(13)
    G = ngan.models.Generator_PG([32, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 32], image_size_init=4, mbstd_group=4)
    G.set_resolution(8, 0.5)
    D.set_resolution(8, 0.5)
    return G.to(DEV), D.to(DEV)


def _mbstd_rank_worker(rank, world, port, q):
    import datetime
    import traceback
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.set_num_threads(4)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    out = {}
    try:
        from __graft_entry__ import load_package
        import test_gpu_epoch_dist as E
        ngan = load_package()
        own = [dist.new_group([r]) for r in range(world)][rank]
        data = {k: v.to(DEV) for k, v in E.draw_batch(900, 8, 32, 8).items()}
        mine = {k: v[4 * rank:4 * rank + 4] for k, v in data.items()}
        tr = ngan.train.PGGANTrainer(*_dp_nets(ngan), learning_rate=1e-3, grad_pen_lambda=10.0)
        ref = ngan.train.PGGANTrainer(*_dp_nets(ngan), learning_rate=1e-3, grad_pen_lambda=10.0, process_group=own)
        assert tr.world == world and ref.world == 1
        tr.d_compute(mine["real"], mine["z_d"], mine["z_gp"], mine["eps"], global_batch=8)
        tr._exchange(tr.flat_d)
        ref.d_compute(data["real"], data["z_d"], data["z_gp"], data["eps"])
        out["critic grad"] = E.grad_error(tr.flat_d, ref.flat_d, world)
        tr.g_compute(mine["real"], mine["z_g"], global_batch=8)
        tr._exchange(tr.flat_g)
        tr.materialize_stem_grad()
        ref.g_compute(data["real"], data["z_g"])
        ref.materialize_stem_grad()
        out["generator grad"] = E.grad_error(tr.flat_g, ref.flat_g, world)
        out["has weight_std"] = "layers.0.weight_std" in tr.flat_d.names
        torch.cuda.synchronize()
    except Exception:  # noqa: BLE001
        out["exception"] = traceback.format_exc()
    finally:
        q.put((rank, out))
        dist.destroy_process_group()


def test_two_ranks_of_four_give_the_gradients_of_one_batch_of_eight():
    """contiguous groups: shares of 4 + 4 at G = 4 hold the very groups of the batch of 8, so the exchanged gradients are the
    one-process gradients within tests/test_gpu_epoch_dist.py's bound for that comparison.  Two gloo ranks on the one GPU, fresh
    child processes, as that file starts them"""
    import torch.multiprocessing as mp
    import test_gpu_epoch_dist as E
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = E._free_port()
    procs = [ctx.Process(target=_mbstd_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(world):
            r, out = q.get(timeout=240)
            got[r] = out
    finally:
        for p in procs:
            p.join(30)
            if p.is_alive():
                p.terminate()
    assert sorted(got) == [0, 1] and all(p.exitcode == 0 for p in procs), ([p.exitcode for p in procs], sorted(got))
    for r in (0, 1):
        assert "exception" not in got[r], got[r]["exception"]
        print(f"STAT rank {r}: {got[r]}")
        assert got[r]["has weight_std"] and got[r]["critic grad"] < E.BOUND and got[r]["generator grad"] < E.BOUND, got[r]
