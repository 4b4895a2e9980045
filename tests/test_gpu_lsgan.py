"""The least-squares objective on the GPU: the two scalar heads (csrc/pointwise.hip) through the C ABI per element against fp64
(bounds settled on the CPU, tests/test_lsgan_bounds_cpu.py), their argument checks, D_LS_loss / G_LS_loss and their parameter
gradients against the CPU oracle, and the trainer with objective="lsgan": the default objective is the trainer without the argument,
eager equals replayed, a fixed batch descends, two ranks with shares 3 and 1 reproduce one rank on the whole batch, and the epoch
driver writes a checkpoint that carries the objective, resumes bit-equal and refuses the other objective.

Per element   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref,   C_ACC = 8, n_round and absref per output in
tests/lsgan_cases.py.  Every output buffer starts as NaN, so an element no thread wrote fails the comparison.

measured on MI355X (a record, not a bound: worst err / bound per output over all cases; 1 is the bound): lsloss_head loss 0.165
mean_real 0.100 mean_fake 0.100; lsloss_head_bwd 0.204 -- the emulation's figures (tests/test_lsgan_bounds_cpu.py) to three digits:
no constant moved.  Two ranks with shares 3 and 1: worst deviation / scale 3.3e-7 (critic), 9.2e-8 (generator) against the bound 2e-4.
The module takes 10 s."""
import ctypes
import datetime
import functools
import os
import socket
import sys
import traceback
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import lsgan_cases as L

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
f32 = np.float32


def _np(t):
    return t.detach().cpu().numpy().copy()


def dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nans(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(family, n_real, n_fake, t_real, t_fake):
    """inputs and fp64 references of one case: computed once, shared, never modified"""
    d = L.inputs(family, n_real, n_fake, t_real, t_fake)
    head = L.lsloss_head_ref(d["scores"], n_real, n_fake, t_real, t_fake)
    bwd = [(p, L.lsloss_head_bwd_ref(d["scores"], n_real, n_fake, t_real, t_fake, *p)["gs"]) for p in L.null_patterns(d["g"])]
    return d, head, bwd


@pytest.mark.parametrize("family", L.FAMILIES)
@pytest.mark.parametrize("n_real,n_fake", L.CASES)
def test_lsloss_head_and_bwd_against_fp64(ngan, n_real, n_fake, family):
    """ngan_lsloss_head; ngan_lsloss_head_bwd with all three output gradients and with each of them null in turn"""
    call = ngan._C.call
    bad = []

    def ck(name, got, ref, tag):
        r, a, n = ref
        worst = L.ratio(_np(got), r, a, n, L.c_acc(name))
        print(f"STAT lsgan {name} {(family, n_real, n_fake) + tag}: {worst:.3f}")
        if not worst <= 1.0:
            bad.append((name, tag, worst))

    for t_real, t_fake in L.TARGETS:
        d, head, bwd = case(family, n_real, n_fake, t_real, t_fake)
        scores = dv(d["scores"])
        loss, mr, mf = nans(1), nans(1), nans(1)
        call("ngan_lsloss_head", scores, n_real, n_fake, t_real, t_fake, loss, mr, mf)
        for k, out in (("loss", loss), ("mean_real", mr), ("mean_fake", mf)):
            ck(f"lsloss_head/{k}", out, head[k], (t_real, t_fake))
        if n_fake == 0:
            assert float(mf) == 0.0                                       # the generator form
        again = nans(1)
        call("ngan_lsloss_head", scores, n_real, n_fake, t_real, t_fake, again, nans(1), nans(1))
        assert torch.equal(again, loss)                                    # fixed summation order: bit-reproducible
        for (gl, gr, gf), ref in bwd:
            gs = nans(n_real + n_fake + 1)
            gs[-1] = 7.0
            ptr = [None if v is None else dv(np.array([v], f32)) for v in (gl, gr, gf)]
            call("ngan_lsloss_head_bwd", scores, n_real, n_fake, t_real, t_fake, ptr[0], ptr[1], ptr[2], gs)
            assert float(gs[-1]) == 7.0, "wrote past the scores"
            ck("lsloss_head_bwd/gs", gs[:-1], ref, (t_real, t_fake, gl is None, gr is None, gf is None))
    if family == "on_target":
        # a score on its target contributes an exact zero to the squared part's gradient
        d, _, _ = case(family, n_real, n_fake, 1.0, 0.0)
        gs = nans(n_real + n_fake)
        call("ngan_lsloss_head_bwd", dv(d["scores"]), n_real, n_fake, 1.0, 0.0, dv(np.array([0.7], f32)), None, None, gs)
        assert not _np(gs)[:(n_real + 3) // 4].any()
    assert not bad, bad


def test_bad_arguments_return_a_status_and_launch_nothing(ngan):
    lib = ngan._C.lib()
    scores = torch.ones(8, device=DEV)
    outs = [torch.full((8,), 7.0, device=DEV) for _ in range(4)]
    one = torch.ones(1, device=DEV)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    got = []
    for n_real, n_fake in ((0, 4), (-1, 4), (4, -1)):
        got.append(lib.ngan_lsloss_head(p(scores), n_real, n_fake, 1.0, 0.0, p(outs[0]), p(outs[1]), p(outs[2]), s))
        got.append(lib.ngan_lsloss_head_bwd(p(scores), n_real, n_fake, 1.0, 0.0, p(one), p(one), p(one), p(outs[3]), s))
    got.append(lib.ngan_lsloss_head(None, 4, 4, 1.0, 0.0, p(outs[0]), p(outs[1]), p(outs[2]), s))
    got.append(lib.ngan_lsloss_head(p(scores), 4, 4, 1.0, 0.0, p(outs[0]), None, p(outs[2]), s))
    got.append(lib.ngan_lsloss_head_bwd(p(scores), 4, 4, 1.0, 0.0, p(one), p(one), p(one), None, s))
    got.append(lib.ngan_lsloss_head_bwd(None, 4, 4, 1.0, 0.0, p(one), p(one), p(one), p(outs[3]), s))
    torch.cuda.synchronize()
    assert all(v < 0 for v in got), got
    assert all(bool((o == 7.0).all()) for o in outs)
    with pytest.raises(RuntimeError, match=r"ngan_lsloss_head failed with status -\d+: .*lsloss_head"):
        ngan._C.call("ngan_lsloss_head", scores, 0, 8, 1.0, 0.0, outs[0], outs[1], outs[2])
    # the Python operator: null incoming gradients reach the kernel as null pointers, and no gradient at all launches nothing
    sc = torch.randn(6, device=DEV, requires_grad=True)
    loss, m_r, m_f = ngan.ops.LSLossHead.apply(sc, 4, 1.0, 0.0)
    (g,) = torch.autograd.grad(m_f, sc)
    assert torch.equal(g, torch.tensor([0, 0, 0, 0, 0.5, 0.5], device=DEV))


# ---------------------------------------------------------------------------------------------------------------------
# the two losses against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [10.0, 0.0])
@pytest.mark.parametrize("n_colors,alpha", [(1, 0.5), (3, 1.0)])
def test_losses_and_gradients_match_oracle(ngan, n_colors, alpha, lam, conv_precision):
    """test_gpu_diffaug.py::test_losses_and_gradients_match_oracle_through_the_transform without the transform and with the two
    least-squares formulae (reference loss_functions.py:99, 133) evaluated over the oracle's scores; its bounds.  The generator's
    gradient is the departure from the reference (which detaches the generated images): it must be there."""
    from oracle import pggan_oracle as O
    res = 16
    torch.manual_seed(11 + n_colors + res)
    G = ngan.models.Generator_PG([32, 16], image_size_init=8, latent_dim=64, N_colors=n_colors)
    D = ngan.models.Discriminator_PG([16, 32], image_size_init=8, N_colors=n_colors)
    G.set_resolution(res, alpha)
    D.set_resolution(res, alpha)
    pg = O.as_leaf_params({k: v.detach().clone() for k, v in G.state_dict().items()})
    pd = O.as_leaf_params({k: v.detach().clone() for k, v in D.state_dict().items()})
    spec = O.NetSpec(image_size_init=8, slope=0.2, alpha=alpha)
    G.to(DEV)
    D.to(DEV)
    b = 4
    x = torch.rand(b, n_colors, res, res) * 2 - 1
    z1, z2, z3 = (O.sample_latent_vec((b, 64)) for _ in range(3))
    eps = torch.rand(b, 1, 1, 1)
    # oracle (CPU): loss_functions.py:79-112 with the latent injected, the penalty added as the loop adds it (train.py:361-362)
    with torch.no_grad():
        fake = O.generator_forward(pg, z1, spec)
    real_score, fake_score = O.discriminator_forward(pd, x, spec), O.discriminator_forward(pd, fake, spec)
    s_r, s_f = real_score.mean(), fake_score.mean()
    d_loss = torch.mean((real_score - 1) ** 2) + torch.mean(fake_score ** 2)
    gp = O.grad_penalty(pg, spec, pd, spec, x, z2, eps, lam)
    (d_loss + gp).backward()
    # HIP path
    LF = ngan.loss_functions
    Gp = LF.D_grad_pen_loss(G, D, lam)
    xd = x.to(DEV)
    d2, sr2, sf2 = LF.D_LS_loss(G, D, xd, z=z1.to(DEV))
    gp2 = Gp(xd, z=z2.to(DEV), epsilon=eps.to(DEV))
    (d2 + gp2).backward()
    got = np.array([float(d2.detach()), float(sr2.detach()), float(sf2.detach()), float(gp2.detach())])
    want = np.array([float(d_loss.detach()), float(s_r.detach()), float(s_f.detach()), float(gp.detach())])
    print("LSGAN losses", got, want)
    assert np.allclose(got, want, rtol=1e-3, atol=2e-5), (got, want)
    assert (lam > 0) == (want[3] > 0)
    tol_l2, tol_out = 2e-3, 1e-3

    def close(got, ref, scale):
        d = (got.cpu().double() - ref.double())
        l2 = float(d.norm() / (ref.double().norm() + 1e-2 * scale))
        outliers = float((d.abs() > 1e-2 * (float(ref.abs().max()) + 1e-2 * scale)).double().mean())
        return l2 < tol_l2 and outliers <= tol_out, (l2, outliers)

    gmax = max(float(v.grad.abs().max()) for v in pd.values() if v.grad is not None)
    n_checked = 0
    for k, p in D.named_parameters():
        if p.grad is not None:
            ok, info = close(p.grad, pd[k].grad, gmax)
            assert ok, ("D", k, info)
            n_checked += 1
    assert n_checked >= 6 and gmax > 0
    # the positional call of the reference, with its unused Lambda, draws its own latents
    d3 = LF.D_LS_loss(G, D, xd, 10.0)
    assert len(d3) == 3 and all(t.dim() == 0 and bool(torch.isfinite(t)) for t in d3)
    g_ref = torch.mean((O.discriminator_forward(pd, O.generator_forward(pg, z3, spec), spec) - 1) ** 2)
    s_g = float(O.discriminator_forward(pd, O.generator_forward(pg, z3, spec), spec).mean().detach())
    g_ref.backward()
    g2, sg2 = LF.G_LS_loss(G, D, xd, z=z3.to(DEV))
    g2.backward()
    assert abs(float(g2.detach()) - float(g_ref.detach())) < 1e-3 * abs(float(g_ref.detach())) + 2e-5
    assert abs(float(sg2) - s_g) < 1e-3 * abs(s_g) + 2e-5
    gmax = max(float(v.grad.abs().max()) for v in pg.values() if v.grad is not None)
    n_checked = 0
    for k, p in G.named_parameters():
        if p.grad is not None:
            ok, info = close(p.grad, pg[k].grad, gmax)
            assert ok, ("G", k, info)
            assert float(p.grad.abs().max()) > 0, k                       # the gradient flows into the generator
            n_checked += 1
    assert n_checked >= 4 and gmax > 0


# ---------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------
LATENT = 32


def small_nets(ngan, seed=6, res=16):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([32, 16], image_size_init=8, latent_dim=LATENT)
    D = ngan.models.Discriminator_PG([16, 32], image_size_init=8)
    if res != 8:
        G.set_resolution(res, 1.0)
        D.set_resolution(res, 1.0)
    return G.to(DEV), D.to(DEV)


def _unit(g, n):
    v = torch.randn(n, LATENT, generator=g)
    return v / v.norm(dim=1, keepdim=True)


def batch_draws(ngan, seed, n, mask=0, res=16):
    """reals, latents, epsilon and (mask: a diffaug policy) augmentation tables of one batch from seeded generators"""
    g = torch.Generator().manual_seed(seed)
    d = dict(real=(torch.rand(n, 1, res, res, generator=g) * 2 - 1).to(DEV), z_d=_unit(g, n).to(DEV), z_gp=_unit(g, n).to(DEV),
             eps=torch.rand(n, 1, 1, 1, generator=g).to(DEV), z_g=_unit(g, n).to(DEV), tables=None)
    if mask:
        u = torch.rand(4 * n, 8, generator=g).to(DEV)
        t = torch.empty((4 * n, 8), dtype=torch.int32, device=DEV)
        ngan.ops.diffaug_params(u, t, res, mask, 1.0)
        d["tables"] = dict(real=t[:n].clone(), fake=t[n:3 * n].clone(), gen=t[3 * n:].clone())
    return d


def state_of(tr):
    ts = [tr.flat_g.flat, tr.flat_d.flat, tr.flat_g.exp_avg, tr.flat_g.exp_avg_sq, tr.flat_d.exp_avg, tr.flat_d.exp_avg_sq,
          tr.flat_g.seg_step, tr.flat_d.seg_step] + ([tr.flat_g.ema] if tr.ema_enabled else [])
    return [_np(t) for t in ts]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def test_the_default_objective_is_the_trainer_without_the_argument(ngan):
    """objective="wasserstein": bit-equal parameters and optimiser state after three iterations, eager and replayed, and the same
    global RNG states; objective="lsgan" ends elsewhere (and draws as much)"""
    def run(replayed, **kw):
        G, D = small_nets(ngan)
        tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3, device_latents=True, **kw)
        torch.manual_seed(21)
        x = batch_draws(ngan, 3, 4)["real"]
        for _ in range(3):
            if replayed:
                tr.step(x)
            else:
                tr.train_iteration(x)
        torch.cuda.synchronize()
        return state_of(tr), torch.cuda.get_rng_state(DEV), torch.get_rng_state()
    for replayed in (False, True):
        want = run(replayed)
        got = run(replayed, objective="wasserstein")
        assert same(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), replayed
        other = run(replayed, objective="lsgan")
        assert not same(other[0], want[0]) and torch.equal(other[1], want[1]) and torch.equal(other[2], want[2]), replayed
        assert all(np.isfinite(v).all() for v in other[0])


def eager_and_replayed(ngan, mask=0, **kw):
    """three eager iterations against capture + three replays, batches of 4, 2 (the ragged last one), 4, with injected draws"""
    batches = [batch_draws(ngan, 40 + i, n, mask=mask) for i, n in enumerate((4, 2, 4))]
    eager = ngan.train.PGGANTrainer(*small_nets(ngan), learning_rate=1e-3, objective="lsgan", **kw)
    stats_e = []
    for d in batches:
        s = eager.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"], tables=d["tables"])
        stats_e.append({k: float(v) for k, v in s.items()})
        assert torch.equal(eager.last_z_g, d["z_g"])
    tr = ngan.train.PGGANTrainer(*small_nets(ngan), learning_rate=1e-3, objective="lsgan", **kw)
    statics, stats_r = {}, []
    for d in batches:
        n = d["real"].size(0)
        own = {k: d[k] for k in ("z_d", "z_gp", "eps", "z_g")}
        if not tr.has_graph(d["real"].shape):
            statics[n] = {k: v.clone() for k, v in own.items()}
            tr.capture(d["real"], draws=statics[n], tables=d["tables"])
        for k, v in own.items():
            statics[n][k].copy_(v)
        s = tr.replay(d["real"], tables=d["tables"])
        stats_r.append({k: float(v) for k, v in s.items()})
    torch.cuda.synchronize()
    assert len(statics) == 2
    return eager, tr, stats_e, stats_r, batches


@pytest.mark.parametrize("lam", [10.0, 0.0])
def test_eager_and_replayed_iterations_are_bit_equal(ngan, lam):
    eager, tr, stats_e, stats_r, batches = eager_and_replayed(ngan, grad_pen_lambda=lam)
    assert stats_e == stats_r and all(np.isfinite(list(s.values())).all() for s in stats_e), (stats_e, stats_r)
    assert same(state_of(eager), state_of(tr))
    assert set(stats_e[0]) == {"D_loss", "score_real", "score_fake", "D_grad_pen", "G_loss"}        # the epoch driver's monitors
    assert all((s["D_grad_pen"] > 0) == (lam > 0) and s["G_loss"] >= 0 for s in stats_e)
    # the objective did act: the same draws under the Wasserstein objective end elsewhere
    plain = ngan.train.PGGANTrainer(*small_nets(ngan), learning_rate=1e-3, grad_pen_lambda=lam)
    for d in batches:
        plain.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"])
    assert not same(state_of(plain), state_of(eager))


def test_eager_and_replayed_with_augmentation_and_average(ngan):
    eager, tr, stats_e, stats_r, _ = eager_and_replayed(ngan, mask=6, diffaug="translation,cutout", ema_beta=0.999)
    assert stats_e == stats_r and all(np.isfinite(list(s.values())).all() for s in stats_e), (stats_e, stats_r)
    assert eager.ema_enabled and same(state_of(eager), state_of(tr))
    assert not torch.equal(eager.flat_g.ema, eager.flat_g.flat)


def test_eager_and_replayed_in_the_bf16_mode(ngan):
    try:
        ngan.ops.set_conv_precision("bf16")
        eager, tr, stats_e, stats_r, _ = eager_and_replayed(ngan)
    finally:
        ngan.ops.set_conv_precision("f32")
    assert stats_e == stats_r and all(np.isfinite(list(s.values())).all() for s in stats_e), (stats_e, stats_r)
    assert same(state_of(eager), state_of(tr)) and all(np.isfinite(v).all() for v in state_of(tr))


def test_critic_descends_on_a_fixed_batch(ngan):
    """twenty critic steps at lambda 0 on one batch with fixed latents: the least-squares critic loss ends below where it began.  First
    on the CPU oracle: from these inputs both plain gradient descent and Adam(0.5, 0.999) at lr 1e-3 do decrease it (0.927 -> 0.771
    and -> 0.003 in fp32 and in fp64 alike), so lr 1e-3, the trainer's Adam, is kept."""
    from oracle import pggan_oracle as O
    d = batch_draws(ngan, 3, 4)
    G, D = small_nets(ngan)
    spec = O.NetSpec(image_size_init=8, slope=0.2, alpha=1.0)
    pg = O.as_leaf_params({k: v.detach().cpu().clone() for k, v in G.state_dict().items()})
    pd = O.as_leaf_params({k: v.detach().cpu().clone() for k, v in D.state_dict().items()})
    x, z = d["real"].cpu(), d["z_d"].cpu()
    with torch.no_grad():
        fake = O.generator_forward(pg, z, spec)
    oracle_loss = lambda: (torch.mean((O.discriminator_forward(pd, x, spec) - 1) ** 2) +          # noqa: E731
                           torch.mean(O.discriminator_forward(pd, fake, spec) ** 2))
    sgd = torch.optim.SGD([v for v in pd.values() if v.requires_grad], lr=1e-3)
    first = float(oracle_loss().detach())
    for _ in range(20):
        sgd.zero_grad()
        oracle_loss().backward()
        sgd.step()
    last = float(oracle_loss().detach())
    print("LSGAN descent, oracle, plain descent at lr 1e-3:", first, last)
    assert last < first
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3, grad_pen_lambda=0.0, objective="lsgan")
    losses = [float(tr.d_step(d["real"], z_d=d["z_d"])["D_loss"]) for _ in range(20)]
    losses.append(float(ngan.loss_functions.D_LS_loss(G, D, d["real"], z=d["z_d"])[0].detach()))
    print("LSGAN descent, trainer:", losses[0], losses[-1])
    assert abs(losses[0] - first) < 1e-3 * first + 2e-5 and np.isfinite(losses).all()
    assert losses[-1] < losses[0]


# ---- two ranks on one GPU, shares 3 and 1 -----------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _share_worker(rank, world, port, fixture, q):
    """tests/test_gpu_dist.py::_worker with objective="lsgan" and unequal shares: the share weight through the squared term"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        from __graft_entry__ import load_package
        from conftest import load_golden
        import test_gpu_models as T
        ngan = load_package()
        dev = torch.device("cuda:0")
        fix = load_golden(fixture)
        own = [dist.new_group([r]) for r in range(world)][rank]          # a one-rank group: the single-process reference
        t = lambda k: torch.from_numpy(fix[k]).to(dev)                   # noqa: E731
        shares = [3, 1]
        assert int(fix["meta"][4]) == sum(shares)
        sl = slice(sum(shares[:rank]), sum(shares[:rank + 1]))
        G, D = T.build_small(ngan, fix)
        tr = ngan.train.PGGANTrainer(G, D, objective="lsgan")            # world = 2: exchanges on
        assert tr.world == world and tr.stem is not None
        Gr, Dr = T.build_small(ngan, fix)
        ref = ngan.train.PGGANTrainer(Gr, Dr, process_group=own, objective="lsgan")      # world = 1 on the whole batch
        assert ref.world == 1

        def check(flat, flat_ref, what):
            worst = 0.0
            for name, p, pr, a in zip(flat.names, flat.params, flat_ref.params, flat.active_host):
                if not a:
                    assert float(p.grad.abs().max()) == 0.0, (what, name)
                    continue
                got, want = p.grad / world, pr.grad                      # the fused Adam applies the 1/world factor
                scale = float(want.abs().max()) + 1e-3 * max(float(v.grad.abs().max()) for v in flat_ref.params)
                worst = max(worst, float((got - want).abs().max()) / scale)
            assert worst < 2e-4, (what, worst)
            return worst

        tr.d_compute(t("real")[sl], t("z_d")[sl], t("z_gp")[sl], t("eps")[sl], global_batch=shares)
        tr._exchange(tr.flat_d)
        ref.d_compute(t("real"), t("z_d"), t("z_gp"), t("eps"))
        wd = check(tr.flat_d, ref.flat_d, "critic step")
        tr.g_compute(t("real")[sl], t("z_g")[sl], global_batch=shares)
        tr._exchange(tr.flat_g)
        ref.g_compute(t("real"), t("z_g"))
        wg = check(tr.flat_g, ref.flat_g, "generator step")
        torch.cuda.synchronize()
        q.put((rank, "ok", wd, wg))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None, None))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_shares_3_and_1_match_the_whole_batch():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_share_worker, args=(r, 2, port, "small_res16_fade_warm", q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    results = sorted(q.get(timeout=5) for _ in range(2))
    print("LSGAN shares 3 + 1, worst deviation / scale (critic, generator) per rank:", [r[2:] for r in results])
    assert [r[:2] for r in results] == [(0, "ok"), (1, "ok")], results
    assert all(p.exitcode == 0 for p in procs)


# ---- epoch driver and checkpoint ----------------------------------------------------------------------------------------------------
DRIVER_CFG = dict(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[2], N_epochs=4, alpha_step=0.5,
                  learning_rate=1e-3, checkpointing_period=1, ID="ls", seed=3)


def driver_draws(epoch, k, n):
    g = torch.Generator().manual_seed(10007 * epoch + k)
    return dict(z_d=_unit(g, n), z_gp=_unit(g, n), eps=torch.rand(n, 1, 1, 1, generator=g), z_g=_unit(g, n))


def driver_run(ngan, f, epochs, resume=False, objective="lsgan"):
    """pggan_train on four synthetic 16 x 16 images in one batch per epoch, replayed graphs, given latents: epoch 1 at 8 x 8, the
    growth step to 16 x 16 (fading in) at epoch 2"""
    cfg = types.SimpleNamespace(**DRIVER_CFG)
    G, D = small_nets(ngan, res=8)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, device_latents=True, alpha_step=cfg.alpha_step, objective=objective)
    data = ngan.train.TensorImageDataset.synthetic(4, 16, device=DEV, seed=8)
    ck = ngan.utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=DEV, trainer=tr,
                                 extra_checkpoint_period=1e3)
    if resume:
        ck.load_state()
    series = ngan.train.pggan_train(tr, data, cfg, checkpoint=ck, epoch_init=epochs[0], epoch_final=epochs[1], use_graph=True,
                                    log=lambda *a: None, draws=driver_draws, on_epoch=lambda ep, t: torch.manual_seed(100 + ep))
    torch.cuda.synchronize()
    return series, state_of(tr), G.image_size


def test_epoch_driver_checkpoint_carries_the_objective_and_resumes(ngan, tmp_path):
    f = str(tmp_path / "a.pth")
    series, state, size = driver_run(ngan, f, (1, 3))
    assert size == 16 and list(series) == ["score_real", "score_fake", "D_loss", "G_loss", "D_grad_pen"]
    assert all(len(v) == 2 and np.isfinite(v).all() for v in series.values()), series
    assert ngan.utils.load_checkpoint_dict(f)["objective"] == "lsgan"
    f2 = str(tmp_path / "b.pth")
    first, _, size1 = driver_run(ngan, f2, (1, 2))                                   # interrupted after epoch 1, before the growth step ...
    assert size1 == 8 and ngan.utils.load_checkpoint_dict(f2)["objective"] == "lsgan"
    with pytest.raises(ValueError, match="lsgan.*wasserstein"):                      # ... not to be resumed as Wasserstein ...
        driver_run(ngan, f2, (2, 3), resume=True, objective="wasserstein")
    more, state2, size2 = driver_run(ngan, f2, (2, 3), resume=True)                  # ... and resumed for epoch 2
    assert size2 == 16 and [first[k] + more[k] for k in series] == [series[k] for k in series]
    assert same(state2, state)
    # a Wasserstein run writes its own name, and an LSGAN trainer refuses its file
    f3 = str(tmp_path / "c.pth")
    _, other, _ = driver_run(ngan, f3, (1, 2), objective="wasserstein")
    assert ngan.utils.load_checkpoint_dict(f3)["objective"] == "wasserstein"
    with pytest.raises(ValueError, match="wasserstein.*lsgan"):
        driver_run(ngan, f3, (2, 3), resume=True)
