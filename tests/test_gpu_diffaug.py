"""Differentiable augmentation on the GPU: the kernels of csrc/diffaug.hip against the fp64 restatement of tests/diffaug_cases.py
(per-element bounds settled on the CPU, tests/test_diffaug_cpu.py), the parameter kernel against the integer arithmetic in numpy,
the three losses against the CPU oracle composed with the transform, and the trainer: off means untouched, eager equals replayed,
the epoch driver is reproducible and resumable, replicas of a data-parallel run stay identical."""
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

import diffaug_cases as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
f64 = np.float64


def _np(t):
    return t.detach().cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def case(B, C, R):
    """inputs and, per table, the fp64 references: computed once per shape, shared by the tests, never modified"""
    x, gy = A.inputs(B, C, R)
    refs = {name: (rows, A.fwd_ref(x, rows), A.bwd_ref(gy, rows)) for name, rows in A.tables(B, R)}
    return x, gy, refs


def run_fwd_bwd(ngan, x, gy, rows, colour=True, fill=0.0):
    ops = ngan.ops
    table = ops.diffaug_table(rows, DEV)
    xd = torch.from_numpy(x).to(DEV).requires_grad_()
    y = ops.DiffAugment.apply(xd, table, colour, fill)
    (gx,) = torch.autograd.grad(y, xd, torch.from_numpy(gy).to(DEV))
    return _np(y), _np(gx)


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,R", A.SHAPES)
def test_forward_and_adjoint_against_fp64(ngan, B, C, R):
    x, gy, refs = case(B, C, R)
    for name, (rows, (ref, absref), (gref, gabs)) in refs.items():
        y, gx = run_fwd_bwd(ngan, x, gy, rows)
        rf, rb = A.ratio(y, ref, absref), A.ratio(gx, gref, gabs)
        print(f"DIFFAUG {(B, C, R)} {name}: fwd err/bound {rf:.3f}, adjoint {rb:.3f}")
        assert rf <= 1.0 and rb <= 1.0, (name, rf, rb)
        # what the definition sets to zero is an exact zero (ratio() returns inf otherwise; stated once more in plain words)
        assert not y[absref == 0].any()
        for n, row in enumerate(rows):
            if row == A.IDENTITY:
                assert np.array_equal(y[n], x[n]) and np.array_equal(gx[n], gy[n]), (name, n)
        # pairing <T x, g> = <x, T^T g> in fp64 over the kernels' outputs, within the summed per-element bounds.  Brightness makes T
        # affine, T x = L x + T 0, and the adjoint is L's: the kernels' own T 0 is taken off first (and its bound added)
        y0, _ = run_fwd_bwd(ngan, np.zeros_like(x), gy, rows)
        assert A.pairing_defect(x, gy, y, y0, gx) <= A.pairing_slack(x, gy, rows), name
        # bit-reproducible
        y2, gx2 = run_fwd_bwd(ngan, x, gy, rows)
        assert np.array_equal(y, y2) and np.array_equal(gx, gx2), name
        # the trainer's fill: the same values, -1 exactly where the definition leaves nothing, the same adjoint
        y4, gx4 = run_fwd_bwd(ngan, x, gy, rows, fill=-1.0)
        assert np.array_equal(y4[absref > 0], y[absref > 0]) and bool((y4[absref == 0] == -1.0).all()) and np.array_equal(gx4, gx), name
        assert A.ratio(y4, *A.fwd_ref(x, rows, -1.0)) <= 1.0
        if all(r[:2] == (0.0, 1.0) for r in rows):
            # without the colour group the single-launch form gives the same bits
            y3, gx3 = run_fwd_bwd(ngan, x, gy, rows, colour=False)
            assert np.array_equal(y, y3) and np.array_equal(gx, gx3), name
    rows = A.colourless(refs["t0"][0])                       # shifts and cutouts alone: a pure masked copy each way
    (ref, absref), (gref, _) = A.fwd_ref(x, rows), A.bwd_ref(gy, rows)
    for colour in (False, True):
        y, gx = run_fwd_bwd(ngan, x, gy, rows, colour)
        assert np.array_equal(y, ref.astype(np.float32)) and np.array_equal(gx, gref.astype(np.float32)), colour


@pytest.mark.parametrize("B,C,R", A.SHAPES)
def test_writes_into_a_row_range_of_a_larger_buffer(ngan, B, C, R):
    ops = ngan.ops
    x, _, refs = case(B, C, R)
    rows = refs["t0"][0]
    table = ops.diffaug_table(rows + [A.IDENTITY], DEV)      # a table longer than the batch is fine
    xd = torch.from_numpy(x).to(DEV)
    alone = ops.diffaug(xd, table)
    for lo in (0, 1, 3):
        buf = torch.full((B + 3, C, R, R), -7.0, device=DEV)
        out = ops.diffaug(xd, table, out=buf[lo:lo + B])
        assert out.data_ptr() == buf[lo].data_ptr()
        assert torch.equal(buf[lo:lo + B], alone) and bool((buf[:lo] == -7.0).all()) and bool((buf[lo + B:] == -7.0).all())
    with pytest.raises(RuntimeError, match="holds"):         # a table shorter than the batch is refused
        ops.diffaug(xd, table[:B - 1])
    with pytest.raises(ValueError, match="out is"):
        ops.diffaug(xd, table, out=torch.empty((B + 1, C, R, R), device=DEV))


def gpu_params(ngan, U, R, mask, p):
    ops = ngan.ops
    table = torch.full((U.shape[0] + 2, 8), 77, dtype=torch.int32, device=DEV)
    ops.diffaug_params(torch.from_numpy(np.asarray(U, np.float32)).to(DEV), table, R, mask, p)
    assert bool((table[U.shape[0]:] == 77).all())            # rows past the batch are not written
    return ops.diffaug_table_rows(table[:U.shape[0]])


def test_parameter_kernel_against_numpy(ngan):
    U = A.chosen_uniforms()                                   # 0, 0.5 and 1 - 2^-24 everywhere, gates both ways
    for R in (4, 16, 512):
        for mask in (7, 5, 2):
            for p in (0.5, 1.0):
                assert gpu_params(ngan, U, R, mask, p) == A.params_ref(U, R, mask, p), (R, mask, p)
    g = torch.Generator(device=DEV).manual_seed(5)
    U = _np(torch.rand((4096, 8), generator=g, device=DEV))
    for R in (16, 512):
        S = A.shift_size(R)
        rows = gpu_params(ngan, U, R, 7, 1.0)
        assert rows == A.params_ref(U, R, 7, 1.0)
        if R == 16:                                           # 25 shift pairs over 4096 draws: every value of [-S, S] occurs
            assert {r[2] for r in rows} == set(range(-S, S + 1)) == {r[3] for r in rows}
        assert all(-S <= r[2] <= S and -S <= r[3] <= S for r in rows)
        assert all(r[:2] != (0.0, 1.0) and r[4] < r[5] and r[6] < r[7] for r in rows)      # p = 1 opens every gate
        assert gpu_params(ngan, U, R, 7, 0.0) == [A.IDENTITY] * 4096 == gpu_params(ngan, U, R, 0, 1.0)
        half = gpu_params(ngan, U, R, 7, 0.5)
        assert half == A.params_ref(U, R, 7, 0.5)
        for open_ in ([r[:2] != (0.0, 1.0) for r in half], [r[4:] != (0, 0, 0, 0) for r in half]):
            assert abs(np.mean(open_) - 0.5) <= 0.032, np.mean(open_)      # four binomial standard deviations at n = 4096
        # the translation gate, from the rows: an open gate still draws (0, 0) once in (2S + 1)^2, so the fraction moved is
        # 0.5 (1 - 1 / (2S + 1)^2), and the 0.032 holds about that
        moved = np.mean([r[2:4] != (0, 0) for r in half])
        assert abs(moved / (1 - 1 / (2 * S + 1) ** 2) - 0.5) <= 0.032, moved


# ---------------------------------------------------------------------------------------------------------------------
# the three losses against the oracle composed with the transform
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_colors,res,alpha", [(1, 16, 0.5), (3, 16, 1.0)])
def test_losses_and_gradients_match_oracle_through_the_transform(ngan, n_colors, res, alpha, conv_precision):
    """test_gpu_models.py::test_losses_and_gradients_match_oracle_on_the_fly with T around every critic input; its bounds"""
    from oracle import pggan_oracle as O
    torch.manual_seed(11 + n_colors + res)
    gw, dw = [32, 16], [16, 32]
    G = ngan.models.Generator_PG(gw, image_size_init=8, latent_dim=64, N_colors=n_colors)
    D = ngan.models.Discriminator_PG(dw, image_size_init=8, N_colors=n_colors)
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
    m = A.master_rows(res)
    rows = dict(real=m[0:4], fake=m[4:8], tilde=m[6:10], gen=m[1:5])
    T = lambda im, r: A.transcription(im, r, ngan.loss_functions.DIFFAUG_FILL)     # noqa: E731  (the hook's default fill)
    # oracle (CPU): loss_functions.py:14-47, 157-180, 59-74 with T around everything the critic sees
    xr = T(x, rows["real"])
    with torch.no_grad():
        fake = T(O.generator_forward(pg, z1, spec), rows["fake"])
        x_tilde = T(O.generator_forward(pg, z2, spec), rows["tilde"])
    real_score = O.discriminator_forward(pd, xr, spec)
    s_r, s_f = real_score.mean(), O.discriminator_forward(pd, fake, spec).mean()
    d_loss = -s_r + s_f + 0.001 * torch.square(real_score).mean()
    x_hat = (eps * xr + (1 - eps) * x_tilde).requires_grad_()
    (g,) = torch.autograd.grad(O.discriminator_forward(pd, x_hat, spec).sum(), x_hat, create_graph=True)
    norms = g.norm(2, dim=(1, 2, 3))
    gp = 10.0 * torch.mean((norms - 1) ** 2)
    (d_loss + gp).backward()
    # HIP path
    LF = ngan.loss_functions
    Dl, Gp, Gl = LF.D_W_loss(G, D, 0.001), LF.D_grad_pen_loss(G, D, 10.0), LF.G_W_loss(G, D)
    hook = LF.DiffAugmentHook(**{k: ngan.ops.diffaug_table(v, DEV) for k, v in rows.items()})
    xd = x.to(DEV)
    d2, sr2, sf2 = Dl(xd, z=z1.to(DEV), augment=hook)
    gp2 = Gp(xd, z=z2.to(DEV), epsilon=eps.to(DEV), augment=hook)
    (d2 + gp2).backward()
    got = np.array([float(d2.detach()), float(sr2.detach()), float(sf2.detach()), float(gp2.detach())])
    want = np.array([float(d_loss.detach()), float(s_r.detach()), float(s_f.detach()), float(gp.detach())])
    print("DIFFAUG losses", got, want)
    assert np.allclose(got, want, rtol=1e-3, atol=2e-5), (got, want)
    assert np.allclose(Gp.last_grad_norms.cpu().numpy(), norms.detach().numpy(), rtol=1e-3)
    tol_l2, tol_out = 2e-3, 1e-3

    def close(got, ref, scale):
        d = (got.cpu().double() - ref.double())
        l2 = float(d.norm() / (ref.double().norm() + 1e-2 * scale))
        outliers = float((d.abs() > 1e-2 * (float(ref.abs().max()) + 1e-2 * scale)).double().mean())
        return l2 < tol_l2 and outliers <= tol_out, (l2, outliers)

    gmax = max(float(v.grad.abs().max()) for v in pd.values() if v.grad is not None)
    for k, p in D.named_parameters():
        if p.grad is not None:
            ok, info = close(p.grad, pd[k].grad, gmax)
            assert ok, ("D", k, info)
    g_ref = -O.discriminator_forward(pd, T(O.generator_forward(pg, z3, spec), rows["gen"]), spec).mean()
    g_ref.backward()
    g2, _ = Gl(xd, z=z3.to(DEV), augment=hook)
    g2.backward()
    assert abs(float(g2.detach()) - float(g_ref.detach())) < 1e-3 * abs(float(g_ref.detach())) + 2e-5
    gmax = max(float(v.grad.abs().max()) for v in pg.values() if v.grad is not None)
    for k, p in G.named_parameters():
        if p.grad is not None:
            ok, info = close(p.grad, pg[k].grad, gmax)
            assert ok, ("G", k, info)


# ---------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------
LATENT = 32


def small_nets(ngan, seed=6):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([32, 16], image_size_init=8, latent_dim=LATENT)
    D = ngan.models.Discriminator_PG([16, 32], image_size_init=8)
    G.set_resolution(16, 1.0)
    D.set_resolution(16, 1.0)
    return G.to(DEV), D.to(DEV)


def _unit(g, n):
    v = torch.randn(n, LATENT, generator=g)
    return v / v.norm(dim=1, keepdim=True)


def batch_draws(ngan, seed, n, tables=True, mask=7):
    """reals, latents, epsilon and (tables) augmentation tables of one batch from seeded generators"""
    g = torch.Generator().manual_seed(seed)
    d = dict(real=(torch.rand(n, 1, 16, 16, generator=g) * 2 - 1).to(DEV), z_d=_unit(g, n).to(DEV), z_gp=_unit(g, n).to(DEV),
             eps=torch.rand(n, 1, 1, 1, generator=g).to(DEV), z_g=_unit(g, n).to(DEV))
    if tables:
        u = torch.rand(4 * n, 8, generator=g).to(DEV)
        t = torch.empty((4 * n, 8), dtype=torch.int32, device=DEV)
        ngan.ops.diffaug_params(u, t, 16, mask, 1.0)
        d["tables"] = dict(real=t[:n].clone(), fake=t[n:3 * n].clone(), gen=t[3 * n:].clone())
    return d


def state_of(tr):
    return [_np(t) for t in (tr.flat_g.flat, tr.flat_d.flat, tr.flat_g.exp_avg, tr.flat_d.exp_avg_sq, tr.flat_g.seg_step)]


def same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def test_a_closed_policy_is_the_trainer_without_the_arguments(ngan):
    """an empty policy and p = 0: bit-equal parameters after three iterations, eager and replayed, and the same global RNG state"""
    def run(replayed, **kw):
        G, D = small_nets(ngan)
        tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3, device_latents=True, **kw)
        torch.manual_seed(21)
        x = batch_draws(ngan, 3, 4, tables=False)["real"]
        for _ in range(3):
            if replayed:
                tr.step(x)
            else:
                tr.train_iteration(x)
        torch.cuda.synchronize()
        return state_of(tr), torch.cuda.get_rng_state(DEV), torch.get_rng_state()
    for replayed in (False, True):
        want = run(replayed)
        for kw in ({"diffaug": ""}, {"diffaug": "color,translation,cutout", "diffaug_p": 0.0, "diffaug_seed": 9}):
            got = run(replayed, **kw)
            assert same(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), (replayed, kw)
    # ... and an open policy does change the run, without touching the global streams
    got = run(True, diffaug="color,translation,cutout")
    assert not same(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


@pytest.mark.parametrize("policy", ["color,translation,cutout", "translation,cutout"])
def test_eager_and_replayed_iterations_are_bit_equal(ngan, policy):
    """injected draws and tables: three eager iterations against capture + three replays, batches of 4, 2 (the ragged last one), 4"""
    mask = A.policy_mask(policy)
    batches = [batch_draws(ngan, 40 + i, n, mask=mask) for i, n in enumerate((4, 2, 4))]
    G, D = small_nets(ngan)
    eager = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3, diffaug=policy)
    stats_e = []
    for d in batches:
        s = eager.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"], tables=d["tables"])
        stats_e.append({k: float(v) for k, v in s.items()})
    G2, D2 = small_nets(ngan)
    tr = ngan.train.PGGANTrainer(G2, D2, learning_rate=1e-3, diffaug=policy)
    table_ptr = tr._aug.table.data_ptr()
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
    assert tr._aug.table.data_ptr() == table_ptr            # the graphs hold this address
    assert stats_e == stats_r and all(np.isfinite(list(s.values())).all() for s in stats_e), (stats_e, stats_r)
    assert same(state_of(eager), state_of(tr))
    # the tables did act: the same draws without them end elsewhere
    G3, D3 = small_nets(ngan)
    plain = ngan.train.PGGANTrainer(G3, D3, learning_rate=1e-3)
    for d in batches:
        plain.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"])
    assert not same(state_of(plain), state_of(eager))


def test_a_deeper_critic_stays_finite_with_every_group_open(ngan):
    """64 x 64, five blocks, p = 1: where shifted-out and cut pixels are exact zeros the penalty's norms leave fp32 within a few
    iterations (tests/test_diffaug_cpu.py shows the mechanism on the oracle); with the trainer's fill they stay of order one"""
    torch.manual_seed(12)
    G = ngan.models.Generator_PG([64, 32, 32, 16, 16], image_size_init=4, latent_dim=LATENT).to(DEV)
    D = ngan.models.Discriminator_PG([16, 16, 32, 32, 64], image_size_init=4).to(DEV)
    G.set_resolution(64, 1.0)
    D.set_resolution(64, 1.0)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3, device_latents=True, diffaug="color,translation,cutout", diffaug_seed=1)
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(8, 1, 64, 64, generator=g) * 2 - 1).to(DEV)
    tr.capture(x)
    worst = 0.0
    for _ in range(12):
        stats = tr.replay(x)
        worst = max(worst, float(tr.gp_loss.last_grad_norms.max()))
        assert all(bool(torch.isfinite(v)) for v in stats.values()), stats
    rows = ngan.ops.diffaug_table_rows(tr._aug.table[:32])
    assert all(r[4] < r[5] and r[6] < r[7] for r in rows)                   # every sample was cut
    print("DIFFAUG deeper critic: largest penalty norm", worst)
    assert worst < 1e3 and all(bool(torch.isfinite(f.flat).all()) for f in (tr.flat_g, tr.flat_d))


DRIVER_CFG = dict(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[], N_epochs=4, alpha_step=0.5,
                  learning_rate=1e-3, checkpointing_period=1, ID="aug", seed=3)


def driver_draws(epoch, k, n):
    g = torch.Generator().manual_seed(10007 * epoch + k)
    return dict(z_d=_unit(g, n), z_gp=_unit(g, n), eps=torch.rand(n, 1, 1, 1, generator=g), z_g=_unit(g, n))


def driver_run(ngan, f, epochs, resume=False, seed=4):
    """pggan_train on 10 synthetic 16 x 16 images in batches of 4, 4, 2 with p = 1, replayed graphs, given latents; the permutation
    of every epoch is seeded at its start, so that a resumed run sees the epoch an uninterrupted one sees"""
    cfg = types.SimpleNamespace(**DRIVER_CFG)
    G, D = small_nets(ngan)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, device_latents=True, diffaug="color,translation,cutout",
                                 diffaug_p=1.0, diffaug_seed=seed)
    data = ngan.train.TensorImageDataset.synthetic(10, 16, device=DEV, seed=8)
    ck = ngan.utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=DEV, trainer=tr,
                                 extra_checkpoint_period=1e3)
    if resume:
        ck.load_state()
    series = ngan.train.pggan_train(tr, data, cfg, checkpoint=ck, epoch_init=epochs[0], epoch_final=epochs[1], use_graph=True,
                                    log=lambda *a: None, draws=driver_draws, on_epoch=lambda ep, t: torch.manual_seed(100 + ep))
    torch.cuda.synchronize()
    return series, state_of(tr), ngan.ops.diffaug_table_rows(tr._aug.table[:16])


def test_epoch_driver_is_reproducible_and_resumable(ngan, tmp_path):
    series, state, rows = driver_run(ngan, str(tmp_path / "a.pth"), (1, 3))
    assert all(len(v) == 2 and np.isfinite(v).all() for v in series.values()), series
    assert any(r != A.IDENTITY for r in rows)
    series2, state2, rows2 = driver_run(ngan, str(tmp_path / "b.pth"), (1, 3))
    assert series2 == series and same(state2, state) and rows2 == rows
    _, other, _ = driver_run(ngan, str(tmp_path / "c.pth"), (1, 3), seed=5)           # the seed is the tables' seed
    assert not same(other, state)
    f = str(tmp_path / "d.pth")
    first, _, _ = driver_run(ngan, f, (1, 2))                                          # interrupted after epoch 1 ...
    more, state3, rows3 = driver_run(ngan, f, (2, 3), resume=True)                      # ... and resumed for epoch 2
    assert [first[k] + more[k] for k in series] == [series[k] for k in series]
    assert same(state3, state) and rows3 == rows


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _two_rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(4)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    out = {}
    try:
        from __graft_entry__ import load_package
        import test_gpu_diffaug as E
        ngan = load_package()
        G, D = E.small_nets(ngan)
        tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3, diffaug="color,translation,cutout", diffaug_seed=2)
        assert tr.world == world
        rows = []
        for it in range(2):
            d = E.batch_draws(ngan, 70 + 10 * it + rank, 3, tables=False)              # every rank its own share
            tr.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"])
            rows.append(ngan.ops.diffaug_table_rows(tr._aug.table[:12]))
        torch.cuda.synchronize()
        state = torch.cat([tr.flat_g.flat, tr.flat_d.flat, tr.flat_g.exp_avg, tr.flat_d.exp_avg_sq]).cpu()
        every = [torch.empty_like(state) for _ in range(world)]
        dist.all_gather(every, state)
        out = dict(rows=rows, equal=all(torch.equal(every[0], v) for v in every[1:]), finite=bool(torch.isfinite(state).all()),
                   moved=float((state - every[0]).abs().max()))
    except Exception:  # noqa: BLE001
        out["exception"] = traceback.format_exc()
    finally:
        q.put((rank, out))
        dist.destroy_process_group()


def test_two_ranks_draw_their_own_tables_and_stay_identical():
    """two gloo ranks on the one GPU (as tests/test_gpu_epoch_dist.py runs them): each rank augments its share with tables from its
    own stream, the exchanged gradients are the same on both, so the replicas stay bit-identical"""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(world):
            r, out = q.get(timeout=240)
            got[r] = out
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.terminate()
    assert sorted(got) == [0, 1] and all(p.exitcode == 0 for p in procs), ([p.exitcode for p in procs], sorted(got))
    for r in (0, 1):
        assert "exception" not in got[r], got[r]["exception"]
        assert got[r]["equal"] and got[r]["finite"], got[r]
    assert got[0]["rows"][0] != got[1]["rows"][0] and got[0]["rows"][1] != got[1]["rows"][1]
    assert got[0]["rows"][0] != got[0]["rows"][1]
