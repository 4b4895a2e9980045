"""Geometric differentiable augmentation on the GPU: the kernels of csrc/diffgeo.hip against the fp64 restatement of
tests/diffgeo_cases.py (per-element bounds derived there, the fp32 emulation held against them in tests/test_diffgeo_cpu.py), the blit
rows against numpy bit for bit, the parameter kernel against numpy, the three losses against the CPU oracle composed with the
transform, and the trainer with the new groups: closed means untouched, eager equals replayed, the epoch driver is reproducible and
resumable, replicas of a data-parallel run stay identical.  Every test here calls the library, the operators or the trainer with a new
group and fails without the feature."""
import datetime
import functools
import os
import sys
import traceback
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import diffaug_cases as A0
import diffgeo_cases as A

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
f64 = np.float64
LATENT = 32


def _np(t):
    return t.detach().cpu().numpy().copy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def case(B, C, R):
    """inputs and, per table, the fp64 references and bounds: computed once per shape, shared by the tests, never modified"""
    x, gy = A.inputs(B, C, R)
    refs = {name: (rows, {fill: A.fwd_ref(x, rows, fill) for fill in A.FILLS}, A.bwd_ref(gy, rows)) for name, rows in A.tables(B, R)}
    return x, gy, refs


def run_fwd_bwd(ngan, x, gy, rows, fill=0.0):
    ops = ngan.ops
    table = ops.diffgeo_table(rows, DEV)
    xd = torch.from_numpy(x).to(DEV).requires_grad_()
    y = ops.DiffGeometry.apply(xd, table, fill)
    (gx,) = torch.autograd.grad(y, xd, torch.from_numpy(gy).to(DEV))
    return _np(y), _np(gx)


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,R", A.SHAPES)
def test_forward_and_adjoint_against_fp64(ngan, B, C, R):
    x, gy, refs = case(B, C, R)
    for name, (rows, fwd, (gref, gbd)) in refs.items():
        outs = {}
        for fill in A.FILLS:
            ref, bd = fwd[fill]
            y, gx = run_fwd_bwd(ngan, x, gy, rows, fill)
            rf, rb = A.ratio(y, ref, bd), A.ratio(gx, gref, gbd)
            print(f"STAT DIFFGEO {(B, C, R)} {name} fill {fill}: fwd err/bound {rf:.3f}, adjoint {rb:.3f}")
            assert rf <= 1.0 and rb <= 1.0, (name, fill, rf, rb)
            outs[fill] = (y, gx)
        assert np.array_equal(bits(outs[0.0][1]), bits(outs[-1.0][1])), name          # the fill has derivative 0
        # the pairing <T x - T 0, g> = <x, T^T g> in fp64 over the kernels' outputs, within the summed per-element bounds
        y, gx = outs[0.0]
        y0, _ = run_fwd_bwd(ngan, np.zeros_like(x), gy, rows)
        defect, slack = A.pairing_defect(x, gy, y, y0, gx), A.pairing_slack(x, gy, rows)
        print(f"STAT DIFFGEO {(B, C, R)} {name}: pairing defect {defect:.3e}, slack {slack:.3e}")
        assert defect <= slack, (name, defect, slack)
        # bit-reproducible
        y2, gx2 = run_fwd_bwd(ngan, x, gy, rows)
        assert np.array_equal(bits(y), bits(y2)) and np.array_equal(bits(gx), bits(gx2)), name


@pytest.mark.parametrize("B,C,R", A.SHAPES)
def test_blits_and_identity_copy_bit_for_bit(ngan, B, C, R):
    x, gy = A.inputs(B, C, R)                                  # a -0.0 among the images and among the gradients
    assert np.signbit(x[x == 0]).any() and np.signbit(gy[gy == 0]).any()
    y, gx = run_fwd_bwd(ngan, x, gy, [A.IDENTITY] * B, fill=-1.0)
    assert np.array_equal(bits(y), bits(x)) and np.array_equal(bits(gx), bits(gy))
    for f in (0, 1):
        for k in range(4):
            rows = [A.affine_row(R, flip=bool(f), k=k)] * B
            blit = lambda a: np.rot90(np.flip(a, -1) if f else a, k, axes=(-2, -1))          # noqa: E731
            unblit = lambda a: (lambda r: np.flip(r, -1) if f else r)(np.rot90(a, -k, axes=(-2, -1)))   # noqa: E731
            y, gx = run_fwd_bwd(ngan, x, gy, rows, fill=-1.0)
            assert np.array_equal(bits(y), bits(blit(x))), (f, k)
            assert np.array_equal(bits(gx), bits(unblit(gy))), (f, k)      # the adjoint of a permutation is its inverse


@pytest.mark.parametrize("B,C,R", A.SHAPES[:3])
def test_writes_into_a_row_range_of_a_larger_buffer(ngan, B, C, R):
    ops = ngan.ops
    x, _, refs = case(B, C, R)
    rows = refs["t1"][0]
    table = ops.diffgeo_table(list(rows) + [A.IDENTITY], DEV)   # a table longer than the batch is fine
    xd = torch.from_numpy(x).to(DEV)
    alone = ops.diffgeo(xd, table, fill=-1.0)
    for lo in (0, 1, 3):
        buf = torch.full((B + 3, C, R, R), -7.0, device=DEV)
        out = ops.diffgeo(xd, table, out=buf[lo:lo + B], fill=-1.0)
        assert out.data_ptr() == buf[lo].data_ptr()
        assert torch.equal(buf[lo:lo + B], alone) and bool((buf[:lo] == -7.0).all()) and bool((buf[lo + B:] == -7.0).all())
    with pytest.raises(RuntimeError, match="holds"):           # a table shorter than the batch is refused
        ops.diffgeo(xd, table[:B - 1])
    with pytest.raises(ValueError, match="out is"):
        ops.diffgeo(xd, table, out=torch.empty((B + 1, C, R, R), device=DEV))


def test_degenerate_rows_stay_inside_their_buffers(ngan):
    """memory safety only: a zero matrix, entries of 1e6, and offsets far off the image; the calls get exact-size views in the middle
    of a larger buffer, so a stray access would land in the neighbouring rows, which are compared"""
    ops = ngan.ops
    B, C, R = 4, 1, 64
    rows = [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (1e6, 1e6, 1e6, 1e6, 1e6, 1e6), (1e6, 0.0, -3e7, 0.0, 1e-6, 5.0), (0.0, 0.0, 31.5, 0.0, 0.0, 31.5)]
    table = ops.diffgeo_table(rows, DEV)
    g = torch.Generator().manual_seed(4)
    big_in = torch.randn((B + 2, C, R, R), generator=g).to(DEV)
    keep = big_in.clone()
    for fwd in (True, False):
        big_out = torch.full((B + 2, C, R, R), -7.0, device=DEV)
        if fwd:
            ops.diffgeo(big_in[1:1 + B], table, out=big_out[1:1 + B], fill=-1.0)
        else:
            ngan._C.call("ngan_diffgeo_bwd", big_in[1:1 + B], table, big_out[1:1 + B], B, C, R, R, B)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(big_out).all()), fwd
        assert bool((big_out[0] == -7.0).all()) and bool((big_out[-1] == -7.0).all()) and torch.equal(big_in, keep), fwd


def gpu_params(ngan, U, R, mask, p):
    ops = ngan.ops
    table = torch.full((U.shape[0] + 2, 8), 77.0, dtype=torch.float32, device=DEV)
    ops.diffgeo_params(torch.from_numpy(np.asarray(U, np.float32)).to(DEV), table, R, mask << 3, p)
    assert bool((table[U.shape[0]:] == 77.0).all()) and bool((table[:U.shape[0], 6:] == 0).all())
    return ops.diffgeo_table_rows(table[:U.shape[0]])


def test_parameter_kernel_against_numpy(ngan):
    for p in (0.5, 1.0):
        U = A.chosen_uniforms(p)                               # 0, 0.25, 0.5 and 1 - 2^-24 everywhere; gates below, at and above p
        for R in (4, 16, 512):
            assert gpu_params(ngan, U, R, 1, p) == A.params_ref(U, R, 1, p), (R, p)       # blit-only rows: exact
            for mask in (2, 3):
                assert A.params_close(gpu_params(ngan, U, R, mask, p), A.params_ref(U, R, mask, p), R), (R, mask, p)
    g = torch.Generator(device=DEV).manual_seed(5)
    U = _np(torch.rand((4096, 8), generator=g, device=DEV))
    for R in (16, 512):
        blits = gpu_params(ngan, U, R, 1, 1.0)
        assert blits == A.params_ref(U, R, 1, 1.0) and set(blits) == set(A.blit_rows(R))   # all eight occur, nothing else
        assert all(v in (0.0, 1.0, -1.0) for r in blits for v in (r[0], r[1], r[3], r[4]))
        assert all(v in (0.0, float(R - 1)) for r in blits for v in (r[2], r[5]))
        rows = gpu_params(ngan, U, R, 3, 1.0)
        assert A.params_close(rows, A.params_ref(U, R, 3, 1.0), R)
        sv = np.array([np.linalg.svd(np.array([[r[0], r[1]], [r[3], r[4]]], f64), compute_uv=False) for r in rows])
        assert sv.min() >= 2.0 ** -0.351 and sv.max() <= 2.0 ** 0.351                      # inside the adjoint's range [1/2, 2]
        c = 0.5 * (R - 1)                                                                  # the centre is the fixed point
        fixed = np.array([[r[0] * c + r[1] * c + r[2] - c, r[3] * c + r[4] * c + r[5] - c] for r in rows])
        assert np.abs(fixed).max() <= 8 * A.EPS * 4 * R
        assert gpu_params(ngan, U, R, 3, 0.0) == [A.IDENTITY] * 4096 == gpu_params(ngan, U, R, 0, 1.0)
        half = gpu_params(ngan, U, R, 3, 0.5)
        assert A.params_close(half, A.params_ref(U, R, 3, 0.5), R)
        moved = np.mean([r != A.IDENTITY for r in half])        # four gates at 1/2, the flip's coin, a quarter of the turns idle
        want = 1 - 0.75 * (0.5 + 0.5 * 0.25) * 0.5 * 0.5
        assert abs(moved - want) <= 0.032, (moved, want)        # four binomial standard deviations at n = 4096 are below 0.032


# ---------------------------------------------------------------------------------------------------------------------
# the three losses against the oracle composed with the transform
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_colors,res,alpha,older", [(1, 16, 0.5, False), (3, 16, 1.0, True)])
def test_losses_and_gradients_match_oracle_through_the_transform(ngan, n_colors, res, alpha, older, conv_precision):
    """test_gpu_diffaug.py::test_losses_and_gradients_match_oracle_through_the_transform with the resampling in front of (older) or
    in place of the colour / translation / cutout transform; its bounds.  The seed is that test's plus one: with that test's nets
    and images and the reals turned by these rows, the split-bf16 mode puts a LeakyReLU input of the critic within its rounding of
    zero and one layer's gradient jumps to 2.3e-3 of its norm (exact fp32 on the same draws: 1.5e-6; split-bf16 on neighbouring
    seeds, and on that seed with rows that do not turn the reals: 1.6e-5) -- the kink's doing, not the transform's."""
    from oracle import pggan_oracle as O
    torch.manual_seed(12 + n_colors + res)
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
    m, m0 = A.master_rows(res), A0.master_rows(res)
    geo = dict(real=m[9:13], fake=m[13:17], tilde=m[15:19], gen=[m[18], m[13], m[5], m[16]])
    old = dict(real=m0[0:4], fake=m0[4:8], tilde=m0[6:10], gen=m0[1:5])
    fill = ngan.loss_functions.DIFFAUG_FILL

    def T(im, kind):
        im = A.transcription(im, geo[kind], fill)
        return A0.transcription(im, old[kind], fill) if older else im

    xr = T(x.double(), "real").float()
    with torch.no_grad():
        fake = T(O.generator_forward(pg, z1, spec).double(), "fake").float()
        x_tilde = T(O.generator_forward(pg, z2, spec).double(), "tilde").float()
    real_score = O.discriminator_forward(pd, xr, spec)
    s_r, s_f = real_score.mean(), O.discriminator_forward(pd, fake, spec).mean()
    d_loss = -s_r + s_f + 0.001 * torch.square(real_score).mean()
    x_hat = (eps * xr + (1 - eps) * x_tilde).requires_grad_()
    (g,) = torch.autograd.grad(O.discriminator_forward(pd, x_hat, spec).sum(), x_hat, create_graph=True)
    norms = g.norm(2, dim=(1, 2, 3))
    gp = 10.0 * torch.mean((norms - 1) ** 2)
    (d_loss + gp).backward()
    LF = ngan.loss_functions
    Dl, Gp, Gl = LF.D_W_loss(G, D, 0.001), LF.D_grad_pen_loss(G, D, 10.0), LF.G_W_loss(G, D)
    kw = {"geo_" + k: ngan.ops.diffgeo_table(v, DEV) for k, v in geo.items()}
    if older:
        kw.update({k: ngan.ops.diffaug_table(v, DEV) for k, v in old.items()})
    hook = LF.DiffAugmentHook(**kw)
    xd = x.to(DEV)
    d2, sr2, sf2 = Dl(xd, z=z1.to(DEV), augment=hook)
    gp2 = Gp(xd, z=z2.to(DEV), epsilon=eps.to(DEV), augment=hook)
    (d2 + gp2).backward()
    got = np.array([float(d2.detach()), float(sr2.detach()), float(sf2.detach()), float(gp2.detach())])
    want = np.array([float(d_loss.detach()), float(s_r.detach()), float(s_f.detach()), float(gp.detach())])
    print("STAT DIFFGEO losses", got, want)
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
    g_ref = -O.discriminator_forward(pd, T(O.generator_forward(pg, z3, spec).double(), "gen").float(), spec).mean()
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
BOTH, ALL5 = "blit,geometry", "color,translation,cutout,blit,geometry"


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


def batch_draws(ngan, seed, n, mask=0):
    """reals, latents, epsilon and (mask) augmentation tables of one batch from seeded generators"""
    g = torch.Generator().manual_seed(seed)
    d = dict(real=(torch.rand(n, 1, 16, 16, generator=g) * 2 - 1).to(DEV), z_d=_unit(g, n).to(DEV), z_gp=_unit(g, n).to(DEV),
             eps=torch.rand(n, 1, 1, 1, generator=g).to(DEV), z_g=_unit(g, n).to(DEV))
    u, v = torch.rand(4 * n, 8, generator=g).to(DEV), torch.rand(4 * n, 8, generator=g).to(DEV)
    d["tables"] = {}
    if mask & 7:
        t = torch.empty((4 * n, 8), dtype=torch.int32, device=DEV)
        ngan.ops.diffaug_params(u, t, 16, mask, 1.0)
        d["tables"].update(real=t[:n].clone(), fake=t[n:3 * n].clone(), gen=t[3 * n:].clone())
    if mask >> 3:
        t = torch.empty((4 * n, 8), dtype=torch.float32, device=DEV)
        ngan.ops.diffgeo_params(v, t, 16, mask, 1.0)
        d["tables"].update(geo_real=t[:n].clone(), geo_fake=t[n:3 * n].clone(), geo_gen=t[3 * n:].clone())
    return d


def state_of(tr):
    return [_np(t) for t in (tr.flat_g.flat, tr.flat_d.flat, tr.flat_g.exp_avg, tr.flat_d.exp_avg_sq, tr.flat_g.seg_step)]


def same(a, b):
    return all(np.array_equal(u, v) for u, v in zip(a, b))


def test_new_groups_at_p_zero_are_the_trainer_without_the_arguments(ngan):
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
        return state_of(tr), torch.cuda.get_rng_state(DEV), torch.get_rng_state(), tr
    for replayed in (False, True):
        want = run(replayed)
        for kw in ({"diffaug": BOTH, "diffaug_p": 0.0, "diffaug_seed": 9}, {"diffaug": ALL5, "diffaug_p": 0.0}):
            got = run(replayed, **kw)
            assert got[3]._aug is None
            assert same(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), (replayed, kw)
    # ... an open policy does change the run, without touching the global streams; only what its groups need is allocated
    got = run(True, diffaug=BOTH)
    assert not same(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    aug = got[3]._aug
    assert aug.table is None and aug.uniforms is None and aug.geo_table.dtype == torch.float32
    assert tuple(aug.geo_table.shape) == (ngan.train.DIFFAUG_ROWS, 8) == tuple(aug.geo_uniforms.shape)
    old = run(True, diffaug="translation")[3]._aug
    assert old.geo_table is None and old.geo_uniforms is None and old.table is not None
    # the older groups' draw comes first on the private stream: an iteration's first draw is the same with and without the new groups
    def first_draw(policy):
        tr = ngan.train.PGGANTrainer(*small_nets(ngan), diffaug=policy, diffaug_seed=4)
        tr.draw_diffaug_tables(4)
        return tr._aug
    a, b = first_draw("color,cutout"), first_draw("color,cutout,blit")
    assert torch.equal(a.uniforms[:16], b.uniforms[:16]) and not torch.equal(b.uniforms[:16], b.geo_uniforms[:16])
    assert torch.equal(a.table[:16], b.table[:16]) and bool((a.uniforms[:16] > 0).any())


@pytest.mark.parametrize("policy", [BOTH, ALL5])
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
    table_ptr = tr._aug.geo_table.data_ptr()
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
    assert tr._aug.geo_table.data_ptr() == table_ptr           # the graphs hold this address
    assert stats_e == stats_r and all(np.isfinite(list(s.values())).all() for s in stats_e), (stats_e, stats_r)
    assert same(state_of(eager), state_of(tr))
    assert ngan.ops.diffgeo_table_rows(tr._aug.geo_real(0, 4)) == ngan.ops.diffgeo_table_rows(batches[-1]["tables"]["geo_real"])
    # the tables did act: the same draws without them end elsewhere
    G3, D3 = small_nets(ngan)
    plain = ngan.train.PGGANTrainer(G3, D3, learning_rate=1e-3)
    for d in batches:
        plain.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"])
    assert not same(state_of(plain), state_of(eager))
    if policy == BOTH:
        with pytest.raises(ValueError, match="names none of their groups"):
            eager.draw_diffaug_tables(4, {"real": torch.zeros((4, 8), dtype=torch.int32, device=DEV)})


def test_a_deeper_critic_stays_finite_with_all_five_groups_open(ngan):
    torch.manual_seed(12)
    G = ngan.models.Generator_PG([64, 32, 32, 16, 16], image_size_init=4, latent_dim=LATENT).to(DEV)
    D = ngan.models.Discriminator_PG([16, 16, 32, 32, 64], image_size_init=4).to(DEV)
    G.set_resolution(64, 1.0)
    D.set_resolution(64, 1.0)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3, device_latents=True, diffaug=ALL5, diffaug_seed=1)
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(8, 1, 64, 64, generator=g) * 2 - 1).to(DEV)
    tr.capture(x)
    worst = 0.0
    for _ in range(12):
        stats = tr.replay(x)
        worst = max(worst, float(tr.gp_loss.last_grad_norms.max()))
        assert all(bool(torch.isfinite(v)) for v in stats.values()), stats
    rows = ngan.ops.diffgeo_table_rows(tr._aug.geo_table[:32])
    assert all(r != A.IDENTITY for r in rows)                   # p = 1: every sample was scaled and rotated
    print("STAT DIFFGEO deeper critic: largest penalty norm", worst)
    assert worst < 1e3 and all(bool(torch.isfinite(f.flat).all()) for f in (tr.flat_g, tr.flat_d))


DRIVER_CFG = dict(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[], N_epochs=4, alpha_step=0.5,
                  learning_rate=1e-3, checkpointing_period=1, ID="geo", seed=3)


def driver_draws(epoch, k, n):
    g = torch.Generator().manual_seed(10007 * epoch + k)
    return dict(z_d=_unit(g, n), z_gp=_unit(g, n), eps=torch.rand(n, 1, 1, 1, generator=g), z_g=_unit(g, n))


def driver_run(ngan, f, epochs, resume=False, seed=4):
    """pggan_train on 10 synthetic 16 x 16 images in batches of 4, 4, 2 with all five groups at p = 1, replayed graphs, given latents"""
    cfg = types.SimpleNamespace(**DRIVER_CFG)
    G, D = small_nets(ngan)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, device_latents=True, diffaug=ALL5, diffaug_p=1.0, diffaug_seed=seed)
    data = ngan.train.TensorImageDataset.synthetic(10, 16, device=DEV, seed=8)
    ck = ngan.utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=DEV, trainer=tr,
                                 extra_checkpoint_period=1e3)
    if resume:
        ck.load_state()
    series = ngan.train.pggan_train(tr, data, cfg, checkpoint=ck, epoch_init=epochs[0], epoch_final=epochs[1], use_graph=True,
                                    log=lambda *a: None, draws=driver_draws, on_epoch=lambda ep, t: torch.manual_seed(100 + ep))
    torch.cuda.synchronize()
    return series, state_of(tr), ngan.ops.diffgeo_table_rows(tr._aug.geo_table[:16]) + ngan.ops.diffaug_table_rows(tr._aug.table[:16])


def test_epoch_driver_is_reproducible_and_resumable(ngan, tmp_path):
    series, state, rows = driver_run(ngan, str(tmp_path / "a.pth"), (1, 3))
    assert all(len(v) == 2 and np.isfinite(v).all() for v in series.values()), series
    assert all(r != A.IDENTITY for r in rows[:16])
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
    import socket
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
        import test_gpu_diffgeo as E
        ngan = load_package()
        G, D = E.small_nets(ngan)
        tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3, diffaug=E.BOTH, diffaug_seed=2)
        assert tr.world == world
        rows = []
        for it in range(2):
            d = E.batch_draws(ngan, 70 + 10 * it + rank, 3)                            # every rank its own share
            tr.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"])
            rows.append(ngan.ops.diffgeo_table_rows(tr._aug.geo_table[:12]))
        torch.cuda.synchronize()
        state = torch.cat([tr.flat_g.flat, tr.flat_d.flat, tr.flat_g.exp_avg, tr.flat_d.exp_avg_sq]).cpu()
        every = [torch.empty_like(state) for _ in range(world)]
        dist.all_gather(every, state)
        out = dict(rows=rows, equal=all(torch.equal(every[0], v) for v in every[1:]), finite=bool(torch.isfinite(state).all()))
    except Exception:  # noqa: BLE001
        out["exception"] = traceback.format_exc()
    finally:
        q.put((rank, out))
        dist.destroy_process_group()


def test_two_ranks_draw_their_own_tables_and_stay_identical():
    """two gloo ranks on the one GPU (as tests/test_gpu_diffaug.py runs them): each rank resamples its share with rows from its own
    stream, the exchanged gradients are the same on both, so the replicas stay bit-identical"""
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
