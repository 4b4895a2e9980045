"""The penalty's forms and lazy regularisation on the GPU: the two entry points of include/ngan_penalty.h (csrc/penalty.hip) through the
C ABI per element against fp64 (bounds settled on the CPU, tests/test_penalty_bounds_cpu.py) and bit for bit against the two-sided
chain where the forms coincide; ops.PenaltyHead and D_grad_pen_loss(mode="lp" | "r1") with their parameter gradients against the CPU
oracle; and PGGANTrainer(grad_pen_mode=, grad_pen_interval=): the defaults are the trainer without the arguments, eager equals
replayed, the penalty is there exactly in the due iterations, captures settle, two ranks with shares 3 and 1 reproduce one rank on the
whole batch, and the epoch driver resumes bit-equal from a checkpoint that carries mode, interval and count.

Per element   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref + carried,   C_ACC = 8; n_round, absref and the carried error of
the rounded norm per output in tests/penalty_cases.py.  Every output buffer starts as NaN between two guards, so an element no thread
wrote fails the comparison and a write outside the buffer fails the guard.

measured on MI355X (a record, not a bound: worst err / bound per output over all cases; 1 is the bound): penalty_head norms 0.167,
penalty 0.069 (form 1) / 0.060 (form 2); penalty_bwd 0.167 (form 1) / 0.107 (form 2) -- the emulation's figures
(tests/test_penalty_bounds_cpu.py) to three digits: no constant moved.  Two ranks with shares 3 and 1 under r1 at interval 2: worst
deviation / scale 1.5e-7 (due) and 2.3e-7 (not due) against the bound 2e-4.  The module takes 12 s."""
import ctypes
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

import penalty_cases as P
import test_gpu_lsgan as TL
from test_gpu_lsgan import batch_draws, same, small_nets, state_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
f32 = np.float32
GUARD = 4                        # floats on either side of an output: 16 bytes, so the output keeps its alignment


def _np(t):
    return t.detach().cpu().numpy().copy()


def dv(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def guarded(n, shift=0):
    """(buffer, view of n floats inside it): NaN between two guards of 7.0; shift: floats by which the view leaves 16-byte alignment"""
    buf = torch.full((n + 2 * GUARD + shift,), float("nan"), device=DEV, dtype=torch.float32)
    buf[:GUARD + shift] = 7.0
    buf[GUARD + shift + n:] = 7.0
    return buf, buf[GUARD + shift:GUARD + shift + n]


def guards_intact(buf, n, shift=0):
    return bool((buf[:GUARD + shift] == 7.0).all()) and bool((buf[GUARD + shift + n:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(B, n, family, form):
    """input and fp64 references of one case: computed once, shared, never modified"""
    g = P.inputs(B, n, family)
    return g, P.head_ref(g, P.LAMBDA, form), P.bwd_ref(g, P.LAMBDA, form, P.G_OUT)


def run_head(ngan, g, B, n, form):
    bn, norms = guarded(B)
    bo, out = guarded(1)
    ws = torch.full((64 * B,), float("nan"), device=DEV)
    ngan._C.call("ngan_penalty_head", g, B, n, form, P.LAMBDA, ws, norms, out)
    assert guards_intact(bn, B) and guards_intact(bo, 1), "the head wrote outside its outputs"
    return norms, out


def run_bwd(ngan, g, norms, B, n, form, g_out, shift=0):
    bg, grad = guarded(B * n, shift)
    ngan._C.call("ngan_penalty_bwd", g, norms, B, n, form, P.LAMBDA, g_out, grad)
    assert guards_intact(bg, B * n, shift), "the backward wrote outside its output"
    return grad


@pytest.mark.parametrize("B,n", P.SHAPES)
def test_both_entry_points_against_fp64_and_the_chain(ngan, B, n):
    call = ngan._C.call
    bad = []

    def ck(name, got, ref, tag):
        r, a, nr, carried = ref
        got = _np(got).reshape(r.shape)
        assert np.isfinite(got).all(), (name, tag, "an element was not written")
        worst = P.ratio_carried(got, r, a, nr, carried, P.c_acc(name))
        print(f"STAT penalty {name} {(B, n) + tag}: {worst:.3f}")
        if not worst <= 1.0:
            bad.append((name, tag, worst))

    g_out = dv(np.array([P.G_OUT], f32))
    for family in P.FAMILIES:
        g = dv(P.inputs(B, n, family))
        # the chain the fused launches stand beside: its norms are the anchor of every case
        chain_norms, ws = torch.empty(B, device=DEV), torch.empty(64 * B, device=DEV)
        call("ngan_sample_l2norm", g, chain_norms, ws, B, n)
        for form in P.FORMS:
            _, head, bwd = case(B, n, family, form)
            norms, out = run_head(ngan, g, B, n, form)
            ck(f"penalty_head{form}/norms", norms, head["norms"], (family,))
            ck(f"penalty_head{form}/penalty", out, head["penalty"], (family,))
            assert torch.equal(norms, chain_norms), "norms differ from ngan_sample_l2norm's bits"
            norms2, out2 = run_head(ngan, g, B, n, form)
            assert torch.equal(norms2, norms) and torch.equal(out2, out)              # fixed order: bit-reproducible
            grad = run_bwd(ngan, g, norms, B, n, form, g_out)
            ck(f"penalty_bwd{form}/grad", grad, bwd["grad"], (family,))
            assert torch.equal(run_bwd(ngan, g, norms, B, n, form, g_out), grad)
            # an output that leaves 16-byte alignment takes the 4-byte path: the same products, the same bits
            assert torch.equal(run_bwd(ngan, g, norms, B, n, form, g_out, shift=1), grad)
            gm = grad.view(B, n)
            if form == P.ONE_SIDED:
                dead = (norms <= 1.0)
                assert not gm[dead].any() and not torch.signbit(gm[dead]).any()       # exact +0.0 rows where n_b <= 1
                assert all(bool(dead[b]) for b in P.exact_one_rows(B, family) + P.zero_rows(B, family))
                assert all(float(norms[b]) == 1.0 for b in P.exact_one_rows(B, family))
            else:
                for b in P.zero_rows(B, family):
                    assert not gm[b].any() and not torch.isnan(gm[b]).any()            # zeros, not 0 / 0
            if family == "above_one" and form == P.ONE_SIDED:
                # every norm above 1: the one-sided form is the two-sided one, bit for bit
                c_out, coef, c_grad = torch.empty((), device=DEV), torch.empty(B, device=DEV), torch.empty(B * n, device=DEV)
                call("ngan_gp_head", chain_norms, B, P.LAMBDA, c_out)
                call("ngan_gp_coef", chain_norms, B, P.LAMBDA, g_out, coef)
                call("ngan_scale_rows", g, coef, c_grad, B, n)
                assert bool((chain_norms > 1).all()) and torch.equal(out.reshape(()), c_out) and torch.equal(grad, c_grad)
    assert not bad, bad


def test_rows_at_or_below_one_are_zero_whatever_they_hold(ngan):
    """form 1 with a stated norm <= 1 writes +0.0 without multiplying: a row of infinities or NaNs gives zeros, not NaN"""
    B, n = 4, 36
    g = torch.randn(B, n, device=DEV)
    g[0], g[1, 5], g[2] = float("inf"), float("nan"), float("-inf")
    norms = torch.tensor([0.5, 1.0, 0.0, 2.0], device=DEV)
    g_out = torch.tensor([0.7], device=DEV)
    grad = run_bwd(ngan, g.reshape(-1), norms, B, n, P.ONE_SIDED, g_out).view(B, n)
    assert not grad[:3].any() and not torch.signbit(grad[:3]).any() and not torch.isnan(grad).any()
    c = f32(0.7) * f32(2) * f32(P.LAMBDA) * f32(1) / (f32(B) * f32(2))
    assert torch.equal(grad[3], g[3] * float(c))
    # a NaN norm counts as not above 1 in the backward and stays NaN in the head's value
    assert not run_bwd(ngan, g.reshape(-1), torch.full((B,), float("nan"), device=DEV), B, n, P.ONE_SIDED, g_out).any()
    _, out = run_head(ngan, g.reshape(-1), B, n, P.ONE_SIDED)
    assert bool(torch.isnan(out).all())


def test_bad_arguments_return_a_status_and_launch_nothing(ngan):
    lib = ngan._C.lib()
    g = torch.ones(4 * 8 + 4, device=DEV)
    outs = [torch.full((64,), 7.0, device=DEV) for _ in range(4)]      # workspace (of one row), norms, out1, grad
    one = torch.ones(1, device=DEV)
    p = lambda t, off=0: None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * off)      # noqa: E731
    s = torch.cuda.current_stream().cuda_stream
    got = []
    for form in (1, 2):
        for B, n in ((0, 8), (-1, 8), (1, 0), (1, -8)):
            got.append(lib.ngan_penalty_head(p(g), B, n, form, 10.0, p(outs[0]), p(outs[1]), p(outs[2]), s))
            got.append(lib.ngan_penalty_bwd(p(g), p(outs[1]), B, n, form, 10.0, p(one), p(outs[3]), s))
        got.append(lib.ngan_penalty_head(None, 1, 8, form, 10.0, p(outs[0]), p(outs[1]), p(outs[2]), s))
        got.append(lib.ngan_penalty_head(p(g), 1, 8, form, 10.0, None, p(outs[1]), p(outs[2]), s))
        got.append(lib.ngan_penalty_head(p(g), 1, 8, form, 10.0, p(outs[0]), p(outs[1]), None, s))
        got.append(lib.ngan_penalty_head(p(g, 1), 1, 8, form, 10.0, p(outs[0]), p(outs[1]), p(outs[2]), s))      # misaligned rows
        got.append(lib.ngan_penalty_head(p(g), 1 + form, 5, form, 10.0, p(outs[0]), p(outs[1]), p(outs[2]), s))  # n % 4 with B > 1
        got.append(lib.ngan_penalty_bwd(p(g), None, 1, 8, form, 10.0, p(one), p(outs[3]), s))
        got.append(lib.ngan_penalty_bwd(p(g), p(outs[1]), 1, 8, form, 10.0, None, p(outs[3]), s))
        got.append(lib.ngan_penalty_bwd(p(g), p(outs[1]), 1, 8, form, 10.0, p(one), None, s))
    for form in (0, 3):
        got.append(lib.ngan_penalty_head(p(g), 1, 8, form, 10.0, p(outs[0]), p(outs[1]), p(outs[2]), s))
        got.append(lib.ngan_penalty_bwd(p(g), p(outs[1]), 1, 8, form, 10.0, p(one), p(outs[3]), s))
    torch.cuda.synchronize()
    assert all(v < 0 for v in got), got
    assert all(bool((o == 7.0).all()) for o in outs)
    with pytest.raises(RuntimeError, match=r"ngan_penalty_head failed with status -\d+: .*unknown form"):
        ngan._C.call("ngan_penalty_head", g, 1, 8, 5, 10.0, outs[0], outs[1], outs[2])
    # the Python operator: norms carry no gradient, no incoming gradient launches nothing, a second derivative is refused
    x = torch.randn(3, 8, device=DEV, requires_grad=True)
    pen, norms = ngan.ops.PenaltyHead.apply(x, 10.0, P.ZERO_CENTRED)
    assert not norms.requires_grad and pen.requires_grad
    (gx,) = torch.autograd.grad(pen, x, create_graph=True)
    assert torch.allclose(gx, x.detach() * (10.0 / 3), rtol=1e-6)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gx.sum(), x)


# ---------------------------------------------------------------------------------------------------------------------
# operator and loss against the oracle
# ---------------------------------------------------------------------------------------------------------------------
LP_SEED = 11


def oracle_case(ngan, n_colors, alpha, seed=LP_SEED, res=16, b=4):
    """nets, their oracle parameters and the draws, on the CPU; the critic's last layer is scaled so that the oracle's |grad D(x_hat)|
    straddle 1 (between the second and the third of the four sorted norms): the one-sided form is compared away from its kink"""
    from oracle import pggan_oracle as O
    torch.manual_seed(seed + n_colors + res)
    G = ngan.models.Generator_PG([32, 16], image_size_init=8, latent_dim=64, N_colors=n_colors)
    D = ngan.models.Discriminator_PG([16, 32], image_size_init=8, N_colors=n_colors)
    G.set_resolution(res, alpha)
    D.set_resolution(res, alpha)
    spec = O.NetSpec(image_size_init=8, slope=0.2, alpha=alpha)
    x = torch.rand(b, n_colors, res, res) * 2 - 1
    z1, z2 = (O.sample_latent_vec((b, 64)) for _ in range(2))
    eps = torch.rand(b, 1, 1, 1)
    pg = O.as_leaf_params({k: v.detach().clone() for k, v in G.state_dict().items()})

    def hat_norms(pd):
        with torch.no_grad():
            x_tilde = O.generator_forward(pg, z2, spec)
        x_hat = (eps * x + (1 - eps) * x_tilde).requires_grad_()
        (g,) = torch.autograd.grad(O.discriminator_forward(pd, x_hat, spec).sum(), x_hat, create_graph=True)
        return x_hat, g.norm(2, dim=(1, 2, 3))

    first = hat_norms(O.as_leaf_params({k: v.detach().clone() for k, v in D.state_dict().items()}))[1].detach().sort().values
    with torch.no_grad():
        last = [m for m in D.layers if getattr(m, "weight", None) is not None][-1]      # the head's final layer: the score is linear in it
        last.weight.mul_(1.0 / float((first[1] * first[2]).sqrt()))
    pd = O.as_leaf_params({k: v.detach().clone() for k, v in D.state_dict().items()})
    return types.SimpleNamespace(O=O, G=G, D=D, pg=pg, pd=pd, spec=spec, x=x, z1=z1, z2=z2, eps=eps, hat_norms=hat_norms, b=b)


def oracle_d_loss(c, objective, xr=None):
    O = c.O
    with torch.no_grad():
        fake = O.generator_forward(c.pg, c.z1, c.spec)
    real_score, fake_score = O.discriminator_forward(c.pd, c.x if xr is None else xr, c.spec), O.discriminator_forward(c.pd, fake, c.spec)
    if objective == "lsgan":
        return torch.mean((real_score - 1) ** 2) + torch.mean(fake_score ** 2)
    return -real_score.mean() + fake_score.mean() + 0.001 * torch.square(real_score).mean()


def oracle_penalty(c, mode, lam, xr=None):
    """-> (penalty, norms): the two formulae over the oracle's critic"""
    if mode == "lp":
        _, norms = c.hat_norms(c.pd)
        near = (norms.detach() - 1).abs()
        assert bool((norms > 1).any()) and bool((norms < 1).any()) and float(near.min()) > 1e-2, norms      # away from the kink
        return lam * torch.mean(torch.clamp(norms - 1, min=0) ** 2), norms
    x = (c.x if xr is None else xr).clone().requires_grad_()
    (g,) = torch.autograd.grad(c.O.discriminator_forward(c.pd, x, c.spec).sum(), x, create_graph=True)
    norms = g.norm(2, dim=(1, 2, 3))
    return (lam / 2) * torch.mean(norms ** 2), norms


def close(got, ref, scale, tol_l2=2e-3, tol_out=1e-3):
    d = (got.cpu().double() - ref.double())
    l2 = float(d.norm() / (ref.double().norm() + 1e-2 * scale))
    outliers = float((d.abs() > 1e-2 * (float(ref.abs().max()) + 1e-2 * scale)).double().mean())
    return l2 < tol_l2 and outliers <= tol_out, (l2, outliers)


def check_critic_gradients(D, pd):
    gmax = max(float(v.grad.abs().max()) for v in pd.values() if v.grad is not None)
    n_checked = 0
    for k, p in D.named_parameters():
        if p.grad is not None:
            ok, info = close(p.grad, pd[k].grad, gmax)
            assert ok, ("D", k, info)
            n_checked += 1
    assert n_checked >= 6 and gmax > 0


@pytest.mark.parametrize("objective", ["wasserstein", "lsgan"])
@pytest.mark.parametrize("mode", ["lp", "r1"])
@pytest.mark.parametrize("n_colors,alpha", [(1, 0.5), (3, 1.0)])
def test_losses_and_gradients_match_oracle(ngan, n_colors, alpha, mode, objective):
    lam = 10.0
    c = oracle_case(ngan, n_colors, alpha)
    d_loss = oracle_d_loss(c, objective)
    pen, norms = oracle_penalty(c, mode, lam)
    (d_loss + pen).backward()
    G, D = c.G.to(DEV), c.D.to(DEV)
    LF = ngan.loss_functions
    Gp = LF.D_grad_pen_loss(G, D, lam, mode=mode)
    xd = c.x.to(DEV)
    if objective == "lsgan":
        d2 = LF.D_LS_loss(G, D, xd, z=c.z1.to(DEV))[0]
    else:
        d2 = LF.D_W_loss(G, D, 0.001)(xd, z=c.z1.to(DEV))[0]
    gp2 = Gp(xd, z=c.z2.to(DEV), epsilon=c.eps.to(DEV))
    (d2 + gp2).backward()
    got = np.array([float(d2.detach()), float(gp2.detach())])
    want = np.array([float(d_loss.detach()), float(pen.detach())])
    print("STAT PENALTY losses", mode, objective, got, want, norms.detach().numpy())
    assert np.allclose(got, want, rtol=1e-3, atol=2e-5) and want[1] > 0, (got, want)
    assert np.allclose(Gp.last_grad_norms.cpu().numpy(), norms.detach().numpy(), rtol=1e-3)
    check_critic_gradients(D, c.pd)
    assert not xd.requires_grad and all(p.grad is None for p in G.parameters())       # r1 left the caller's images as they were


def test_r1_differentiates_at_the_augmented_reals(ngan):
    """all five groups with injected tables: the W-loss and the zero-centred penalty both see T(real)"""
    import diffaug_cases as A0
    import diffgeo_cases as A
    lam, res = 10.0, 16
    c = oracle_case(ngan, 1, 0.5)
    m, m0 = A.master_rows(res), A0.master_rows(res)
    geo, old = dict(real=m[9:13], fake=m[13:17]), dict(real=m0[0:4], fake=m0[4:8])
    fill = ngan.loss_functions.DIFFAUG_FILL
    T = lambda im, kind: A0.transcription(A.transcription(im, geo[kind], fill), old[kind], fill)      # noqa: E731
    xr = T(c.x.double(), "real").float()
    with torch.no_grad():
        fake = T(c.O.generator_forward(c.pg, c.z1, c.spec).double(), "fake").float()
    real_score = c.O.discriminator_forward(c.pd, xr, c.spec)
    d_loss = -real_score.mean() + c.O.discriminator_forward(c.pd, fake, c.spec).mean() + 0.001 * torch.square(real_score).mean()
    pen, norms = oracle_penalty(c, "r1", lam, xr=xr)
    plain = float(oracle_penalty(c, "r1", lam)[0].detach())
    (d_loss + pen).backward()
    G, D = c.G.to(DEV), c.D.to(DEV)
    LF = ngan.loss_functions
    kw = {"geo_" + k: ngan.ops.diffgeo_table(v, DEV) for k, v in geo.items()}
    kw.update({k: ngan.ops.diffaug_table(v, DEV) for k, v in old.items()})
    hook = LF.DiffAugmentHook(**kw)
    Gp = LF.D_grad_pen_loss(G, D, lam, mode="r1")
    xd = c.x.to(DEV)
    d2 = LF.D_W_loss(G, D, 0.001)(xd, z=c.z1.to(DEV), augment=hook)[0]
    gp2 = Gp(xd, augment=hook)
    (d2 + gp2).backward()
    got, want = np.array([float(d2.detach()), float(gp2.detach())]), np.array([float(d_loss.detach()), float(pen.detach())])
    print("STAT PENALTY r1 through the transform", got, want, plain)
    assert np.allclose(got, want, rtol=1e-3, atol=2e-5), (got, want)
    assert abs(plain - want[1]) > 1e-2 * want[1]                                       # the transform did move the penalty
    assert np.allclose(Gp.last_grad_norms.cpu().numpy(), norms.detach().numpy(), rtol=1e-3)
    check_critic_gradients(D, c.pd)


# ---------------------------------------------------------------------------------------------------------------------
# the trainer
# ---------------------------------------------------------------------------------------------------------------------
class LaunchCount:
    """a launch probe (ngan._C.set_probe) that times nothing and counts every entry-point call"""

    def __init__(self):
        self.n = 0

    def wants(self, name, args):
        self.n += 1
        return False


def test_the_defaults_are_the_trainer_without_the_arguments(ngan):
    def run(replayed, **kw):
        tr = ngan.train.PGGANTrainer(*small_nets(ngan), learning_rate=1e-3, device_latents=True, **kw)
        torch.manual_seed(21)
        x = batch_draws(ngan, 3, 4)["real"]
        stats = []
        for _ in range(3):
            s = tr.step(x) if replayed else tr.train_iteration(x)
            stats.append({k: float(v) for k, v in s.items()})
        probe = LaunchCount()
        ngan._C.set_probe(probe)
        try:
            tr.train_iteration(x)
        finally:
            ngan._C.set_probe(None)
        torch.cuda.synchronize()
        return state_of(tr), stats, probe.n, torch.cuda.get_rng_state(DEV), list(tr._graphs)
    for replayed in (False, True):
        want = run(replayed)
        got = run(replayed, grad_pen_mode="gp", grad_pen_interval=1)
        assert same(got[0], want[0]) and got[1] == want[1] and got[2] == want[2] > 0 and torch.equal(got[3], want[3]), replayed
        assert got[4] == want[4] == ([(4, 1, 16, 16)] if replayed else [])           # interval 1: today's key
        other = run(replayed, grad_pen_mode="r1")
        assert not same(other[0], want[0]) and other[2] < want[2]                     # no second generator batch, no interpolate


def eager_and_replayed(ngan, n_iter=7, mask=0, nets=small_nets, **kw):
    """n_iter eager iterations against capture-on-first-sight + replay from the same state with the same injected draws, batches of 4"""
    batches = [batch_draws(ngan, 60 + i, 4, mask=mask) for i in range(n_iter)]
    eager = ngan.train.PGGANTrainer(*nets(ngan), learning_rate=1e-3, **kw)
    stats_e = []
    for d in batches:
        s = eager.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"], tables=d["tables"])
        stats_e.append({k: float(v) for k, v in s.items()})
    tr = ngan.train.PGGANTrainer(*nets(ngan), learning_rate=1e-3, **kw)
    statics, stats_r, captured_at = {}, [], []
    for i, d in enumerate(batches):
        own = {k: d[k] for k in ("z_d", "z_gp", "eps", "z_g")}
        key = tr._graph_key(d["real"].shape)
        if not tr.has_graph(d["real"].shape):
            before = state_of(tr), torch.cuda.get_rng_state(DEV), torch.get_rng_state(), tr.grad_pen_iteration
            statics[key] = {k: v.clone() for k, v in own.items()}
            tr.capture(d["real"], draws=statics[key], tables=d["tables"])
            torch.cuda.synchronize()
            after = state_of(tr), torch.cuda.get_rng_state(DEV), torch.get_rng_state(), tr.grad_pen_iteration
            assert same(before[0], after[0]) and torch.equal(before[1], after[1]) and torch.equal(before[2], after[2])
            assert before[3] == after[3] == i                                           # capture() trains nothing and holds the count
            captured_at.append(i)
        for k, v in own.items():
            statics[key][k].copy_(v)
        s = tr.replay(d["real"], tables=d["tables"])
        stats_r.append({k: float(v) for k, v in s.items()})
        assert tr.grad_pen_iteration == i + 1
    torch.cuda.synchronize()
    return eager, tr, stats_e, stats_r, captured_at


def check_schedule(stats, k, lam=True):
    for i, s in enumerate(stats):
        assert np.isfinite(list(s.values())).all(), (i, s)
        if lam and i % k == 0:
            assert s["D_grad_pen"] > 0, (i, s)
        else:
            assert s["D_grad_pen"] == 0.0, (i, s)


def steep_nets(ngan, base=None):
    """small_nets (or `base`'s nets) with the critic's last layer scaled so that every |grad D(x_hat)| of the first batch is 2 or more: the freshly
    initialised critic's input gradients are far below 1, where the one-sided penalty is (rightly) zero"""
    G, D = (base or small_nets)(ngan)
    d = batch_draws(ngan, 60, 4)
    probe = ngan.loss_functions.D_grad_pen_loss(G, D, 10.0)
    probe(d["real"], z=d["z_gp"], epsilon=d["eps"])
    last = [m for m in D.layers if getattr(m, "weight", None) is not None][-1]
    with torch.no_grad():
        last.weight.mul_(2.0 / float(probe.last_grad_norms.min()))
    return G, D                          # (the trainer's constructor re-packs the weights: ops.bump_weight_epoch)


@pytest.mark.parametrize("mode,k", [("lp", 1), ("r1", 1), ("gp", 3), ("r1", 3)])
def test_eager_and_replayed_iterations_are_bit_equal(ngan, mode, k):
    nets = steep_nets if mode == "lp" else small_nets
    eager, tr, stats_e, stats_r, captured_at = eager_and_replayed(ngan, nets=nets, grad_pen_mode=mode, grad_pen_interval=k)
    assert stats_e == stats_r, (stats_e, stats_r)
    assert same(state_of(eager), state_of(tr)) and eager.grad_pen_iteration == tr.grad_pen_iteration == 7
    check_schedule(stats_e, k)
    assert captured_at and max(captured_at) <= 2 * k + 1 and len(captured_at) <= 3, captured_at      # the captures settle
    assert captured_at[0] == 0 and (k == 1 or 1 in captured_at)
    assert len(tr._graphs) == (1 if k == 1 else 2)
    if k > 1:
        # k times the weight in the due iterations: the first one's penalty is k times the interval-1 trainer's
        one = ngan.train.PGGANTrainer(*nets(ngan), learning_rate=1e-3, grad_pen_mode=mode)
        d = batch_draws(ngan, 60, 4)
        first = float(one.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"])["D_grad_pen"])
        assert abs(stats_e[0]["D_grad_pen"] - k * first) <= 1e-5 * k * first


def test_with_augmentation_and_average(ngan):
    eager, tr, stats_e, stats_r, _ = eager_and_replayed(ngan, n_iter=4, mask=6, diffaug="translation,cutout", ema_beta=0.999,
                                                        grad_pen_mode="r1", grad_pen_interval=3)
    assert stats_e == stats_r and eager.ema_enabled and same(state_of(eager), state_of(tr))
    check_schedule(stats_e, 3)


def mbstd_nets(ngan):
    torch.manual_seed(6)
    G = ngan.models.Generator_PG([32, 16], image_size_init=8, latent_dim=TL.LATENT)
    D = ngan.models.Discriminator_PG([16, 32], image_size_init=8, mbstd_group=2)
    G.set_resolution(16, 1.0)
    D.set_resolution(16, 1.0)
    return G.to(DEV), D.to(DEV)


def test_with_minibatch_standard_deviation(ngan):
    for mode, nets in (("lp", lambda ngan: steep_nets(ngan, mbstd_nets)), ("r1", mbstd_nets)):
        eager, tr, stats_e, stats_r, _ = eager_and_replayed(ngan, n_iter=3, nets=nets, grad_pen_mode=mode, grad_pen_interval=2)
        assert stats_e == stats_r and same(state_of(eager), state_of(tr))
        check_schedule(stats_e, 2)


def test_in_the_bf16_storage_mode(ngan):
    try:
        ngan.ops.set_conv_precision("bf16")
        eager, tr, stats_e, stats_r, _ = eager_and_replayed(ngan, n_iter=4, grad_pen_mode="r1", grad_pen_interval=3)
        lp = eager_and_replayed(ngan, n_iter=2, nets=steep_nets, grad_pen_mode="lp")
    finally:
        ngan.ops.set_conv_precision("f32")
    assert stats_e == stats_r and same(state_of(eager), state_of(tr)) and all(np.isfinite(v).all() for v in state_of(tr))
    check_schedule(stats_e, 3)
    assert lp[2] == lp[3] and same(state_of(lp[0]), state_of(lp[1]))
    check_schedule(lp[2], 1)


def test_two_critic_steps_share_the_iteration_phase(ngan):
    tr = ngan.train.PGGANTrainer(*steep_nets(ngan), learning_rate=1e-3, n_critic=2, grad_pen_mode="lp", grad_pen_interval=2)
    seen = []
    inner = tr.d_step
    tr.d_step = lambda *a, **kw: seen.append((tr.grad_pen_iteration, tr.penalty_due)) or inner(*a, **kw)
    stats = []
    for i in range(4):
        d = batch_draws(ngan, 80 + i, 4)
        stats.append({k: float(v) for k, v in tr.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"]).items()})
    assert seen == [(0, True), (0, True), (1, False), (1, False), (2, True), (2, True), (3, False), (3, False)]
    check_schedule(stats, 2)
    # d_step on its own reads the phase as it stands and does not advance it; n_critic = 0 monitors in the phase likewise
    assert tr.grad_pen_iteration == 4 and float(inner(d["real"])["D_grad_pen"]) > 0 and tr.grad_pen_iteration == 4
    tr.n_critic = 0
    assert float(tr.train_iteration(d["real"])["D_grad_pen"]) > 0 and tr.grad_pen_iteration == 5
    assert float(tr.train_iteration(d["real"])["D_grad_pen"]) == 0.0 and tr.grad_pen_iteration == 6


def test_r1_runs_the_generator_on_b_latents(ngan):
    rows = {}
    for mode in ("gp", "lp", "r1"):
        G, D = small_nets(ngan)
        tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3, device_latents=True, grad_pen_mode=mode, grad_pen_interval=2)
        seen = []
        G.register_forward_hook(lambda mod, inp, out: seen.append(inp[0].shape[0]))
        x = batch_draws(ngan, 3, 4)["real"]
        tr.d_step(x)                       # due
        tr.grad_pen_iteration = 1
        tr.d_step(x)                       # not due
        rows[mode] = seen
    assert rows == {"gp": [8, 4], "lp": [8, 4], "r1": [4, 4]}


# ---- two ranks on one GPU, shares 3 and 1 -----------------------------------------------------------------------------------------
def _share_worker(rank, world, port, fixture, q):
    """tests/test_gpu_lsgan.py::_share_worker with grad_pen_mode="r1", grad_pen_interval=2: a due and a not-due critic step"""
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
        kw = dict(grad_pen_mode="r1", grad_pen_interval=2)
        G, D = T.build_small(ngan, fix)
        tr = ngan.train.PGGANTrainer(G, D, **kw)                          # world = 2: exchanges on
        assert tr.world == world
        Gr, Dr = T.build_small(ngan, fix)
        ref = ngan.train.PGGANTrainer(Gr, Dr, process_group=own, **kw)   # world = 1 on the whole batch
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

        worst = []
        for it, due in ((0, True), (1, False)):
            tr.grad_pen_iteration = ref.grad_pen_iteration = it
            s = tr.d_compute(t("real")[sl], t("z_d")[sl], t("z_gp")[sl], t("eps")[sl], global_batch=shares)
            tr._exchange(tr.flat_d)
            sr = ref.d_compute(t("real"), t("z_d"), t("z_gp"), t("eps"))
            assert (float(s["D_grad_pen"]) > 0) == due == (float(sr["D_grad_pen"]) > 0)
            worst.append(check(tr.flat_d, ref.flat_d, f"critic step, due {due}"))
        torch.cuda.synchronize()
        q.put((rank, "ok", worst[0], worst[1]))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None, None))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_shares_3_and_1_match_the_whole_batch():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = TL._free_port()
    procs = [ctx.Process(target=_share_worker, args=(r, 2, port, "small_res16_fade_warm", q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    results = sorted(q.get(timeout=5) for _ in range(2))
    print("PENALTY r1 shares 3 + 1, worst deviation / scale (due, not due) per rank:", [r[2:] for r in results])
    assert [r[:2] for r in results] == [(0, "ok"), (1, "ok")], results
    assert all(p.exitcode == 0 for p in procs)


# ---- epoch driver and checkpoint ----------------------------------------------------------------------------------------------------
def driver_run(ngan, f, epochs, resume=False, mode="r1", k=3):
    """tests/test_gpu_lsgan.py::driver_run with the penalty's arguments: one batch, so one iteration, per epoch"""
    cfg = types.SimpleNamespace(**TL.DRIVER_CFG)
    G, D = small_nets(ngan, res=8)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, device_latents=True, alpha_step=cfg.alpha_step, grad_pen_mode=mode,
                                 grad_pen_interval=k)
    data = ngan.train.TensorImageDataset.synthetic(4, 16, device=DEV, seed=8)
    ck = ngan.utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=DEV, trainer=tr,
                                 extra_checkpoint_period=1e3)
    if resume:
        ck.load_state()
    series = ngan.train.pggan_train(tr, data, cfg, checkpoint=ck, epoch_init=epochs[0], epoch_final=epochs[1], use_graph=True,
                                    log=lambda *a: None, draws=TL.driver_draws, on_epoch=lambda ep, t: torch.manual_seed(100 + ep))
    torch.cuda.synchronize()
    return series, state_of(tr), tr.grad_pen_iteration


def test_epoch_driver_resumes_the_schedule_bit_equal(ngan, tmp_path):
    f = str(tmp_path / "a.pth")
    series, state, count = driver_run(ngan, f, (1, 5))                                # four epochs straight: iterations 0 .. 3
    assert count == 4 and [v > 0 for v in series["D_grad_pen"]] == [True, False, False, True], series
    assert all(len(v) == 4 and np.isfinite(v).all() for v in series.values()), series
    f2 = str(tmp_path / "b.pth")
    first, _, count1 = driver_run(ngan, f2, (1, 3))                                   # two epochs, the checkpoint ...
    d = ngan.utils.load_checkpoint_dict(f2)
    assert count1 == 2 and (d["grad_pen_mode"], d["grad_pen_interval"], d["grad_pen_iteration"]) == ("r1", 3, 2)
    with pytest.raises(ValueError, match="grad_pen_mode=r1.*grad_pen_mode=lp"):       # ... not to be resumed under another mode ...
        driver_run(ngan, f2, (3, 5), resume=True, mode="lp")
    more, state2, count2 = driver_run(ngan, f2, (3, 5), resume=True)                  # ... and resumed for two more
    assert count2 == 4 and [first[k] + more[k] for k in series] == [series[k] for k in series]
    assert same(state2, state)
