"""The pairwise similarity loss of the generator on the GPU: the kernels of csrc/simloss.hip through the entry points of
include/nganx.h against the fp64 oracle of tests/simloss_cases.py at the bounds derived and settled there (the emulation's worst
err / bound on the CPU: G 0.02, S 0.004, L 0.75, M 0.98 -- its one fp32 rounding --, gradient 0.3), then the autograd node, the
trainer, two ranks, and the epoch driver with its checkpoint.

measured on MI355X (a record, not a bound: worst err / bound over the kernel cases; 1 is the bound): G 0.10 (B = 16, N = 16), S 0.044,
L 0.65, M 0.99 (its one fp32 rounding), r 0.85, gradient 0.39; G, S, M and every gradient element equal the emulation's bits.  The
trainer's G_sim_loss against the oracle: 0.65 of its bound; critic part + oracle term against one backward pass: relative l2 5.0e-7
against 2e-3.  Two ranks with shares 4 + 4 and 5 + 3: worst deviation / scale of the generator gradient 8.5e-8 and 4.7e-7 against
the bound 2e-4.  The module takes 11 s."""
import types

import numpy as np
import pytest
import torch

import simloss_cases as L
from test_gpu_specloss import (_free_port, batch_draws, driver_draws, same, small_nets, state_of, target16, DRIVER_CFG)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
SENTINEL = -7.0
LAM = 0.7


class Guarded:
    """a device buffer of n elements with PAD sentinel elements on either side (16-byte alignment of the payload is kept)"""

    def __init__(self, n, dtype):
        self.whole = torch.full((n + 2 * PAD,), SENTINEL, device=DEV, dtype=dtype)
        self.view = self.whole[PAD:PAD + n]

    def intact(self):
        return bool((self.whole[:PAD] == SENTINEL).all()) and bool((self.whole[PAD + self.view.numel():] == SENTINEL).all())

    def untouched(self):
        return bool((self.whole == SENTINEL).all())


def raw(ngan, x, z, lam, center, upstream=1.0, addend=None, alias=False):
    """the three entry points on guarded buffers -> (outputs as numpy, guards).  alias: the addend is written into grad first and
    handed over as grad itself"""
    C = ngan._C
    lib = C.lib()
    xd, zd = torch.as_tensor(x).to(DEV).contiguous(), torch.as_tensor(z).to(DEV).contiguous()
    b, n, nz = x.shape[0], x.shape[1], z.shape[1]
    bufs = {"gx": Guarded(b * b, torch.float64), "sx": Guarded(b, torch.float64), "gz": Guarded(b * b, torch.float64),
            "sz": Guarded(b, torch.float64), "wx": Guarded(lib.nganx_pair_gram_workspace_bytes(b, n) // 8, torch.float64),
            "wz": Guarded(lib.nganx_pair_gram_workspace_bytes(b, nz) // 8, torch.float64), "loss": Guarded(4, torch.float32),
            "sim": Guarded(b * b, torch.float64), "mix": Guarded(b * b, torch.float32), "shift": Guarded(b, torch.float32),
            "grad": Guarded(b * n, torch.float32)}
    v = {k: g.view for k, g in bufs.items()}
    C.call("nganx_pair_gram", xd, v["gx"], v["sx"], v["wx"], b, n)
    C.call("nganx_pair_gram", zd, v["gz"], v["sz"], v["wz"], b, nz)
    lam_dev, up = torch.tensor(float(lam), device=DEV), torch.tensor(float(upstream), device=DEV)
    C.call("nganx_simloss_head", v["gx"], v["sx"], v["gz"], lam_dev, b, n, int(center), v["loss"], v["sim"], v["mix"], v["shift"])
    add = None
    if addend is not None:
        if alias:
            v["grad"].copy_(torch.as_tensor(addend).reshape(-1))
            add = v["grad"]
        else:
            add = torch.as_tensor(addend).to(DEV).contiguous()
    C.call("nganx_pair_mix", xd, v["mix"], v["shift"], up, add, v["grad"], b, n)
    torch.cuda.synchronize()
    assert bool((v["loss"][1:] == SENTINEL).all()), "the head wrote beyond loss[0]"
    gx, sx = v["gx"].view(b, b).cpu().numpy(), v["sx"].cpu().numpy()
    mean = sx / n if center else np.zeros(b)
    out = {"G": gx - n * (mean[:, None] * mean[None, :]), "G_raw": gx, "sums": sx, "Gz": v["gz"].view(b, b).cpu().numpy(),
           "L": v["loss"][0].cpu().numpy(), "S": v["sim"].view(b, b).cpu().numpy(), "M": v["mix"].view(b, b).cpu().numpy(),
           "r": v["shift"].cpu().numpy(), "grad": v["grad"].view(b, n).cpu().numpy()}
    return out, bufs


def n_of(spec):
    return (128 * 128 + 4) if spec == "tail" else spec


SHAPES = [(b, n) for b in (2, 3, 5, 16) for n in (16, 64 * 64, "tail")] + [(64, 32 * 32)]


@pytest.mark.parametrize("center", [False, True], ids=["raw", "centred"])
@pytest.mark.parametrize("b, n", SHAPES)
def test_kernels_per_element_against_fp64(ngan, b, n, center):
    """every element of G, the sums' effect, S, L, M, r and the gradient within the bounds of simloss_cases; upstream 1 without an
    addend and 0.37 with one, the addend apart and aliasing grad (the same bits); guard bands intact; a second call gives the same bits"""
    n = n_of(n)
    family = "micrograph" if n == 64 * 64 else "cancel" if n == 16 else "noise"
    x, z = L.images(family, b, n), L.latents(b)
    addend = np.random.default_rng(b).uniform(-1e-3, 1e-3, x.shape).astype(np.float32)
    for up, add in ((1.0, None), (0.37, addend)):
        got, bufs = raw(ngan, x, z, LAM, center, up, add)
        assert all(g.intact() for g in bufs.values()), [k for k, g in bufs.items() if not g.intact()]
        r = L.ratios(got, x, z, LAM, center, up, add)
        print(f"STAT simloss B={b} N={n} {family} center={int(center)} up={up:g} addend={int(add is not None)} err/bound: "
              + " ".join(f"{k} {v:.4f}" for k, v in r.items()))
        assert max(r.values()) <= 1.0, r
        assert np.array_equal(got["G_raw"], got["G_raw"].T), "the Gram matrix is not symmetric bit for bit"
        again, _ = raw(ngan, x, z, LAM, center, up, add)
        assert all(np.array_equal(again[k], got[k], equal_nan=True) for k in got), "two calls differ"
    aliased, bufs = raw(ngan, x, z, LAM, center, 0.37, addend, alias=True)
    assert np.array_equal(aliased["grad"], got["grad"]) and all(g.intact() for g in bufs.values())
    emu = L.emulate(x, z, LAM, center, 0.37, addend)
    print(f"STAT simloss B={b} N={n} equal to the emulation's bits: G {100 * (emu['G'] == got['G']).mean():.1f} % "
          f"S {100 * (emu['S'] == got['S']).mean():.1f} % M {100 * (emu['M'] == got['M']).mean():.1f} % "
          f"grad {100 * (emu['grad'] == got['grad']).mean():.2f} %")


def test_the_real_stage_shape(ngan):
    """(4, 1, 512, 512): the slab count and the tail of the flagship stage"""
    x, z = L.images("micrograph", 4, 512 * 512), L.latents(4)
    for center in (False, True):
        got, bufs = raw(ngan, x, z, LAM, center)
        r = L.ratios(got, x, z, LAM, center)
        print(f"STAT simloss B=4 N=512x512 center={int(center)} err/bound: " + " ".join(f"{k} {v:.4f}" for k, v in r.items()))
        assert max(r.values()) <= 1.0 and all(g.intact() for g in bufs.values()), r


def test_refusals_launch_nothing(ngan):
    """B = 1 and 65, N = 18, a null pointer and a misaligned one: a status, a message that names the argument, untouched outputs"""
    C = ngan._C
    lib = C.lib()
    x = torch.zeros(65 * 64 + 4, device=DEV)
    out64, out32 = Guarded(65 * 65 + 65, torch.float64), Guarded(65 * 64, torch.float32)
    ws = torch.empty(1 << 16, device=DEV, dtype=torch.float64)
    one = torch.ones((), device=DEV)
    g, s = out64.view[:64 * 64], out64.view[64 * 64:64 * 64 + 64]
    assert lib.nganx_pair_gram_workspace_bytes(1, 64) == lib.nganx_pair_gram_workspace_bytes(65, 64) == 0
    assert lib.nganx_pair_gram_workspace_bytes(2, 18) == lib.nganx_pair_gram_workspace_bytes(2, 12) == 0

    def refused(name, word, *args):
        with pytest.raises(RuntimeError, match=word) as e:
            C.call(name, *args)
        assert "status -" in str(e.value)
    for b, n, word in ((1, 64, "B=1"), (65, 64, "B=65"), (2, 18, "N=18")):
        refused("nganx_pair_gram", word, x, g, s, ws, b, n)
        refused("nganx_simloss_head", word, g, s, g, one, b, n, 1, out32.view[:1], g, out32.view[:16], out32.view[:4])
        refused("nganx_pair_mix", word, x, out32.view[:16], out32.view[:4], one, None, out32.view, b, n)
    refused("nganx_pair_gram", "rows is a null", None, g, s, ws, 2, 64)
    refused("nganx_pair_gram", "workspace is a null", x, g, s, None, 2, 64)
    refused("nganx_simloss_head", "lambda is a null", g, s, g, None, 2, 64, 0, out32.view[:1], g, out32.view[:16], out32.view[:4])
    refused("nganx_pair_mix", "grad is a null", x, out32.view[:16], out32.view[:4], one, None, None, 2, 64)
    refused("nganx_pair_gram", "rows must start on a 16-byte", x[1:], g, s, ws, 2, 64)
    refused("nganx_pair_mix", "addend must start on a 16-byte", x, out32.view[:16], out32.view[:4], one, x[1:], out32.view, 2, 64)
    refused("nganx_pair_mix", "grad must start on a 16-byte", x, out32.view[:16], out32.view[:4], one, None, out32.view[1:], 2, 64)
    torch.cuda.synchronize()
    assert out64.untouched() and out32.untouched()


def test_a_zero_norm_row_gives_nan_and_stays_in_bounds(ngan):
    """no epsilon: a constant row under centring (and a zero row without) has squared norm 0; L, r, every gradient element, the row's
    cosines and every M entry that meets the row (its row, its column and, through sum_j A_ij S_ij, the diagonal) are NaN, as the
    reference's division gives, and nothing is written out of bounds"""
    for center, value in ((True, 0.25), (False, 0.0)):
        x = L.images("noise", 5, 1024)
        x[2] = value
        got, bufs = raw(ngan, x, L.latents(5), LAM, center)
        touched = np.eye(5, dtype=bool)                  # every M_ii sums A_i2 S_i2; row and column 2 divide by the zero norm
        touched[2, :] = touched[:, 2] = True
        assert np.isnan(got["L"]) and np.isnan(got["M"][touched]).all() and np.isfinite(got["M"][~touched]).all()
        assert np.isnan(got["r"]).all() and np.isnan(got["grad"]).all() and all(g.intact() for g in bufs.values())
        assert np.isnan(got["S"][2]).all() and np.isnan(got["S"][:, 2]).all()
        assert np.isfinite(np.delete(np.delete(got["S"], 2, 0), 2, 1)).all()


# ---- the autograd node -------------------------------------------------------------------------------------------------------------
def test_operator_gradient_against_fp64_autograd(ngan):
    x = torch.tensor(L.images("noise", 5, 32 * 32)).view(5, 1, 32, 32).to(DEV).requires_grad_()
    z = torch.tensor(L.latents(5)).to(DEV).requires_grad_()
    lam = torch.tensor(LAM, device=DEV)
    for center in (False, True):
        x.grad = None
        images, loss, sim = ngan.ops.SimilarityLoss.apply(x, z, lam, center)
        assert images.data_ptr() == x.data_ptr() and not sim.requires_grad and sim.dtype == torch.float64
        weight = torch.linspace(-1, 1, x.numel(), device=DEV).view_as(x)
        (0.37 * loss + (images * weight).sum()).backward()            # a gradient arrives at the pass-through as well
        xn, zn = x.detach().view(5, -1).cpu().numpy(), z.detach().cpu().numpy()
        add = weight.view(5, -1).cpu().numpy()
        ref, bnd = L.oracle(xn, zn, LAM, center, 0.37, add), L.bounds(xn, zn, LAM, center, 0.37, add)
        r = {"L": L.ratio(float(loss), ref["L"], bnd["L"]), "grad": L.ratio(x.grad.view(5, -1).cpu().numpy(), ref["grad"], bnd["grad"])}
        print(f"STAT SimilarityLoss center={int(center)} err/bound: L {r['L']:.4f} grad {r['grad']:.4f}")
        assert max(r.values()) <= 1.0 and z.grad is None, r
        public = ngan.loss_functions.G_similarity_loss(x.detach(), z.detach(), Lambda=LAM, center=center)
        assert float(public) == float(loss) and float(ngan.loss_functions.G_similarity_loss(x.detach(), z.detach(), lam, center)) == float(loss)
    _, loss, _ = ngan.ops.SimilarityLoss.apply(x, z, lam, False)
    with pytest.raises((NotImplementedError, RuntimeError), match="second derivative"):
        torch.autograd.grad(loss, x, create_graph=True)
    one = ngan.loss_functions.G_similarity_loss(x[:1], z[:1].detach())           # no pair: the zero scalar
    assert float(one) == 0.0
    with pytest.raises(ValueError, match="64"):
        ngan.ops.SimilarityLoss.apply(torch.zeros(65, 16, device=DEV), torch.zeros(65, 16, device=DEV), lam, False)


# ---- the trainer -------------------------------------------------------------------------------------------------------------------
def trainer(ngan, on="generated", lam=0.5, nets=None, **kw):
    tr = ngan.train.PGGANTrainer(*(nets or small_nets(ngan)), learning_rate=1e-3, device_latents=True,
                                 **({} if on is None else {"sim_loss_on": on}), **kw)
    if on == "generated":
        tr.set_sim_lambda(lam)
    return tr


def test_the_default_is_the_trainer_without_the_arguments(ngan):
    """sim_loss_on="real": bit-equal parameters and optimiser state after two iterations, eager and replayed, the same RNG states, no
    new attribute; "generated" ends elsewhere and draws as much"""
    def run(replayed, on):
        tr = trainer(ngan, on)
        torch.manual_seed(21)
        x = batch_draws(ngan, 3, 4)["real"]
        stats = [tr.step(x) if replayed else tr.train_iteration(x) for _ in range(2)][-1]
        torch.cuda.synchronize()
        return state_of(tr), torch.cuda.get_rng_state(DEV), torch.get_rng_state(), tr, set(stats)
    for replayed in (False, True):
        want, off, on = run(replayed, None), run(replayed, "real"), run(replayed, "generated")
        assert same(off[0], want[0]) and torch.equal(off[1], want[1]) and torch.equal(off[2], want[2]), replayed
        assert set(vars(off[3])) == set(vars(want[3])) and not any("sim" in k for k in vars(off[3])) and off[4] == want[4]
        assert not off[3].similarity_enabled and "G_sim_loss" not in off[4]
        assert not same(on[0], want[0]) and torch.equal(on[1], want[1]) and torch.equal(on[2], want[2]), replayed
        assert on[4] == want[4] | {"G_sim_loss"} and all(np.isfinite(v).all() for v in on[0])
    with pytest.raises(ValueError, match="real"):
        off[3].set_sim_lambda(1.0)
    with pytest.raises(ValueError, match="sim_loss_on"):
        ngan.train.PGGANTrainer(*small_nets(ngan), sim_loss_on="fake")
    with pytest.raises(ValueError, match="at most 64"):
        big = batch_draws(ngan, 4, 65)
        trainer(ngan).g_compute(big["real"], big["z_g"])


VARIANTS = {"plain": {}, "centred": dict(sim_loss_center=True), "lsgan": dict(objective="lsgan"),
            "diffaug": dict(diffaug="color,translation"), "spectral": dict(spec_loss_lambda=1.0),
            "rmsprop_ema_mbstd": dict(optimizer="rmsprop", ema_beta=0.999), "lp": dict(grad_pen_mode="lp"), "r1": dict(grad_pen_mode="r1"),
            "bf16": dict()}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_eager_and_replayed_iterations_are_bit_equal(ngan, variant):
    """three eager iterations against capture + three replays with injected draws, the term on, under the switches it must work with"""
    if variant == "bf16":
        ngan.ops.set_conv_precision("bf16")
    try:
        kw = VARIANTS[variant]
        mask = 3 if "diffaug" in kw else 0
        nets = lambda: small_nets(ngan, mbstd_group=4 if "mbstd" in variant else 0)      # noqa: E731
        batches = [batch_draws(ngan, 40 + i, 4, mask=mask) for i in range(3)]

        def make():
            tr = trainer(ngan, nets=nets(), **kw)
            if "spec_loss_lambda" in kw:
                tr.set_spectral_target(16, target16())
            return tr
        eager, stats_e = make(), []
        for d in batches:
            s = eager.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"], tables=d["tables"])
            stats_e.append({k: float(v) for k, v in s.items()})
        tr, static, stats_r = make(), None, []
        for d in batches:
            own = {k: d[k] for k in ("z_d", "z_gp", "eps", "z_g")}
            if static is None:
                static = {k: v.clone() for k, v in own.items()}
                tr.capture(d["real"], draws=static, tables=d["tables"])
            for k, v in own.items():
                static[k].copy_(v)
            stats_r.append({k: float(v) for k, v in tr.replay(d["real"], tables=d["tables"]).items()})
        torch.cuda.synchronize()
        assert stats_e == stats_r and all(np.isfinite(list(s.values())).all() for s in stats_e), (stats_e, stats_r)
        assert same(state_of(eager), state_of(tr))
        assert all(s["G_sim_loss"] > 0 for s in stats_e)
    finally:
        ngan.ops.set_conv_precision("f32")


def test_lambda_is_read_live_by_the_captured_graph(ngan):
    """the same graph replayed with lambda 0, 0.5 and 0 again from the same state: the first and the third run are bit-equal, the second
    differs; with lambda = 0 the tap contributes exact zeros: the run equals the trainer without the term"""
    d = batch_draws(ngan, 50, 4)
    draws = {k: d[k] for k in ("z_d", "z_gp", "eps", "z_g")}
    tr = trainer(ngan, lam=0.25)
    tr.capture(d["real"], draws=draws)
    graphs = dict(tr._graphs)
    start = [t.clone() for t in tr._training_state()]

    def run(lam):
        for t, s in zip(tr._training_state(), start):      # back to the state the graph was captured at, as capture() itself restores it
            t.copy_(s)
        ngan.ops.bump_weight_epoch()
        tr.opt_g.repack()
        tr.opt_d.repack()
        ngan.ops.refresh_packed()
        tr.set_sim_lambda(lam)
        stats = tr.replay(d["real"])
        torch.cuda.synchronize()
        return state_of(tr), float(stats["G_sim_loss"]), float(stats["G_loss"])
    first, second, third = run(0.0), run(0.5), run(0.0)
    assert dict(tr._graphs) == graphs and len(graphs) == 1, "the graphs were captured again"
    assert same(first[0], third[0]) and first[1:] == third[1:] and first[1] == 0.0
    assert not same(first[0], second[0]) and second[1] > 0.0
    plain = trainer(ngan, None)
    plain.train_iteration(d["real"], **draws)
    assert same(state_of(plain), first[0]), "lambda = 0 is not exact zeros"


def test_one_generator_step_against_a_plain_torch_composition(ngan):
    """G_sim_loss on given latents against the fp64 oracle on the generator's own images, within its bound; the generator's parameter
    gradient with the term on equals the critic's part (a trainer without the term) plus the oracle's image gradient pushed through the
    generator by autograd, at the tolerance tests/test_gpu_specloss.py uses for the same comparison"""
    lam, d = 2.5, batch_draws(ngan, 60, 4)
    for center in (False, True):
        tr = trainer(ngan, lam=lam, sim_loss_center=center)
        tr.fused_stem = False
        stats = tr.g_compute(d["real"], d["z_g"])
        with torch.no_grad():
            images = tr.G(d["z_g"])
        assert images.dtype == torch.float32 and tuple(images.shape) == (4, 1, 16, 16)
        xn, zn = images.view(4, -1).cpu().numpy(), d["z_g"].cpu().numpy()
        ref, bnd = L.oracle(xn, zn, lam, center), L.bounds(xn, zn, lam, center)
        r = L.ratio(float(stats["G_sim_loss"]), ref["L"], bnd["L"])
        print(f"STAT trainer center={int(center)} G_sim_loss {float(stats['G_sim_loss']):.6g} (oracle {ref['L']:.6g}) err/bound {r:.4f}")
        assert r <= 1.0 and ref["L"] > 0
        both = [p.grad.detach().clone() for p in tr.flat_g.params]
        plain = trainer(ngan, None)
        plain.fused_stem = False
        assert float(plain.g_compute(d["real"], d["z_g"])["G_loss"]) == float(stats["G_loss"])      # G_loss stays the adversarial term
        critic = [p.grad.detach().clone() for p in plain.flat_g.params]
        alone = trainer(ngan, None)
        alone.flat_g.ensure_grad_views()
        alone.flat_g.zero_grad()
        alone.G(d["z_g"]).backward(torch.tensor(ref["grad"], dtype=torch.float32, device=DEV).view(4, 1, 16, 16))
        term = [p.grad.detach().clone() for p in alone.flat_g.params]
        gmax = max(float((c + s).abs().max()) for c, s in zip(critic, term))
        worst = 0.0
        for name, got, c, s in zip(tr.flat_g.names, both, critic, term):
            want = (c + s).double()
            diff = got.double() - want
            l2 = float(diff.norm() / (want.norm() + 1e-2 * gmax))
            outliers = float((diff.abs() > 1e-2 * (float(want.abs().max()) + 1e-2 * gmax)).double().mean())
            worst = max(worst, l2)
            assert l2 < 2e-3 and outliers <= 1e-3, (name, l2, outliers)
        assert max(float(s.abs().max()) for s in term) > 0 and max(float(c.abs().max()) for c in critic) > 0
        print(f"STAT critic part + oracle term against one backward pass, center={int(center)}: worst relative l2 {worst:.3e}")


# ---- epoch driver and checkpoint ---------------------------------------------------------------------------------------------------
def driver_run(ngan, f, on, epochs=(1, 5), resume=False, center=False):
    """pggan_train on four synthetic 16 x 16 images, one batch per epoch, replayed graphs, given latents; sim_loss_lambda 0.5 decaying
    by 0.1 per epoch"""
    cfg = types.SimpleNamespace(**dict(DRIVER_CFG, sim_loss_lambda=0.5, sim_loss_lambda_decay_rate=0.1, N_epochs=4, ID="sim"))
    G, D = small_nets(ngan, res=8)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, device_latents=True, alpha_step=cfg.alpha_step,
                                 **({} if on is None else {"sim_loss_on": on, "sim_loss_center": center}))
    data = ngan.train.TensorImageDataset.synthetic(4, 16, device=DEV, seed=8)
    ck = ngan.utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=torch.device(DEV), trainer=tr,
                                 extra_checkpoint_period=1e3)
    if resume:
        ck.load_state()
    lines = []
    series = ngan.train.pggan_train(tr, data, cfg, checkpoint=ck, epoch_init=epochs[0], epoch_final=epochs[1], use_graph=True,
                                    log=lambda *a: lines.append(" ".join(map(str, a))), draws=driver_draws,
                                    on_epoch=lambda ep, t: torch.manual_seed(100 + ep))
    torch.cuda.synchronize()
    return series, state_of(tr), tr, lines


def test_epoch_driver_series_checkpoint_and_resume(ngan, tmp_path, capsys):
    five = ["score_real", "score_fake", "D_loss", "G_loss", "D_grad_pen"]
    f = str(tmp_path / "a.pth")
    on, state, tr, _ = driver_run(ngan, f, "generated")
    assert list(on) == five + ["G_sim_loss"] and all(len(v) == 4 and np.isfinite(v).all() for v in on.values()), on
    assert all(v > 0 for v in on["G_sim_loss"]) and tr.has_graph((4, 1, 16, 16))
    assert float(tr._sim_lambda) == float(np.float32(0.5 * 0.9 ** 3))
    saved = ngan.utils.load_checkpoint_dict(f)
    assert saved["sim_loss_on"] == "generated" and saved["sim_loss_center"] is False
    g = str(tmp_path / "b.pth")
    head, _, _, _ = driver_run(ngan, g, "generated", epochs=(1, 3))
    tail, state2, _, _ = driver_run(ngan, g, "generated", epochs=(3, 5), resume=True)
    assert {k: head[k] + tail[k] for k in on} == on and same(state, state2), "the resumed run does not continue bit-equal"
    h = str(tmp_path / "c.pth")
    real, _, tr0, _ = driver_run(ngan, h, None, epochs=(1, 3))
    assert list(real) == five and ngan.utils.load_checkpoint_dict(h)["sim_loss_on"] == "real" and not tr0.similarity_enabled
    capsys.readouterr()                                              # resuming under other values is allowed, and said
    driver_run(ngan, h, "generated", epochs=(3, 4), resume=True, center=True)
    assert "sim_loss_on=real" in capsys.readouterr().out and ngan.utils.load_checkpoint_dict(h)["sim_loss_center"] is True


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------------
def _share_worker(rank, world, port, q):
    """a batch of 8 in shares 4 + 4 and 5 + 3: each rank's G_sim_loss is a single process's term on that rank's rows, and the exchanged
    generator gradient is the share-weighted sum of the single-process gradients on the two shares"""
    import datetime
    import os
    import sys
    import traceback
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        from __graft_entry__ import load_package
        ngan = load_package()
        own = [dist.new_group([r]) for r in range(world)][rank]          # a one-rank group: the single-process reference
        d = batch_draws(ngan, 80, 8)
        tr = ngan.train.PGGANTrainer(*small_nets(ngan), sim_loss_on="generated", sim_loss_center=True)       # world = 2: exchanges on
        ref = ngan.train.PGGANTrainer(*small_nets(ngan), process_group=own, sim_loss_on="generated", sim_loss_center=True)
        assert tr.world == world and ref.world == 1
        for t in (tr, ref):
            t.set_sim_lambda(1.5)
        worst = []
        for shares in ([4, 4], [5, 3]):
            cuts = [slice(sum(shares[:r]), sum(shares[:r + 1])) for r in range(world)]
            s = tr.g_compute(d["real"][cuts[rank]], d["z_g"][cuts[rank]], global_batch=shares)
            tr._exchange(tr.flat_g)
            want = [torch.zeros_like(p) for p in ref.flat_g.params]
            for r in range(world):                                       # sum_r (n_r / n) * the single-process gradient on share r
                s_ref = ref.g_compute(d["real"][cuts[r]], d["z_g"][cuts[r]])
                if r == rank:
                    assert float(s_ref["G_sim_loss"]) == float(s["G_sim_loss"]) > 0, (shares, rank)
                for acc, p in zip(want, ref.flat_g.params):
                    acc += (shares[r] / sum(shares)) * p.grad
            w, gmax = 0.0, max(float(v.abs().max()) for v in want)
            for name, p, v, a in zip(tr.flat_g.names, tr.flat_g.params, want, tr.flat_g.active_host):
                if not a:
                    assert float(p.grad.abs().max()) == 0.0, name
                    continue
                w = max(w, float((p.grad / world - v).abs().max()) / (float(v.abs().max()) + 1e-3 * gmax))
            assert w < 2e-4, (shares, w)
            worst.append(w)
        torch.cuda.synchronize()
        q.put((rank, "ok", worst))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_keep_their_pairs_local_and_weigh_the_shares():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_share_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    results = sorted(q.get(timeout=5) for _ in range(2))
    print("STAT similarity term, shares 4 + 4 and 5 + 3, worst deviation / scale of the generator gradient per rank:", [r[2] for r in results])
    assert [r[:2] for r in results] == [(0, "ok"), (1, "ok")], results
    assert all(p.exitcode == 0 for p in procs)
