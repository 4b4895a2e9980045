"""Pin the CPU oracle (oracle/pggan_oracle.py) against golden vectors captured from the reference's own
models.py (oracle/make_golden.py).  CPU only."""
import numpy as np
import pytest
import torch

from conftest import load_golden, split_state
from oracle import pggan_oracle as O

SMALL = ["small_fresh4", "small_res8_init", "small_res8_warm", "small_res16_fade_init", "small_res16_fade_warm",
         "small_res16_warm"]


def _specs(fix):
    res, alpha, init, latent, batch, lr = fix["meta"]
    spec = O.NetSpec(image_size_init=int(init), slope=0.2, alpha=float(alpha))
    return spec, int(batch), float(lr)


def _rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("name", SMALL)
def test_forward_matches_reference(name):
    fix = load_golden(name)
    spec, _, _ = _specs(fix)
    pg = O.as_leaf_params(split_state(fix, "G/"))
    pd = O.as_leaf_params(split_state(fix, "D/"))
    with torch.no_grad():
        img = O.generator_forward(pg, torch.from_numpy(fix["z_d"]), spec)
        score = O.discriminator_forward(pd, torch.from_numpy(fix["real"]), spec)
    assert _rel(img.numpy(), fix["G_of_z_d"]) < 2e-6
    assert _rel(score.numpy(), fix["D_of_real"]) < 2e-6


@pytest.mark.parametrize("name", SMALL)
def test_train_step_matches_reference(name):
    fix = load_golden(name)
    spec, batch, lr = _specs(fix)
    pg = O.as_leaf_params(split_state(fix, "G/"))
    pd = O.as_leaf_params(split_state(fix, "D/"))
    t = lambda k: torch.from_numpy(fix[k])
    # gradient penalty internals (loss_functions.py:175-176)
    gp, norms = O.grad_penalty(pg, spec, pd, spec, t("real"), t("z_gp"), t("eps"), 10.0, return_norms=True)
    assert _rel(norms.detach().numpy(), fix["grad_norms"]) < 5e-6
    assert abs(float(gp.detach()) - fix["scalars"][3]) / abs(fix["scalars"][3]) < 5e-6
    # one full iteration with per-parameter gradient capture.  Each Adam step is taken on the reference's own gradients once ours are
    # pinned: a first step moves a weight by lr * g / (|g| + 1e-8), so an entry whose gradient is rounding noise of the size of eps
    # (the host's summation order: vector width, thread count) moves by a noise-dependent fraction of lr -- up to 0.06 lr on some hosts
    # with gradients inside the 2e-5 pin.  On identical gradients the two optimisers must agree to within the bound below.
    opt_g, opt_d = O.make_adam(pg, lr), O.make_adam(pd, lr)
    O.zero_grads(pd)
    d_loss, s_real, s_fake = O.d_w_loss(pg, spec, pd, spec, t("real"), t("z_d"), 0.001)
    gp = O.grad_penalty(pg, spec, pd, spec, t("real"), t("z_gp"), t("eps"), 10.0)
    (d_loss + gp).backward()
    for k, v in split_state(fix, "Dgrad/").items():
        assert _rel(pd[k].grad.numpy(), v) < 2e-5, k
        pd[k].grad = torch.from_numpy(v.copy())
    opt_d.step()
    O.zero_grads(pg)
    O.zero_grads(pd)
    g_loss = O.g_w_loss(pg, spec, pd, spec, t("z_g"))
    g_loss.backward()
    for k, v in split_state(fix, "Ggrad/").items():
        assert _rel(pg[k].grad.numpy(), v) < 2e-5, k
        pg[k].grad = torch.from_numpy(v.copy())
    opt_g.step()
    got = np.array([float((d_loss + gp).detach()), float(s_real.detach()), float(s_fake.detach()), float(gp.detach()), float(g_loss.detach())])
    assert np.allclose(got, fix["scalars"], rtol=5e-6, atol=1e-8)
    # Adam moves every weight by ~lr; an update is g/(|g|+eps)-like, so compare the step itself loosely
    for k, v in split_state(fix, "G_after/").items():
        assert np.abs(pg[k].detach().numpy() - v).max() < 0.05 * lr, k
    for k, v in split_state(fix, "D_after/").items():
        if k != "alpha":
            assert np.abs(pd[k].detach().numpy() - v).max() < 0.05 * lr, k


def test_pixelnorm_second_order_fp64():
    """gradcheck / gradgradcheck of the oracle PixelNorm∘LReLU (the only op with a non-zero Hessian)."""
    torch.manual_seed(0)
    x = torch.randn(2, 6, 3, 3, dtype=torch.float64, requires_grad=True)
    f = lambda v: O.pixel_norm(O.lrelu(v, 0.2))
    assert torch.autograd.gradcheck(f, (x,), atol=1e-6)
    assert torch.autograd.gradgradcheck(f, (x,), atol=1e-6)


def test_flop_model_matches_survey():
    """F_G / F_D at the four stages (GFLOP per image per forward)."""
    g = [128, 64, 32, 32, 16, 16]
    d = [16, 16, 32, 32, 64, 128]
    want = {(16, 1.0): (0.1091, 0.0756), (64, 0.5): (0.5624, 0.3024), (256, 1.0): (2.0741, 0.9081), (512, 1.0): (4.4963, 1.5184)}
    for (res, alpha), (fg, fd) in want.items():
        got = O.forward_flops(g, d, 16, res, 512, alpha)
        assert abs(got[0] / 1e9 - fg) < 2e-4 and abs(got[1] / 1e9 - fd) < 2e-4, (res, got)


def test_package_work_model_matches_oracle_and_survey(ngan):
    """neuron-gan_amd/workmodel.py (what bench.py divides by) against the oracle's independent count and SURVEY.md 8(d)'s
    W_alg and E columns."""
    wm = ngan.workmodel
    g = [128, 64, 32, 32, 16, 16]
    d = [16, 16, 32, 32, 64, 128]
    want = {(16, 1.0): (1.604, 2.50), (64, 0.5): (7.046, 15.48), (256, 1.0): (23.084, 102.50), (512, 1.0): (43.739, 308.61)}
    for (res, alpha), (w_alg, e) in want.items():
        assert wm.forward_flops(g, d, 16, res, 512, alpha) == O.forward_flops(g, d, 16, res, 512, alpha)
        assert abs(wm.iteration_flops(g, d, 16, res, 512, alpha) / 1e9 - w_alg) < 1e-3
        assert abs(wm.iteration_io_elements(g, d, 16, res, 512, alpha) / 1e6 - e) < 1e-2
    # other widths / colours / fade-in stages: the two counts are independent implementations
    for res, alpha, nc in [(32, 0.3, 3), (128, 1.0, 1), (512, 0.5, 1)]:
        a = wm.forward_flops([64, 32, 32, 16, 16, 16], [16, 32, 32, 32, 64, 64], 16, res, 128, alpha, nc)
        b = O.forward_flops([64, 32, 32, 16, 16, 16], [16, 32, 32, 32, 64, 64], 16, res, 128, alpha, nc)
        assert a == b, (res, alpha, a, b)


def test_latent_sampler_pin():
    """seed 7 -> z[0,:3]."""
    torch.manual_seed(7)
    z = O.sample_latent_vec((4, 512))
    assert np.allclose(z[0, :3].numpy(), [-0.03830601, 0.01847874, 0.04198530], atol=1e-7)
    assert np.allclose(z.norm(dim=1).numpy(), 1.0, atol=1e-6)


def test_reduced_precision_error_budget_rules_out_the_1e3_bar():
    """The error budget of the reduced-precision configurations BASELINE.json names, kept reproducible.  Emulating
    on the warmed reduced-width fixture what the product's bf16 mode rounds (bf16 storage of every activation and activation gradient,
    bf16 conv weights, one rounding of a resampled conv input; fp32 arithmetic inside a layer) moves |grad D| by ~1e-2 and the parameter
    gradients by several per cent -- ten times the north star's 1e-3 bar, which is why that mode has its OWN tolerance
    (tests/test_gpu_bf16.py) and is never the headline; fp8 operands (C5) miss the bar by two orders of magnitude and stay declined.
    (tests/lowprec_budget.py prints the full table, all six reduced-width fixtures and the C1 / C2 shapes.)"""
    import lowprec_budget as L
    rows = L.budget("small", *L.small_case("small_res16_warm"))
    assert 3e-3 < rows["bf16"]["|grad D|"] < 5e-2 and rows["bf16"]["D grads (rel L2)"] > 5e-3
    assert 3e-3 < rows["bf16mode"]["|grad D|"] < 1e-1 and 5e-3 < rows["bf16mode"]["D grads (rel L2)"] < 3e-1
    assert rows["fp8"]["|grad D|"] > 1e-2 and rows["fp8"]["D grads (rel L2)"] > 5e-2
    # and the emulation harness itself is neutral: installing no rounding reproduces the fixture's numbers
    restore = L.install("f32")
    restore()
