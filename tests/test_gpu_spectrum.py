"""The radial power spectrum on the GPU: the kernels of csrc/spectrum.hip against the fp64 restatement of tests/spectrum_cases.py
(definition, bound, input families and shapes are described there), the accumulation, `evaluate_spectrum`, and its promise to leave a
run alone.

Measured on the CPU with the emulation in kernel order (tests/test_spectrum_cpu.py prints every figure): the worst emulated
err / bound with C_ACC = 8 is 0.04 per element (the impulse, whose A = 1 leaves the bound no slack from cancellation) and 0.015 per
bin; the kernels are held to err / bound <= 1 for every element and every bin."""
import ctypes
import types

import numpy as np
import pytest
import torch

import spectrum_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64 = np.float64


def host(t):
    return t.detach().cpu().numpy().astype(f64)


def check(M, x, ref, on, names, tag):
    """power per element and radial per bin against the reference; returns (radial, power) of the whole batch"""
    n = x.shape[0]
    radial, power = M.power_spectrum(x.to(DEV), window=on)
    R, C = x.shape[1], x.shape[3]
    assert tuple(radial.shape) == (n, R // 2 + 1) and radial.dtype == torch.float64
    assert tuple(power.shape) == (n, C, R, R // 2 + 1) and power.dtype == torch.float32
    rp = (np.abs(host(power) - ref["power"][:n]) / ref["power_bound"][:n]).max((1, 2, 3))
    rr = (np.abs(host(radial) - ref["radial"][:n]) / ref["radial_bound"][:n]).max(1)
    for name, a, b in zip(names, rp, rr):
        print(f"{tag} {name:10s} worst err/bound: power {a:.4f} radial {b:.4f}")
    assert rp.max() <= 1.0, f"{tag}: power err / bound {rp.max():.3f} ({names[int(rp.argmax())]})"
    assert rr.max() <= 1.0, f"{tag}: radial err / bound {rr.max():.3f} ({names[int(rr.argmax())]})"
    return radial, power


# ---- the kernels against fp64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", (True, False))
@pytest.mark.parametrize("c", S.COLORS)
@pytest.mark.parametrize("size", S.SMALL_SIZES)
def test_power_and_rings_against_fp64(ngan, size, c, on):
    """every family, every element of the half plane and every bin; 1, 3 and all images in one launch (the grids take one image per
    workgroup plane: all 7 span several); with and without the power output; two calls"""
    M = ngan.metrics
    x, ref = S.case(size, c, on)
    tag = f"R={size} C={c} window={int(on)}"
    full, power = check(M, x, ref, on, S.FAMILIES, tag)
    for n in (3, 1):
        r, p = M.power_spectrum(x[:n].to(DEV), window=on)
        assert torch.equal(r, full[:n]) and torch.equal(p, power[:n]), f"{tag} B={n}: an image's values depend on the rest of the batch"
    assert torch.equal(M.radial_spectrum(x.to(DEV), window=on), full), f"{tag}: radial differs without the power output"
    again = M.power_spectrum(x.to(DEV), window=on)
    assert torch.equal(again[0], full) and torch.equal(again[1], power), f"{tag}: two calls differ"


@pytest.mark.parametrize("size", S.SMALL_SIZES + S.LARGE_SIZES)
def test_rings_family_pins_every_bin(ngan, size):
    """window off: every bin k >= 1 holds its own cosine, and its reference exceeds 100 times the bound of its neighbours -- a shift by
    one bin, a wrong Hermitian weight on the columns 0 and R/2 or a sign error in the frequency wrap cannot hide in the bound; the
    corner cosine (k > R/2, dropped) leaves every kept bin below its bound; the impulse gives 1 / R^2 in every bin"""
    M = ngan.metrics
    fams = S.FAMILIES if size in S.SMALL_SIZES else S.LARGE_FAMILIES
    x, ref = S.case(size, 1, False, fams)
    i = fams.index("rings")
    val, bound = ref["radial"][i], ref["radial_bound"][i]
    K = size // 2 + 1
    for k in range(1, K):
        for j in (k - 1, k + 1):
            if 1 <= j < K:
                assert val[k] > 100 * bound[j], (size, k, j, val[k], bound[j])
    got = host(M.radial_spectrum(x.to(DEV), window=False))
    r = np.abs(got - ref["radial"]) / ref["radial_bound"]
    print(f"R={size} rings err/bound {r[i].max():.4f}, impulse {r[fams.index('impulse')].max():.4f}")
    assert r.max() <= 1.0
    j = fams.index("impulse")
    assert (np.abs(got[j] - 1.0 / size ** 2) <= ref["radial_bound"][j]).all() and ref["radial_bound"][j].max() < 3e-5 / size ** 2
    if "corner" in fams:
        j = fams.index("corner")
        assert (got[j] <= ref["radial_bound"][j]).all(), "the corner cosine leaked into a kept bin"


@pytest.mark.parametrize("size", S.LARGE_SIZES)
def test_large_sizes_single_image(ngan, size):
    """B = 1, C = 1: the sizes with 2, 4 and 8 butterflies per thread; impulse and rings without the window, white with it"""
    M = ngan.metrics
    for on, fams in ((False, ("impulse", "rings")), (True, ("white",))):
        x, ref = S.case(size, 1, on, S.LARGE_FAMILIES)
        for f in fams:
            i = S.LARGE_FAMILIES.index(f)
            one = {k: v[i:i + 1] for k, v in ref.items()}
            check(M, x[i:i + 1].contiguous(), one, on, (f,), f"R={size} window={int(on)}")


def test_refusals_return_an_error_and_launch_nothing(ngan):
    lib = ngan._C.lib()
    x = torch.zeros(2, 32, 32, 3, device=DEV)
    out = torch.full((2, 17), -7.0, device=DEV, dtype=torch.float64)
    ws = torch.zeros(1 << 16, device=DEV, dtype=torch.float64)
    stream = torch.cuda.current_stream().cuda_stream

    def call(images=x.data_ptr(), workspace=ws.data_ptr(), R=32, C=1, B=1):
        return lib.ngan_spectrum_radial(images, out.data_ptr(), None, workspace, B, R, C, 1, stream)
    for kw, word in (({"R": 24}, "R=24"), ({"R": 8}, "R=8"), ({"R": 2048}, "R=2048"), ({"C": 2}, "C=2"), ({"B": 0}, "B=0"),
                     ({"images": x.data_ptr() + 4}, "16-byte"), ({"workspace": None}, "workspace"), ({"images": None}, "null")):
        assert call(**kw) != 0, kw
        assert word in lib.ngan_last_error().decode(), (kw, lib.ngan_last_error())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((ws == 0).all()), "a refused call wrote something"
    assert lib.ngan_spectrum_workspace_bytes(1, 24, 1) == 0 and lib.ngan_spectrum_workspace_bytes(1, 32, 2) == 0
    assert lib.ngan_spectrum_workspace_bytes(2, 32, 3) == 2 * 3 * 17 * 32 * 8 + 2 * 3 * 2 * 17 * 8
    buf = (ctypes.c_float * 32)()
    assert lib.ngan_spectrum_window(ctypes.cast(buf, ctypes.c_void_p), 24) != 0 and "R=24" in lib.ngan_last_error().decode()
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[0] != -7.0).all()) and bool((out[1] == -7.0).all())


# ---- accumulation and the metric ---------------------------------------------------------------------------------------------------------
def test_accumulation_over_uneven_minibatches(ngan):
    M = ngan.metrics
    real, fake = S.white_set(32, 8, 1, c=3), S.upsampled_set(32, 8, 2, c=3)
    once = M.Spectrum(32, n_colors=3, device=DEV)
    once.feed("real", real)
    once.feed("fake", fake)
    m = M.Spectrum(32, n_colors=3, device=DEV)
    for lo, hi in ((0, 1), (1, 4), (4, 8)):
        m.feed("real", real[lo:hi].permute(0, 3, 1, 2).contiguous())                  # as (B, C, R, R)
        m.feed("fake", fake[lo:hi])
    a, b = once.result(), m.result()
    for key in ("real", "fake", "real_sem", "fake_sem", "ratio_db"):
        np.testing.assert_allclose(b[key], a[key], rtol=1e-12, atol=0)
    ref = S.metric_ref(S.radial_ref(real.numpy()), S.radial_ref(fake.numpy()))
    assert b["images"] == 8 and b["k"] == list(range(17)) and b["skipped_bins"] == 0
    np.testing.assert_allclose(b["real"], ref["real"], rtol=1e-5)
    np.testing.assert_allclose(b["fake"], ref["fake"], rtol=1e-5)
    np.testing.assert_allclose(b["ratio_db"], ref["ratio_db"], atol=1e-4)
    assert abs(b["distance_db"] - ref["distance_db"]) < 1e-4 and abs(b["high_db"] - ref["high_db"]) < 1e-4
    sem = host(M.radial_spectrum(real.to(DEV))).std(0, ddof=1) / 8 ** 0.5
    np.testing.assert_allclose(b["real_sem"], sem, rtol=1e-6)
    text = M.format_spectrum(b)
    assert "distance_db" in text and "high_db" in text and len(text.splitlines()) == 2 + 5 + 1      # k = 1, 2, 4, 8, 16
    m.feed("real", real[:1])
    with pytest.raises(ValueError):
        m.result()


def test_upsampled_samples_lack_the_top_octave(ngan):
    """through the product path: 32 bilinearly upsampled fields against 32 white ones at R = 32"""
    M = ngan.metrics
    m = M.Spectrum(32, device=DEV)
    m.feed("real", S.white_set(32, 32, 3))
    m.feed("fake", S.upsampled_set(32, 32, 4))
    res = m.result()
    print(f"high_db {res['high_db']:.2f} distance_db {res['distance_db']:.2f}")
    assert res["high_db"] <= -10.0
    same = M.Spectrum(32, device=DEV)
    same.feed("real", S.white_set(32, 16, 5))
    same.feed("fake", S.white_set(32, 16, 6))
    res = same.result()
    assert abs(res["high_db"]) <= 1.0 and res["distance_db"] <= 1.0
    flat = M.Spectrum(16, window=False, device=DEV)                                       # constant images, no window: DC alone
    flat.feed("real", torch.full((2, 16, 16, 1), -1.0))
    flat.feed("fake", torch.full((2, 16, 16, 1), 0.5))
    res = flat.result()
    assert res["ratio_db"][0] is not None and all(v is None for v in res["ratio_db"][1:])
    assert res["skipped_bins"] == 8 and res["distance_db"] is None and res["high_db"] is None
    assert "left out" in M.format_spectrum(res)


# ---- evaluate_spectrum -------------------------------------------------------------------------------------------------------------------
def small_nets(ngan, widths=(32, 16)):
    G = ngan.models.Generator_PG(list(widths), image_size_init=8, latent_dim=32).to(DEV)
    D = ngan.models.Discriminator_PG(list(widths)[::-1], image_size_init=8).to(DEV)
    return G, D


def small_dataset(ngan, size=16):
    g = torch.Generator().manual_seed(9)
    return ngan.data.NeuronDataset(torch.rand(8, 1, size, size, generator=g), augmentations=True, im_translation=0.05, device=DEV, seed=3)


def test_evaluate_spectrum_is_seeded_and_leaves_no_trace(ngan):
    M = ngan.metrics
    torch.manual_seed(7)
    G, _ = small_nets(ngan, (32, 16, 16))
    G.set_resolution(32, 1.0)
    data = small_dataset(ngan, 32)
    data.set_image_size(8)
    host_rng, device_rng, aug = torch.get_rng_state(), torch.cuda.get_rng_state(DEV), data.gen.get_state()
    own = data.gen
    kw = dict(n_images=7, batch_size=3, seed=2)
    first, metric = M.evaluate_spectrum(G, data, return_metric=True, **kw)
    assert first["images"] == 7 and first["k"] == list(range(17)) and np.isfinite(first["distance_db"]) and np.isfinite(first["high_db"])
    assert torch.equal(torch.get_rng_state(), host_rng), "torch's global generator was consumed"
    assert torch.equal(torch.cuda.get_rng_state(DEV), device_rng), "the device generator was consumed"
    assert data.gen is own and torch.equal(data.gen.get_state(), aug) and data.image_size == 8, "the data set's stream or stage moved"
    assert M.evaluate_spectrum(G, data, **kw) == first                            # seeded: the same numbers again
    assert M.evaluate_spectrum(G, None, real_from=metric, **kw) == first          # the data's side taken over, the data set untouched
    other = M.evaluate_spectrum(G, data, **{**kw, "seed": 3})
    assert other["fake"] != first["fake"] and other["real"] != first["real"]
    # the real side by hand: the same augmented batches
    data.gen = torch.Generator(device="cpu").manual_seed(2 + 1)
    data.set_image_size(32)
    vals = [M.radial_spectrum(M.channels_last(data.batch([(i + j) % len(data) for j in range(min(3, 7 - i))]))) for i in range(0, 7, 3)]
    data.gen = own
    data.set_image_size(8)
    np.testing.assert_allclose(first["real"], host(torch.cat(vals)).mean(0), rtol=1e-12)
    G8, _ = small_nets(ngan)                                                      # a stage below 16 x 16: said, not raised
    below = M.evaluate_spectrum(G8, data, **kw)
    assert below["k"] == [] and below["high_db"] is None and "16 x 16" in below["note"]


# ---- no side effects ---------------------------------------------------------------------------------------------------------------------
def same(x, y):
    if torch.is_tensor(x):
        return torch.is_tensor(y) and torch.equal(x, y)
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return isinstance(y, (list, tuple)) and len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    return x == y


def two_epochs(ngan, tmp_path, tag, spectrum_period, ema_beta):
    cfg = types.SimpleNamespace(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[1], N_epochs=2,
                                alpha_step=0.5, learning_rate=2e-3, checkpointing_period=1, ID=tag, spectrum_period=spectrum_period,
                                spectrum_images=6, spectrum_seed=1)
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    G, D = small_nets(ngan)
    data = small_dataset(ngan)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, alpha_step=cfg.alpha_step, device_latents=True, ema_beta=ema_beta)
    f = str(tmp_path / f"GenDisc_{tag}.pth")
    ck = ngan.utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=torch.device(DEV), trainer=tr,
                                 extra_checkpoint_period=1e3)
    lines = []
    series = ngan.train.pggan_train(tr, data, cfg, checkpoint=ck, epoch_final=3, log=lambda *a: lines.append(" ".join(map(str, a))))
    torch.cuda.synchronize()
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(DEV), data.gen.get_state())
    return series, ngan.utils.load_checkpoint_dict(f), lines, tr, f, rng


@pytest.mark.parametrize("ema_beta", (0.0, 0.9))
def test_a_scored_run_trains_bit_identically(ngan, tmp_path, ema_beta, capsys):
    """two epochs at 16 x 16 (grown at epoch 1, fading in; captured graphs replayed) with a checkpoint and a score after each"""
    plain, saved0, lines0, _, _, rng0 = two_epochs(ngan, tmp_path, "s000", 0, ema_beta)
    scored, saved1, lines1, tr, f, rng1 = two_epochs(ngan, tmp_path, "s001", 1, ema_beta)
    assert tr.G.image_size == 16 and tr.has_graph((4, 1, 16, 16)), "the run did not train through a captured graph"
    assert plain == scored, "the monitor series changed when the metric was turned on"
    for key in ("Generator_state", "Discriminator_state", "optimizer_state") + (("Generator_ema_state",) if ema_beta else ()):
        assert key in saved0 and same(saved0[key], saved1[key]), f"{key} changed when the metric was turned on"
    for name, x, y in zip(("torch's CPU generator", "the device generator", "the data set's generator"), rng0, rng1):
        assert torch.equal(x, y), f"{name} ended in another state"
    assert "SPECTRUM" not in saved0 and not any("spectrum" in l for l in lines0)
    entries = saved1["SPECTRUM"]
    assert [e["epoch"] for e in entries] == [1, 2] and "SWD" not in saved1 and "MSSSIM" not in saved1
    keys = {"epoch", "image_size", "images", "k", "real", "fake", "ratio_db", "distance_db", "high_db"}
    assert all(set(e) == keys | ({"distance_db_ema", "high_db_ema"} if ema_beta else set()) for e in entries)
    assert all(e["image_size"] == 16 and e["images"] == 6 and e["k"] == list(range(9)) and len(e["ratio_db"]) == 9 for e in entries)
    assert entries[0]["real"] == entries[1]["real"] and entries[0]["fake"] != entries[1]["fake"]     # the same seed, another generator
    if ema_beta:
        assert all(np.isfinite(e["high_db_ema"]) and e["high_db_ema"] != e["high_db"] for e in entries)
    scored_lines = [l for l in lines1 if "spectrum" in l]
    assert len(scored_lines) == 2 and all(("averaged generator" in l) == bool(ema_beta) and "top octave" in l for l in scored_lines)
    # the eval tool prints the table for the checkpoint, and the averaged generator's after it when asked
    images = str(tmp_path / "images.pt")
    torch.save(torch.rand(8, 1, 16, 16, generator=torch.Generator().manual_seed(9)) * 2 - 1, images)
    capsys.readouterr()
    assert ngan.eval.main(["-weights", f, "--spectrum", "8", "--images", images] + (["--ema"] if ema_beta else [])) == 0
    out = capsys.readouterr().out
    assert out.count("Radial power spectrum") == (2 if ema_beta else 1) and ("averaged generator" in out) == bool(ema_beta)
    assert out.count("(8 images per side)") == out.count("distance_db") == out.count("high_db") == (2 if ema_beta else 1)
