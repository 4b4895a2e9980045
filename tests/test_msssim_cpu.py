"""MS-SSIM between pairs without a GPU: the restatement of tests/msssim_cases.py against scipy and the textbook single formula, its
identities, the fp32 emulation of the kernel against it (every emulated err / bound is printed and at most 0.5: this is where C_ACC
is settled, before a kernel is looked at), host-side validation of the new entry points, the configuration names and flags, and the
checkpoint list.  The kernels themselves are tested on the GPU (tests/test_gpu_msssim.py)."""
import ctypes

import numpy as np
import pytest
import torch

import msssim_cases as S

f64 = np.float64


def test_restatement_agrees_with_scipy_and_the_single_formula():
    signal = pytest.importorskip("scipy.signal")
    a, b = S.pairs(32, 3)
    pick = [S.FAMILIES.index(f) for f in ("corr 0.3", "negated", "neuron", "corner")]
    g = S.window()
    w2 = np.outer(g, g)
    c1, c2 = S.constants()
    f = lambda x: signal.correlate2d(x, w2, mode="valid")   # noqa: E731
    maps = S.scale_maps(a[pick], b[pick])
    for i, p in enumerate(pick):
        for ch in range(3):
            x, y = a[p, :, :, ch].double().numpy(), b[p, :, :, ch].double().numpy()
            mx, my = f(x), f(y)
            sx, sy, sxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
            ssim = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sx + sy + c2))      # the textbook formula
            cs = (2 * sxy + c2) / (sx + sy + c2)
            assert ssim.shape == (22, 22)
            assert np.abs(maps["ssim"][0][i, :, :, ch].numpy() - ssim).max() < 1e-12
            assert np.abs(maps["cs"][0][i, :, :, ch].numpy() - cs).max() < 1e-12
    # the window: 11 positive taps, symmetric, summing to 1 within fp32 rounding, each an fp32 number
    assert g.shape == (11,) and (g > 0).all() and np.array_equal(g, g[::-1]) and abs(g.sum() - 1) < 11 * 2.0 ** -25
    assert np.array_equal(g.astype(np.float32).astype(f64), g) and abs(g[5] / g[4] - np.exp(1 / 4.5)) < 1e-6


def test_identities_and_scale_counts():
    assert [S.n_scales(r) for r in (4, 8, 16, 32, 64, 128, 256, 512, 1024)] == [0, 0, 1, 2, 3, 4, 5, 5, 5]
    for s in range(1, 6):
        w = S.weights(s)
        assert len(w) == s and abs(w.sum() - 1) < 1e-15 and np.allclose(w / w[0], np.array(S.WEIGHTS[:s]) / S.WEIGHTS[0])
    a, b = S.pairs(64, 3)
    ab, _ = S.msssim_ref(a, b)
    ba, _ = S.msssim_ref(b, a)
    assert np.abs(ab - ba).max() < 1e-14, "not symmetric"
    aa, _ = S.msssim_ref(a, a)
    assert np.abs(aa - 1).max() < 1e-12, "msssim(a, a) is not 1"
    for flip in ((1,), (2,), (1, 2)):
        fl, _ = S.msssim_ref(a.flip(flip), b.flip(flip))
        assert np.abs(fl - ab).max() < 1e-12, f"not invariant under the flip {flip} of both images"
    # the families do what they are there for: equal pairs give 1, the negated pair reaches the clamp, the rest lie strictly between
    fam = dict(zip(S.FAMILIES, ab))
    assert all(abs(fam[k] - 1) < 1e-12 for k in ("same", "neuron same", "constant equal"))
    assert fam["negated"] == 0.0 and S.scale_ref(a, b)["cs"][0][S.FAMILIES.index("negated")] < 0
    assert all(0 < fam[k] < 1 for k in ("corr 0.9", "corr 0.3", "neuron vs flat", "corner")), fam
    assert fam["corr 0.9"] > fam["corr 0.3"]
    # most windows of a neuron-like image are flat: the cancellation case is really in the batch
    arb = a[S.FAMILIES.index("neuron")].double()[None]
    var = S.filt(arb * arb) - S.filt(arb) ** 2
    assert float((var.abs() < 1e-6).double().mean()) > 0.2       # (not 0: the rounded taps sum to 1 within 3e-9 only)


@pytest.mark.parametrize("c", S.COLORS)
@pytest.mark.parametrize("size", S.SCALE_SIZES)
def test_scale_emulation_within_half_the_bound(size, c):
    a, b, ref = S.scale_case(size, c)
    emu = S.scale_emu(a.numpy(), b.numpy())
    for name in ("cs", "ssim"):
        val, bound = ref[name]
        r = np.abs(emu[name] - val) / bound
        for fam, ri, v in zip(S.FAMILIES, r, val):
            print(f"scale {size} C={c} {name:4s} {fam:20s} ref {v:+.6f} err/bound {ri:.4f}")
        assert r.shape == (len(S.FAMILIES),) and r.max() <= 0.5, f"{name} {size} C={c}: {r.max():.3f} ({S.FAMILIES[int(r.argmax())]})"


@pytest.mark.parametrize("c", S.COLORS)
@pytest.mark.parametrize("size", S.METRIC_SIZES)
def test_metric_emulation_within_half_the_bound(size, c):
    a, b, ref, bound = S.metric_case(size, c)
    emu = S.msssim_emu(a.numpy(), b.numpy())
    r = np.abs(emu - ref) / (bound + 1e-300)
    for i in range(len(ref)):
        print(f"metric {size} C={c} pair {i}: ref {ref[i]:.6f} emu {emu[i]:.6f} bound {bound[i]:.2e} err/bound {r[i]:.4f}")
    assert emu[0] == 1.0 and (emu[ref == 0.0] == 0.0).all()  # equal images: exactly 1; a clamped reference: exactly the clamp
    assert r.max() <= 0.5, f"metric {size} C={c}: {r.max():.3f}"


def test_pool_emulation_is_one_rounding():
    a, _ = S.pairs(32, 3)
    ref = S.pool2_ref(a.double()).numpy()
    assert (np.abs(S.pool2_emu(a.numpy()).astype(f64) - ref) <= 2.0 ** -24 * np.abs(ref)).all()


def test_entry_points_are_bound_and_validate_on_the_host(ngan):
    lib = ngan._C.lib()
    one = ctypes.c_void_p(64)            # any non-null address: every check below comes before the launch
    N = None
    err = lambda: lib.ngan_last_error()  # noqa: E731
    assert {"ngan_msssim_scale", "ngan_msssim_pool2", "ngan_msssim_window", "ngan_msssim_workspace_bytes"} <= set(ngan._C.exported_symbols())
    for args in ((N, one, one, one), (one, N, one, one), (one, one, N, one), (one, one, one, N)):
        assert lib.ngan_msssim_scale(*args, 1, 16, 1, 2.0, None) < 0 and b"null" in err()
        assert lib.ngan_msssim_pool2(*args, 1, 16, 1, None) < 0 and b"null" in err()
    for c in (0, 2, 4):
        assert lib.ngan_msssim_scale(one, one, one, one, 1, 16, c, 2.0, None) < 0 and b"C=" in err()
        assert lib.ngan_msssim_pool2(one, one, one, one, 1, 16, c, None) < 0 and b"C=" in err()
    for h in (8, 11, 12, 24, 48, 0, -16):                    # too small for the window, or not a power of two
        assert lib.ngan_msssim_scale(one, one, one, one, 1, h, 1, 2.0, None) < 0 and b"H=" in err()
        assert lib.ngan_msssim_workspace_bytes(1, h) == 0
    for h in (3, 12, 0):
        assert lib.ngan_msssim_pool2(one, one, one, one, 1, h, 1, None) < 0 and b"H=" in err()
    for p in (0, -1, 65536):
        assert lib.ngan_msssim_scale(one, one, one, one, p, 16, 1, 2.0, None) < 0 and b"P=" in err()
    for rng in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.ngan_msssim_scale(one, one, one, one, 1, 16, 1, rng, None) < 0 and b"data_range" in err()
    assert lib.ngan_msssim_window(N) < 0 and b"null" in err()
    # one pair of doubles per 32 x 32 tile of the valid map and pair
    assert lib.ngan_msssim_workspace_bytes(1, 16) == 16 and lib.ngan_msssim_workspace_bytes(3, 64) == 3 * 4 * 16
    assert lib.ngan_msssim_workspace_bytes(2, 512) == 2 * 256 * 16 and lib.ngan_msssim_workspace_bytes(0, 16) == 0
    # the kernel's window is the restatement's, bit for bit
    assert np.array_equal(ngan.metrics.msssim_window().double().numpy(), S.window())
    M = ngan.metrics
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.msssim_scale(torch.zeros(1, 16, 16, 1), torch.zeros(1, 16, 16, 1))
    with pytest.raises(ValueError):
        M.msssim_scale(torch.zeros(1, 16, 16, 2), torch.zeros(1, 16, 16, 2))
    with pytest.raises(ValueError):
        M.msssim(torch.zeros(1, 16, 16, 1), torch.zeros(2, 16, 16, 1))
    with pytest.raises(ValueError, match="below 16 x 16"):
        M.msssim(torch.zeros(1, 8, 8, 1), torch.zeros(1, 8, 8, 1))


def test_metric_object_on_the_host(ngan):
    M = ngan.metrics
    assert M.DATA_RANGE == 2.0 and [M.msssim_scales(r) for r in (8, 16, 32, 64, 128, 256, 512)] == [0, 1, 2, 3, 4, 5, 5]
    for s in range(1, 6):
        assert np.allclose(M.msssim_weights(s), S.weights(s), rtol=0, atol=1e-16) and abs(sum(M.msssim_weights(s)) - 1) < 1e-15
    m = M.MSSSIM(64, n_colors=3, device="cpu")
    assert m.scales == 3 and m.weights == M.msssim_weights(3) and m.data_range == 2.0
    with pytest.raises(ValueError, match="no generated pair"):
        m.result()
    with pytest.raises(ValueError):
        m.feed("fake", torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError):
        m.feed("other", torch.zeros(2, 3, 64, 64), torch.zeros(2, 3, 64, 64))
    for bad in (dict(image_size=48), dict(image_size=64, n_colors=2), dict(image_size=64, data_range=0.0)):
        with pytest.raises(ValueError):
            M.MSSSIM(**bad)
    # 8 x 8: no scale -- said, not raised, and no number
    small = M.MSSSIM(8, device="cpu")
    small.feed("fake", torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8))
    res = small.result()
    assert res["scales"] == 0 and res["fake"] is None and res["real"] is None and res["pairs"] == 0 and "16 x 16" in res["note"]
    assert "16 x 16" in M.format_msssim(res) and "16 x 16" in M.format_table(res)
    table = M.format_msssim({"scales": 2, "weights": [0.1, 0.9], "fake": 0.25, "fake_sem": 0.01, "real": 0.125, "real_sem": None,
                             "pairs": 7})
    assert "2 scales, 7 pairs" in table and "0.25000 +- 0.01000" in table and "0.12500" in table and len(table.splitlines()) == 3


def test_flags_and_configuration_names(ngan):
    cfg, train = ngan.config, ngan.train
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    try:
        assert (cfg.configs_name["msssim_period"], cfg.configs_name["msssim_pairs"], cfg.configs_name["msssim_seed"]) == (0, 10000, 0)
        none = train.cli_overrides([], train.build_arg_parser().parse_args([]), cfg.configs_name)
        assert not any(k.startswith("msssim") for k in none)
        argv = ["--msssim_period", "2", "--msssim_pairs", "256", "--msssim_seed", "7"]
        over = train.cli_overrides(argv, train.build_arg_parser().parse_args(argv), cfg.configs_name)
        assert over == {"msssim_period": 2, "msssim_pairs": 256, "msssim_seed": 7}
        cfg.set_configs(**over)
        cfg.validate_configs()
        assert (cfg.msssim_period, cfg.msssim_pairs, cfg.msssim_seed) == (2, 256, 7)
        for name, bad in (("msssim_period", -1), ("msssim_pairs", 0), ("msssim_seed", -3), ("msssim_period", 1.5)):
            cfg.set_configs(**{**over, name: bad})
            with pytest.raises(ValueError, match=name):
                cfg.validate_configs()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    # the rank launcher hands the training flags through untouched
    plan = ngan.launch.launch_plan(2, ["--pggan", "--msssim_period", "2", "--msssim_pairs", "256", "--gpus", "2"], port=29500, environ={})
    assert all(" ".join(["--msssim_period", "2", "--msssim_pairs", "256"]) in " ".join(argv_i) for argv_i, _ in plan)
    p = ngan.eval.build_arg_parser()
    d = p.parse_args([])
    assert (d.msssim, d.msssim_seed, d.swd) == (None, 0, None)
    assert p.parse_args(["--msssim"]).msssim == 10000
    o = p.parse_args(["--msssim", "512", "--ema", "--dataset_dir", "d", "--swd", "64"])
    assert (o.msssim, o.ema, o.dataset_dir, o.swd) == (512, True, "d", 64)


def nets(ngan, seed):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([16, 16, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 16, 16], image_size_init=4)
    return G, D


def test_checkpoint_list_round_trip(ngan, tmp_path):
    utils = ngan.utils
    G, D = nets(ngan, 1)
    f = str(tmp_path / "GenDisc_m.pth")
    ck = utils.Checkpointer(G, D, 1e-4, f, N_epochs=10, verbose=False)
    ck.save_state(1)
    assert "MSSSIM" not in utils.load_checkpoint_dict(f)              # nothing scored: the file of a build without the feature
    entries = [{"epoch": 2, "image_size": 16, "scales": 1, "fake": 0.4375, "fake_ema": None, "real": 0.25, "pairs": 100},
               {"epoch": 4, "image_size": 32, "scales": 2, "fake": 0.5, "fake_ema": 0.53125, "real": None, "pairs": 100}]
    ck.MSSSIM.extend(entries)
    ck.save_state(4)
    saved = utils.load_checkpoint_dict(f)                              # the weights-only unpickler accepts the list
    assert saved["MSSSIM"] == entries and "SWD" not in saved
    G2, D2 = nets(ngan, 2)
    ck2 = utils.Checkpointer(G2, D2, 1e-4, f, N_epochs=10, verbose=False)
    ck2.load_state()
    assert ck2.MSSSIM == entries and ck2.SWD == [] and ck2.epoch == 4
    ck2.MSSSIM.append({"epoch": 6, "image_size": 32, "scales": 2, "fake": 0.75, "fake_ema": None, "real": 0.5, "pairs": 10})
    ck2.save_state(6)                                                  # a resumed run continues the list
    assert [e["epoch"] for e in utils.load_checkpoint_dict(f)["MSSSIM"]] == [2, 4, 6]
    f0 = str(tmp_path / "GenDisc_0.pth")
    utils.Checkpointer(G, D, 1e-4, f0, N_epochs=10, verbose=False).save_state(3)
    ck3 = utils.Checkpointer(G2, D2, 1e-4, f0, N_epochs=10, verbose=False)
    ck3.load_state()
    assert ck3.MSSSIM == [] and ck3.epoch == 3
