"""The radial power spectrum without a GPU: the restatement of tests/spectrum_cases.py against brute force and Parseval, the fp32
emulation of the kernels against it (every emulated err / bound is printed and at most 0.5: this is where C_ACC is settled, before a
kernel is looked at), what the metric says on known sets, host-side validation of the new entry points, the bookkeeping of
`Spectrum.result()`, the configuration names and flags, and the checkpoint list.  The kernels themselves are tested on the GPU
(tests/test_gpu_spectrum.py)."""
import ctypes

import numpy as np
import pytest
import torch

import spectrum_cases as S

f64 = np.float64
ALL_SIZES = S.SMALL_SIZES + S.LARGE_SIZES


@pytest.mark.parametrize("size", ALL_SIZES)
def test_ring_rule_and_counts_against_brute_force(ngan, size):
    f = np.arange(-size // 2, size // 2, dtype=np.int64)
    d = f[:, None] ** 2 + f[None, :] ** 2
    brute = np.floor(np.sqrt(d.astype(f64)) + 0.5).astype(np.int64)          # exact: sqrt(d) + 1/2 is never within an ulp of an integer
    assert np.array_equal(S.ring_of(d), brute)                              # for d < 2^20 unless it is one, and then the rule agrees
    counts = np.bincount(brute.ravel())
    assert np.array_equal(S.ring_counts(size), counts[:size // 2 + 1])
    assert counts[:size // 2 + 1].sum() + counts[size // 2 + 1:].sum() == size * size and counts[size // 2 + 1:].sum() > 0
    assert np.array_equal(ngan.metrics.spectrum_ring_counts(size).numpy(), S.ring_counts(size))       # the library's host function
    assert np.array_equal(ngan.metrics.spectrum_window(size).double().numpy(), S.window(size))        # its taps, bit for bit
    h = S.window(size)
    assert h[0] == 0.0 and h[size // 2] == 1.0 and np.allclose(h[1:], h[1:][::-1], rtol=0, atol=2.0 ** -24)
    assert abs(S.norm(size) / S.norm_separable(size) - 1) < 2.0 ** -24 and S.norm(size, False) == S.norm_separable(size, False) == size ** 2


@pytest.mark.parametrize("on", (True, False))
@pytest.mark.parametrize("size", (16, 64))
def test_parseval(size, on):
    x = S.images(size, 3)
    ref = S.spectrum_ref(x.numpy(), on)
    idx, n = S.ring_index(size), S.ring_counts(size)
    wx = S.windowed(x.numpy(), on).astype(f64)
    energy = (wx ** 2).sum((1, 2, 3)) * size ** 2 / S.norm(size, on)
    dropped = ref["full"][:, :, idx > size // 2].sum((1, 2))
    kept = 3 * (ref["radial"] * n).sum(1)
    assert np.allclose(kept + dropped, energy, rtol=1e-12, atol=1e-9)
    white = S.white_set(64, 64, 0).numpy()                                  # white noise of variance 1/3: that level in every bin
    level = S.radial_ref(white, on).mean(0)
    assert np.abs(level[1:] / (1.0 / 3.0) - 1).max() < 0.3 and abs(level[8:].mean() * 3 - 1) < 0.02


@pytest.mark.parametrize("on", (True, False))
@pytest.mark.parametrize("c", S.COLORS)
@pytest.mark.parametrize("size", S.SMALL_SIZES)
def test_emulation_within_half_the_bound(size, c, on):
    x, ref = S.case(size, c, on)
    emu = S.spectrum_emu(x.numpy(), on)
    rp = (np.abs(emu["power"].astype(f64) - ref["power"]) / ref["power_bound"]).max((1, 2, 3))
    rr = (np.abs(emu["radial"] - ref["radial"]) / ref["radial_bound"]).max(1)
    for fam, a, b in zip(S.FAMILIES, rp, rr):
        print(f"R={size} C={c} window={int(on)} {fam:10s} emulated err/bound: power {a:.4f} radial {b:.4f}")
    assert max(rp.max(), rr.max()) <= 0.5, (size, c, on, rp, rr)


@pytest.mark.parametrize("size", S.LARGE_SIZES)
def test_emulation_within_half_the_bound_large(size):
    for on in (False, True):
        x, ref = S.case(size, 1, on, S.LARGE_FAMILIES)
        emu = S.spectrum_emu(x.numpy(), on)
        rp = (np.abs(emu["power"].astype(f64) - ref["power"]) / ref["power_bound"]).max((1, 2, 3))
        rr = (np.abs(emu["radial"] - ref["radial"]) / ref["radial_bound"]).max(1)
        for fam, a, b in zip(S.LARGE_FAMILIES, rp, rr):
            print(f"R={size} C=1 window={int(on)} {fam:10s} emulated err/bound: power {a:.4f} radial {b:.4f}")
        assert max(rp.max(), rr.max()) <= 0.5, (size, on, rp, rr)


@pytest.mark.parametrize("size", ALL_SIZES)
def test_families_do_what_they_are_there_for(size):
    fams = S.FAMILIES if size in S.SMALL_SIZES else S.LARGE_FAMILIES
    x, ref = S.case(size, 1, False, fams)
    K = size // 2 + 1
    freqs = S.ring_frequencies(size)
    assert sorted({k for k, _, _, _ in freqs}) == list(range(1, K))
    assert any(u == 0 for _, u, _, _ in freqs) and any(v == 0 for _, _, v, _ in freqs)
    assert any(u == -size // 2 for _, u, _, _ in freqs) and any(v == -size // 2 for _, _, v, _ in freqs)
    assert any(u != 0 and v != 0 and abs(u) != abs(v) for _, u, v, _ in freqs)
    val, bound = ref["radial"][fams.index("rings")], ref["radial_bound"][fams.index("rings")]
    n = S.ring_counts(size)
    for k in range(1, K - 1):                                               # one cosine: a_k^2 R^4 / (2 n_k norm), norm = R^2; the image
        assert abs(val[k] / ((1 + k / size) ** 2 * size ** 2 / (2 * n[k])) - 1) < 1e-6         # is rounded to fp32
    for k in range(1, K):
        assert all(val[k] > 100 * bound[j] for j in (k - 1, k + 1) if 1 <= j < K), k
    imp = ref["radial"][fams.index("impulse")]
    assert np.abs(imp * size ** 2 - 1).max() < 1e-12
    if "corner" in fams:
        assert (ref["radial"][fams.index("corner")] < 1e-10).all()            # (what is there is the image's fp32 rounding)
        assert ref["full"][fams.index("corner")].sum() > 0.4 * size ** 2    # all of it in the dropped corners
        const = ref["radial"][fams.index("constant")]
        assert const[0] == size ** 2 and (const[1:] == 0).all()             # no window: DC alone
        hann = S.case(size, 1, True)[1]["radial"][S.FAMILIES.index("constant")]
        assert hann[0] > 0 and hann[1] > 0 and (hann[3:] < 1e-12 * hann[0]).all()      # the Hann window leaks into bins 1 and 2 only


def test_metric_on_known_sets():
    up, wh = S.radial_ref(S.upsampled_set(32, 32, 4).numpy()), S.radial_ref(S.white_set(32, 32, 3).numpy())
    m = S.metric_ref(wh, up)
    print(f"upsampled against white, R = 32, window on: high_db {m['high_db']:.2f}, distance_db {m['distance_db']:.2f}")
    assert m["high_db"] <= -10.0
    m = S.metric_ref(S.radial_ref(S.white_set(32, 16, 5).numpy()), S.radial_ref(S.white_set(32, 16, 6).numpy()))
    print(f"two white sets of 16: high_db {m['high_db']:+.3f}, distance_db {m['distance_db']:.3f}")
    assert abs(m["high_db"]) <= 1.0 and m["distance_db"] <= 1.0


def test_entry_points_are_bound_and_validate_on_the_host(ngan):
    lib = ngan._C.lib()
    one = ctypes.c_void_p(64)            # any aligned non-null address: every check below comes before the launch
    odd = ctypes.c_void_p(68)
    N = None
    err = lambda: lib.ngan_last_error()  # noqa: E731
    assert {"ngan_spectrum_window", "ngan_spectrum_ring_counts", "ngan_spectrum_workspace_bytes", "ngan_spectrum_radial"} \
        <= set(ngan._C.exported_symbols())
    assert lib.ngan_spectrum_radial(N, one, N, one, 1, 16, 1, 1, None) < 0 and b"null" in err()
    assert lib.ngan_spectrum_radial(one, N, N, one, 1, 16, 1, 1, None) < 0 and b"null" in err()
    assert lib.ngan_spectrum_radial(one, one, N, N, 1, 16, 1, 1, None) < 0 and b"workspace" in err()
    for bad in ((odd, one, N, one), (one, one, odd, one), (one, one, N, odd), (one, ctypes.c_void_p(66), N, one)):
        assert lib.ngan_spectrum_radial(*bad, 1, 16, 1, 1, None) < 0 and b"boundary" in err()
    for r in (8, 24, 2048, 0, -16):
        assert lib.ngan_spectrum_radial(one, one, N, one, 1, r, 1, 1, None) < 0 and b"R=" in err()
        assert lib.ngan_spectrum_workspace_bytes(1, r, 1) == 0
        assert lib.ngan_spectrum_window(one, r) < 0 and lib.ngan_spectrum_ring_counts(one, r) < 0
    for c in (0, 2, 4):
        assert lib.ngan_spectrum_radial(one, one, N, one, 1, 16, c, 1, None) < 0 and b"C=" in err()
    for b in (0, -1, 65536):
        assert lib.ngan_spectrum_radial(one, one, N, one, b, 16, 1, 1, None) < 0 and b"B=" in err()
    assert lib.ngan_spectrum_window(N, 16) < 0 and b"null" in err() and lib.ngan_spectrum_ring_counts(N, 16) < 0
    # the half spectrum (B C (R/2+1) R complex values) and one double per bin, column group, channel and image
    assert lib.ngan_spectrum_workspace_bytes(1, 16, 1) == 9 * 16 * 8 + 2 * 9 * 8
    assert lib.ngan_spectrum_workspace_bytes(64, 512, 1) == 64 * (257 * 512 * 8 + 33 * 257 * 8)
    M = ngan.metrics
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.radial_spectrum(torch.zeros(1, 16, 16, 1))
    with pytest.raises(ValueError):
        M.radial_spectrum(torch.zeros(1, 16, 16, 2))
    with pytest.raises(ValueError):
        M.power_spectrum(torch.zeros(1, 16, 32, 1))


def test_metric_object_on_the_host(ngan):
    M = ngan.metrics
    m = M.Spectrum(64, n_colors=3, device="cpu")
    assert m.bins == 33 and m.window is True
    with pytest.raises(ValueError, match="feed both sets equally"):
        m.result()
    with pytest.raises(ValueError):
        m.feed("fake", torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError):
        m.feed("other", torch.zeros(2, 3, 64, 64))
    for bad in (dict(image_size=48), dict(image_size=64, n_colors=2), dict(image_size=2048)):
        with pytest.raises(ValueError):
            M.Spectrum(**bad)
    small = M.Spectrum(8, device="cpu")                                      # 8 x 8: no ring -- said, not raised, and no number
    small.feed("real", torch.zeros(2, 1, 8, 8))
    res = small.result()
    assert res["k"] == [] and res["distance_db"] is None and res["high_db"] is None and res["images"] == 0 and "16 x 16" in res["note"]
    assert "16 x 16" in M.format_spectrum(res)
    # the bookkeeping of result(), on accumulators filled by hand: R = 16, two images per side
    m = M.Spectrum(16, device="cpu")
    real = torch.tensor([[4.0, 2, 2, 2, 1, 1, 1, 0, 1], [4.0, 2, 2, 2, 3, 1, 1, 0, 1]], dtype=torch.float64)
    fake = real * torch.tensor([1.0, 1, 10, 0.1, 1, 0.01, 0.01, 1, 0], dtype=torch.float64)
    for which, s in (("real", real), ("fake", fake)):
        m.sums[which], m.count[which] = torch.stack([s.sum(0), s.square().sum(0)]), 2
    res = m.result()
    assert res["k"] == list(range(9)) and res["images"] == 2 and res["real"] == [4, 2, 2, 2, 2, 1, 1, 0, 1]
    assert res["ratio_db"][7] is None and res["ratio_db"][8] is None and res["skipped_bins"] == 2
    assert np.allclose(res["ratio_db"][:7], [0, 0, 10, -10, 0, -20, -20], atol=1e-12)
    assert abs(res["distance_db"] - 60.0 / 6) < 1e-12 and abs(res["high_db"] - (-40.0 / 2)) < 1e-12     # bins 1..6; bins 5, 6 of 5..8
    assert res["real_sem"][0] == 0.0 and abs(res["real_sem"][4] - 1.0) < 1e-12 and res["fake_sem"][8] == 0.0
    table = M.format_spectrum(res, "T")
    assert table.splitlines()[0] == "T (2 images per side)" and len(table.splitlines()) == 2 + 4 + 1 and "2 bins without power" in table
    assert "distance_db 10.00" in table and "high_db -20.00" in table
    m.count["fake"] = 3
    with pytest.raises(ValueError, match="feed both sets equally"):
        m.result()


def test_flags_and_configuration_names(ngan):
    cfg, train = ngan.config, ngan.train
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    try:
        assert (cfg.configs_name["spectrum_period"], cfg.configs_name["spectrum_images"], cfg.configs_name["spectrum_seed"]) == (0, 8192, 0)
        d = train.build_arg_parser().parse_args([])
        assert (d.spectrum_period, d.spectrum_images, d.spectrum_seed) == (0, 8192, 0)
        none = train.cli_overrides([], d, cfg.configs_name)
        assert not any(k.startswith("spectrum") for k in none)
        argv = ["--spectrum_period", "10", "--spectrum_images", "256", "--spectrum_seed", "7"]
        over = train.cli_overrides(argv, train.build_arg_parser().parse_args(argv), cfg.configs_name)
        assert over == {"spectrum_period": 10, "spectrum_images": 256, "spectrum_seed": 7}
        cfg.set_configs(**over)
        cfg.validate_configs()
        assert (cfg.spectrum_period, cfg.spectrum_images, cfg.spectrum_seed) == (10, 256, 7)
        for name, bad in (("spectrum_period", -1), ("spectrum_images", 0), ("spectrum_seed", -3), ("spectrum_period", 1.5),
                          ("spectrum_period", True), ("spectrum_images", True)):
            cfg.set_configs(**{**over, name: bad})
            with pytest.raises(ValueError, match=name):
                cfg.validate_configs()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    plan = ngan.launch.launch_plan(2, ["--pggan", "--spectrum_period", "10", "--gpus", "2"], port=29500, environ={})
    assert all("--spectrum_period 10" in " ".join(argv_i) for argv_i, _ in plan)
    p = ngan.eval.build_arg_parser()
    d = p.parse_args([])
    assert (d.spectrum, d.spectrum_seed, d.msssim, d.swd) == (None, 0, None, None)
    assert p.parse_args(["--spectrum"]).spectrum == 8192
    o = p.parse_args(["--spectrum", "512", "--ema", "--dataset_dir", "d", "--swd", "64", "--msssim", "32"])
    assert (o.spectrum, o.ema, o.dataset_dir, o.swd, o.msssim) == (512, True, "d", 64, 32)


def nets(ngan, seed):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([16, 16, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 16, 16], image_size_init=4)
    return G, D


def entry(epoch, ema=False):
    e = {"epoch": epoch, "image_size": 16, "images": 8, "k": list(range(9)), "real": [0.5] * 9, "fake": [0.25] * 9,
         "ratio_db": [-3.0] * 8 + [None], "distance_db": 3.0, "high_db": -3.0}
    if ema:
        e.update(distance_db_ema=2.5, high_db_ema=-2.5)
    return e


def test_checkpoint_list_round_trip(ngan, tmp_path):
    utils = ngan.utils
    G, D = nets(ngan, 1)
    f = str(tmp_path / "GenDisc_s.pth")
    ck = utils.Checkpointer(G, D, 1e-4, f, N_epochs=10, verbose=False)
    ck.save_state(1)
    assert "SPECTRUM" not in utils.load_checkpoint_dict(f)            # nothing scored: the file of a build without the feature
    entries = [entry(2), entry(4, ema=True)]
    ck.SPECTRUM.extend(entries)
    ck.save_state(4)
    saved = utils.load_checkpoint_dict(f)                              # the weights-only unpickler accepts the list
    assert saved["SPECTRUM"] == entries and "SWD" not in saved and "MSSSIM" not in saved
    G2, D2 = nets(ngan, 2)
    ck2 = utils.Checkpointer(G2, D2, 1e-4, f, N_epochs=10, verbose=False)
    ck2.load_state()
    assert ck2.SPECTRUM == entries and ck2.SWD == [] and ck2.MSSSIM == [] and ck2.epoch == 4
    ck2.SPECTRUM.append(entry(6))
    ck2.save_state(6)                                                  # a resumed run continues the list
    assert [e["epoch"] for e in utils.load_checkpoint_dict(f)["SPECTRUM"]] == [2, 4, 6]
    f0 = str(tmp_path / "GenDisc_0.pth")
    utils.Checkpointer(G, D, 1e-4, f0, N_epochs=10, verbose=False).save_state(3)
    ck3 = utils.Checkpointer(G2, D2, 1e-4, f0, N_epochs=10, verbose=False)
    ck3.load_state()
    assert ck3.SPECTRUM == [] and ck3.epoch == 3
