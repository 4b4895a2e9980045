"""Arbor morphology without a GPU: the restatement of tests/morph_cases.py against scipy's labelling and against closed forms, the mask
families doing what they are there for, what the metric says on known sets, host-side validation of the new entry points, the
bookkeeping of `Morphology.result()`, the configuration names and flags, and the checkpoint list.  The kernels themselves are tested on
the GPU (tests/test_gpu_morph.py); their union-find text also runs serially on the host (tools/morph_host_check.cpp)."""
import ctypes

import numpy as np
import pytest
import torch

import morph_cases as MC
import multiotsu_ref as OT

f64 = np.float64


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (16, 32, 64))
def test_labelling_against_scipy(size):
    ndimage = pytest.importorskip("scipy.ndimage")
    masks, refs = MC.case(size)
    for name, m, (lab, stats, _) in zip(MC.FAMILIES, masks, refs):
        got, n = ndimage.label(m, structure=np.ones((3, 3), int))
        assert n == stats[1], name
        # the same partition: scipy's label of a pixel <-> the canonical label, one to one
        pairs = {(int(a), int(b)) for a, b in zip(got.ravel(), lab.ravel())}
        assert len(pairs) == n + (1 if (m == 0).any() else 0) and ((0, -1) in pairs) == bool((m == 0).any()), name
        roots = np.unique(lab[lab >= 0])
        assert all(lab.ravel()[r] == r and (lab.ravel()[:r] != r).all() for r in roots), name      # the smallest index of its component


@pytest.mark.parametrize("size", (16, 64))
def test_run_labelling_equals_the_flood_fill(size):
    masks, refs = MC.case(size)
    for name, m, (lab, stats, kept) in zip(MC.FAMILIES, masks, refs):
        got = MC.label_runs_ref(m)
        assert np.array_equal(got, lab), name
        for min_size in (1, 2, 8):
            _, st, kp = MC.stats_ref(m, min_size)
            st2, kp2 = MC.stats_of_labels(got, min_size)
            assert st2 == st and np.array_equal(kp2, kp), (name, min_size)


@pytest.mark.parametrize("size", MC.SIZES)
def test_families_do_what_they_are_there_for(size):
    R = size
    masks, refs = MC.case(R)
    st = {name: ref[1] for name, ref in zip(MC.FAMILIES, refs)}
    lab = {name: ref[0] for name, ref in zip(MC.FAMILIES, refs)}
    assert st["empty"] == [0, 0, 0, 0] and st["full"] == [R * R, 1, R * R, R * R] and st["single"] == [1, 1, 1, 1]
    assert lab["single"][R - 1, R - 1] == R * R - 1
    assert st["checkerboard"] == [R * R // 2, 1, R * R // 2, R * R // 2]
    assert len(MC.label_ref(MC.family("checkerboard", R), connectivity=4)[1]) == R * R // 2
    for name in ("diagonal", "antidiagonal"):
        assert st[name] == [R, 1, R, R] and len(MC.label_ref(MC.family(name, R), connectivity=4)[1]) == R
    assert lab["antidiagonal"][R - 1, 0] == R - 1
    n_snake = R * R // 2 + R // 2 - 1
    assert st["snake"] == [n_snake, 1, n_snake, n_snake] and (lab["snake"][R - 2] == 0).all()
    n_comb = (R // 2) * (R - 1) + R
    for name in ("comb", "comb_flip", "comb_t"):
        assert st[name] == [n_comb, 1, n_comb, n_comb], name
    assert (lab["comb"][0, 0::2] == 0).all()                                      # every tooth carries the first tooth's label
    k = (R // 8 - 1) ** 2
    assert st["corners"] == [2 * k, k, 2 if k else 0, 2 * k]
    assert MC.stats_ref(MC.family("corners", R), 3)[1] == [2 * k, 0, 2 if k else 0, 0]
    assert len(MC.label_ref(MC.family("corners", R), connectivity=4)[1]) == 2 * k
    n_gap = max(R // 64, 1)
    assert st["gaps"] == [R * (R - n_gap), n_gap, R * (R - n_gap) // n_gap, R * (R - n_gap)] and lab["gaps"][R - 1, R - 1] == (1 if R <= 64 else 65)
    assert st["rings"][1] == R // 4 and st["rings"][2] == 4 * (R - 1)
    assert st["random41"][1] > 3 and st["random41"][2] > 0.1 * st["random41"][0]   # many components, some of them large
    assert st["arbor"][1] == 1 and st["arbor"][0] > R


def test_box_counts_and_dimension_closed_forms():
    for R in (32, 64, 128):
        L = R.bit_length() - 1
        row = MC.box_counts_ref(MC.family("row", R))
        diag = MC.box_counts_ref(MC.family("diagonal", R))
        assert row == diag == [R >> k for k in range(L + 1)]
        assert abs(MC.dimension_ref(row, R) - 1.0) < 1e-12
        assert MC.box_counts_ref(MC.family("full", R)) == [(R >> k) ** 2 for k in range(L + 1)]
        assert abs(MC.dimension_ref(MC.box_counts_ref(MC.family("full", R)), R) - 2.0) < 1e-12
        assert MC.box_counts_ref(MC.family("corner_boxes", R)) == [4] * L + [1]
        assert MC.box_counts_ref(MC.family("empty", R)) == [0] * (L + 1) and np.isnan(MC.dimension_ref([0] * (L + 1), R))
        disc = MC.dimension_ref(MC.box_counts_ref(MC.family("disc", R)), R)
        print(f"R={R}: dimension of a row 1.000, of a disc of radius 0.4 R {disc:.3f}")
        assert abs(disc - {32: 1.685, 64: 1.763, 128: 1.819}[R]) < 5e-4


def test_level_rule_round_trips_every_byte():
    v = np.arange(256, dtype=np.uint8).reshape(1, 16, 16)
    x = MC.from_bytes(v)[..., None]
    assert np.array_equal(MC.levels_ref(x), v)
    # the fused form's single rounding: an exact rational evaluation, rounded once to fp32, gives the same levels
    from fractions import Fraction
    for xv, got in zip(x.ravel()[::7], MC.levels_ref(x).ravel()[::7]):
        exact = Fraction(float(xv)) * Fraction(255, 2) + 128
        assert int(np.float32(float(exact))) == int(got)
    out = MC.levels_ref(np.array([-3.0, -1.0, 1.0, 3.0, 0.0, 0.999], np.float32).reshape(1, 1, 6, 1))
    assert out.ravel().tolist() == [0, 0, 255, 255, 128, 255]
    rgb = np.random.default_rng(0).uniform(-1, 1, (1, 4, 4, 3)).astype(np.float32)
    mean = ((rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]) * np.float32(1.0 / 3.0)
    assert mean.dtype == np.float32 and np.array_equal(MC.levels_ref(rgb), MC.levels_ref(mean[..., None]))


def test_ks_statistic():
    assert MC.ks_ref([1, 2, 3], [1, 2, 3]) == 0.0 and MC.ks_ref([1, 2, 3], [4, 5, 6]) == 1.0
    assert abs(MC.ks_ref([1, 2, 3, 4], [3, 4, 5, 6]) - 0.5) < 1e-15
    assert abs(MC.ks_ref([0.0, 0.0, 1.0], [0.0, 1.0, 1.0]) - 1.0 / 3.0) < 1e-15       # ties
    rng = np.random.default_rng(1)
    a, b = rng.normal(size=37), rng.normal(0.5, 1.0, size=23)
    brute = max(abs((a <= t).mean() - (b <= t).mean()) for t in np.concatenate([a, b]))
    assert abs(MC.ks_ref(a, b) - brute) < 1e-15


def test_metric_on_known_sets():
    """16 intact random-walk trees against the same cut along every sixth row and column, R = 64; and the images that carry them through
    the threshold: t0 lies between the noise floor and the dimmest foreground band for every one"""
    whole, cut = MC.arbor_set(64, 16, 1), MC.arbor_set(64, 16, 1, cut=True)
    real = [MC.arbor_statistics_ref(m) for m in whole]
    fake = [MC.arbor_statistics_ref(m) for m in cut]
    res = MC.morphology_ref(real, fake)
    print("intact: largest_share {:.3f}, components {:.1f}; cut: largest_share {:.3f} (max {:.3f}), components {:.1f} (min {:.0f})".format(
        res["largest_share"]["real"], res["components"]["real"], res["largest_share"]["fake"], max(f["largest_share"] for f in fake),
        res["components"]["fake"], min(f["components"] for f in fake)))
    assert all(r["largest_share"] == 1.0 and r["components"] == 1 for r in real)
    assert all(f["largest_share"] <= 0.10 and f["components"] >= 33 for f in fake)
    assert res["largest_share"]["ks"] == 1.0 and res["skipped_real"] == res["skipped_fake"] == 0
    again = MC.morphology_ref(real, [MC.arbor_statistics_ref(m) for m in MC.arbor_set(64, 16, 1)])
    assert again["largest_share"]["ks"] == 0.0
    for masks, seed in ((whole, 5), (cut, 6), (MC.arbor_set(64, 16, 2), 7)):
        img, _ = MC.mask_images(masks, seed)
        for i, m in zip(img, masks):
            t0 = OT.multiotsu4(np.bincount(i.ravel(), minlength=256))[0][0]
            assert 20 <= t0 <= 89 and np.array_equal(i > t0, m != 0)


# ---- the library on the host ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_bound_and_validate_on_the_host(ngan):
    lib = ngan._C.lib()
    one = ctypes.c_void_p(64)            # any aligned non-null address: every check below comes before the launch
    odd = ctypes.c_void_p(68)
    N = None
    err = lambda: lib.ngan_last_error()  # noqa: E731
    assert {"ngan_morph_levels", "ngan_morph_mask", "ngan_morph_label", "ngan_morph_boxcount", "ngan_morph_workspace_bytes"} \
        <= set(ngan._C.exported_symbols())
    calls = {
        "levels": lambda B=1, R=16, C=1, p=(one, one, one): lib.ngan_morph_levels(*p, B, R, C, None),
        "mask": lambda B=1, R=16, C=1, p=(one, one, one): lib.ngan_morph_mask(*p, B, R, None),
        "label": lambda B=1, R=16, C=1, p=(one, one, one, N, one), min_size=1: lib.ngan_morph_label(*p, B, R, min_size, None),
        "boxcount": lambda B=1, R=16, C=1, p=(one, one): lib.ngan_morph_boxcount(*p, B, R, None),
    }
    for name, call in calls.items():
        for r in (8, 24, 2048, 0, -16):
            assert call(R=r) < 0 and b"R=" in err() and name.encode() in err(), (name, r)
        for b in (0, -1, 65536):
            assert call(B=b) < 0 and b"B=" in err(), (name, b)
    for c in (0, 2, 4):
        assert calls["levels"](C=c) < 0 and b"C=" in err()
    for p in ((N, one, one), (one, N, one), (one, one, N)):
        assert calls["levels"](p=p) < 0 and b"null" in err()
        assert calls["mask"](p=p) < 0 and b"null" in err()
    for p in ((N, one, one, N, one), (one, N, one, N, one), (one, one, N, N, one)):
        assert calls["label"](p=p) < 0 and b"null" in err()
    assert calls["label"](p=(one, one, one, N, N)) < 0 and b"workspace" in err()
    for p in ((N, one), (one, N)):
        assert calls["boxcount"](p=p) < 0 and b"null" in err()
    for p in ((odd, one, one), (one, odd, one), (one, one, ctypes.c_void_p(66))):
        assert calls["levels"](p=p) < 0 and b"boundary" in err()
    for p in ((odd, one, one), (one, one, odd), (one, ctypes.c_void_p(66), one)):
        assert calls["mask"](p=p) < 0 and b"boundary" in err()
    for p in ((odd, one, one, N, one), (one, odd, one, N, one), (one, one, one, odd, one), (one, one, one, N, odd),
              (one, one, ctypes.c_void_p(66), N, one)):
        assert calls["label"](p=p) < 0 and b"boundary" in err()
    for p in ((odd, one), (one, ctypes.c_void_p(66))):
        assert calls["boxcount"](p=p) < 0 and b"boundary" in err()
    for m in (0, -1):
        assert calls["label"](min_size=m) < 0 and b"min_size" in err()
    assert lib.ngan_morph_workspace_bytes(1, 16) == 16 * 16 * 4 and lib.ngan_morph_workspace_bytes(64, 512) == 64 * 512 * 512 * 4
    for r in (8, 24, 2048, 0):
        assert lib.ngan_morph_workspace_bytes(1, r) == 0
    assert lib.ngan_morph_workspace_bytes(0, 16) == 0 and lib.ngan_morph_workspace_bytes(65536, 16) == 0
    M = ngan.metrics
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.morph_levels(torch.zeros(1, 16, 16, 1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.connected_components(torch.zeros(1, 16, 16, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.box_counts(torch.zeros(1, 16, 16, dtype=torch.uint8))
    with pytest.raises(ValueError):
        M.morph_levels(torch.zeros(1, 16, 16, 2))
    with pytest.raises(ValueError):
        M.morph_levels(torch.zeros(1, 16, 32, 1))
    with pytest.raises(TypeError):
        M.box_counts(torch.zeros(1, 16, 16))
    with pytest.raises(ValueError):
        M.arbor_statistics(torch.zeros(1, 16, 16, 1), otsu_class=4)
    with pytest.raises(ValueError):
        M.arbor_statistics(torch.zeros(1, 16, 16, 1), min_size=0)


def test_box_dimension_and_ks_on_the_host(ngan):
    M = ngan.metrics
    for R in (16, 64, 1024):
        L = R.bit_length() - 1
        counts = torch.tensor([[R >> k for k in range(L + 1)], [(R >> k) ** 2 for k in range(L + 1)], [0] * (L + 1),
                               MC.box_counts_ref(MC.family("disc", min(R, 128))) + [1] * (L - min(R, 128).bit_length() + 1)], dtype=torch.int32)
        d = M.box_dimension(counts, R)
        assert d.dtype == torch.float64 and abs(float(d[0]) - 1.0) < 1e-12 and abs(float(d[1]) - 2.0) < 1e-12 and bool(torch.isnan(d[2]))
        assert abs(float(d[3]) - MC.dimension_ref(counts[3].tolist(), R)) < 1e-12
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=37), np.round(rng.normal(0.3, 1.0, size=23), 1)
    assert abs(M.ks_distance(torch.tensor(a), torch.tensor(b)) - MC.ks_ref(a, b)) < 1e-15
    assert M.ks_distance(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.0])) == 0.0


def test_metric_object_on_the_host(ngan):
    M = ngan.metrics
    m = M.Morphology(64, n_colors=3, device="cpu")
    assert m.active and (m.otsu_class, m.min_size) == (1, 1)
    with pytest.raises(ValueError, match="feed both sets equally"):
        m.result()
    with pytest.raises(ValueError):
        m.feed("fake", torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError):
        m.feed("other", torch.zeros(2, 3, 64, 64))
    for bad in (dict(image_size=48), dict(image_size=64, n_colors=2), dict(image_size=2048), dict(image_size=64, otsu_class=0),
                dict(image_size=64, min_size=0), dict(image_size=64, min_size=1.5)):
        with pytest.raises(ValueError):
            M.Morphology(**bad)
    small = M.Morphology(8, device="cpu")                                    # 8 x 8: said, not raised, and no number
    small.feed("real", torch.zeros(2, 1, 8, 8))
    res = small.result()
    assert res["images"] == 0 and "fill" not in res and "16 x 16" in res["note"] and "16 x 16" in M.format_morphology(res)
    # the bookkeeping of result(), on values filled by hand: rows fill, components, largest_share, dimension, scored
    nan = float("nan")
    real = torch.tensor([[0.10, 0.20, 0.30, 0.0], [1, 1, 2, 0], [1.0, 1.0, 0.75, nan], [1.2, 1.3, 1.4, nan], [1, 1, 1, 0]], dtype=torch.float64)
    fake = torch.tensor([[0.10, 0.05, 0.0, 0.15], [9, 12, 0, 30], [0.2, 0.1, nan, 0.05], [1.0, 0.9, nan, 1.1], [1, 1, 0, 1]], dtype=torch.float64)
    m = M.Morphology(16, device="cpu")
    m.values["real"], m.count["real"] = [real[:, :1], real[:, 1:]], 4          # two feeds
    m.values["fake"], m.count["fake"] = [fake], 4
    res = m.result()
    rs = [{k: float(real[i, j]) for i, k in enumerate(MC.STATISTICS)} | {"scored": bool(real[4, j])} for j in range(4)]
    fs = [{k: float(fake[i, j]) for i, k in enumerate(MC.STATISTICS)} | {"scored": bool(fake[4, j])} for j in range(4)]
    ref = MC.morphology_ref(rs, fs)
    assert (res["images"], res["skipped_real"], res["skipped_fake"]) == (4, 1, 1) and set(res) == set(ref)
    for name in MC.STATISTICS:
        for k, v in ref[name].items():
            assert abs(res[name][k] - v) < 1e-12, (name, k)
    assert res["largest_share"]["ks"] == 1.0 and abs(res["fill"]["ks"] - 2.0 / 3.0) < 1e-12 and abs(res["components"]["real"] - 4.0 / 3.0) < 1e-12
    table = M.format_morphology(res, "T")
    assert table.splitlines()[0].startswith("T (4 images per side; not scored: 1 of the data, 1 generated)") and len(table.splitlines()) == 2 + 4
    assert all(name in table for name in MC.STATISTICS) and "KS" in table
    m.values["fake"] = [fake * torch.tensor([[1.0], [1], [1], [1], [0]], dtype=torch.float64)]       # no generated image scored
    res = m.result()
    assert "fill" not in res and res["skipped_fake"] == 4 and "generated" in res["note"] and "generated" in M.format_morphology(res)
    one = M.Morphology(16, device="cpu")                                      # one image per side: no standard error
    one.values["real"], one.values["fake"], one.count = [real[:, :1]], [fake[:, :1]], {"real": 1, "fake": 1}
    res = one.result()
    assert res["fill"]["real_sem"] is None and res["fill"]["fake_sem"] is None and "+-" not in M.format_morphology(res)
    m.count["fake"] = 3
    with pytest.raises(ValueError, match="feed both sets equally"):
        m.result()


def test_flags_and_configuration_names(ngan):
    cfg, train = ngan.config, ngan.train
    names = ("morph_period", "morph_images", "morph_seed", "morph_min_size")
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    try:
        assert tuple(cfg.configs_name[n] for n in names) == (0, 8192, 0, 1)
        d = train.build_arg_parser().parse_args([])
        assert tuple(getattr(d, n) for n in names) == (0, 8192, 0, 1)
        none = train.cli_overrides([], d, cfg.configs_name)
        assert not any(k.startswith("morph") for k in none)
        argv = ["--morph_period", "10", "--morph_images", "256", "--morph_seed", "7", "--morph_min_size", "8"]
        over = train.cli_overrides(argv, train.build_arg_parser().parse_args(argv), cfg.configs_name)
        assert over == {"morph_period": 10, "morph_images": 256, "morph_seed": 7, "morph_min_size": 8}
        cfg.set_configs(**over)
        cfg.validate_configs()
        assert tuple(getattr(cfg, n) for n in names) == (10, 256, 7, 8)
        for name, bad in (("morph_period", -1), ("morph_images", 0), ("morph_seed", -3), ("morph_min_size", 0), ("morph_period", 1.5),
                          ("morph_period", True), ("morph_min_size", True)):
            cfg.set_configs(**{**over, name: bad})
            with pytest.raises(ValueError, match=name):
                cfg.validate_configs()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    plan = ngan.launch.launch_plan(2, ["--pggan", "--morph_period", "10", "--morph_min_size", "4", "--gpus", "2"], port=29500, environ={})
    assert all("--morph_period 10 --morph_min_size 4" in " ".join(argv_i) for argv_i, _ in plan)
    p = ngan.eval.build_arg_parser()
    d = p.parse_args([])
    assert (d.morph, d.morph_seed, d.morph_min_size, d.spectrum, d.msssim, d.swd) == (None, 0, 1, None, None, None)
    assert p.parse_args(["--morph"]).morph == 8192
    o = p.parse_args(["--morph", "512", "--morph_min_size", "4", "--ema", "--dataset_dir", "d", "--swd", "64", "--msssim", "32", "--spectrum", "16"])
    assert (o.morph, o.morph_min_size, o.ema, o.dataset_dir, o.swd, o.msssim, o.spectrum) == (512, 4, True, "d", 64, 32, 16)


def nets(ngan, seed):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([16, 16, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 16, 16], image_size_init=4)
    return G, D


def entry(epoch, ema=False):
    row = {"real": 0.5, "real_sem": 0.01, "fake": 0.25, "fake_sem": None, "ks": 0.75}
    e = {"epoch": epoch, "image_size": 16, "images": 8, "min_size": 1, "skipped_real": 0, "skipped_fake": 1}
    e.update({name: dict(row) for name in MC.STATISTICS})
    if ema:
        e["skipped_fake_ema"] = 0
        e.update({name + "_ema": {"fake": 0.3, "fake_sem": 0.02, "ks": 0.5} for name in MC.STATISTICS})
    return e


def test_checkpoint_list_round_trip(ngan, tmp_path):
    utils = ngan.utils
    G, D = nets(ngan, 1)
    f = str(tmp_path / "GenDisc_m.pth")
    ck = utils.Checkpointer(G, D, 1e-4, f, N_epochs=10, verbose=False)
    ck.save_state(1)
    assert "MORPH" not in utils.load_checkpoint_dict(f)               # nothing scored: the file of a build without the feature
    entries = [entry(2), entry(4, ema=True), {"epoch": 5, "image_size": 8, "images": 0, "min_size": 1, "skipped_real": 0,
                                              "skipped_fake": 0, "note": "8 x 8 images are below 16 x 16: nothing to label"}]
    ck.MORPH.extend(entries)
    ck.save_state(5)
    saved = utils.load_checkpoint_dict(f)                              # the weights-only unpickler accepts the list
    assert saved["MORPH"] == entries and "SWD" not in saved and "MSSSIM" not in saved and "SPECTRUM" not in saved
    G2, D2 = nets(ngan, 2)
    ck2 = utils.Checkpointer(G2, D2, 1e-4, f, N_epochs=10, verbose=False)
    ck2.load_state()
    assert ck2.MORPH == entries and ck2.SWD == [] and ck2.SPECTRUM == [] and ck2.epoch == 5
    ck2.MORPH.append(entry(6))
    ck2.save_state(6)                                                  # a resumed run continues the list
    assert [e["epoch"] for e in utils.load_checkpoint_dict(f)["MORPH"]] == [2, 4, 5, 6]
    f0 = str(tmp_path / "GenDisc_0.pth")
    utils.Checkpointer(G, D, 1e-4, f0, N_epochs=10, verbose=False).save_state(3)
    ck3 = utils.Checkpointer(G2, D2, 1e-4, f0, N_epochs=10, verbose=False)
    ck3.load_state()
    assert ck3.MORPH == [] and ck3.epoch == 3
