"""Arbor skeleton without a GPU: the properties of the restatement of tests/skeleton_cases.py on every mask family, closed forms, what
the metric says on known sets, host-side validation of the two entry points, the bookkeeping of `Skeleton.result()`, the
configuration names and flags, and the checkpoint list.  The kernel itself is tested on the GPU (tests/test_gpu_skeleton.py); its
bit-sliced text also runs serially on the host (tools/skel_host_check.cpp)."""
import ctypes

import numpy as np
import pytest
import torch

import morph_cases as MC
import skeleton_cases as SC

f64 = np.float64


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (16, 32, 64))
def test_properties_of_the_thinning(size):
    masks, refs = SC.case(size)
    for name, m, (sk, st) in zip(SC.FAMILIES, masks, refs):
        assert set(np.unique(sk)) <= {0, 1} and not (sk & ~(m != 0)).any(), f"{name}: the skeleton is no subset of the mask"
        again, passes = SC.thin_ref(sk)
        assert np.array_equal(again, sk) and passes == 2, f"{name}: thinning the skeleton changed it"
        assert st[6] % 2 == 0 and st[6] >= 2 and st[7] == int((m != 0).sum()) and st[:6] == SC.counts_ref(sk), name
    by_name = dict(zip(SC.FAMILIES, refs))
    assert by_name["full"][1][0] == 1 and by_name["full"][1][6] == size + 2
    assert by_name["block2"][1][0] == 1 and by_name["disc"][1][0] == 1
    assert by_name["empty"][1] == [0, 0, 0, 0, 0, 0, 2, 0]


@pytest.mark.parametrize("size", (16, 32, 64))
def test_thinning_keeps_the_component_count(size):
    ndimage = pytest.importorskip("scipy.ndimage")
    eight = np.ones((3, 3), int)
    masks, refs = SC.case(size)
    for name, m, (sk, _) in zip(SC.FAMILIES, masks, refs):
        assert ndimage.label(sk, structure=eight)[1] == ndimage.label(m, structure=eight)[1], name


def test_closed_forms_at_32():
    """arms run from 2 to R - 3; columns: pixels, tips, junctions, orth, diag, passes (None: not stated)"""
    table = {"row": (32, 2, 0, 31, 0, 2), "bar3": (26, 2, 0, 25, 0, 4), "plus": (55, 4, 1, 54, 0, 2), "plus3": (51, 4, 1, 50, 0, 6),
             "tee": (53, 3, 1, 52, 0, 2), "diagonal": (32, 2, 0, 0, 31, 2), "cross_x": (64, 4, 0, 4, 60, None),
             "rings": (512, 0, 0, 480, 32, 4)}
    for name, (pixels, tips, junctions, orth, diag, passes) in table.items():
        _, st = SC.stats_ref(SC.family(name, 32))
        assert [st[0], st[1], st[2], st[4], st[5]] == [pixels, tips, junctions, orth, diag], (name, st)
        assert passes is None or st[6] == passes, (name, st)
        assert st[3] == 0, name
    m = SC.family("tee", 32)
    assert m[4, 2:30].all() and m[4:30, 16].all() and int(m.sum()) == 53
    single = SC.counts_ref(MC.family("single", 32))
    assert single == [1, 0, 0, 1, 0, 0]
    stair = np.zeros((16, 16), np.uint8)                              # a staircase corner: one orthogonal step each, no diagonal
    stair[4, 4] = stair[4, 5] = stair[5, 5] = 1
    assert SC.counts_ref(stair)[4:] == [2, 0]


def test_the_families_do_what_they_are_there_for():
    for R in (32, 64, 128):
        v, h = SC.family("bars_v", R), SC.family("bars_h", R)
        assert np.array_equal(h, v.T) and v[2, 31] == 1 and v[R - 3, 31] == 1
        if R >= 64:
            assert v[2, 30:33].all() and not v[2, 33] and v[R - 3, 31:34].all() and not v[R - 3, 30]
        if R >= 128:
            assert v[2, 62:65].all() and v[R - 3, 63:66].all()
    f = SC.family("frame", 32)
    assert f[0].all() and f[:, 0].all() and f[31].all() and f[:, 31].all() and not f[3:29, 3:29].any() and f[2, 2:30].all()
    assert int(SC.family("block2", 32).sum()) == 4
    a, t = MC.family("arbor", 64), SC.family("thick_arbor", 64)
    assert (t[a != 0] == 1).all() and int(t.sum()) > 2 * int(a.sum())
    assert set(MC.FAMILIES) < set(SC.FAMILIES) and {"row", "disc"} < set(SC.FAMILIES)


# ---- the metric on known sets --------------------------------------------------------------------------------------------------------------
def test_known_sets_at_64():
    whole, cut, other = MC.arbor_set(64, 16, 1), MC.arbor_set(64, 16, 1, cut=True), MC.arbor_set(64, 16, 2)
    sw, sc, so = ([SC.skeleton_statistics_ref(a) for a in s] for s in (whole, cut, other))
    res = SC.skeleton_ref(sw, sc)
    assert res["tips"]["ks"] == 1.0 and res["junctions"]["ks"] == 1.0
    assert MC.ks_ref([s["pixels"] for s in sw], [s["pixels"] for s in sc]) == 1.0
    assert abs(res["tips"]["real"] - 23.6) < 0.05 and abs(res["tips"]["fake"] - 113.4) < 0.05
    assert SC.skeleton_ref(sw, so)["tips"]["ks"] == 0.1875
    fat = [SC.skeleton_statistics_ref(SC.dilate(a)) for a in whole]
    res = SC.skeleton_ref(sw, fat)
    assert abs(res["width"]["real"] - 1.363) < 5e-4 and abs(res["width"]["fake"] - 6.09) < 5e-3 and res["width"]["ks"] == 1.0
    assert all(s["scored"] for s in sw + sc + so + fat)
    empty = SC.skeleton_statistics_ref(np.zeros((16, 16), np.uint8))
    assert not empty["scored"]


# ---- the library on the host ---------------------------------------------------------------------------------------------------------------
def test_entry_points_are_bound_and_validate_on_the_host(ngan):
    lib = ngan._C.lib()
    one = ctypes.c_void_p(64)            # any aligned non-null address: every check below comes before the launch
    odd = ctypes.c_void_p(68)
    N = None
    err = lambda: lib.ngan_last_error()  # noqa: E731
    assert {"ngan_skel_thin", "ngan_skel_counts"} <= set(ngan._C.exported_symbols())
    calls = {
        "thin": lambda B=1, R=16, p=(one, one, one): lib.ngan_skel_thin(*p, B, R, None),
        "counts": lambda B=1, R=16, p=(one, one): lib.ngan_skel_counts(*p, B, R, None),
    }
    for name, call in calls.items():
        for r in (8, 24, 1024, 2048, 0, -16):
            assert call(R=r) < 0 and f"R={r}".encode() in err() and name.encode() in err(), (name, r)
        for b in (0, -1, 65536):
            assert call(B=b) < 0 and f"B={b}".encode() in err(), (name, b)
    for p in ((N, one, one), (one, one, N), (N, N, one)):
        assert calls["thin"](p=p) < 0 and b"null" in err()
    for p in ((N, one), (one, N)):
        assert calls["counts"](p=p) < 0 and b"null" in err()
    for p in ((odd, one, one), (one, odd, one), (odd, N, one), (one, one, ctypes.c_void_p(66)), (one, N, ctypes.c_void_p(66))):
        assert calls["thin"](p=p) < 0 and b"boundary" in err()
    for p in ((odd, one), (one, ctypes.c_void_p(66))):
        assert calls["counts"](p=p) < 0 and b"boundary" in err()
    M = ngan.metrics
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.thin(torch.zeros(1, 16, 16, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.skeleton_counts(torch.zeros(1, 16, 16, dtype=torch.uint8))
    with pytest.raises(TypeError):
        M.thin(torch.zeros(1, 16, 16))
    with pytest.raises(TypeError):
        M.skeleton_counts(torch.zeros(1, 16, 32, dtype=torch.uint8))
    with pytest.raises(ValueError):
        M.skeleton_statistics(torch.zeros(1, 16, 16, 1), otsu_class=4)
    with pytest.raises(ValueError):
        M.skeleton_statistics(torch.zeros(1, 16, 16, 1), min_size=0)
    assert M.SKELETON_STATISTICS == ("length", "tips", "junctions", "width") and M.SKEL_STATS == SC.STAT_NAMES
    assert M.MORPH_STATISTICS == ("fill", "components", "largest_share", "dimension")


def test_metric_object_on_the_host(ngan):
    M = ngan.metrics
    m = M.Skeleton(64, n_colors=3, device="cpu")
    assert m.active and (m.otsu_class, m.min_size) == (1, 1)
    with pytest.raises(ValueError, match="feed both sets equally"):
        m.result()
    with pytest.raises(ValueError):
        m.feed("fake", torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError):
        m.feed("other", torch.zeros(2, 3, 64, 64))
    for bad in (dict(image_size=48), dict(image_size=64, n_colors=2), dict(image_size=64, otsu_class=0), dict(image_size=64, min_size=0),
                dict(image_size=64, min_size=1.5)):
        with pytest.raises(ValueError):
            M.Skeleton(**bad)
    small = M.Skeleton(8, device="cpu")                                       # 8 x 8: said, not raised, and no number
    small.feed("real", torch.zeros(2, 1, 8, 8))
    res = small.result()
    assert res["images"] == 0 and "length" not in res and "16 x 16" in res["note"] and "16 x 16" in M.format_skeleton(res)
    large = M.Skeleton(1024, device="cpu")                                    # above the kernel's 512: the same
    assert not large.active and M.Skeleton(512, device="cpu").active
    large.feed("fake", torch.zeros(1, 1, 1024, 1024))
    res = large.result()
    assert res["images"] == 0 and "length" not in res and "512 x 512" in res["note"] and "512 x 512" in M.format_skeleton(res)
    assert M.Morphology(1024, device="cpu").active                            # the morphology score still takes that stage
    # the bookkeeping of result(), on values filled by hand: rows length, tips, junctions, width, scored
    nan = float("nan")
    real = torch.tensor([[1.5, 2.5, 3.5, 0.0], [4, 6, 9, 0], [1, 2, 3, 0], [1.4, 1.3, 1.2, nan], [1, 1, 1, 0]], dtype=torch.float64)
    fake = torch.tensor([[0.5, 0.7, 0.0, 0.9], [40, 60, 0, 90], [0, 1, 0, 2], [3.0, 2.9, nan, 3.1], [1, 1, 0, 1]], dtype=torch.float64)
    m = M.Skeleton(16, device="cpu")
    m.values["real"], m.count["real"] = [real[:, :1], real[:, 1:]], 4          # two feeds
    m.values["fake"], m.count["fake"] = [fake], 4
    res = m.result()
    rs = [{k: float(real[i, j]) for i, k in enumerate(SC.STATISTICS)} | {"scored": bool(real[4, j])} for j in range(4)]
    fs = [{k: float(fake[i, j]) for i, k in enumerate(SC.STATISTICS)} | {"scored": bool(fake[4, j])} for j in range(4)]
    ref = SC.skeleton_ref(rs, fs)
    assert (res["images"], res["skipped_real"], res["skipped_fake"]) == (4, 1, 1) and set(res) == set(ref)
    for name in SC.STATISTICS:
        assert set(res[name]) == {"real", "real_sem", "fake", "fake_sem", "ks"}
        for k, v in ref[name].items():
            assert abs(res[name][k] - v) < 1e-12, (name, k)
    assert res["length"]["ks"] == 1.0 and res["width"]["ks"] == 1.0 and abs(res["junctions"]["ks"] - 1.0 / 3.0) < 1e-12
    table = M.format_skeleton(res, "T")
    assert table.splitlines()[0].startswith("T (4 images per side; not scored: 1 of the data, 1 generated)") and len(table.splitlines()) == 2 + 4
    assert all(name in table for name in SC.STATISTICS) and "KS" in table
    m.values["fake"] = [fake * torch.tensor([[1.0], [1], [1], [1], [0]], dtype=torch.float64)]       # no generated image scored
    res = m.result()
    assert "length" not in res and res["skipped_fake"] == 4 and "generated" in res["note"] and "generated" in M.format_skeleton(res)
    m.values["fake"], m.values["real"] = m.values["real"], m.values["fake"]                           # and none of the data
    res = m.result()
    assert "length" not in res and res["skipped_real"] == 4 and "data" in res["note"]
    one = M.Skeleton(16, device="cpu")                                        # one image per side: no standard error
    one.values["real"], one.values["fake"], one.count = [real[:, :1]], [fake[:, :1]], {"real": 1, "fake": 1}
    res = one.result()
    assert res["length"]["real_sem"] is None and res["length"]["fake_sem"] is None and "+-" not in M.format_skeleton(res)
    m.count["fake"] = 3
    with pytest.raises(ValueError, match="feed both sets equally"):
        m.result()


def test_flags_and_configuration_names(ngan):
    cfg, train = ngan.config, ngan.train
    names = ("skeleton_period", "skeleton_images", "skeleton_seed", "skeleton_min_size")
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    try:
        assert tuple(cfg.configs_name[n] for n in names) == (0, 8192, 0, 1)
        d = train.build_arg_parser().parse_args([])
        assert tuple(getattr(d, n) for n in names) == (0, 8192, 0, 1)
        none = train.cli_overrides([], d, cfg.configs_name)
        assert not any(k.startswith("skeleton") for k in none)
        argv = ["--skeleton_period", "10", "--skeleton_images", "256", "--skeleton_seed", "7", "--skeleton_min_size", "8"]
        over = train.cli_overrides(argv, train.build_arg_parser().parse_args(argv), cfg.configs_name)
        assert over == {"skeleton_period": 10, "skeleton_images": 256, "skeleton_seed": 7, "skeleton_min_size": 8}
        cfg.set_configs(**over)
        cfg.validate_configs()
        assert tuple(getattr(cfg, n) for n in names) == (10, 256, 7, 8)
        for name, bad in (("skeleton_period", -1), ("skeleton_images", 0), ("skeleton_seed", -3), ("skeleton_min_size", 0),
                          ("skeleton_period", 1.5), ("skeleton_period", True), ("skeleton_min_size", True)):
            cfg.set_configs(**{**over, name: bad})
            with pytest.raises(ValueError, match=name):
                cfg.validate_configs()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    plan = ngan.launch.launch_plan(2, ["--pggan", "--skeleton_period", "10", "--skeleton_min_size", "4", "--gpus", "2"], port=29500, environ={})
    assert all("--skeleton_period 10 --skeleton_min_size 4" in " ".join(argv_i) for argv_i, _ in plan)
    p = ngan.eval.build_arg_parser()
    d = p.parse_args([])
    assert (d.skeleton, d.skeleton_seed, d.skeleton_min_size, d.morph, d.spectrum, d.msssim, d.swd) == (None, 0, 1, None, None, None, None)
    assert p.parse_args(["--skeleton"]).skeleton == 8192
    o = p.parse_args(["--skeleton", "512", "--skeleton_min_size", "4", "--ema", "--dataset_dir", "d", "--swd", "64", "--msssim", "32",
                      "--spectrum", "16", "--morph", "8"])
    assert (o.skeleton, o.skeleton_min_size, o.ema, o.dataset_dir, o.swd, o.msssim, o.spectrum, o.morph) == (512, 4, True, "d", 64, 32, 16, 8)
    assert callable(train.score_skeleton)


def nets(ngan, seed):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([16, 16, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 16, 16], image_size_init=4)
    return G, D


def entry(epoch, ema=False):
    row = {"real": 0.5, "real_sem": 0.01, "fake": 0.25, "fake_sem": None, "ks": 0.75}
    e = {"epoch": epoch, "image_size": 16, "images": 8, "min_size": 1, "skipped_real": 0, "skipped_fake": 1}
    e.update({name: dict(row) for name in SC.STATISTICS})
    if ema:
        e["skipped_fake_ema"] = 0
        e.update({name + "_ema": {"fake": 0.3, "fake_sem": 0.02, "ks": 0.5} for name in SC.STATISTICS})
    return e


def test_checkpoint_list_round_trip(ngan, tmp_path):
    utils = ngan.utils
    G, D = nets(ngan, 1)
    f = str(tmp_path / "GenDisc_s.pth")
    ck = utils.Checkpointer(G, D, 1e-4, f, N_epochs=10, verbose=False)
    ck.save_state(1)
    assert "SKELETON" not in utils.load_checkpoint_dict(f)            # nothing scored: the file of a build without the feature
    entries = [entry(2), entry(4, ema=True), {"epoch": 5, "image_size": 8, "images": 0, "min_size": 1, "skipped_real": 0,
                                              "skipped_fake": 0, "note": "8 x 8 images are below 16 x 16: nothing to thin"}]
    ck.SKELETON.extend(entries)
    ck.save_state(5)
    saved = utils.load_checkpoint_dict(f)                              # the weights-only unpickler accepts the list
    assert saved["SKELETON"] == entries and "MORPH" not in saved and "SPECTRUM" not in saved
    G2, D2 = nets(ngan, 2)
    ck2 = utils.Checkpointer(G2, D2, 1e-4, f, N_epochs=10, verbose=False)
    ck2.load_state()
    assert ck2.SKELETON == entries and ck2.MORPH == [] and ck2.epoch == 5
    ck2.SKELETON.append(entry(6))
    ck2.save_state(6)                                                  # a resumed run continues the list
    assert [e["epoch"] for e in utils.load_checkpoint_dict(f)["SKELETON"]] == [2, 4, 5, 6]
    f0 = str(tmp_path / "GenDisc_0.pth")
    utils.Checkpointer(G, D, 1e-4, f0, N_epochs=10, verbose=False).save_state(3)
    ck3 = utils.Checkpointer(G2, D2, 1e-4, f0, N_epochs=10, verbose=False)
    ck3.load_state()
    assert ck3.SKELETON == [] and ck3.epoch == 3
