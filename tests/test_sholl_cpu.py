"""Arbor geometry without a GPU: the restatement of tests/sholl_cases.py against a brute-force search, scipy and closed forms, what the
metric says on known sets, host-side validation of the three entry points, the bookkeeping of `Sholl.result()`, the configuration names
and flags, and the checkpoint list.  The kernels are tested on the GPU (tests/test_gpu_sholl.py); their integer text also runs serially
on the host (tools/geom_host_check.cpp)."""
import ctypes

import numpy as np
import pytest
import torch

import morph_cases as MC
import multiotsu_ref as OT
import sholl_cases as GC
import skeleton_cases as SC

f64 = np.float64


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (16, 32))
def test_distance_transform_against_the_brute_force_search(size):
    masks, refs = GC.case(size)
    for name, m, (d, soma) in zip(GC.FAMILIES, masks, refs):
        assert np.array_equal(d, GC.edt2_brute(m)), name
        assert not d[m == 0].any() and (d[m != 0] > 0).all(), name
        if m.any():
            assert d[soma[0], soma[1]] == soma[2] == d.max() and soma[0] * size + soma[1] == np.flatnonzero(d.ravel() == d.max())[0], name
        else:
            assert soma == [-1, -1, 0]


@pytest.mark.parametrize("size", (64, 128))
def test_distance_transform_against_scipy(size):
    ndimage = pytest.importorskip("scipy.ndimage")
    masks, refs = GC.case(size)
    for name, m, (d, _) in zip(GC.FAMILIES, masks, refs):
        want = np.rint(ndimage.distance_transform_edt(np.pad(m, 1)) ** 2).astype(np.int64)[1:-1, 1:-1]
        assert np.array_equal(d, want), name


def test_closed_forms():
    for R in (16, 32, 64, 128):
        assert np.array_equal(GC.edt2_ref(GC.family("full", R)), GC.full_ref(R))
        assert np.array_equal(GC.edt2_ref(GC.family("hole", R)), GC.hole_ref(R))
        assert GC.soma_ref(GC.full_ref(R)) == [R // 2 - 1, R // 2 - 1, (R // 2) ** 2]
        hy, hx = GC.hole_at(R)
        assert GC.family("hole", R)[hy, hx] == 0 and int(GC.family("hole", R).sum()) == R * R - 1
    w = GC.edt2_ref(GC.family("wedge", 32))
    assert w[10, 12] == 2 and w[10, 14] == 8 and w[5, 6] == 1                      # the nearest background lies diagonally
    d = GC.edt2_ref(GC.family("two_discs", 64))
    assert d[16, 16] == d[48, 48] == 65 == d.max() and GC.soma_ref(d) == [16, 16, 65]      # 65 = 1 + 64 is the first sum of two squares above 8^2; the tie goes to the smaller index
    for R in (64, 128):                                                              # (at 32 the disc, radius 4, is no wider than the tree's own clumps)
        a = GC.family("soma_arbor", R)
        s = GC.soma_ref(GC.edt2_ref(a))
        assert (s[0] - R // 2) ** 2 + (s[1] - R // 2) ** 2 <= (R // 8) ** 2 and s[2] >= (R // 8) ** 2
        assert (a[SC.family("thick_arbor", R) != 0] == 1).all()
    bar = np.zeros((32, 32), np.uint8)                                               # a bar of odd width w scores calibre w
    bar[14:19, 4:28] = 1
    st = GC.sholl_statistics_ref(bar)
    assert st["soma"] == 3.0 and abs(st["calibre"] - 5.0) < 0.2


def test_ring_index_and_step():
    assert [GC.sholl_step(R) for R in (16, 32, 64, 128, 256, 512, 1024)] == [2, 2, 2, 2, 4, 8, 16]
    for s in (2, 16):
        d2 = np.arange(0, 40000, dtype=np.int64)
        k = GC.ring_index(d2, s)
        assert ((k * s) ** 2 <= d2).all() and (((k + 1) * s) ** 2 > d2).all()
    for R in (16, 32, 64, 128, 256, 512, 1024):                                      # 91 bins hold every ring of every size
        assert int(GC.ring_index(2 * (R - 1) ** 2, GC.sholl_step(R))) <= GC.SHOLL_BINS - 1
    assert int(GC.ring_index(2 * 511 ** 2, 8)) == 90 and int(GC.ring_index(2 * 1023 ** 2, 16)) == 90


def test_crossings_of_known_shapes():
    p = GC.family("plus", 64)
    d = GC.edt2_ref(p)
    soma = GC.soma_ref(d)
    assert soma == [32, 32, 2]                                                       # (the diagonal neighbours of the crossing are off)
    c, roots = GC.sholl_ref(p, d, soma)
    assert c[0] == 0 and c[1:15].tolist() == [4] * 14 and int(c[16:].sum()) == 0
    assert abs(roots - (np.sqrt(2.0) + (int(p.sum()) - 1))) < 1e-12
    for R in (64, 512):
        x = SC.family("cross_x", R)
        c, _ = GC.sholl_ref(x, GC.edt2_ref(x), (0, 0))
        last = int(np.floor(np.sqrt(2.0) * (R - 1) / GC.sholl_step(R)))
        assert np.flatnonzero(c)[-1] == last and c[0] == 0
        if R == 512:
            assert last == GC.SHOLL_BINS - 1                                         # the last bin exists and is reached
    c, roots = GC.sholl_ref(p, d, (-1, -1, 0))
    assert not c.any() and roots == 0.0
    stair = np.zeros((16, 16), np.uint8)                                             # a staircase corner: no diagonal edge
    stair[4, 4] = stair[4, 5] = stair[5, 5] = 1
    assert int(GC.sholl_ref(stair, GC.edt2_ref(stair), (4, 3))[0].sum()) == 1        # (4, 4) - (4, 5) leaves ring 0; (4, 4) - (5, 5) is no edge
    empty = GC.sholl_statistics_ref(np.zeros((16, 16), np.uint8))
    assert not empty["scored"] and empty["reach"] == 0.0 and empty["sholl_radius"] == 0.0 and empty["sholl_peak"] == 0.0


# ---- the metric on known sets --------------------------------------------------------------------------------------------------------------
def test_known_sets_at_64():
    W, fat, cropped = GC.known("W"), GC.known("fat"), GC.known("cropped")
    assert all(s["scored"] for s in W + fat + cropped)
    res = GC.sholl_result_ref(W, fat, 64)
    assert abs(res["calibre"]["real"] - 5.766) < 5e-4 and abs(res["calibre"]["fake"] - 12.073) < 5e-4 and res["calibre"]["ks"] == 1.0
    res = GC.sholl_result_ref(W, cropped, 64)
    assert abs(res["reach"]["real"] - 0.572) < 5e-4 and abs(res["reach"]["fake"] - 0.314) < 5e-4 and res["reach"]["ks"] == 1.0
    prof = res["profile"]
    assert len(prof["radius"]) == len(prof["real"]) == len(prof["fake"]) and prof["radius"][1] == 2 / 64.0
    assert not any(prof["fake"][13:]) and prof["fake"][12] > 0 and (prof["real"][-1] > 0 or prof["fake"][-1] > 0)
    for masks, seed in zip(GC.known_sets(), (5, 6, 7)):
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
    assert {"ngan_geom_workspace_bytes", "ngan_geom_edt", "ngan_geom_sholl"} <= set(ngan._C.exported_symbols())
    calls = {
        "edt": lambda B=1, R=16, p=(one, one, one, one): lib.ngan_geom_edt(*p, B, R, None),
        "sholl": lambda B=1, R=16, p=(one, one, one, one, one): lib.ngan_geom_sholl(*p, B, R, None),
    }
    for name, call in calls.items():
        for r in (8, 24, 2048, 0, -16):
            assert call(R=r) < 0 and f"R={r}".encode() in err() and name.encode() in err(), (name, r)
        for b in (0, -1, 65536):
            assert call(B=b) < 0 and f"B={b}".encode() in err(), (name, b)
    for i in range(4):
        assert calls["edt"](p=tuple(N if j == i else one for j in range(4))) < 0 and b"null" in err()
    for i in range(5):
        assert calls["sholl"](p=tuple(N if j == i else one for j in range(5))) < 0 and b"null" in err()
    for p in ((odd, one, one, one), (one, odd, one, one), (one, one, ctypes.c_void_p(66), one), (one, one, one, odd)):
        assert calls["edt"](p=p) < 0 and b"boundary" in err()
    for p in ((odd, one, one, one, one), (one, odd, one, one, one), (one, one, ctypes.c_void_p(66), one, one),
              (one, one, one, ctypes.c_void_p(66), one), (one, one, one, one, odd)):
        assert calls["sholl"](p=p) < 0 and b"boundary" in err()
    ws = lib.ngan_geom_workspace_bytes
    for R in (16, 64, 512, 1024):
        assert ws(1, R) >= 2 * R * R and ws(3, R) >= 3 * 2 * R * R and ws(3, R) % 16 == 0
    assert [ws(1, r) for r in (8, 24, 2048, 0, -16)] == [0] * 5 and ws(0, 16) == 0 and ws(65536, 16) == 0
    M = ngan.metrics
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)  # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.distance_transform(u8(1, 16, 16))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.sholl_crossings(u8(1, 16, 16), torch.zeros(1, 16, 16, dtype=torch.int32), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(TypeError):
        M.distance_transform(torch.zeros(1, 16, 16))
    with pytest.raises(TypeError):
        M.sholl_crossings(u8(1, 16, 16), torch.zeros(1, 16, 16), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(TypeError):
        M.sholl_crossings(u8(1, 16, 16), torch.zeros(1, 16, 16, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32))
    with pytest.raises(ValueError):
        M.sholl_statistics(torch.zeros(1, 16, 16, 1), otsu_class=4)
    with pytest.raises(ValueError):
        M.sholl_statistics(torch.zeros(1, 16, 16, 1), min_size=0)
    assert M.SHOLL_STATISTICS == GC.STATISTICS and M.SHOLL_BINS == GC.SHOLL_BINS == 91
    assert [M.sholl_step(R) for R in (16, 128, 256, 512, 1024)] == [GC.sholl_step(R) for R in (16, 128, 256, 512, 1024)]
    assert M.SKELETON_STATISTICS == ("length", "tips", "junctions", "width")
    assert M.MORPH_STATISTICS == ("fill", "components", "largest_share", "dimension")


def hand_values(stats, scored, crossings):
    """what Sholl.feed keeps: five statistic rows, `scored`, 91 crossing rows"""
    return torch.cat([torch.tensor(stats, dtype=torch.float64), torch.tensor([scored], dtype=torch.float64),
                      torch.tensor(crossings, dtype=torch.float64).t()])


def test_metric_object_on_the_host(ngan):
    M = ngan.metrics
    m = M.Sholl(64, n_colors=3, device="cpu")
    assert m.active and (m.otsu_class, m.min_size) == (1, 1) and isinstance(m, M.Skeleton)
    with pytest.raises(ValueError, match="feed both sets equally"):
        m.result()
    with pytest.raises(ValueError):
        m.feed("fake", torch.zeros(2, 3, 32, 32))
    for bad in (dict(image_size=48), dict(image_size=64, n_colors=2), dict(image_size=64, otsu_class=0), dict(image_size=64, min_size=0)):
        with pytest.raises(ValueError):
            M.Sholl(**bad)
    small = M.Sholl(8, device="cpu")                                          # 8 x 8: said, not raised, and no number
    small.feed("real", torch.zeros(2, 1, 8, 8))
    res = small.result()
    assert res["images"] == 0 and "calibre" not in res and "profile" not in res and "16 x 16" in res["note"] and "16 x 16" in M.format_sholl(res)
    large = M.Sholl(1024, device="cpu")                                       # above the thinning kernel's 512: the same
    assert not large.active and M.Sholl(512, device="cpu").active and M.Sholl(16, device="cpu").active
    large.feed("fake", torch.zeros(1, 1, 1024, 1024))
    res = large.result()
    assert res["images"] == 0 and "calibre" not in res and "512 x 512" in res["note"] and "512 x 512" in M.format_sholl(res)
    # the bookkeeping of result(), on values filled by hand
    rng = np.random.default_rng(3)
    nan = float("nan")
    real = [[5.5, 6.5, 7.5, 0.0], [9, 8, 7, 0], [4, 6, 9, 0], [0.25, 0.5, 0.125, 0], [0.5, 0.75, 0.625, nan]]
    fake = [[2.5, 2.75, 0.0, 2.9], [3, 4, 0, 5], [1, 2, 0, 2], [0.125, 0.25, 0, 0.0625], [0.25, 0.3125, nan, 0.375]]
    rs, fs = [1, 1, 1, 0], [1, 1, 0, 1]
    rc, fc = rng.integers(0, 12, (4, 91)), rng.integers(0, 7, (4, 91))
    rc[:, 0] = fc[:, 0] = 0
    rc[:3, 40:] = 0                                                          # the last ring either scored side reaches is 47
    fc[[0, 1, 3], 48:] = 0
    fc[:, 47] = 0
    fc[0, 47] = 3
    m = M.Sholl(16, device="cpu")
    vr, vf = hand_values(real, rs, rc), hand_values(fake, fs, fc)
    m.values["real"], m.count["real"] = [vr[:, :1], vr[:, 1:]], 4           # two feeds
    m.values["fake"], m.count["fake"] = [vf], 4
    res = m.result()
    as_ref = lambda t, s, c: [{k: float(t[i][j]) for i, k in enumerate(GC.STATISTICS)} | {"scored": bool(s[j]), "crossings": c[j]}  # noqa: E731
                              for j in range(4)]
    ref = GC.sholl_result_ref(as_ref(real, rs, rc), as_ref(fake, fs, fc), 16)
    assert (res["images"], res["skipped_real"], res["skipped_fake"]) == (4, 1, 1) and set(res) == set(ref)
    for name in GC.STATISTICS:
        assert set(res[name]) == {"real", "real_sem", "fake", "fake_sem", "ks"}
        for k, v in ref[name].items():
            assert abs(res[name][k] - v) < 1e-12, (name, k)
    assert set(res["profile"]) == {"radius", "real", "fake"} and len(res["profile"]["radius"]) == 48
    for k in ("radius", "real", "fake"):
        assert len(res["profile"][k]) == 48 and np.abs(np.array(res["profile"][k]) - np.array(ref["profile"][k])).max() <= 1e-12, k
    assert res["profile"]["fake"][47] == 1.0 and res["profile"]["radius"][47] == 47 * 2 / 16.0
    table = M.format_sholl(res, "T")
    assert table.splitlines()[0].startswith("T (4 images per side; not scored: 1 of the data, 1 generated)") and len(table.splitlines()) == 2 + 5 + 2
    assert all(name in table for name in GC.STATISTICS) and "KS" in table and "profile" in table
    assert len(table.splitlines()[-1].split()) == 1 + 48
    none = M.Sholl(16, device="cpu")                                          # no crossing anywhere: an empty profile
    none.values["real"], none.values["fake"], none.count = [hand_values(real, rs, rc * 0)], [hand_values(fake, fs, fc * 0)], {"real": 4, "fake": 4}
    res0 = none.result()
    assert res0["profile"] == {"radius": [], "real": [], "fake": []} and len(M.format_sholl(res0).splitlines()) == 9
    m.values["fake"] = [hand_values(fake, [0, 0, 0, 0], fc)]                 # no generated image scored
    res = m.result()
    assert "calibre" not in res and "profile" not in res and res["skipped_fake"] == 4 and "generated" in res["note"]
    assert "generated" in M.format_sholl(res)
    m.count["fake"] = 3
    with pytest.raises(ValueError, match="feed both sets equally"):
        m.result()
    sk = M.Skeleton(16, device="cpu")                                         # the two older classes slice their own number of rows
    sk.values["real"], sk.values["fake"], sk.count = [vr[[0, 1, 2, 3, 5]]], [vf[[0, 1, 2, 3, 5]]], {"real": 4, "fake": 4}
    assert sk.result()["length"]["real"] == 6.5 and sk.result()["skipped_fake"] == 1


def test_flags_and_configuration_names(ngan):
    cfg, train = ngan.config, ngan.train
    names = ("sholl_period", "sholl_images", "sholl_seed", "sholl_min_size")
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    try:
        assert tuple(cfg.configs_name[n] for n in names) == (0, 8192, 0, 1)
        d = train.build_arg_parser().parse_args([])
        assert tuple(getattr(d, n) for n in names) == (0, 8192, 0, 1)
        none = train.cli_overrides([], d, cfg.configs_name)
        assert not any(k.startswith("sholl") for k in none)
        argv = ["--sholl_period", "10", "--sholl_images", "256", "--sholl_seed", "7", "--sholl_min_size", "8"]
        over = train.cli_overrides(argv, train.build_arg_parser().parse_args(argv), cfg.configs_name)
        assert over == {"sholl_period": 10, "sholl_images": 256, "sholl_seed": 7, "sholl_min_size": 8}
        cfg.set_configs(**over)
        cfg.validate_configs()
        assert tuple(getattr(cfg, n) for n in names) == (10, 256, 7, 8)
        for name, bad in (("sholl_period", -1), ("sholl_images", 0), ("sholl_seed", -3), ("sholl_min_size", 0),
                          ("sholl_period", 1.5), ("sholl_period", True), ("sholl_min_size", True)):
            cfg.set_configs(**{**over, name: bad})
            with pytest.raises(ValueError, match=name):
                cfg.validate_configs()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    plan = ngan.launch.launch_plan(2, ["--pggan", "--sholl_period", "10", "--sholl_min_size", "4", "--gpus", "2"], port=29500, environ={})
    assert all("--sholl_period 10 --sholl_min_size 4" in " ".join(argv_i) for argv_i, _ in plan)
    p = ngan.eval.build_arg_parser()
    d = p.parse_args([])
    assert (d.sholl, d.sholl_seed, d.sholl_min_size, d.skeleton, d.morph, d.spectrum, d.msssim, d.swd) == (None, 0, 1, None, None, None, None, None)
    assert p.parse_args(["--sholl"]).sholl == 8192
    o = p.parse_args(["--sholl", "512", "--sholl_min_size", "4", "--ema", "--dataset_dir", "d", "--swd", "64", "--msssim", "32",
                      "--spectrum", "16", "--morph", "8", "--skeleton", "4"])
    assert (o.sholl, o.sholl_min_size, o.ema, o.dataset_dir, o.swd, o.msssim, o.spectrum, o.morph, o.skeleton) == (512, 4, True, "d", 64, 32, 16, 8, 4)
    assert callable(train.score_sholl)


def nets(ngan, seed):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([16, 16, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 16, 16], image_size_init=4)
    return G, D


def entry(epoch, ema=False):
    row = {"real": 0.5, "real_sem": 0.01, "fake": 0.25, "fake_sem": None, "ks": 0.75}
    e = {"epoch": epoch, "image_size": 16, "images": 8, "min_size": 1, "skipped_real": 0, "skipped_fake": 1}
    e.update({name: dict(row) for name in GC.STATISTICS})
    e["profile"] = {"radius": [0.0, 0.125, 0.25], "real": [0.0, 2.5, 1.0], "fake": [0.0, 1.25, 0.0]}
    if ema:
        e["skipped_fake_ema"] = 0
        e.update({name + "_ema": {"fake": 0.3, "fake_sem": 0.02, "ks": 0.5} for name in GC.STATISTICS})
        e["profile_ema"] = {"fake": [0.0, 1.5, 0.5]}
    return e


def test_checkpoint_list_round_trip(ngan, tmp_path):
    utils = ngan.utils
    G, D = nets(ngan, 1)
    f = str(tmp_path / "GenDisc_s.pth")
    ck = utils.Checkpointer(G, D, 1e-4, f, N_epochs=10, verbose=False)
    ck.save_state(1)
    assert "SHOLL" not in utils.load_checkpoint_dict(f)               # nothing scored: the file of a build without the feature
    entries = [entry(2), entry(4, ema=True), {"epoch": 5, "image_size": 8, "images": 0, "min_size": 1, "skipped_real": 0,
                                              "skipped_fake": 0, "note": "8 x 8 images are below 16 x 16: nothing to thin"}]
    ck.SHOLL.extend(entries)
    ck.save_state(5)
    saved = utils.load_checkpoint_dict(f)                              # the weights-only unpickler accepts the list
    assert saved["SHOLL"] == entries and "SKELETON" not in saved and "MORPH" not in saved
    G2, D2 = nets(ngan, 2)
    ck2 = utils.Checkpointer(G2, D2, 1e-4, f, N_epochs=10, verbose=False)
    ck2.load_state()
    assert ck2.SHOLL == entries and ck2.SKELETON == [] and ck2.epoch == 5
    ck2.SHOLL.append(entry(6))
    ck2.save_state(6)                                                  # a resumed run continues the list
    assert [e["epoch"] for e in utils.load_checkpoint_dict(f)["SHOLL"]] == [2, 4, 5, 6]
    f0 = str(tmp_path / "GenDisc_0.pth")
    utils.Checkpointer(G, D, 1e-4, f0, N_epochs=10, verbose=False).save_state(3)
    ck3 = utils.Checkpointer(G2, D2, 1e-4, f0, N_epochs=10, verbose=False)
    ck3.load_state()
    assert ck3.SHOLL == [] and ck3.epoch == 3
