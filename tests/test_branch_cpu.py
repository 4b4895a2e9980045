"""Arbor branches without a GPU: the restatement of tests/branch_cases.py on shapes whose answer is known, its identities on every
family, the host-side checks of the two entry points, the bookkeeping of metrics.Branches on values filled by hand, the flags and the
checkpoint list."""
import ctypes
import math

import numpy as np
import pytest
import torch

import branch_cases as BC
import morph_cases as MC
import multiotsu_ref as OT
import skeleton_cases as SC

S = {name: i for i, name in enumerate(BC.STAT_NAMES)}


def stats_of(name, R, spur=1):
    return dict(zip(BC.STAT_NAMES, (int(v) for v in BC.graph_ref(BC.family(name, R), spur)[1])))


# ---- the restatement on known shapes ---------------------------------------------------------------------------------------------------------
def test_known_shapes():
    s = stats_of("plus", 32)                                                  # arms from 2 to 29 through (16, 16): 13, 13, 14 and 14 pixels
    assert (s["nodes"], s["node_pixels"], s["forks"], s["terminal"], s["links"], s["free"], s["spurs"]) == (1, 1, 1, 4, 0, 0, 0)
    assert s["term_orth"] / s["terminal"] == 13.5 and s["term_diag"] == 0 and s["longest"] == 14
    st = BC.statistics_of(32, 1, BC.graph_ref(BC.family("plus", 32), 1)[1], np.zeros(64))
    assert st["terminal_length"] == 13.5 / 32 and st["link_length"] == 0.0 and st["longest"] == 14 / 32 and st["scored"]
    labels, _, hist = BC.graph_ref(BC.family("plus", 32), 1)
    assert labels[16, 16] == -2 - (16 * 32 + 16) and labels[2, 16] == 2 * 32 + 16 and labels[16, 2] == 16 * 32 + 2 and labels[0, 0] == -1
    assert labels[29, 16] == 17 * 32 + 16 and hist[13] == 2 and hist[14] == 2 and hist.sum() == 4
    for R in (16, 32, 64):
        s = stats_of("cross_x", R)                                            # the four pixels round the centre see three edges each
        assert (s["nodes"], s["node_pixels"], s["forks"], s["terminal"], s["node_orth"], s["node_diag"]) == (1, 4, 1, 4, 4, 0)
        assert SC.counts_ref(SC.family("cross_x", R))[2] == 0                 # where the per-pixel junction count sees none
        s = stats_of("checkerboard", R)
        assert s["nodes"] == 1 and s["node_pixels"] == SC.counts_ref(SC.family("checkerboard", R))[2] > 1 and s["forks"] == 1
        s = stats_of("rings", R)
        assert s["branches"] == s["free"] == R // 4 and s["nodes"] == s["terminal"] == s["links"] == s["spurs"] == s["forks"] == 0
        s = stats_of("tee", R)
        assert (s["nodes"], s["terminal"], s["forks"]) == (1, 3, 1)
        s = stats_of("single", R)
        assert (s["pixels"], s["branches"], s["free"], s["longest"]) == (1, 1, 1, 0)
        assert not BC.graph_ref(BC.family("empty", R), 1)[1].any()
    s = stats_of("loop", 32)                                                  # the ring is one link from the corner node back to itself
    assert (s["nodes"], s["links"], s["terminal"], s["forks"], s["link_orth"], s["term_orth"]) == (1, 1, 1, 1, 60, 6)
    assert stats_of("loop", 32, spur=8)["forks"] == 0 and stats_of("loop", 32, spur=8)["spurs"] == 1      # the tail pruned: two attachments left
    s = stats_of("double_t", 32)
    assert (s["nodes"], s["links"], s["terminal"], s["forks"], s["link_orth"]) == (2, 1, 4, 2, 3)
    arbor = dict(zip(BC.STAT_NAMES, BC.graph_ref(BC.family("thin:arbor", 64), 1)[1]))
    assert (arbor["node_pixels"], arbor["nodes"], arbor["terminal"]) == (128, 61, 21)
    assert SC.counts_ref(BC.family("thin:arbor", 64))[2] == 117
    short = sum(b["a"] == 1 and b["n"] < 4 for b in BC.structure(BC.family("thin:arbor", 64)).branches.values())
    assert short == 16 == BC.graph_ref(BC.family("thin:arbor", 64), 4)[1][S["spurs"]]


def test_burrs_lose_forks_as_spur_rises():
    for R in (32, 64, 128):
        rows = [stats_of("burrs", R, spur) for spur in (1, 2, 3, 4)]
        forks = [r["forks"] for r in rows]
        assert forks[0] > forks[1] > forks[2] > forks[3] == 1, (R, forks)     # only the crossing survives every stub's pruning
        assert [r["spurs"] for r in rows] == sorted(r["spurs"] for r in rows) and rows[0]["spurs"] == 0
        assert all(r["terminal"] + r["spurs"] == rows[0]["terminal"] for r in rows)      # pruning only moves branches between the two
        assert len({r["nodes"] for r in rows}) == 1 and rows[0]["forks"] == rows[0]["nodes"]
    seam = BC.family("seam", 128)
    assert seam[63, 63] and seam[63, 64] and seam[64, 63] and BC.graph_ref(seam, 1)[0][63, 63] == -2 - (63 * 128 + 63)


@pytest.mark.parametrize("size", (16, 32, 64))
def test_identities_on_every_family(size):
    for name, mask in zip(BC.FAMILIES, BC.case(size)):
        counts = SC.counts_ref(mask)
        st = BC.structure(mask)
        for b in st.branches.values():                                        # a simple path or a cycle, at most two attachments
            assert b["a"] <= 2 and all(v <= 2 for v in b["inner"].values()), (name, size)
            assert b["edges"] in (b["n"] - 1, b["n"]) and (b["edges"] == b["n"] - 1 or (b["a"] == 0 and b["n"] >= 3)), (name, size)
            assert b["o"] + b["d"] == b["edges"] + b["a"]
        for spur in (1, 2, 4):
            labels, s, hist = BC.graph_ref(mask, spur)
            assert s[S["branches"]] == s[S["terminal"]] + s[S["links"]] + s[S["free"]] + s[S["spurs"]], (name, size, spur)
            assert s[[8, 10, 12, 14, 16]].sum() == counts[4] and s[[9, 11, 13, 15, 17]].sum() == counts[5], (name, size, spur)
            assert s[S["pixels"]] == counts[0] and hist.sum() == s[S["terminal"]] + s[S["links"]] and s[S["forks"]] <= s[S["nodes"]]
            assert (labels >= 0).sum() + (labels <= -2).sum() == counts[0] and (labels <= -2).sum() == s[S["node_pixels"]]
            assert len(np.unique(labels[labels >= 0])) == s[S["branches"]] and len(np.unique(labels[labels <= -2])) == s[S["nodes"]]


def test_separation_sets_are_what_the_gpu_test_takes_them_for():
    """the images' class above t0 is the mask, and the reference says what the GPU test asserts"""
    W, burred = BC.separation_sets()
    for masks, seed in ((W, 5), (burred, 6)):
        img, _ = MC.mask_images(masks, seed)
        for i, m in zip(img, masks):
            t0 = OT.multiotsu4(np.bincount(i.ravel(), minlength=256))[0][0]
            assert 20 <= t0 <= 89 and np.array_equal(i > t0, m != 0)
    for spur in (None, 4):
        ref = BC.branches_ref([BC.branch_statistics_ref(x, spur=spur) for x in W], [BC.branch_statistics_ref(x, spur=spur) for x in burred], 64)
        assert ref["spurs"]["ks"] == 1.0 and ref["nodes"]["ks"] == 1.0
    assert abs(ref["forks"]["fake"] - ref["forks"]["real"]) < 1.0 and ref["nodes"]["fake"] > 2 * ref["nodes"]["real"]


# ---- the library on the host ---------------------------------------------------------------------------------------------------------------
def test_isqrt_of_the_shared_text():
    """the reference's math.isqrt against the bit-by-bit root of branch_bits.h, restated here line for line"""
    def isqrt(v):
        r, bit = 0, 1 << 62
        while bit:
            if v >= r + bit:
                v -= r + bit
                r = (r >> 1) + bit
            else:
                r >>= 1
            bit >>= 2
        return r
    ds = list(range(0, 4097)) + [2 ** k + j for k in range(12, 19) for j in (-1, 0, 1) if 2 ** k + j <= 2 ** 18] + list(range(2 ** 18 - 64, 2 ** 18 + 1))
    rng = np.random.default_rng(1)
    ds += [int(v) for v in rng.integers(0, 2 ** 18 + 1, 4096)]
    for d in ds:
        assert isqrt(2 * d * d) == math.isqrt(2 * d * d) == BC.floor_length(0, d), d
    assert isqrt(2 ** 64 - 1) == 2 ** 32 - 1


def test_entry_points_are_bound_and_validate_on_the_host(ngan):
    lib = ngan._C.lib()
    one = ctypes.c_void_p(64)            # any aligned non-null address: every check below comes before the launch
    odd = ctypes.c_void_p(68)
    N = None
    err = lambda: lib.ngan_last_error()  # noqa: E731
    assert {"ngan_branch_workspace_bytes", "ngan_branch_graph"} <= set(ngan._C.exported_symbols())
    call = lambda B=1, R=16, spur=1, p=(one, one, one, one, one): lib.ngan_branch_graph(*p, B, R, spur, None)  # noqa: E731
    for r in (8, 24, 1024, 2048, 0, -16):
        assert call(R=r) == -2 and f"R={r}".encode() in err() and b"branch_graph" in err(), r
    for b in (0, -1, 65536):
        assert call(B=b) == -2 and f"B={b}".encode() in err(), b
    for spur in (0, -1):
        assert call(spur=spur) == -1 and f"spur={spur}".encode() in err()
    for i in (0, 2, 3, 4):                                                    # labels alone may be null
        assert call(p=tuple(N if j == i else one for j in range(5))) == -1 and b"null" in err()
    for p in ((odd, one, one, one, one), (one, odd, one, one, one), (one, one, ctypes.c_void_p(66), one, one),
              (one, one, one, ctypes.c_void_p(66), one), (one, one, one, one, odd)):
        assert call(p=p) == -1 and b"boundary" in err()
    ws = lib.ngan_branch_workspace_bytes
    for R in (16, 64, 512):
        assert ws(1, R) == 13 * R * R and ws(3, R) == 3 * 13 * R * R and ws(3, R) % 16 == 0
    assert [ws(1, r) for r in (8, 24, 1024, 0, -16)] == [0] * 5 and ws(0, 16) == 0 and ws(65536, 16) == 0
    M = ngan.metrics
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)  # noqa: E731
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.branch_graph(u8(1, 16, 16))
    with pytest.raises(TypeError):
        M.branch_graph(torch.zeros(1, 16, 16))
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="spur"):
            M.branch_graph(u8(1, 16, 16), spur=bad)
    for r in (8, 1024):
        with pytest.raises(ValueError, match="16 .. 512"):
            M.branch_graph(u8(1, r, r))
    with pytest.raises(ValueError):
        M.branch_statistics(torch.zeros(1, 16, 16, 1), otsu_class=4)
    with pytest.raises(ValueError):
        M.branch_statistics(torch.zeros(1, 16, 16, 1), min_size=0)
    with pytest.raises(ValueError, match="spur"):
        M.branch_statistics(torch.zeros(1, 16, 16, 1), spur=0)
    assert M.BRANCH_STATISTICS == BC.STATISTICS == ("forks", "nodes", "terminals", "spurs", "terminal_length", "link_length", "longest")
    assert M.BRANCH_BINS == BC.BINS == 64 and M.BRANCH_STATS == BC.STAT_NAMES
    assert [M.default_spur(R) for R in (16, 32, 64, 128, 512)] == [BC.default_spur(R) for R in (16, 32, 64, 128, 512)] == [2, 2, 2, 4, 16]
    assert M.SHOLL_STATISTICS == ("calibre", "soma", "sholl_peak", "sholl_radius", "reach")
    assert M.SKELETON_STATISTICS == ("length", "tips", "junctions", "width")


def hand_values(stats, scored, hist):
    """what Branches.feed keeps: seven statistic rows, `scored`, 64 histogram rows"""
    return torch.cat([torch.tensor(stats, dtype=torch.float64), torch.tensor([scored], dtype=torch.float64),
                      torch.tensor(hist, dtype=torch.float64).t()])


def test_metric_object_on_the_host(ngan):
    M = ngan.metrics
    m = M.Branches(64, n_colors=3, device="cpu")
    assert m.active and (m.otsu_class, m.min_size, m.spur) == (1, 1, 2) and isinstance(m, M.Skeleton)
    assert M.Branches(512, device="cpu").spur == 16 and M.Branches(512, device="cpu", spur=5).spur == 5
    with pytest.raises(ValueError, match="feed both sets equally"):
        m.result()
    with pytest.raises(ValueError):
        m.feed("fake", torch.zeros(2, 3, 32, 32))
    for bad in (dict(image_size=48), dict(image_size=64, n_colors=2), dict(image_size=64, otsu_class=0), dict(image_size=64, min_size=0),
                dict(image_size=64, spur=0), dict(image_size=64, spur=2.0), dict(image_size=64, spur=True)):
        with pytest.raises(ValueError):
            M.Branches(**bad)
    small = M.Branches(8, device="cpu")                                       # 8 x 8: said, not raised, and no number
    small.feed("real", torch.zeros(2, 1, 8, 8))
    res = small.result()
    assert res["images"] == 0 and "forks" not in res and "profile" not in res and "16 x 16" in res["note"] and "16 x 16" in M.format_branches(res)
    large = M.Branches(1024, device="cpu")                                    # above the thinning kernel's 512: the same
    assert not large.active and M.Branches(512, device="cpu").active and M.Branches(16, device="cpu").active
    large.feed("fake", torch.zeros(1, 1, 1024, 1024))
    res = large.result()
    assert res["images"] == 0 and "forks" not in res and "512 x 512" in res["note"] and "512 x 512" in M.format_branches(res)
    # the bookkeeping of result(), on values filled by hand
    rng = np.random.default_rng(3)
    real = [[5, 6, 7, 0], [9, 8, 7, 0], [4, 6, 9, 0], [1, 0, 2, 0], [0.25, 0.5, 0.125, 0], [0.5, 0.75, 0.625, 0], [0.5, 0.75, 0.625, 0]]
    fake = [[2, 3, 0, 2], [3, 4, 0, 5], [1, 2, 0, 2], [7, 9, 0, 8], [0.125, 0.25, 0, 0.0625], [0.25, 0.3125, 0, 0.375], [0.3, 0.4, 0, 0.5]]
    rs, fs = [1, 1, 1, 0], [1, 1, 0, 1]
    rc, fc = rng.integers(0, 12, (4, 64)), rng.integers(0, 7, (4, 64))
    rc[:3, 30:] = 0                                                          # the last bin either scored side fills is 41
    fc[[0, 1, 3], 42:] = 0
    fc[:, 41] = 0
    fc[0, 41] = 3
    m = M.Branches(256, device="cpu")
    vr, vf = hand_values(real, rs, rc), hand_values(fake, fs, fc)
    m.values["real"], m.count["real"] = [vr[:, :1], vr[:, 1:]], 4           # two feeds
    m.values["fake"], m.count["fake"] = [vf], 4
    res = m.result()
    as_ref = lambda t, s, c: [{k: float(t[i][j]) for i, k in enumerate(BC.STATISTICS)} | {"scored": bool(s[j]), "hist": c[j]}  # noqa: E731
                              for j in range(4)]
    ref = BC.branches_ref(as_ref(real, rs, rc), as_ref(fake, fs, fc), 256)
    assert (res["images"], res["skipped_real"], res["skipped_fake"]) == (4, 1, 1) and set(res) == set(ref)
    for name in BC.STATISTICS:
        assert set(res[name]) == {"real", "real_sem", "fake", "fake_sem", "ks"}
        for k, v in ref[name].items():
            assert abs(res[name][k] - v) < 1e-12, (name, k)
    assert set(res["profile"]) == {"length", "real", "fake"}
    for k in ("length", "real", "fake"):
        assert len(res["profile"][k]) == 42 and np.abs(np.array(res["profile"][k]) - np.array(ref["profile"][k])).max() <= 1e-12, k
    assert res["profile"]["fake"][41] == 1.0 and res["profile"]["length"][41] == 41 * 2 / 256.0             # bins 2 pixels wide at 256
    table = M.format_branches(res, "T")
    assert table.splitlines()[0].startswith("T (4 images per side; not scored: 1 of the data, 1 generated)") and len(table.splitlines()) == 2 + 7 + 2
    assert all(name in table for name in BC.STATISTICS) and "KS" in table and "profile" in table
    assert len(table.splitlines()[-1].split()) == 1 + 42
    assert M.format_branches(res).startswith("Arbor branches (")
    none = M.Branches(16, device="cpu")                                       # no terminal or link branch anywhere: an empty profile
    none.values["real"], none.values["fake"], none.count = [hand_values(real, rs, rc * 0)], [hand_values(fake, fs, fc * 0)], {"real": 4, "fake": 4}
    res0 = none.result()
    assert res0["profile"] == {"length": [], "real": [], "fake": []} and len(M.format_branches(res0).splitlines()) == 11
    m.values["fake"] = [hand_values(fake, [0, 0, 0, 0], fc)]                 # no generated image scored
    res = m.result()
    assert "forks" not in res and "profile" not in res and res["skipped_fake"] == 4 and "generated" in res["note"]
    assert "generated" in M.format_branches(res)
    m.count["fake"] = 3
    with pytest.raises(ValueError, match="feed both sets equally"):
        m.result()


def test_feed_with_stubbed_statistics(ngan):
    """feed() -> _rows() -> result() on the host, the kernels replaced by a table: images that are not scored are skipped in every
    statistic and in the profile, which is cut after the last bin either side fills"""
    M = ngan.metrics
    table = {}

    class Stub(M.Branches):
        def _statistics(self, x):
            rows = [table[float(v)] for v in x[:, 0, 0, 0]]
            out = {name: torch.tensor([r[0][i] for r in rows], dtype=torch.float64) for i, name in enumerate(M.BRANCH_STATISTICS)}
            out["scored"] = torch.tensor([r[1] for r in rows])
            out["hist"] = torch.tensor([r[2] for r in rows], dtype=torch.int32)
            return out
    rng = np.random.default_rng(11)
    refs = {"real": [], "fake": []}
    images = {"real": torch.zeros(5, 1, 16, 16), "fake": torch.zeros(5, 1, 16, 16)}
    for which in ("real", "fake"):
        for j in range(5):
            key = float(j + (10 if which == "fake" else 0))
            hist = rng.integers(0, 5, 64)
            hist[20 if which == "real" else 27:] = 0
            scored = not (which == "real" and j == 1) and not (which == "fake" and j in (0, 4))
            if not scored:
                hist[40] = 9                                                  # would lengthen the profile if it were counted
            stats = [float(v) for v in rng.integers(0, 30, 4)] + [float(v) for v in rng.random(3)]
            table[key] = (stats, scored, hist.tolist())
            images[which][j] = key
            refs[which].append(dict(zip(BC.STATISTICS, stats)) | {"scored": scored, "hist": hist})
    m = Stub(16, device="cpu")
    for lo, hi in ((0, 2), (2, 5)):
        m.feed("real", images["real"][lo:hi])
        m.feed("fake", images["fake"][lo:hi].permute(0, 2, 3, 1).contiguous())       # channels-last is taken as it is
    res, ref = m.result(), BC.branches_ref(refs["real"], refs["fake"], 16)
    assert (res["images"], res["skipped_real"], res["skipped_fake"]) == (5, 1, 2) == (ref["images"], ref["skipped_real"], ref["skipped_fake"])
    for name in BC.STATISTICS:
        for k, v in ref[name].items():
            assert abs(res[name][k] - v) < 1e-12, (name, k)
    assert len(res["profile"]["length"]) == len(ref["profile"]["length"]) <= 27
    for k in ("length", "real", "fake"):
        assert np.abs(np.array(res["profile"][k]) - np.array(ref["profile"][k])).max() <= 1e-12, k
    assert res["profile"]["length"][1] == 1 / 16.0                            # bins one pixel wide below 256


class _Net(torch.nn.Module):
    """what _evaluate_two_sets asks of a generator; it is never run: every call below ends before the first minibatch"""
    image_size, latent_dim, N_colors = 64, 8, 1

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))


def test_real_from_must_match_spur(ngan):
    M = ngan.metrics
    G = _Net()
    fed = M.Branches(64, device="cpu", spur=3)
    fed.count["real"], fed.values["real"] = 4, [torch.zeros(8 + 64, 4, dtype=torch.float64)]
    for kw in (dict(spur=4), dict(spur=None), dict(spur=3, min_size=2), dict(spur=3, n_images=5)):
        with pytest.raises(ValueError, match="other settings"):
            M.evaluate_branches(G, None, **{"n_images": 4, "batch_size": 2, "real_from": fed, **kw})
    with pytest.raises(ValueError, match="other settings"):                   # another class's data side has no spur at all
        sk = M.Skeleton(64, device="cpu")
        sk.count["real"] = 4
        M.evaluate_branches(G, None, n_images=4, batch_size=2, real_from=sk, spur=3)
    with pytest.raises(ValueError, match="spur"):
        M.evaluate_branches(G, None, n_images=4, spur=0)
    below = _Net()
    below.image_size = 8
    res, metric = M.evaluate_branches(below, None, n_images=4, return_metric=True)
    assert "16 x 16" in res["note"] and isinstance(metric, M.Branches)


def test_flags_and_configuration_names(ngan):
    cfg, train = ngan.config, ngan.train
    names = ("branch_period", "branch_images", "branch_seed", "branch_min_size", "branch_spur")
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    try:
        assert tuple(cfg.configs_name[n] for n in names) == (0, 8192, 0, 1, 0)
        d = train.build_arg_parser().parse_args([])
        assert tuple(getattr(d, n) for n in names) == (0, 8192, 0, 1, 0)
        none = train.cli_overrides([], d, cfg.configs_name)
        assert not any(k.startswith("branch") for k in none)
        argv = ["--branch_period", "10", "--branch_images", "256", "--branch_seed", "7", "--branch_min_size", "8", "--branch_spur", "5"]
        over = train.cli_overrides(argv, train.build_arg_parser().parse_args(argv), cfg.configs_name)
        assert over == {"branch_period": 10, "branch_images": 256, "branch_seed": 7, "branch_min_size": 8, "branch_spur": 5}
        cfg.set_configs(**over)
        cfg.validate_configs()
        assert tuple(getattr(cfg, n) for n in names) == (10, 256, 7, 8, 5)
        for name, bad in (("branch_period", -1), ("branch_images", 0), ("branch_seed", -3), ("branch_min_size", 0), ("branch_spur", -1),
                          ("branch_period", 1.5), ("branch_period", True), ("branch_spur", True), ("branch_spur", 2.0)):
            cfg.set_configs(**{**over, name: bad})
            with pytest.raises(ValueError, match=name):
                cfg.validate_configs()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    plan = ngan.launch.launch_plan(2, ["--pggan", "--branch_period", "10", "--branch_spur", "4", "--gpus", "2"], port=29500, environ={})
    assert all("--branch_period 10 --branch_spur 4" in " ".join(argv_i) for argv_i, _ in plan)
    p = ngan.eval.build_arg_parser()
    d = p.parse_args([])
    assert (d.branches, d.branch_seed, d.branch_min_size, d.branch_spur, d.sholl, d.skeleton, d.morph) == (None, 0, 1, 0, None, None, None)
    assert p.parse_args(["--branches"]).branches == 8192
    o = p.parse_args(["--branches", "512", "--branch_min_size", "4", "--branch_spur", "6", "--ema", "--dataset_dir", "d", "--sholl", "64"])
    assert (o.branches, o.branch_min_size, o.branch_spur, o.ema, o.dataset_dir, o.sholl) == (512, 4, 6, True, "d", 64)
    assert callable(train.score_branches)


def nets(ngan, seed):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([16, 16, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 16, 16], image_size_init=4)
    return G, D


def entry(epoch, ema=False):
    row = {"real": 0.5, "real_sem": 0.01, "fake": 0.25, "fake_sem": None, "ks": 0.75}
    e = {"epoch": epoch, "image_size": 16, "images": 8, "min_size": 1, "spur": 2, "skipped_real": 0, "skipped_fake": 1}
    e.update({name: dict(row) for name in BC.STATISTICS})
    e["profile"] = {"length": [0.0, 0.0625, 0.125], "real": [0.0, 2.5, 1.0], "fake": [0.0, 1.25, 0.0]}
    if ema:
        e["skipped_fake_ema"] = 0
        e.update({name + "_ema": {"fake": 0.3, "fake_sem": 0.02, "ks": 0.5} for name in BC.STATISTICS})
        e["profile_ema"] = {"fake": [0.0, 1.5, 0.5]}
    return e


def test_checkpoint_list_round_trip(ngan, tmp_path):
    utils = ngan.utils
    assert utils.BRANCH_KEY == "BRANCH"
    G, D = nets(ngan, 1)
    f = str(tmp_path / "GenDisc_b.pth")
    ck = utils.Checkpointer(G, D, 1e-4, f, N_epochs=10, verbose=False)
    ck.save_state(1)
    assert "BRANCH" not in utils.load_checkpoint_dict(f)              # nothing scored: the file of a build without the feature
    entries = [entry(2), entry(4, ema=True), {"epoch": 5, "image_size": 8, "images": 0, "min_size": 1, "spur": 2, "skipped_real": 0,
                                              "skipped_fake": 0, "note": "8 x 8 images are below 16 x 16: nothing to thin"}]
    ck.BRANCH.extend(entries)
    ck.save_state(5)
    saved = utils.load_checkpoint_dict(f)                              # the weights-only unpickler accepts the list
    assert saved["BRANCH"] == entries and "SHOLL" not in saved and "SKELETON" not in saved
    G2, D2 = nets(ngan, 2)
    ck2 = utils.Checkpointer(G2, D2, 1e-4, f, N_epochs=10, verbose=False)
    ck2.load_state()
    assert ck2.BRANCH == entries and ck2.SHOLL == [] and ck2.epoch == 5
    ck2.BRANCH.append(entry(6))
    ck2.save_state(6)                                                  # a resumed run continues the list
    assert [e["epoch"] for e in utils.load_checkpoint_dict(f)["BRANCH"]] == [2, 4, 5, 6]
    f0 = str(tmp_path / "GenDisc_0.pth")
    utils.Checkpointer(G, D, 1e-4, f0, N_epochs=10, verbose=False).save_state(3)
    ck3 = utils.Checkpointer(G2, D2, 1e-4, f0, N_epochs=10, verbose=False)
    ck3.load_state()
    assert ck3.BRANCH == [] and ck3.epoch == 3
