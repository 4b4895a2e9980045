"""Arbor geometry on the GPU: the kernels of csrc/sholl.hip against the numpy restatement of tests/sholl_cases.py (definitions and mask
families are described there), the metric on known sets, `evaluate_sholl`, and its promise to leave a run alone.  Every kernel output but
`roots` is an integer and is compared exactly.  `roots` and the fp64 summaries formed on the Python side are held to 1e-12 relative, the
skeleton tests' tolerance: a partial sum of the kernel holds at most R^2 / 256 + 8 fp64 additions of positive terms, whatever their
partition each relative error is below (1024 + 8) * 2^-53 = 1.2e-13, and numpy's own pairwise sum is closer still."""
import types

import numpy as np
import pytest
import torch

import morph_cases as MC
import multiotsu_ref as OT
import sholl_cases as GC
import skeleton_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-12


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def close(a, b):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= RTOL * max(1.0, abs(b))


def check_transform(M, masks, refs, names, tag):
    """dist2 and soma of a batch against the reference pairs; returns the two tensors"""
    dist2, soma = M.distance_transform(dev(masks))
    n, R = masks.shape[0], masks.shape[1]
    assert tuple(dist2.shape) == (n, R, R) and dist2.dtype == torch.int32 and tuple(soma.shape) == (n, 3) and soma.dtype == torch.int32
    got_d, got_s = dist2.cpu().numpy(), soma.cpu().numpy()
    for i, (name, (d, s)) in enumerate(zip(names, refs)):
        assert np.array_equal(got_d[i], d), f"{tag} {name}: {(got_d[i] != d).sum()} squared distances differ"
        assert got_s[i].tolist() == s, f"{tag} {name}: soma {got_s[i].tolist()} != {s}"
    return dist2, soma


# ---- the transform and the soma against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("size", GC.SIZES)
def test_transform_against_the_restatement(ngan, size):
    """every family in one batch (16: sixteen rows per workgroup of the row pass, 128: two); then 3 images and 1 image of the same, a
    second call, other non-zero bytes, and a call straight into the middle of a guarded buffer"""
    M = ngan.metrics
    masks, refs = GC.case(size)
    tag = f"R={size}"
    dist2, soma = check_transform(M, masks, refs, GC.FAMILIES, tag)
    for n in (3, 1):
        d, s = M.distance_transform(dev(masks[:n]))
        assert torch.equal(d, dist2[:n]) and torch.equal(s, soma[:n]), f"{tag} B={n}: an image's values depend on the rest of the batch"
    d, s = M.distance_transform(dev(masks))
    assert torch.equal(d, dist2) and torch.equal(s, soma), f"{tag}: two calls differ"
    d, s = M.distance_transform(dev(masks * 255))                                                 # any non-zero byte is foreground
    assert torch.equal(d, dist2) and torch.equal(s, soma)
    lib = ngan._C.lib()
    n = len(masks)
    guarded = torch.full((n + 2, size, size), -7, device=DEV, dtype=torch.int32)                  # one slot of guard before and after
    soma_g = torch.full((n + 2, 3), -7, device=DEV, dtype=torch.int32)
    ws = torch.empty(lib.ngan_geom_workspace_bytes(n, size), device=DEV, dtype=torch.uint8)
    src = dev(masks)
    assert lib.ngan_geom_edt(src.data_ptr(), guarded[1].data_ptr(), soma_g[1].data_ptr(), ws.data_ptr(), n, size,
                             torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(guarded[1:-1], dist2) and torch.equal(soma_g[1:-1], soma)
    assert bool((guarded[0] == -7).all()) and bool((guarded[-1] == -7).all()) and bool((soma_g[0] == -7).all()) and bool((soma_g[-1] == -7).all())


def test_transform_at_512(ngan):
    """the workload's size: one row per workgroup of 512 threads; `full` walks 256 steps per pixel in the middle"""
    M = ngan.metrics
    arbor = GC.family("thick_arbor", 512)
    d = GC.edt2_ref(arbor)
    masks = np.stack([arbor, GC.family("full", 512), GC.family("hole", 512)])
    refs = [(d, GC.soma_ref(d))] + [(x, GC.soma_ref(x)) for x in (GC.full_ref(512), GC.hole_ref(512))]
    check_transform(M, masks, refs, ("thick_arbor", "full", "hole"), "R=512")


def test_transform_at_1024(ngan):
    """the largest image: 1024 threads per row, column distances up to 512"""
    M = ngan.metrics
    masks = np.stack([GC.family("full", 1024), GC.family("hole", 1024)])
    refs = [(x, GC.soma_ref(x)) for x in (GC.full_ref(1024), GC.hole_ref(1024))]
    _, soma = check_transform(M, masks, refs, ("full", "hole"), "R=1024")
    assert soma[0].tolist() == [511, 511, 512 * 512]


# ---- the crossings against the restatement ------------------------------------------------------------------------------------------------
def check_crossings(M, skeletons, dist2, centres, names, tag):
    crossings, roots = M.sholl_crossings(dev(skeletons), dev(dist2, torch.int32), dev(np.asarray(centres), torch.int32))
    n = len(skeletons)
    assert tuple(crossings.shape) == (n, GC.SHOLL_BINS) and crossings.dtype == torch.int32 and tuple(roots.shape) == (n,) and roots.dtype == torch.float64
    got_c, got_r = crossings.cpu().numpy(), roots.cpu().numpy()
    for i, name in enumerate(names):
        c, r = GC.sholl_ref(skeletons[i], dist2[i], centres[i])
        assert got_c[i].tolist() == c.tolist(), f"{tag} {name} about {list(centres[i][:2])}: crossings {got_c[i].tolist()} != {c.tolist()}"
        assert abs(got_r[i] - r) <= RTOL * max(1.0, r), f"{tag} {name}: roots {got_r[i]!r} != {r!r}"
    return crossings, roots


@pytest.mark.parametrize("size", GC.SIZES)
def test_crossings_against_the_restatement(ngan, size):
    """the thinned families about their own soma, about the first pixel and about the last (`cross_x` then reaches the last ring the
    size has); the unthinned ones too; a second call; 3 images and 1 image of the batch"""
    M = ngan.metrics
    masks, refs = GC.case(size)
    skeletons = M.thin(dev(masks))[0].cpu().numpy()                       # (the thinning has its own tests)
    dist2 = np.stack([d for d, _ in refs])
    somas = [s for _, s in refs]
    tag = f"R={size}"
    first, roots = check_crossings(M, skeletons, dist2, somas, GC.FAMILIES, tag)
    assert not bool(first[:, 0].any()) and not bool(first[GC.FAMILIES.index("empty")].any())
    for corner in ((0, 0, 0), (size - 1, size - 1, 0)):
        c, _ = check_crossings(M, skeletons, dist2, [list(corner)] * len(masks), GC.FAMILIES, tag)
        last = int(np.floor(np.sqrt(2.0) * (size - 1) / GC.sholl_step(size)))
        row = c[GC.FAMILIES.index("cross_x")].cpu().numpy()
        assert np.flatnonzero(row)[-1] == last, f"{tag}: cross_x about {corner[:2]} ends in ring {np.flatnonzero(row)[-1]}, not {last}"
    check_crossings(M, masks, dist2, somas, GC.FAMILIES, tag + " unthinned")
    args = (dev(skeletons), dev(dist2, torch.int32), dev(np.asarray(somas), torch.int32))
    again = M.sholl_crossings(*args)
    assert torch.equal(again[0], first) and torch.equal(again[1], roots), f"{tag}: two calls differ"
    for n in (3, 1):
        c, r = M.sholl_crossings(*(a[:n].contiguous() for a in args))
        assert torch.equal(c, first[:n]) and torch.equal(r, roots[:n]), f"{tag} B={n}: an image's values depend on the rest of the batch"


def test_crossings_at_512_and_1024(ngan):
    M = ngan.metrics
    arbor = GC.family("thick_arbor", 512)
    d = GC.edt2_ref(arbor)
    sk = M.thin(dev(arbor[None]))[0].cpu().numpy()
    check_crossings(M, sk, d[None], [GC.soma_ref(d)], ("thick_arbor",), "R=512")
    x = SC.family("cross_x", 512)
    c, _ = check_crossings(M, x[None], x[None].astype(np.int64), [[0, 0, 0]], ("cross_x",), "R=512")
    assert int(c[0, 90]) > 0                                               # the last bin exists and is reached
    plus = SC.family("plus", 1024)                                         # one pixel thick: dist2 is 1, and 2 where the arms cross
    d = plus.astype(np.int64)
    d[512, 512] = 2
    dist2, soma = check_transform(M, plus[None], [(d, [512, 512, 2])], ("plus",), "R=1024")
    c, _ = check_crossings(M, plus[None], d[None], [[512, 512, 2]], ("plus",), "R=1024")
    assert c[0, 1:31].tolist() == [4] * 30 and int(c[0, 33:].sum()) == 0


def test_an_empty_image_in_the_batch(ngan):
    M = ngan.metrics
    masks = np.stack([GC.family("soma_arbor", 64), GC.family("empty", 64), GC.family("plus", 64)])
    dist2, soma = M.distance_transform(dev(masks))
    assert soma[1].tolist() == [-1, -1, 0] and not bool(dist2[1].any())
    skeleton, _ = M.thin(dev(masks))
    crossings, roots = M.sholl_crossings(skeleton, dist2, soma)
    assert not bool(crossings[1].any()) and float(roots[1]) == 0.0
    assert int(crossings[0].sum()) > 0 and crossings[2, 1:15].tolist() == [4] * 14
    for i in (0, 2):
        d, s = M.distance_transform(dev(masks[i:i + 1]))
        c, r = M.sholl_crossings(skeleton[i:i + 1].contiguous(), d, s)
        assert torch.equal(d[0], dist2[i]) and torch.equal(s[0], soma[i]) and torch.equal(c[0], crossings[i]) and torch.equal(r[0], roots[i])
    # a set skeleton with the centre of an empty mask: zeros, not the sum over the skeleton
    c, r = M.sholl_crossings(skeleton[2:3].contiguous(), dist2[2:3].contiguous(), soma[1:2].contiguous())
    assert not bool(c.any()) and float(r[0]) == 0.0


def test_refusals_return_an_error_and_write_nothing(ngan):
    lib = ngan._C.lib()
    stream = torch.cuda.current_stream().cuda_stream
    mask = torch.ones(2, 32, 32, device=DEV, dtype=torch.uint8)
    outs = {"dist2": torch.full((2, 32, 32), -7, device=DEV, dtype=torch.int32), "soma": torch.full((2, 3), -7, device=DEV, dtype=torch.int32),
            "crossings": torch.full((2, 91), -7, device=DEV, dtype=torch.int32), "roots": torch.full((2,), -7.0, device=DEV, dtype=torch.float64)}
    ws = torch.zeros(lib.ngan_geom_workspace_bytes(2, 32), device=DEV, dtype=torch.uint8)
    good = torch.ones(2, 32, 32, device=DEV, dtype=torch.int32)
    centre = torch.tensor([[16, 16, 0], [16, 16, 0]], device=DEV, dtype=torch.int32)
    sentinel = {k: v.clone() for k, v in outs.items()}
    p = {k: v.data_ptr() for k, v in outs.items()}

    def edt(src=mask.data_ptr(), dist2=p["dist2"], soma=p["soma"], w=ws.data_ptr(), B=1, R=32):
        return lib.ngan_geom_edt(src, dist2, soma, w, B, R, stream)

    def sholl(src=mask.data_ptr(), dist2=good.data_ptr(), c=centre.data_ptr(), crossings=p["crossings"], roots=p["roots"], B=1, R=32):
        return lib.ngan_geom_sholl(src, dist2, c, crossings, roots, B, R, stream)
    cases = [(edt, {"R": 8}, "R=8"), (edt, {"R": 24}, "R=24"), (edt, {"R": 2048}, "R=2048"), (edt, {"B": 0}, "B=0"), (edt, {"B": 65536}, "B=65536"),
             (edt, {"src": mask.data_ptr() + 1}, "16-byte"), (edt, {"dist2": p["dist2"] + 4}, "16-byte"), (edt, {"w": ws.data_ptr() + 8}, "16-byte"),
             (edt, {"soma": p["soma"] + 2}, "4-byte"), (edt, {"src": None}, "null"), (edt, {"dist2": None}, "null"), (edt, {"soma": None}, "null"),
             (edt, {"w": None}, "null"),
             (sholl, {"R": 8}, "R=8"), (sholl, {"R": 2048}, "R=2048"), (sholl, {"B": 0}, "B=0"), (sholl, {"B": 65536}, "B=65536"),
             (sholl, {"src": mask.data_ptr() + 3}, "16-byte"), (sholl, {"dist2": good.data_ptr() + 4}, "16-byte"),
             (sholl, {"c": centre.data_ptr() + 1}, "4-byte"), (sholl, {"crossings": p["crossings"] + 2}, "4-byte"),
             (sholl, {"roots": p["roots"] + 4}, "8-byte"), (sholl, {"src": None}, "null"), (sholl, {"dist2": None}, "null"),
             (sholl, {"c": None}, "null"), (sholl, {"crossings": None}, "null"), (sholl, {"roots": None}, "null")]
    for fn, kw, word in cases:
        assert fn(**kw) != 0, (fn.__name__, kw)
        assert word in lib.ngan_last_error().decode(), (fn.__name__, kw, lib.ngan_last_error())
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], sentinel[k]), f"a refused call wrote {k}"
    assert edt() == 0 and sholl() == 0                                                            # one image of the two
    torch.cuda.synchronize()
    assert torch.equal(outs["dist2"][0].cpu(), torch.from_numpy(GC.full_ref(32)).to(torch.int32)) and outs["soma"][0].tolist() == [15, 15, 256]
    assert float(outs["roots"][0]) == 1024.0 and int(outs["crossings"][0].sum()) > 0 and int(outs["crossings"][0, 0]) == 0
    for k in outs:
        assert torch.equal(outs[k][1], sentinel[k][1]), f"{k} of the image that was not asked for changed"


# ---- the whole chain -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (32, 64, 128))
def test_sholl_statistics_of_micrographs(ngan, size):
    M = ngan.metrics
    img = np.stack([OT.micrograph(seed, size) for seed in range(4)])
    x = dev(MC.from_bytes(img)[..., None])
    hists = [np.bincount(i.ravel(), minlength=256) for i in img]
    for kw, cut_of, min_size in ((dict(), lambda h: OT.multiotsu4(h)[0][0], 1),
                                 (dict(otsu_class=2, min_size=4), lambda h: OT.multiotsu4(h)[0][1], 4),
                                 (dict(threshold=100), lambda h: 100, 1)):
        st = M.sholl_statistics(x, **kw)
        assert set(st) == set(GC.STATISTICS) | {"scored", "crossings"}
        assert all(st[n].dtype == torch.float64 and st[n].is_cuda for n in GC.STATISTICS) and st["crossings"].dtype == torch.int32
        for i in range(4):
            ref = GC.sholl_statistics_ref(img[i] > cut_of(hists[i]), min_size=min_size)
            assert bool(st["scored"][i]) == ref["scored"], (size, kw, i)
            assert st["crossings"][i].tolist() == ref["crossings"].tolist(), (size, kw, i)
            for name in GC.STATISTICS:
                a, b = float(st[name][i]), ref[name]
                assert close(a, b), (size, kw, i, name, a, b)


def compare_results(res, ref):
    assert set(res) == set(ref) and (res["images"], res["skipped_real"], res["skipped_fake"]) == (ref["images"], 0, 0)
    for name in GC.STATISTICS:
        for k, v in ref[name].items():
            assert close(res[name][k], v), (name, k, res[name][k], v)
    for k in ("radius", "real", "fake"):
        assert len(res["profile"][k]) == len(ref["profile"][k]), k
        assert all(close(a, b) for a, b in zip(res["profile"][k], ref["profile"][k])), k


@pytest.mark.parametrize("pair", ("fat", "cropped"))
def test_known_sets_through_the_metric(ngan, pair):
    """16 dilated random-walk trees at 64 x 64 against their own dilation (thicker processes) and against themselves cropped to a disc of
    radius 16 (a bunched arbor), through images whose class above t0 is the tree; fed in uneven minibatches, one side as (B, C, R, R)"""
    M = ngan.metrics
    W, fat, cropped = GC.known_sets()
    other, seed = (fat, 6) if pair == "fat" else (cropped, 7)
    xw, xo = (torch.from_numpy(MC.mask_images(m, s)[1]) for m, s in ((W, 5), (other, seed)))
    m = M.Sholl(64, device=DEV)
    for lo, hi in ((0, 1), (1, 7), (7, 16)):
        m.feed("real", xw[lo:hi].permute(0, 3, 1, 2).contiguous())
        m.feed("fake", xo[lo:hi])
    res = m.result()
    print(M.format_sholl(res))
    compare_results(res, GC.sholl_result_ref(GC.known("W"), GC.known(pair), 64))
    if pair == "fat":
        assert res["calibre"]["ks"] == 1.0 and res["calibre"]["fake"] > 2 * res["calibre"]["real"]
    else:
        assert res["reach"]["ks"] == 1.0 and not any(res["profile"]["fake"][13:]) and res["profile"]["fake"][12] > 0
        assert any(res["profile"]["real"][13:])
    assert len(M.format_sholl(res).splitlines()) == 2 + 5 + 2
    m.feed("real", xw[:1])
    with pytest.raises(ValueError):
        m.result()


# ---- evaluate_sholl ------------------------------------------------------------------------------------------------------------------------
def small_nets(ngan, widths=(32, 16)):
    G = ngan.models.Generator_PG(list(widths), image_size_init=8, latent_dim=32).to(DEV)
    D = ngan.models.Discriminator_PG(list(widths)[::-1], image_size_init=8).to(DEV)
    return G, D


def small_dataset(ngan, size=16):
    g = torch.Generator().manual_seed(9)
    return ngan.data.NeuronDataset(torch.rand(8, 1, size, size, generator=g), augmentations=True, im_translation=0.05, device=DEV, seed=3)


def test_evaluate_sholl_is_seeded_and_leaves_no_trace(ngan):
    M = ngan.metrics
    torch.manual_seed(7)
    G, _ = small_nets(ngan, (32, 16, 16))
    G.set_resolution(32, 1.0)
    data = small_dataset(ngan, 32)
    data.set_image_size(8)
    host_rng, device_rng, aug = torch.get_rng_state(), torch.cuda.get_rng_state(DEV), data.gen.get_state()
    own = data.gen
    kw = dict(n_images=7, batch_size=3, seed=2)
    first, metric = M.evaluate_sholl(G, data, return_metric=True, **kw)
    assert isinstance(metric, M.Sholl) and first["images"] == 7 and metric.count == {"real": 7, "fake": 7}
    assert torch.equal(torch.get_rng_state(), host_rng), "torch's global generator was consumed"
    assert torch.equal(torch.cuda.get_rng_state(DEV), device_rng), "the device generator was consumed"
    assert data.gen is own and torch.equal(data.gen.get_state(), aug) and data.image_size == 8, "the data set's stream or stage moved"
    assert M.evaluate_sholl(G, data, **kw) == first                               # seeded: the same numbers again
    assert M.evaluate_sholl(G, None, real_from=metric, **kw) == first             # the data's side taken over, the data set untouched
    with pytest.raises(ValueError):
        M.evaluate_sholl(G, None, real_from=metric, **{**kw, "min_size": 2})
    G8, _ = small_nets(ngan)                                                      # a stage below 16 x 16: said, not raised
    below = M.evaluate_sholl(G8, data, **kw)
    assert below["images"] == 0 and "calibre" not in below and "16 x 16" in below["note"]


# ---- no side effects -----------------------------------------------------------------------------------------------------------------------
def same(x, y):
    if torch.is_tensor(x):
        return torch.is_tensor(y) and torch.equal(x, y)
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return isinstance(y, (list, tuple)) and len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    return x == y


def two_epochs(ngan, tmp_path, tag, sholl_period, ema_beta):
    cfg = types.SimpleNamespace(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[1], N_epochs=2,
                                alpha_step=0.5, learning_rate=2e-3, checkpointing_period=1, ID=tag, sholl_period=sholl_period,
                                sholl_images=6, sholl_seed=1, sholl_min_size=1)
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
    plain, saved0, lines0, _, _, rng0 = two_epochs(ngan, tmp_path, "g000", 0, ema_beta)
    scored, saved1, lines1, tr, f, rng1 = two_epochs(ngan, tmp_path, "g001", 1, ema_beta)
    assert tr.G.image_size == 16 and tr.has_graph((4, 1, 16, 16)), "the run did not train through a captured graph"
    assert plain == scored, "the monitor series changed when the metric was turned on"
    for key in ("Generator_state", "Discriminator_state", "optimizer_state") + (("Generator_ema_state",) if ema_beta else ()):
        assert key in saved0 and same(saved0[key], saved1[key]), f"{key} changed when the metric was turned on"
    for name, x, y in zip(("torch's CPU generator", "the device generator", "the data set's generator"), rng0, rng1):
        assert torch.equal(x, y), f"{name} ended in another state"
    assert "SHOLL" not in saved0 and not any("sholl" in l for l in lines0)
    entries = saved1["SHOLL"]
    assert [e["epoch"] for e in entries] == [1, 2] and "SKELETON" not in saved1 and "MORPH" not in saved1 and "SWD" not in saved1
    base = {"epoch", "image_size", "images", "min_size", "skipped_real", "skipped_fake"}
    for e in entries:
        assert base <= set(e) and e["image_size"] == 16 and e["images"] == 6 and e["min_size"] == 1
        extra = set(e) - base
        if "note" in e:                                              # a side without a scored image: said, no statistic stored
            assert extra <= {"note", "skipped_fake_ema"}
        else:
            assert {n for n in extra if not n.endswith("_ema")} == set(GC.STATISTICS) | {"profile"}
            assert all(set(e[n]) == {"real", "real_sem", "fake", "fake_sem", "ks"} and 0.0 <= e[n]["ks"] <= 1.0 for n in GC.STATISTICS)
            prof = e["profile"]
            assert set(prof) == {"radius", "real", "fake"} and len(prof["radius"]) == len(prof["real"]) == len(prof["fake"]) <= 12
            assert all(isinstance(v, float) for k in prof for v in prof[k])
            if ema_beta and "calibre_ema" in e:
                assert {n for n in extra if n.endswith("_ema")} == {n + "_ema" for n in GC.STATISTICS} | {"profile_ema", "skipped_fake_ema"}
                assert set(e["calibre_ema"]) == {"fake", "fake_sem", "ks"} and len(e["profile_ema"]["fake"]) == len(prof["radius"])
        assert ("skipped_fake_ema" in e) == bool(ema_beta)
    assert entries[0]["skipped_real"] == entries[1]["skipped_real"]                                   # the same seed: the same data side
    if "calibre" in entries[0] and "calibre" in entries[1]:
        assert entries[0]["calibre"]["real"] == entries[1]["calibre"]["real"]
    assert len([l for l in lines1 if "sholl" in l]) == 2
    # the eval tool prints the table for the checkpoint after the skeleton table, and the averaged generator's after it when asked
    images = str(tmp_path / "images.pt")
    torch.save(torch.rand(8, 1, 16, 16, generator=torch.Generator().manual_seed(9)) * 2 - 1, images)
    capsys.readouterr()
    assert ngan.eval.main(["-weights", f, "--sholl", "8", "--skeleton", "8", "--images", images] + (["--ema"] if ema_beta else [])) == 0
    out = capsys.readouterr().out
    n = 2 if ema_beta else 1
    assert out.count("Arbor geometry") == n and out.count("Arbor skeleton") == n
    assert out.count("Arbor geometry, averaged generator") == (1 if ema_beta else 0)
    assert out.index("Arbor skeleton") < out.index("Arbor geometry")
    if ema_beta:
        assert out.rindex("Arbor skeleton") < out.index("Arbor geometry")
