"""Arbor morphology on the GPU: the kernels of csrc/morph.hip against the numpy restatement of tests/morph_cases.py (definitions and
mask families are described there), the metric on known sets, `evaluate_morphology`, and its promise to leave a run alone.  Every
result of the kernels is an integer, so every comparison with the restatement is exact; the fp64 summaries formed from them on the
Python side (dimension, means, standard errors, KS) are held to 1e-12."""
import types

import numpy as np
import pytest
import torch

import morph_cases as MC
import multiotsu_ref as OT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def check_labelling(M, masks, refs, names, tag, min_size=1):
    """labels, stats and kept of a batch against the reference triples; returns the three tensors"""
    labels, stats, kept = M.connected_components(dev(masks), min_size)
    n, R = masks.shape[0], masks.shape[1]
    assert tuple(labels.shape) == (n, R, R) and labels.dtype == torch.int32 and tuple(stats.shape) == (n, 4) and stats.dtype == torch.int32
    assert tuple(kept.shape) == (n, R, R) and kept.dtype == torch.uint8
    got_l, got_s, got_k = labels.cpu().numpy(), stats.cpu().numpy(), kept.cpu().numpy()
    for i, (name, (lab, st, kp)) in enumerate(zip(names, refs)):
        assert got_s[i].tolist() == st, f"{tag} {name}: stats {got_s[i].tolist()} != {st}"
        assert np.array_equal(got_l[i], lab), f"{tag} {name}: {(got_l[i] != lab).sum()} labels differ"
        assert np.array_equal(got_k[i], kp), f"{tag} {name}: kept mask differs"
    return labels, stats, kept


# ---- connected components ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", MC.SIZES)
def test_components_against_the_flood_fill(ngan, size):
    """every family in one batch (16 below any tile, 128 two tiles each way); then 3 images and 1 image of the same, a second call, and
    the call without the kept mask"""
    M = ngan.metrics
    masks, refs = MC.case(size)
    tag = f"R={size}"
    labels, stats, kept = check_labelling(M, masks, refs, MC.FAMILIES, tag)
    for n in (3, 1):
        l, s, k = M.connected_components(dev(masks[:n]))
        assert torch.equal(l, labels[:n]) and torch.equal(s, stats[:n]) and torch.equal(k, kept[:n]), \
            f"{tag} B={n}: an image's values depend on the rest of the batch"
    l, s, k = M.connected_components(dev(masks))
    assert torch.equal(l, labels) and torch.equal(s, stats) and torch.equal(k, kept), f"{tag}: two calls differ"
    l, s, k = M.connected_components(dev(masks), want_kept=False)
    assert k is None and torch.equal(l, labels) and torch.equal(s, stats), f"{tag}: labels or stats differ without the kept mask"
    l, _, _ = M.connected_components(dev(masks * 255))                                           # any non-zero byte is foreground
    assert torch.equal(l, labels)


@pytest.mark.parametrize("name", ("snake", "random41"))
def test_components_at_512(ngan, name):
    """one image of 8 x 8 tiles: the snake crosses every border and its minimum travels 131 327 pixels; the reference is the run
    labelling that tests/test_morph_cpu.py holds against the flood fill"""
    M = ngan.metrics
    m = MC.family(name, 512)
    lab = MC.label_runs_ref(m)
    st, kp = MC.stats_of_labels(lab)
    if name == "snake":
        assert st == [512 * 512 // 2 + 255, 1, 512 * 512 // 2 + 255, 512 * 512 // 2 + 255] and lab.max() == 0
    check_labelling(M, m[None], [(lab, st, kp)], (name,), "R=512")


@pytest.mark.parametrize("size", (64, 128))
def test_min_size_drops_small_components(ngan, size):
    M = ngan.metrics
    names = ("random20", "corners")
    masks = np.stack([MC.family(f, size) for f in names])
    for min_size in (1, 2, 8, 3):
        refs = [MC.stats_ref(m, min_size) for m in masks]
        _, stats, kept = check_labelling(M, masks, refs, names, f"R={size} min_size={min_size}", min_size)
        if min_size == 3:
            k = (size // 8 - 1) ** 2
            assert stats[1].tolist() == [2 * k, 0, 2, 0] and not bool(kept[1].any())


# ---- box counts ----------------------------------------------------------------------------------------------------------------------------
BOX_FAMILIES = MC.FAMILIES + ("corner_boxes", "row", "disc")


@pytest.mark.parametrize("size", MC.SIZES)
def test_box_counts_and_dimension(ngan, size):
    M = ngan.metrics
    L = size.bit_length() - 1
    masks = np.stack([MC.family(f, size) for f in BOX_FAMILIES])
    ref = np.array([MC.box_counts_ref(m) for m in masks])
    counts = M.box_counts(dev(masks))
    assert tuple(counts.shape) == (len(BOX_FAMILIES), L + 1) and counts.dtype == torch.int32
    got = counts.cpu().numpy()
    for name, a, b in zip(BOX_FAMILIES, got, ref):
        assert a.tolist() == b.tolist(), f"R={size} {name}: {a.tolist()} != {b.tolist()}"
    assert np.array_equal(got[:, 0], masks.reshape(len(masks), -1).sum(1)) and set(got[:, L].tolist()) <= {0, 1}
    for n in (3, 1):
        assert torch.equal(M.box_counts(dev(masks[:n])), counts[:n]), f"R={size} B={n}: counts depend on the rest of the batch"
    assert torch.equal(M.box_counts(dev(masks)), counts)
    d = M.box_dimension(counts, size)
    assert d.dtype == torch.float64 and d.is_cuda
    want = np.array([MC.dimension_ref(c, size) for c in ref])
    d = d.cpu().numpy()
    assert np.array_equal(np.isnan(d), np.isnan(want)) and np.nanmax(np.abs(d - want)) <= 1e-12
    if size >= 32:
        line, diag, disc = (d[BOX_FAMILIES.index(f)] for f in ("row", "diagonal", "disc"))
        print(f"R={size}: dimension row {line:.3f} diagonal {diag:.3f} disc {disc:.3f}")
        assert abs(line - 1.0) <= 1e-12 and abs(diag - 1.0) <= 1e-12 and disc - line >= 0.5


@pytest.mark.parametrize("size", (256, 512, 1024))
def test_box_counts_above_the_tile(ngan, size):
    """the sizes whose upper levels (one, two and three of them) come from the tiles' occupancy: sparse fields that leave boxes of
    every level empty, the corner boxes, one pixel, nothing and everything"""
    M = ngan.metrics
    rng = np.random.default_rng(size)
    sparse = (rng.random((size, size)) < 6.0 / size ** 2).astype(np.uint8)
    half = np.zeros((size, size), np.uint8)
    half[size // 2:, : size // 4] = MC.family("checkerboard", size)[size // 2:, : size // 4]
    names = ("sparse", "half", "corner_boxes", "single", "empty", "full", "snake")
    masks = np.stack([sparse, half] + [MC.family(f, size) for f in names[2:]])
    ref = [MC.box_counts_ref(m) for m in masks]
    assert ref[1][-2] == 1 and ref[1][-3] == 2                                                   # `half` leaves upper boxes empty
    counts = M.box_counts(dev(masks))
    for name, a, b in zip(names, counts.cpu().numpy(), ref):
        assert a.tolist() == b, f"R={size} {name}: {a.tolist()} != {b}"
    assert torch.equal(M.box_counts(dev(masks[:1])), counts[:1])


# ---- levels and masks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (32, 64, 128))
def test_levels_histogram_and_otsu_mask(ngan, size):
    M = ngan.metrics
    img = np.stack([OT.micrograph(seed, size) for seed in range(4)])
    x = dev(MC.from_bytes(img)[..., None])
    levels, hist = M.morph_levels(x)
    assert levels.dtype == torch.uint8 and tuple(levels.shape) == (4, size, size) and tuple(hist.shape) == (4, 256)
    assert np.array_equal(levels.cpu().numpy(), img), "levels differ from the source bytes"
    want_hist = np.stack([np.bincount(i.ravel(), minlength=256) for i in img])
    assert np.array_equal(hist.cpu().numpy(), want_hist)
    thresholds, status = M.otsu_thresholds(hist)
    assert status.tolist() == [0] * 4
    mask = M.morph_mask(levels, thresholds[:, 0])
    for i in range(4):
        triplet, best, second = OT.multiotsu4(want_hist[i])
        gap = OT.relative_gap(best, second)
        print(f"R={size} seed={i}: t0 {triplet[0]}, relative gap {gap:.3e}")
        assert gap >= 1e-9, "the threshold of this case is not decided: it may not be left out, find another seed"
        assert thresholds[i].tolist() == list(triplet)
        assert np.array_equal(mask[i].cpu().numpy(), (img[i] > triplet[0]).astype(np.uint8)), (size, i)
    for n in (3, 1):
        l, h = M.morph_levels(x[:n].contiguous())
        assert torch.equal(l, levels[:n]) and torch.equal(h, hist[:n])
    fixed = M.morph_mask(levels, 100)
    assert np.array_equal(fixed.cpu().numpy(), (img > 100).astype(np.uint8))
    assert not bool(M.morph_mask(levels, 255).any()) and bool(M.morph_mask(levels, -1).all())
    st = M.arbor_statistics(x)                                                                     # the whole chain on the same images
    for i in range(4):
        ref = MC.arbor_statistics_ref(img[i] > OT.multiotsu4(want_hist[i])[0][0])
        assert bool(st["scored"][i]) == ref["scored"]
        for name in MC.STATISTICS:
            assert abs(float(st[name][i]) - ref[name]) <= 1e-12, (size, i, name)
    st2 = M.arbor_statistics(x, otsu_class=2, min_size=4)
    for i in range(4):
        ref = MC.arbor_statistics_ref(img[i] > OT.multiotsu4(want_hist[i])[0][1], min_size=4)
        for name in MC.STATISTICS:
            assert abs(float(st2[name][i]) - ref[name]) <= 1e-12, (size, i, name)
    st3 = M.arbor_statistics(x, threshold=100)
    assert abs(float(st3["fill"][0]) - MC.arbor_statistics_ref(img[0] > 100)["fill"]) <= 1e-12


def test_levels_of_three_channels_and_out_of_range_values(ngan):
    M = ngan.metrics
    rng = np.random.default_rng(4)
    for size, n in ((16, 3), (64, 2)):
        x = rng.uniform(-1.2, 1.2, (n, size, size, 3)).astype(np.float32)
        x[0, 0, :6, :] = np.array([-3.0, -1.0, 1.0, 3.0, 0.0, 0.999], np.float32)[:, None]
        want = MC.levels_ref(x)
        levels, hist = M.morph_levels(dev(x))
        assert np.array_equal(levels.cpu().numpy(), want), f"R={size}: {(levels.cpu().numpy() != want).sum()} levels differ"
        assert np.array_equal(hist.cpu().numpy(), np.stack([np.bincount(w.ravel(), minlength=256) for w in want]))
        assert want[0, 0, :6].tolist() == [0, 0, 255, 255, 128, 255]
        one = MC.levels_ref(x[..., :1])
        assert np.array_equal(M.morph_levels(dev(x[..., :1]))[0].cpu().numpy(), one)


def test_an_image_without_four_levels_is_not_scored(ngan):
    M = ngan.metrics
    img = np.zeros((2, 32, 32), np.uint8)
    img[0, 8:24, 8:24] = 200
    img[0, 12, 12] = 90                                              # three occupied levels
    img[1] = MC.mask_images(MC.arbor_set(32, 1, 3), 1)[0][0]          # a proper one next to it
    x = dev(MC.from_bytes(img)[..., None])
    levels, hist = M.morph_levels(x)
    thresholds, status = M.otsu_thresholds(hist)
    assert status[0].item() != 0 and status[1].item() == 0
    st = M.arbor_statistics(x)
    assert st["scored"].tolist() == [False, True] and float(st["fill"][0]) == 0.0 and float(st["components"][0]) == 0.0
    m = M.Morphology(32, device=DEV)
    m.feed("real", x)
    m.feed("fake", x.flip(0))
    res = m.result()
    assert (res["images"], res["skipped_real"], res["skipped_fake"]) == (2, 1, 1) and res["fill"]["ks"] == 0.0
    m = M.Morphology(32, device=DEV)
    m.feed("real", x[1:])
    m.feed("fake", x[:1])
    res = m.result()
    assert "fill" not in res and res["skipped_fake"] == 1 and "generated" in res["note"]


# ---- the metric on known sets --------------------------------------------------------------------------------------------------------------
def test_cut_trees_against_intact_ones(ngan):
    """16 random-walk trees against the same trees with every sixth row and column cleared, R = 64, through images whose class above t0
    is the tree (tests/test_morph_cpu.py checks that); fed in uneven minibatches, one side as (B, C, R, R)"""
    M = ngan.metrics
    whole, cut, other = MC.arbor_set(64, 16, 1), MC.arbor_set(64, 16, 1, cut=True), MC.arbor_set(64, 16, 2)
    xw, xc, xo = (torch.from_numpy(MC.mask_images(m, s)[1]) for m, s in ((whole, 5), (cut, 6), (other, 7)))
    m = M.Morphology(64, device=DEV)
    for lo, hi in ((0, 1), (1, 7), (7, 16)):
        m.feed("real", xw[lo:hi].permute(0, 3, 1, 2).contiguous())
        m.feed("fake", xc[lo:hi])
    res = m.result()
    ref = MC.morphology_ref([MC.arbor_statistics_ref(a) for a in whole], [MC.arbor_statistics_ref(a) for a in cut])
    print(M.format_morphology(res))
    assert set(res) == set(ref) and (res["images"], res["skipped_real"], res["skipped_fake"]) == (16, 0, 0)
    for name in MC.STATISTICS:
        for k, v in ref[name].items():
            assert abs(res[name][k] - v) <= 1e-12, (name, k, res[name][k], v)
    assert res["largest_share"]["real"] >= 0.99 and res["largest_share"]["fake"] <= 0.25 and res["largest_share"]["ks"] == 1.0
    assert res["components"]["real"] == 1.0 and res["components"]["fake"] >= 33
    same = M.Morphology(64, device=DEV)
    same.feed("real", xw)
    same.feed("fake", xo)
    res = same.result()
    assert res["largest_share"]["ks"] == 0.0 and res["components"]["ks"] == 0.0
    assert len(M.format_morphology(res).splitlines()) == 2 + 4
    same.feed("real", xw[:1])
    with pytest.raises(ValueError):
        same.result()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_an_error_and_write_nothing(ngan):
    lib = ngan._C.lib()
    stream = torch.cuda.current_stream().cuda_stream
    x = torch.zeros(2, 32, 32, 3, device=DEV)
    mask = torch.ones(2, 32, 32, device=DEV, dtype=torch.uint8)
    cut = torch.zeros(2, device=DEV, dtype=torch.int32)
    outs = {"levels": torch.full((2, 32, 32), 7, device=DEV, dtype=torch.uint8), "hist": torch.full((2, 256), -7, device=DEV, dtype=torch.int32),
            "mask": torch.full((2, 32, 32), 7, device=DEV, dtype=torch.uint8), "labels": torch.full((2, 32, 32), -7, device=DEV, dtype=torch.int32),
            "stats": torch.full((2, 4), -7, device=DEV, dtype=torch.int32), "kept": torch.full((2, 32, 32), 7, device=DEV, dtype=torch.uint8),
            "ws": torch.full((2 * 32 * 32,), -7, device=DEV, dtype=torch.int32), "counts": torch.full((2, 6), -7, device=DEV, dtype=torch.int32)}
    sentinel = {k: v.clone() for k, v in outs.items()}
    p = {k: v.data_ptr() for k, v in outs.items()}

    def levels(images=x.data_ptr(), out=p["levels"], hist=p["hist"], B=1, R=32, C=1):
        return lib.ngan_morph_levels(images, out, hist, B, R, C, stream)

    def to_mask(src=mask.data_ptr(), c=cut.data_ptr(), out=p["mask"], B=1, R=32):
        return lib.ngan_morph_mask(src, c, out, B, R, stream)

    def label(src=mask.data_ptr(), labels=p["labels"], stats=p["stats"], kept=p["kept"], ws=p["ws"], B=1, R=32, min_size=1):
        return lib.ngan_morph_label(src, labels, stats, kept, ws, B, R, min_size, stream)

    def boxes(src=mask.data_ptr(), counts=p["counts"], B=1, R=32):
        return lib.ngan_morph_boxcount(src, counts, B, R, stream)
    cases = [(levels, {"R": 24}, "R=24"), (levels, {"R": 8}, "R=8"), (levels, {"R": 2048}, "R=2048"), (levels, {"C": 2}, "C=2"),
             (levels, {"B": 0}, "B=0"), (levels, {"images": x.data_ptr() + 4}, "16-byte"), (levels, {"hist": None}, "null"),
             (to_mask, {"R": 24}, "R=24"), (to_mask, {"B": 65536}, "B=65536"), (to_mask, {"src": mask.data_ptr() + 1}, "16-byte"),
             (to_mask, {"c": None}, "null"),
             (label, {"R": 48}, "R=48"), (label, {"B": 0}, "B=0"), (label, {"min_size": 0}, "min_size=0"), (label, {"ws": None}, "workspace"),
             (label, {"labels": p["labels"] + 4}, "16-byte"), (label, {"ws": p["ws"] + 8}, "16-byte"), (label, {"src": None}, "null"),
             (label, {"kept": p["kept"] + 2}, "16-byte"),
             (boxes, {"R": 8}, "R=8"), (boxes, {"B": -1}, "B=-1"), (boxes, {"src": mask.data_ptr() + 3}, "16-byte"), (boxes, {"counts": None}, "null")]
    for fn, kw, word in cases:
        assert fn(**kw) != 0, (fn.__name__, kw)
        assert word in lib.ngan_last_error().decode(), (fn.__name__, kw, lib.ngan_last_error())
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], sentinel[k]), f"a refused call wrote {k}"
    assert lib.ngan_morph_workspace_bytes(1, 24) == 0 and lib.ngan_morph_workspace_bytes(2, 32) == 2 * 32 * 32 * 4
    assert levels() == 0 and to_mask() == 0 and label() == 0 and boxes() == 0                     # one image of the two
    torch.cuda.synchronize()
    assert bool((outs["levels"][0] == 128).all()) and outs["hist"][0, 128].item() == 1024 and outs["hist"][0].sum().item() == 1024
    assert bool((outs["mask"][0] == 1).all()) and bool((outs["labels"][0] == 0).all()) and outs["stats"][0].tolist() == [1024] + [1, 1024, 1024]
    assert bool((outs["kept"][0] == 1).all()) and outs["counts"][0].tolist() == [1024, 256, 64, 16, 4, 1]
    for k in ("levels", "hist", "mask", "labels", "stats", "kept", "counts"):
        assert torch.equal(outs[k][1], sentinel[k][1]), f"{k} of the image that was not asked for changed"


# ---- evaluate_morphology -------------------------------------------------------------------------------------------------------------------
def small_nets(ngan, widths=(32, 16)):
    G = ngan.models.Generator_PG(list(widths), image_size_init=8, latent_dim=32).to(DEV)
    D = ngan.models.Discriminator_PG(list(widths)[::-1], image_size_init=8).to(DEV)
    return G, D


def small_dataset(ngan, size=16):
    g = torch.Generator().manual_seed(9)
    return ngan.data.NeuronDataset(torch.rand(8, 1, size, size, generator=g), augmentations=True, im_translation=0.05, device=DEV, seed=3)


def test_evaluate_morphology_is_seeded_and_leaves_no_trace(ngan):
    M = ngan.metrics
    torch.manual_seed(7)
    G, _ = small_nets(ngan, (32, 16, 16))
    G.set_resolution(32, 1.0)
    data = small_dataset(ngan, 32)
    data.set_image_size(8)
    host_rng, device_rng, aug = torch.get_rng_state(), torch.cuda.get_rng_state(DEV), data.gen.get_state()
    own = data.gen
    kw = dict(n_images=7, batch_size=3, seed=2)
    first, metric = M.evaluate_morphology(G, data, return_metric=True, **kw)
    assert first["images"] == 7 and metric.count == {"real": 7, "fake": 7}
    assert torch.equal(torch.get_rng_state(), host_rng), "torch's global generator was consumed"
    assert torch.equal(torch.cuda.get_rng_state(DEV), device_rng), "the device generator was consumed"
    assert data.gen is own and torch.equal(data.gen.get_state(), aug) and data.image_size == 8, "the data set's stream or stage moved"
    assert M.evaluate_morphology(G, data, **kw) == first                          # seeded: the same numbers again
    assert M.evaluate_morphology(G, None, real_from=metric, **kw) == first        # the data's side taken over, the data set untouched
    with pytest.raises(ValueError):
        M.evaluate_morphology(G, None, real_from=metric, **{**kw, "min_size": 2})
    # both sides by hand: the same augmented batches, the same latents
    data.gen = torch.Generator(device="cpu").manual_seed(2 + 1)
    data.set_image_size(32)
    lat = torch.Generator(device="cpu").manual_seed(2 + 2)
    by_hand = M.Morphology(32, device=DEV)
    for i in range(0, 7, 3):
        b = min(3, 7 - i)
        by_hand.feed("real", data.batch([(i + j) % len(data) for j in range(b)]))
        z = torch.randn(b, G.latent_dim, generator=lat).clamp(-5, 5)
        with torch.no_grad():
            by_hand.feed("fake", G((z / z.norm(p=2, dim=1, keepdim=True)).to(DEV)))
    data.gen = own
    data.set_image_size(8)
    assert by_hand.result() == first
    other, m2 = M.evaluate_morphology(G, data, return_metric=True, **{**kw, "seed": 3})
    assert not torch.equal(torch.cat(m2.values["real"], 1), torch.cat(metric.values["real"], 1))
    G8, _ = small_nets(ngan)                                                      # a stage below 16 x 16: said, not raised
    below = M.evaluate_morphology(G8, data, **kw)
    assert below["images"] == 0 and "fill" not in below and "16 x 16" in below["note"]


# ---- no side effects -----------------------------------------------------------------------------------------------------------------------
def same(x, y):
    if torch.is_tensor(x):
        return torch.is_tensor(y) and torch.equal(x, y)
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return isinstance(y, (list, tuple)) and len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    return x == y


def two_epochs(ngan, tmp_path, tag, morph_period, ema_beta):
    cfg = types.SimpleNamespace(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[1], N_epochs=2,
                                alpha_step=0.5, learning_rate=2e-3, checkpointing_period=1, ID=tag, morph_period=morph_period,
                                morph_images=6, morph_seed=1, morph_min_size=1)
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
    plain, saved0, lines0, _, _, rng0 = two_epochs(ngan, tmp_path, "m000", 0, ema_beta)
    scored, saved1, lines1, tr, f, rng1 = two_epochs(ngan, tmp_path, "m001", 1, ema_beta)
    assert tr.G.image_size == 16 and tr.has_graph((4, 1, 16, 16)), "the run did not train through a captured graph"
    assert plain == scored, "the monitor series changed when the metric was turned on"
    for key in ("Generator_state", "Discriminator_state", "optimizer_state") + (("Generator_ema_state",) if ema_beta else ()):
        assert key in saved0 and same(saved0[key], saved1[key]), f"{key} changed when the metric was turned on"
    for name, x, y in zip(("torch's CPU generator", "the device generator", "the data set's generator"), rng0, rng1):
        assert torch.equal(x, y), f"{name} ended in another state"
    assert "MORPH" not in saved0 and not any("morphology" in l for l in lines0)
    entries = saved1["MORPH"]
    assert [e["epoch"] for e in entries] == [1, 2] and "SWD" not in saved1 and "MSSSIM" not in saved1 and "SPECTRUM" not in saved1
    base = {"epoch", "image_size", "images", "min_size", "skipped_real", "skipped_fake"}
    for e in entries:
        assert base <= set(e) and e["image_size"] == 16 and e["images"] == 6 and e["min_size"] == 1
        extra = set(e) - base
        if "note" in e:                                              # a side without a scored image: said, no statistic stored
            assert extra <= {"note", "skipped_fake_ema"}
        else:
            assert {n for n in extra if not n.endswith("_ema")} == set(MC.STATISTICS)
            assert all(set(e[n]) == {"real", "real_sem", "fake", "fake_sem", "ks"} and 0.0 <= e[n]["ks"] <= 1.0 for n in MC.STATISTICS)
        assert ("skipped_fake_ema" in e) == bool(ema_beta)
    assert entries[0]["skipped_real"] == entries[1]["skipped_real"]                                   # the same seed: the same data side
    if "fill" in entries[0] and "fill" in entries[1]:
        assert entries[0]["fill"]["real"] == entries[1]["fill"]["real"]
    scored_lines = [l for l in lines1 if "morphology" in l]
    assert len(scored_lines) == 2
    # the eval tool prints the table for the checkpoint, and the averaged generator's after it when asked; with --spectrum, both
    images = str(tmp_path / "images.pt")
    torch.save(torch.rand(8, 1, 16, 16, generator=torch.Generator().manual_seed(9)) * 2 - 1, images)
    capsys.readouterr()
    assert ngan.eval.main(["-weights", f, "--morph", "8", "--spectrum", "8", "--images", images] + (["--ema"] if ema_beta else [])) == 0
    out = capsys.readouterr().out
    n = 2 if ema_beta else 1
    assert out.count("Arbor morphology") == n and out.count("Radial power spectrum") == n
    assert out.count("Arbor morphology, averaged generator") == (1 if ema_beta else 0)
    assert out.index("Radial power spectrum") < out.index("Arbor morphology")
