"""Arbor skeleton on the GPU: the kernel of csrc/skeleton.hip against the numpy restatement of tests/skeleton_cases.py (definitions and
mask families are described there), the metric on known sets, `evaluate_skeleton`, and its promise to leave a run alone.  Every result
of the kernel is an integer, so every comparison with the restatement is exact; the fp64 summaries formed from them on the Python side
(length, width, means, standard errors, KS) are held to 1e-12."""
import types

import numpy as np
import pytest
import torch

import morph_cases as MC
import multiotsu_ref as OT
import skeleton_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def check_thinning(M, masks, refs, names, tag):
    """skeleton and the eight stats of a batch against the reference pairs; returns the two tensors"""
    skeleton, stats = M.thin(dev(masks))
    n, R = masks.shape[0], masks.shape[1]
    assert tuple(skeleton.shape) == (n, R, R) and skeleton.dtype == torch.uint8 and tuple(stats.shape) == (n, 8) and stats.dtype == torch.int32
    got_k, got_s = skeleton.cpu().numpy(), stats.cpu().numpy()
    for i, (name, (sk, st)) in enumerate(zip(names, refs)):
        assert got_s[i].tolist() == st, f"{tag} {name}: stats {dict(zip(SC.STAT_NAMES, got_s[i].tolist()))} != {dict(zip(SC.STAT_NAMES, st))}"
        assert np.array_equal(got_k[i], sk), f"{tag} {name}: {(got_k[i] != sk).sum()} skeleton pixels differ"
    return skeleton, stats


# ---- against the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SC.SIZES)
def test_thinning_against_the_restatement(ngan, size):
    """every family in one batch (16: half a word per row; 128: four words per row, `full` runs 130 passes); then 3 images and 1 image
    of the same, a second call, the call without the skeleton, other non-zero bytes, and the counts alone"""
    M = ngan.metrics
    masks, refs = SC.case(size)
    tag = f"R={size}"
    skeleton, stats = check_thinning(M, masks, refs, SC.FAMILIES, tag)
    if size == 128:
        assert stats[SC.FAMILIES.index("full")].tolist() == [1, 0, 0, 1, 0, 0, 130, 128 * 128]
    for n in (3, 1):
        k, s = M.thin(dev(masks[:n]))
        assert torch.equal(k, skeleton[:n]) and torch.equal(s, stats[:n]), f"{tag} B={n}: an image's values depend on the rest of the batch"
    k, s = M.thin(dev(masks))
    assert torch.equal(k, skeleton) and torch.equal(s, stats), f"{tag}: two calls differ"
    k, s = M.thin(dev(masks), want_skeleton=False)
    assert k is None and torch.equal(s, stats), f"{tag}: stats differ without the skeleton"
    k, s = M.thin(dev(masks * 255))                                                               # any non-zero byte is foreground
    assert torch.equal(k, skeleton) and torch.equal(s, stats)
    counts = M.skeleton_counts(dev(masks))                                                        # the unthinned families
    assert tuple(counts.shape) == (len(masks), 8) and counts.dtype == torch.int32
    for name, m, got in zip(SC.FAMILIES, masks, counts.cpu().numpy()):
        want = SC.counts_ref(m)
        assert got.tolist() == want + [0, want[0]], f"{tag} {name}: counts {got.tolist()} != {want + [0, want[0]]}"
    again = M.skeleton_counts(skeleton)                                                           # the fused counts, on their own
    assert torch.equal(again[:, :6], stats[:, :6]) and torch.equal(again[:, 7], stats[:, 0]) and not bool(again[:, 6].any())
    assert torch.equal(M.skeleton_counts(dev(masks[:1])), counts[:1])


@pytest.mark.parametrize("name", ("thick_arbor", "snake"))
def test_thinning_at_512(ngan, name):
    """the largest image the kernel takes: 16 words per row, eight words per thread, all 32 KiB of bit rows"""
    M = ngan.metrics
    m = SC.family(name, 512)
    check_thinning(M, m[None], [SC.stats_ref(m)], (name,), "R=512")


# ---- the whole chain -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (32, 64, 128))
def test_skeleton_statistics_of_micrographs(ngan, size):
    M = ngan.metrics
    img = np.stack([OT.micrograph(seed, size) for seed in range(4)])
    x = dev(MC.from_bytes(img)[..., None])
    hists = [np.bincount(i.ravel(), minlength=256) for i in img]
    for kw, cut_of, min_size in ((dict(), lambda h: OT.multiotsu4(h)[0][0], 1),
                                 (dict(otsu_class=2, min_size=4), lambda h: OT.multiotsu4(h)[0][1], 4),
                                 (dict(threshold=100), lambda h: 100, 1)):
        st = M.skeleton_statistics(x, **kw)
        assert set(st) == set(SC.STATISTICS) | {"scored"} and all(st[n].dtype == torch.float64 and st[n].is_cuda for n in SC.STATISTICS)
        for i in range(4):
            ref = SC.skeleton_statistics_ref(img[i] > cut_of(hists[i]), min_size=min_size)
            assert bool(st["scored"][i]) == ref["scored"], (size, kw, i)
            for name in SC.STATISTICS:
                a, b = float(st[name][i]), ref[name]
                assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-12, (size, kw, i, name, a, b)


def test_cut_trees_against_intact_ones(ngan):
    """16 random-walk trees against the same trees with every sixth row and column cleared, R = 64, through images whose class above t0
    is the tree; fed in uneven minibatches, one side as (B, C, R, R)"""
    M = ngan.metrics
    whole, cut = MC.arbor_set(64, 16, 1), MC.arbor_set(64, 16, 1, cut=True)
    xw, xc = (torch.from_numpy(MC.mask_images(m, s)[1]) for m, s in ((whole, 5), (cut, 6)))
    m = M.Skeleton(64, device=DEV)
    for lo, hi in ((0, 1), (1, 7), (7, 16)):
        m.feed("real", xw[lo:hi].permute(0, 3, 1, 2).contiguous())
        m.feed("fake", xc[lo:hi])
    res = m.result()
    ref = SC.skeleton_ref([SC.skeleton_statistics_ref(a) for a in whole], [SC.skeleton_statistics_ref(a) for a in cut])
    print(M.format_skeleton(res))
    assert set(res) == set(ref) and (res["images"], res["skipped_real"], res["skipped_fake"]) == (16, 0, 0)
    for name in SC.STATISTICS:
        for k, v in ref[name].items():
            assert abs(res[name][k] - v) <= 1e-12, (name, k, res[name][k], v)
    assert res["tips"]["ks"] == 1.0 and res["junctions"]["ks"] == 1.0 and res["tips"]["fake"] > 4 * res["tips"]["real"]
    assert len(M.format_skeleton(res).splitlines()) == 2 + 4
    m.feed("real", xw[:1])
    with pytest.raises(ValueError):
        m.result()


def test_an_image_without_four_levels_is_skipped_and_counted(ngan):
    M = ngan.metrics
    img = np.zeros((2, 32, 32), np.uint8)
    img[0, 8:24, 8:24] = 200
    img[0, 12, 12] = 90                                              # three occupied levels
    img[1] = MC.mask_images(MC.arbor_set(32, 1, 3), 1)[0][0]          # a proper one next to it
    x = dev(MC.from_bytes(img)[..., None])
    st = M.skeleton_statistics(x)
    assert st["scored"].tolist() == [False, True] and float(st["length"][0]) == 0.0 and float(st["tips"][0]) == 0.0
    m = M.Skeleton(32, device=DEV)
    m.feed("real", x)
    m.feed("fake", x.flip(0))
    res = m.result()
    assert (res["images"], res["skipped_real"], res["skipped_fake"]) == (2, 1, 1) and res["length"]["ks"] == 0.0
    m = M.Skeleton(32, device=DEV)
    m.feed("real", x[1:])
    m.feed("fake", x[:1])
    res = m.result()
    assert "length" not in res and res["skipped_fake"] == 1 and "generated" in res["note"]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_return_an_error_and_write_nothing(ngan):
    lib = ngan._C.lib()
    stream = torch.cuda.current_stream().cuda_stream
    mask = torch.ones(2, 32, 32, device=DEV, dtype=torch.uint8)
    outs = {"skeleton": torch.full((2, 32, 32), 7, device=DEV, dtype=torch.uint8), "stats": torch.full((2, 8), -7, device=DEV, dtype=torch.int32),
            "counts": torch.full((2, 8), -7, device=DEV, dtype=torch.int32)}
    sentinel = {k: v.clone() for k, v in outs.items()}
    p = {k: v.data_ptr() for k, v in outs.items()}

    def thin(src=mask.data_ptr(), skeleton=p["skeleton"], stats=p["stats"], B=1, R=32):
        return lib.ngan_skel_thin(src, skeleton, stats, B, R, stream)

    def counts(src=mask.data_ptr(), stats=p["counts"], B=1, R=32):
        return lib.ngan_skel_counts(src, stats, B, R, stream)
    cases = [(thin, {"R": 8}, "R=8"), (thin, {"R": 24}, "R=24"), (thin, {"R": 1024}, "R=1024"), (thin, {"B": 0}, "B=0"),
             (thin, {"B": 65536}, "B=65536"), (thin, {"src": mask.data_ptr() + 1}, "16-byte"), (thin, {"skeleton": p["skeleton"] + 4}, "16-byte"),
             (thin, {"stats": p["stats"] + 2}, "4-byte"), (thin, {"src": None}, "null"), (thin, {"stats": None}, "null"),
             (counts, {"R": 8}, "R=8"), (counts, {"R": 24}, "R=24"), (counts, {"R": 1024}, "R=1024"), (counts, {"B": 0}, "B=0"),
             (counts, {"B": 65536}, "B=65536"), (counts, {"src": mask.data_ptr() + 3}, "16-byte"), (counts, {"stats": p["counts"] + 1}, "4-byte"),
             (counts, {"src": None}, "null"), (counts, {"stats": None}, "null")]
    for fn, kw, word in cases:
        assert fn(**kw) != 0, (fn.__name__, kw)
        assert word in lib.ngan_last_error().decode(), (fn.__name__, kw, lib.ngan_last_error())
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], sentinel[k]), f"a refused call wrote {k}"
    assert thin() == 0 and counts() == 0                                                          # one image of the two
    torch.cuda.synchronize()
    assert outs["stats"][0].tolist() == [1, 0, 0, 1, 0, 0, 34, 1024] and int(outs["skeleton"][0].sum()) == 1
    assert outs["counts"][0, 0].item() == 1024 and outs["counts"][0, 6].item() == 0 and outs["counts"][0, 7].item() == 1024
    assert outs["counts"][0, 4].item() == 2 * 32 * 31 and outs["counts"][0, 5].item() == 0
    for k in outs:
        assert torch.equal(outs[k][1], sentinel[k][1]), f"{k} of the image that was not asked for changed"


# ---- evaluate_skeleton ---------------------------------------------------------------------------------------------------------------------
def small_nets(ngan, widths=(32, 16)):
    G = ngan.models.Generator_PG(list(widths), image_size_init=8, latent_dim=32).to(DEV)
    D = ngan.models.Discriminator_PG(list(widths)[::-1], image_size_init=8).to(DEV)
    return G, D


def small_dataset(ngan, size=16):
    g = torch.Generator().manual_seed(9)
    return ngan.data.NeuronDataset(torch.rand(8, 1, size, size, generator=g), augmentations=True, im_translation=0.05, device=DEV, seed=3)


def test_evaluate_skeleton_is_seeded_and_leaves_no_trace(ngan):
    M = ngan.metrics
    torch.manual_seed(7)
    G, _ = small_nets(ngan, (32, 16, 16))
    G.set_resolution(32, 1.0)
    data = small_dataset(ngan, 32)
    data.set_image_size(8)
    host_rng, device_rng, aug = torch.get_rng_state(), torch.cuda.get_rng_state(DEV), data.gen.get_state()
    own = data.gen
    kw = dict(n_images=7, batch_size=3, seed=2)
    first, metric = M.evaluate_skeleton(G, data, return_metric=True, **kw)
    assert isinstance(metric, M.Skeleton) and first["images"] == 7 and metric.count == {"real": 7, "fake": 7}
    assert torch.equal(torch.get_rng_state(), host_rng), "torch's global generator was consumed"
    assert torch.equal(torch.cuda.get_rng_state(DEV), device_rng), "the device generator was consumed"
    assert data.gen is own and torch.equal(data.gen.get_state(), aug) and data.image_size == 8, "the data set's stream or stage moved"
    assert M.evaluate_skeleton(G, data, **kw) == first                            # seeded: the same numbers again
    assert M.evaluate_skeleton(G, None, real_from=metric, **kw) == first          # the data's side taken over, the data set untouched
    with pytest.raises(ValueError):
        M.evaluate_skeleton(G, None, real_from=metric, **{**kw, "min_size": 2})
    # both sides by hand: the same augmented batches, the same latents
    data.gen = torch.Generator(device="cpu").manual_seed(2 + 1)
    data.set_image_size(32)
    lat = torch.Generator(device="cpu").manual_seed(2 + 2)
    by_hand = M.Skeleton(32, device=DEV)
    for i in range(0, 7, 3):
        b = min(3, 7 - i)
        by_hand.feed("real", data.batch([(i + j) % len(data) for j in range(b)]))
        z = torch.randn(b, G.latent_dim, generator=lat).clamp(-5, 5)
        with torch.no_grad():
            by_hand.feed("fake", G((z / z.norm(p=2, dim=1, keepdim=True)).to(DEV)))
    data.gen = own
    data.set_image_size(8)
    assert by_hand.result() == first
    other, m2 = M.evaluate_skeleton(G, data, return_metric=True, **{**kw, "seed": 3})
    assert not torch.equal(torch.cat(m2.values["real"], 1), torch.cat(metric.values["real"], 1))
    G8, _ = small_nets(ngan)                                                      # a stage below 16 x 16: said, not raised
    below = M.evaluate_skeleton(G8, data, **kw)
    assert below["images"] == 0 and "length" not in below and "16 x 16" in below["note"]


# ---- no side effects -----------------------------------------------------------------------------------------------------------------------
def same(x, y):
    if torch.is_tensor(x):
        return torch.is_tensor(y) and torch.equal(x, y)
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return isinstance(y, (list, tuple)) and len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    return x == y


def two_epochs(ngan, tmp_path, tag, skeleton_period, ema_beta):
    cfg = types.SimpleNamespace(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[1], N_epochs=2,
                                alpha_step=0.5, learning_rate=2e-3, checkpointing_period=1, ID=tag, skeleton_period=skeleton_period,
                                skeleton_images=6, skeleton_seed=1, skeleton_min_size=1)
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
    plain, saved0, lines0, _, _, rng0 = two_epochs(ngan, tmp_path, "k000", 0, ema_beta)
    scored, saved1, lines1, tr, f, rng1 = two_epochs(ngan, tmp_path, "k001", 1, ema_beta)
    assert tr.G.image_size == 16 and tr.has_graph((4, 1, 16, 16)), "the run did not train through a captured graph"
    assert plain == scored, "the monitor series changed when the metric was turned on"
    for key in ("Generator_state", "Discriminator_state", "optimizer_state") + (("Generator_ema_state",) if ema_beta else ()):
        assert key in saved0 and same(saved0[key], saved1[key]), f"{key} changed when the metric was turned on"
    for name, x, y in zip(("torch's CPU generator", "the device generator", "the data set's generator"), rng0, rng1):
        assert torch.equal(x, y), f"{name} ended in another state"
    assert "SKELETON" not in saved0 and not any("skeleton" in l for l in lines0)
    entries = saved1["SKELETON"]
    assert [e["epoch"] for e in entries] == [1, 2] and "MORPH" not in saved1 and "SWD" not in saved1 and "SPECTRUM" not in saved1
    base = {"epoch", "image_size", "images", "min_size", "skipped_real", "skipped_fake"}
    for e in entries:
        assert base <= set(e) and e["image_size"] == 16 and e["images"] == 6 and e["min_size"] == 1
        extra = set(e) - base
        if "note" in e:                                              # a side without a scored image: said, no statistic stored
            assert extra <= {"note", "skipped_fake_ema"}
        else:
            assert {n for n in extra if not n.endswith("_ema")} == set(SC.STATISTICS)
            assert all(set(e[n]) == {"real", "real_sem", "fake", "fake_sem", "ks"} and 0.0 <= e[n]["ks"] <= 1.0 for n in SC.STATISTICS)
        assert ("skipped_fake_ema" in e) == bool(ema_beta)
    assert entries[0]["skipped_real"] == entries[1]["skipped_real"]                                   # the same seed: the same data side
    if "length" in entries[0] and "length" in entries[1]:
        assert entries[0]["length"]["real"] == entries[1]["length"]["real"]
    assert len([l for l in lines1 if "skeleton" in l]) == 2
    # the eval tool prints the table for the checkpoint after the morphology table, and the averaged generator's after it when asked
    images = str(tmp_path / "images.pt")
    torch.save(torch.rand(8, 1, 16, 16, generator=torch.Generator().manual_seed(9)) * 2 - 1, images)
    capsys.readouterr()
    assert ngan.eval.main(["-weights", f, "--skeleton", "8", "--morph", "8", "--images", images] + (["--ema"] if ema_beta else [])) == 0
    out = capsys.readouterr().out
    n = 2 if ema_beta else 1
    assert out.count("Arbor skeleton") == n and out.count("Arbor morphology") == n
    assert out.count("Arbor skeleton, averaged generator") == (1 if ema_beta else 0)
    assert out.index("Arbor morphology") < out.index("Arbor skeleton")
    if ema_beta:
        assert out.rindex("Arbor morphology") < out.index("Arbor skeleton")
