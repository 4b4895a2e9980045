"""Arbor branches on the GPU: the kernels of csrc/branch.hip against the restatement of tests/branch_cases.py (definitions and mask
families are described there), the metric on known sets, `evaluate_branches`, and its promise to leave a run alone.  Every kernel output
is an integer and is compared exactly.  The three lengths that branch_statistics forms on the Python side in fp64 are held to 1e-12
relative, the bound of the arbor-geometry tests for their fp64 summaries: each is two integer-to-fp64 conversions (exact), one product
with sqrt 2, one sum and two quotients, five roundings of 2^-53 each at most on either side."""
import types

import numpy as np
import pytest
import torch

import branch_cases as BC
import morph_cases as MC
import skeleton_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-12
SPURS = (1, 2, 4)


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def close(a, b):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= RTOL * max(1.0, abs(b))


def check_graph(M, masks, refs, names, spur, tag):
    """labels, stats and hist of a batch against the reference triples; returns the three tensors"""
    labels, stats, hist = M.branch_graph(dev(masks), spur, want_labels=True)
    n, R = masks.shape[0], masks.shape[1]
    assert tuple(labels.shape) == (n, R, R) and labels.dtype == torch.int32 and tuple(stats.shape) == (n, 20) and stats.dtype == torch.int32
    assert tuple(hist.shape) == (n, 64) and hist.dtype == torch.int32
    got_l, got_s, got_h = labels.cpu().numpy(), stats.cpu().numpy(), hist.cpu().numpy()
    for i, (name, (l, s, h)) in enumerate(zip(names, refs)):
        print(f"{tag} spur={spur} {name}: {dict(zip(BC.STAT_NAMES, got_s[i].tolist()))}")
        assert got_s[i].tolist() == s.tolist(), f"{tag} spur={spur} {name}: stats {dict(zip(BC.STAT_NAMES, got_s[i].tolist()))} != {dict(zip(BC.STAT_NAMES, s.tolist()))}"
        assert got_h[i].tolist() == h.tolist(), f"{tag} spur={spur} {name}: hist {got_h[i].tolist()} != {h.tolist()}"
        assert np.array_equal(got_l[i], l), f"{tag} spur={spur} {name}: {(got_l[i] != l).sum()} labels differ"
    return labels, stats, hist


# ---- the graph against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", BC.SIZES)
def test_graph_against_the_restatement(ngan, size):
    """every family, raw and thinned, in one batch at spur 1, 2 and 4 (16: one workgroup per image, 128: 64 and the `seam` node on pixel
    63 / 64); then 3 images and 1 image of the same, a second call, no labels, other non-zero bytes, both identities against
    skeleton_counts, and a call straight into the middle of guarded buffers"""
    M = ngan.metrics
    masks = BC.case(size)
    tag = f"R={size}"
    src = dev(masks)
    counts = M.skeleton_counts(src).cpu().numpy()
    for spur in SPURS:
        labels, stats, hist = check_graph(M, masks, BC.reference(size, spur), BC.FAMILIES, spur, tag)
        for n in (3, 1):
            l, s, h = M.branch_graph(dev(masks[:n]), spur, want_labels=True)
            assert torch.equal(l, labels[:n]) and torch.equal(s, stats[:n]) and torch.equal(h, hist[:n]), \
                f"{tag} B={n}: an image's values depend on the rest of the batch"
        l, s, h = M.branch_graph(src, spur, want_labels=True)
        assert torch.equal(l, labels) and torch.equal(s, stats) and torch.equal(h, hist), f"{tag}: two calls differ"
        l, s, h = M.branch_graph(src, spur)
        assert l is None and torch.equal(s, stats) and torch.equal(h, hist), f"{tag}: stats or hist differ without labels"
        l, s, h = M.branch_graph(dev(masks * 255), spur, want_labels=True)                      # any non-zero byte is set
        assert torch.equal(l, labels) and torch.equal(s, stats) and torch.equal(h, hist)
        st = stats.cpu().numpy().astype(np.int64)
        assert np.array_equal(st[:, 3], st[:, 4] + st[:, 5] + st[:, 6] + st[:, 7]), f"{tag}: branches != terminal + links + free + spurs"
        assert np.array_equal(st[:, [8, 10, 12, 14, 16]].sum(1), counts[:, 4]), f"{tag}: the orth sums are not skeleton_counts' orth"
        assert np.array_equal(st[:, [9, 11, 13, 15, 17]].sum(1), counts[:, 5]), f"{tag}: the diag sums are not skeleton_counts' diag"
        assert np.array_equal(st[:, 0], counts[:, 0])
    lib = ngan._C.lib()
    n = len(masks)
    g_labels = torch.full((n + 2, size, size), -7, device=DEV, dtype=torch.int32)                 # one slot of guard before and after
    g_stats = torch.full((n + 2, 20), -7, device=DEV, dtype=torch.int32)
    g_hist = torch.full((n + 2, 64), -7, device=DEV, dtype=torch.int32)
    ws = torch.empty(lib.ngan_branch_workspace_bytes(n, size), device=DEV, dtype=torch.uint8)
    assert ws.numel() == 13 * n * size * size
    assert lib.ngan_branch_graph(src.data_ptr(), g_labels[1].data_ptr(), g_stats[1].data_ptr(), g_hist[1].data_ptr(), ws.data_ptr(), n, size,
                                 SPURS[-1], torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(g_labels[1:-1], labels) and torch.equal(g_stats[1:-1], stats) and torch.equal(g_hist[1:-1], hist)
    for g in (g_labels, g_stats, g_hist):
        assert bool((g[0] == -7).all()) and bool((g[-1] == -7).all())


def test_graph_at_512(ngan):
    """the workload's size: the largest indices (`seam`, whose arms reach pixel 509), the densest node (`checkerboard`: one node of
    130050 pixels), the workload's own shape raw and thinned, and nothing; spur 1, 2, 4 and the default, 16"""
    M = ngan.metrics
    masks = BC.case(512, BC.LARGE_FAMILIES)
    assert BC.default_spur(512) == 16 == M.default_spur(512)
    for spur in SPURS + (16,):
        labels, stats, hist = check_graph(M, masks, BC.reference(512, spur, BC.LARGE_FAMILIES), BC.LARGE_FAMILIES, spur, "R=512")
        l, s, h = M.branch_graph(dev(masks[1:2]), spur)
        assert l is None and torch.equal(s, stats[1:2]) and torch.equal(h, hist[1:2])
    assert not bool(stats[BC.LARGE_FAMILIES.index("empty")].any()) and not bool(hist[BC.LARGE_FAMILIES.index("empty")].any())
    assert stats[BC.LARGE_FAMILIES.index("checkerboard"), 2].item() == 1


def test_refusals_return_an_error_and_write_nothing(ngan):
    lib = ngan._C.lib()
    stream = torch.cuda.current_stream().cuda_stream
    mask = torch.from_numpy(SC.family("plus", 32)).to(DEV).repeat(2, 1, 1).contiguous()
    outs = {"labels": torch.full((2, 32, 32), -7, device=DEV, dtype=torch.int32), "stats": torch.full((2, 20), -7, device=DEV, dtype=torch.int32),
            "hist": torch.full((2, 64), -7, device=DEV, dtype=torch.int32)}
    assert lib.ngan_branch_workspace_bytes(2, 8) == 0 and lib.ngan_branch_workspace_bytes(2, 1024) == 0
    assert lib.ngan_branch_workspace_bytes(0, 32) == 0 and lib.ngan_branch_workspace_bytes(65536, 32) == 0
    ws = torch.zeros(lib.ngan_branch_workspace_bytes(2, 32) + 16, device=DEV, dtype=torch.uint8)
    sentinel = {k: v.clone() for k, v in outs.items()}
    p = {k: v.data_ptr() for k, v in outs.items()}
    ARG, SHAPE = -1, -2                                                 # NGAN_ERR_ARG, NGAN_ERR_SHAPE (include/ngan.h)

    def graph(src=mask.data_ptr(), labels=p["labels"], stats=p["stats"], hist=p["hist"], w=ws.data_ptr(), B=1, R=32, spur=1):
        return lib.ngan_branch_graph(src, labels, stats, hist, w, B, R, spur, stream)
    cases = [({"R": 8}, SHAPE, "R=8"), ({"R": 1024}, SHAPE, "R=1024"), ({"R": 48}, SHAPE, "R=48"), ({"B": 0}, SHAPE, "B=0"),
             ({"B": 65536}, SHAPE, "B=65536"), ({"spur": 0}, ARG, "spur=0"), ({"spur": -3}, ARG, "spur=-3"),
             ({"src": mask.data_ptr() + 1}, ARG, "16-byte"), ({"labels": p["labels"] + 4}, ARG, "16-byte"), ({"w": ws.data_ptr() + 8}, ARG, "16-byte"),
             ({"stats": p["stats"] + 2}, ARG, "4-byte"), ({"hist": p["hist"] + 1}, ARG, "4-byte"),
             ({"src": None}, ARG, "null"), ({"stats": None}, ARG, "null"), ({"hist": None}, ARG, "null"), ({"w": None}, ARG, "null")]
    for kw, code, word in cases:
        assert graph(**kw) == code, kw
        assert word in lib.ngan_last_error().decode(), (kw, lib.ngan_last_error())
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], sentinel[k]), f"a refused call wrote {k}"
    assert graph() == 0                                                                           # one image of the two
    torch.cuda.synchronize()
    _, s, h = BC.graph_ref(SC.family("plus", 32), 1)
    assert outs["stats"][0].tolist() == s.tolist() and outs["hist"][0].tolist() == h.tolist()
    assert outs["stats"][0, [2, 4, 19]].tolist() == [1, 4, 1] and outs["hist"][0, 13:15].tolist() == [2, 2]      # arms of 13, 13, 14, 14
    for k in outs:
        assert torch.equal(outs[k][1], sentinel[k][1]), f"{k} of the image that was not asked for changed"


# ---- the whole chain -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", (32, 64, 128))
def test_branch_statistics_of_mask_images(ngan, size):
    """images whose level is 200 on the mask and 20 off it, cut at the fixed threshold 100: the thick and the thin families; the default
    spur and spur 3, min_size 1 and 4"""
    M = ngan.metrics
    names = ("thick_arbor", "plus3", "bar3", "frame", "disc", "arbor", "burrs", "loop", "double_t", "random41", "empty", "full")
    masks = np.stack([BC.family(f, size) for f in names])
    img = np.where(masks != 0, 200, 20).astype(np.uint8)
    x = dev(MC.from_bytes(img)[..., None])
    for kw in (dict(), dict(spur=3, min_size=4), dict(spur=1)):
        st = M.branch_statistics(x, threshold=100, **kw)
        assert set(st) == set(BC.STATISTICS) | {"scored", "hist"}
        assert all(st[n].dtype == torch.float64 and st[n].is_cuda for n in BC.STATISTICS) and st["hist"].dtype == torch.int32
        for i, name in enumerate(names):
            ref = BC.branch_statistics_ref(masks[i], min_size=kw.get("min_size", 1), spur=kw.get("spur"))
            assert bool(st["scored"][i]) == ref["scored"], (size, kw, name)
            assert st["hist"][i].tolist() == ref["hist"].tolist(), (size, kw, name)
            for n in ("forks", "nodes", "terminals", "spurs"):
                assert float(st[n][i]) == ref[n], (size, kw, name, n, float(st[n][i]), ref[n])
            for n in ("terminal_length", "link_length", "longest"):
                assert close(float(st[n][i]), ref[n]), (size, kw, name, n, float(st[n][i]), ref[n])


def compare_results(res, ref):
    assert set(res) == set(ref) and (res["images"], res["skipped_real"], res["skipped_fake"]) == (ref["images"], 0, 0)
    for name in BC.STATISTICS:
        for k, v in ref[name].items():
            assert close(res[name][k], v), (name, k, res[name][k], v)
    for k in ("length", "real", "fake"):
        assert len(res["profile"][k]) == len(ref["profile"][k]), k
        assert all(close(a, b) for a, b in zip(res["profile"][k], ref["profile"][k])), k


@pytest.mark.parametrize("spur", (None, 4))
def test_burrs_separate_spurs_and_nodes_not_forks(ngan, spur):
    """the skeletons of sixteen `thick_arbor` trees at 64 x 64 against the same skeletons with two-pixel burrs, through images whose class
    above t0 is the mask; fed in uneven minibatches, one side as (B, C, R, R).  Every expected value is branches_ref's: burrs add nodes
    and spurs to every tree (KS 1); at spur 4, which prunes them, the forks move by a fraction of one per tree, and at the default
    spur of this size, 2, they move by what the reference says"""
    M = ngan.metrics
    W, burred = BC.separation_sets()
    xw, xb = (torch.from_numpy(MC.mask_images(m, s)[1]) for m, s in ((W, 5), (burred, 6)))
    m = M.Branches(64, device=DEV, spur=spur)
    assert m.spur == (2 if spur is None else spur)
    for lo, hi in ((0, 1), (1, 7), (7, 16)):
        m.feed("real", xw[lo:hi].permute(0, 3, 1, 2).contiguous())
        m.feed("fake", xb[lo:hi])
    res = m.result()
    print(M.format_branches(res))
    ref = BC.branches_ref([BC.branch_statistics_ref(x, spur=spur) for x in W], [BC.branch_statistics_ref(x, spur=spur) for x in burred], 64)
    compare_results(res, ref)
    assert ref["spurs"]["ks"] == 1.0 and ref["nodes"]["ks"] == 1.0 and res["spurs"]["ks"] == 1.0 and res["nodes"]["ks"] == 1.0
    assert abs(res["forks"]["fake"] - res["forks"]["real"]) <= abs(ref["forks"]["fake"] - ref["forks"]["real"]) * (1 + RTOL)
    if spur == 4:
        assert abs(ref["forks"]["fake"] - ref["forks"]["real"]) < 1.0 and ref["nodes"]["fake"] > 2 * ref["nodes"]["real"]
    assert len(M.format_branches(res).splitlines()) == 2 + 7 + 2
    m.feed("real", xw[:1])
    with pytest.raises(ValueError):
        m.result()


# ---- evaluate_branches ---------------------------------------------------------------------------------------------------------------------
def small_nets(ngan, widths=(32, 16)):
    G = ngan.models.Generator_PG(list(widths), image_size_init=8, latent_dim=32).to(DEV)
    D = ngan.models.Discriminator_PG(list(widths)[::-1], image_size_init=8).to(DEV)
    return G, D


def small_dataset(ngan, size=16):
    g = torch.Generator().manual_seed(9)
    return ngan.data.NeuronDataset(torch.rand(8, 1, size, size, generator=g), augmentations=True, im_translation=0.05, device=DEV, seed=3)


def test_evaluate_branches_is_seeded_and_leaves_no_trace(ngan):
    M = ngan.metrics
    torch.manual_seed(7)
    G, _ = small_nets(ngan, (32, 16, 16))
    G.set_resolution(32, 1.0)
    data = small_dataset(ngan, 32)
    data.set_image_size(8)
    host_rng, device_rng, aug = torch.get_rng_state(), torch.cuda.get_rng_state(DEV), data.gen.get_state()
    own = data.gen
    kw = dict(n_images=7, batch_size=3, seed=2)
    first, metric = M.evaluate_branches(G, data, return_metric=True, **kw)
    assert isinstance(metric, M.Branches) and first["images"] == 7 and metric.count == {"real": 7, "fake": 7} and metric.spur == 2
    assert torch.equal(torch.get_rng_state(), host_rng), "torch's global generator was consumed"
    assert torch.equal(torch.cuda.get_rng_state(DEV), device_rng), "the device generator was consumed"
    assert data.gen is own and torch.equal(data.gen.get_state(), aug) and data.image_size == 8, "the data set's stream or stage moved"
    assert M.evaluate_branches(G, data, **kw) == first                            # seeded: the same numbers again
    assert M.evaluate_branches(G, None, real_from=metric, **kw) == first          # the data's side taken over, the data set untouched
    assert M.evaluate_branches(G, None, real_from=metric, spur=2, **kw) == first  # the default, spelled out
    with pytest.raises(ValueError):
        M.evaluate_branches(G, None, real_from=metric, **{**kw, "min_size": 2})
    with pytest.raises(ValueError):
        M.evaluate_branches(G, None, real_from=metric, spur=3, **kw)
    G8, _ = small_nets(ngan)                                                      # a stage below 16 x 16: said, not raised
    below = M.evaluate_branches(G8, data, **kw)
    assert below["images"] == 0 and "forks" not in below and "16 x 16" in below["note"]


# ---- no side effects -----------------------------------------------------------------------------------------------------------------------
def same(x, y):
    if torch.is_tensor(x):
        return torch.is_tensor(y) and torch.equal(x, y)
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return isinstance(y, (list, tuple)) and len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    return x == y


def two_epochs(ngan, tmp_path, tag, branch_period, ema_beta):
    cfg = types.SimpleNamespace(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[1], N_epochs=2,
                                alpha_step=0.5, learning_rate=2e-3, checkpointing_period=1, ID=tag, branch_period=branch_period,
                                branch_images=6, branch_seed=1, branch_min_size=1, branch_spur=0)
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
    plain, saved0, lines0, _, _, rng0 = two_epochs(ngan, tmp_path, "b000", 0, ema_beta)
    scored, saved1, lines1, tr, f, rng1 = two_epochs(ngan, tmp_path, "b001", 1, ema_beta)
    assert tr.G.image_size == 16 and tr.has_graph((4, 1, 16, 16)), "the run did not train through a captured graph"
    assert plain == scored, "the monitor series changed when the metric was turned on"
    for key in ("Generator_state", "Discriminator_state", "optimizer_state") + (("Generator_ema_state",) if ema_beta else ()):
        assert key in saved0 and same(saved0[key], saved1[key]), f"{key} changed when the metric was turned on"
    for name, x, y in zip(("torch's CPU generator", "the device generator", "the data set's generator"), rng0, rng1):
        assert torch.equal(x, y), f"{name} ended in another state"
    assert "BRANCH" not in saved0 and not any("branches" in l for l in lines0)
    entries = saved1["BRANCH"]
    assert [e["epoch"] for e in entries] == [1, 2] and "SHOLL" not in saved1 and "SKELETON" not in saved1 and "MORPH" not in saved1
    base = {"epoch", "image_size", "images", "min_size", "spur", "skipped_real", "skipped_fake"}
    for e in entries:
        assert base <= set(e) and e["image_size"] == 16 and e["images"] == 6 and e["min_size"] == 1 and e["spur"] == 2
        extra = set(e) - base
        if "note" in e:                                              # a side without a scored image: said, no statistic stored
            assert extra <= {"note", "skipped_fake_ema"}
        else:
            assert {n for n in extra if not n.endswith("_ema")} == set(BC.STATISTICS) | {"profile"}
            assert all(set(e[n]) == {"real", "real_sem", "fake", "fake_sem", "ks"} and 0.0 <= e[n]["ks"] <= 1.0 for n in BC.STATISTICS)
            prof = e["profile"]
            assert set(prof) == {"length", "real", "fake"} and len(prof["length"]) == len(prof["real"]) == len(prof["fake"]) <= 64
            assert all(isinstance(v, float) for k in prof for v in prof[k])
            if ema_beta and "forks_ema" in e:
                assert {n for n in extra if n.endswith("_ema")} == {n + "_ema" for n in BC.STATISTICS} | {"profile_ema", "skipped_fake_ema"}
                assert set(e["forks_ema"]) == {"fake", "fake_sem", "ks"} and len(e["profile_ema"]["fake"]) == len(prof["length"])
        assert ("skipped_fake_ema" in e) == bool(ema_beta)
    assert entries[0]["skipped_real"] == entries[1]["skipped_real"]                                   # the same seed: the same data side
    if "forks" in entries[0] and "forks" in entries[1]:
        assert entries[0]["forks"]["real"] == entries[1]["forks"]["real"]
    assert len([l for l in lines1 if "branches" in l]) == 2
    # the eval tool prints the table for the checkpoint after the geometry table, and the averaged generator's after it when asked
    images = str(tmp_path / "images.pt")
    torch.save(torch.rand(8, 1, 16, 16, generator=torch.Generator().manual_seed(9)) * 2 - 1, images)
    capsys.readouterr()
    assert ngan.eval.main(["-weights", f, "--branches", "8", "--sholl", "8", "--branch_spur", "3", "--images", images]
                          + (["--ema"] if ema_beta else [])) == 0
    out = capsys.readouterr().out
    n = 2 if ema_beta else 1
    assert out.count("Arbor branches") == n and out.count("Arbor geometry") == n
    assert out.count("Arbor branches, averaged generator") == (1 if ema_beta else 0)
    assert out.index("Arbor geometry") < out.index("Arbor branches")
    if ema_beta:
        assert out.rindex("Arbor geometry") < out.index("Arbor branches")
