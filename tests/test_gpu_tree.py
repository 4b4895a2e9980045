"""Arbor trees on the GPU: the kernels of csrc/tree.hip, through the C ABI of include/ngtree.h, against the restatement of
tests/tree_cases.py (definition and mask families are described there); then the Python layer: `tree_statistics`, `evaluate_tree` on
two sets that differ, and `export_arbors`.  Every integer output is compared exactly, and so is tip_cost, an integer held in fp64.
`contraction` is held to (n + 4) 2^-52 sum |terms| of the fp64 oracle, n the number of tips with a cost: every term is one square root
and two divisions of exactly converted integers, each rounded once (3 x 2^-53 relative, below 2^-51), and adding n terms in any order
rounds n - 1 times, each by at most 2^-53 of a partial sum that is below sum |terms|.  The means that tree_statistics forms on the Python
side in fp64 are held to 1e-12 relative plus that bound, as the other arbor tests hold theirs."""
import itertools
import os

import numpy as np
import pytest
import torch

import morph_cases as MC
import tree_cases as TC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-12
GUARD = -7


def dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def trace_abi(ngan, masks, centres, want_order=True):
    """ngtree_trace straight into the middle of guarded buffers: (cost, parent, order or None, stats, sums), the guards checked"""
    lib = ngan._C.lib()
    n, R = masks.shape[0], masks.shape[1]
    src, ctr = dev(masks), dev(centres, torch.int32)
    planes = [torch.full((n + 2, R, R), GUARD, device=DEV, dtype=torch.int32) for _ in range(3)]
    stats = torch.full((n + 2, 12), GUARD, device=DEV, dtype=torch.int32)
    sums = torch.full((n + 2, 2), float(GUARD), device=DEV, dtype=torch.float64)
    size = lib.ngtree_workspace_bytes(n, R)
    assert size == 17 * n * R * R
    ws = torch.full((size + 32,), 0x5A, device=DEV, dtype=torch.uint8)
    status = lib.ngtree_trace(src.data_ptr(), ctr.data_ptr(), planes[0][1].data_ptr(), planes[1][1].data_ptr(),
                              planes[2][1].data_ptr() if want_order else None, stats[1].data_ptr(), sums[1].data_ptr(), ws[16:].data_ptr(), n, R,
                              torch.cuda.current_stream().cuda_stream)
    assert status == 0, lib.ngan_last_error()
    torch.cuda.synchronize()
    for g in planes + [stats, sums]:
        assert bool((g[0] == GUARD).all()) and bool((g[-1] == GUARD).all()), "a guard slot was written"
    assert bool((ws[:16] == 0x5A).all()) and bool((ws[16 + size:] == 0x5A).all()), "the workspace was overrun"
    if not want_order:
        assert bool((planes[2] == GUARD).all()), "order was written without being asked for"
    assert torch.equal(src, dev(masks)) and torch.equal(ctr, dev(centres, torch.int32)), "an input was written"
    return planes[0][1:-1], planes[1][1:-1], planes[2][1:-1] if want_order else None, stats[1:-1], sums[1:-1]


def check_trace(ngan, masks, centres, refs, names, tag):
    cost, parent, order, stats, sums = trace_abi(ngan, masks, centres)
    got = [t.cpu().numpy() for t in (cost, parent, order, stats, sums)]
    for i, (name, ref) in enumerate(zip(names, refs)):
        st = dict(zip(TC.STAT_NAMES, got[3][i].tolist()))
        print(f"{tag} {name}: {st} sums {got[4][i].tolist()} (oracle contraction {ref['contraction']!r}, bound {TC.contraction_bound(ref['terms']):.3e})")
        assert got[3][i].tolist() == ref["stats"].tolist(), f"{tag} {name}: stats {st} != {dict(zip(TC.STAT_NAMES, ref['stats'].tolist()))}"
        for k, plane in zip(("cost", "parent", "order"), got[:3]):
            assert np.array_equal(plane[i], ref[k]), f"{tag} {name}: {(plane[i] != ref[k]).sum()} entries of {k} differ"
        assert got[4][i, 0] == float(ref["tip_cost"]), f"{tag} {name}: tip_cost {got[4][i, 0]} != {ref['tip_cost']}"
        assert abs(got[4][i, 1] - ref["contraction"]) <= TC.contraction_bound(ref["terms"]), \
            f"{tag} {name}: contraction {got[4][i, 1]!r} against {ref['contraction']!r}, bound {TC.contraction_bound(ref['terms'])!r}"
    bare = trace_abi(ngan, masks, centres, want_order=False)
    assert bare[2] is None and all(torch.equal(a, b) for a, b in zip((cost, parent, stats, sums), (bare[0], bare[1], bare[3], bare[4]))), \
        f"{tag}: the outputs differ without order"
    return cost, parent, order, stats, sums


# ---- the kernels against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", TC.SIZES)
def test_trace_against_the_restatement(ngan, size):
    """every family in one batch (16: the smallest legal size and one workgroup of 64 threads, 64: one labelling tile, 128: tile seams,
    dense masks that overflow the LDS list, and the `seam` node on pixel 63 / 64); then a second call, other non-zero bytes, and the
    first three images alone"""
    masks, centres, refs = TC.case(size)
    out = check_trace(ngan, masks, centres, refs, TC.FAMILIES, f"R={size}")
    again = trace_abi(ngan, masks, centres)
    assert all(torch.equal(a, b) for a, b in zip(out, again)), f"R={size}: two calls differ"
    bytes255 = trace_abi(ngan, masks * 255, centres)
    assert all(torch.equal(a, b) for a, b in zip(out, bytes255)), f"R={size}: a byte other than 1 is not taken as set"
    few = trace_abi(ngan, masks[:3], centres[:3])
    assert all(torch.equal(a[:3], b) for a, b in zip(out, few)), f"R={size}: an image's values depend on the rest of the batch"
    st = out[3].cpu().numpy().astype(np.int64)
    counts = ngan.metrics.skeleton_counts(dev(masks)).cpu().numpy()
    valid = centres[:, 0] >= 0
    assert np.array_equal(st[valid][:, [0, 2, 3]], counts[valid][:, [0, 4, 5]]), "pixels, orth and diag are not skeleton_counts'"
    assert np.array_equal(st[:, 4], st[:, 2] + st[:, 3] - st[:, 0] + st[:, 1]) and (st[:, 4] >= 0).all()


def test_trace_at_512(ngan):
    """the workload's size: the largest indices and costs (`seam`), a mask far beyond the LDS list (`checkerboard`: 131072 pixels, diag
    edges alone), the workload's own shape raw and thinned, and nothing"""
    masks, centres, refs = TC.case(512, TC.LARGE_FAMILIES)
    out = check_trace(ngan, masks, centres, refs, TC.LARGE_FAMILIES, "R=512")
    i = TC.LARGE_FAMILIES.index("empty")
    assert out[3][i].tolist() == [0] * 10 + [-1, 0] and out[4][i].tolist() == [0.0, 0.0]
    one = trace_abi(ngan, masks[1:2], centres[1:2])
    assert all(torch.equal(a[1:2], b) for a, b in zip(out, one))


def test_a_batch_in_every_order_gives_the_same_bits(ngan):
    names = ("thin:thick_arbor", "rings", "two_trees")
    pairs = [TC.family(n, 64) for n in names]
    masks, centres = np.stack([p[0] for p in pairs]), np.array([p[1] for p in pairs], np.int32)
    base = trace_abi(ngan, masks, centres)
    for perm in itertools.permutations(range(3)):
        got = trace_abi(ngan, masks[list(perm)], centres[list(perm)])
        for a, b in zip(base, got):
            assert torch.equal(a[list(perm)], b), f"order {perm}: an image's values depend on its place in the batch"


def test_images_without_a_root(ngan):
    """an empty mask about a centre inside the image, and set pixels about the soma of an empty mask, {-1, -1, 0}: background values,
    zero statistics, main_root = -1"""
    R = 32
    plus = TC.family("plus", R)[0]
    masks = np.stack([np.zeros((R, R), np.uint8), plus, plus])
    centres = np.array([[5, 7, 0], [-1, -1, 0], [R // 2, R // 2, 0]], np.int32)
    refs = [TC.trace_ref(m, c) for m, c in zip(masks, centres)]
    cost, parent, order, stats, sums = check_trace(ngan, masks, centres, refs, ("empty about (5, 7)", "plus without a soma", "plus"), "no root")
    for i in (0, 1):
        assert bool((cost[i] == -1).all()) and bool((parent[i] == -2).all()) and bool((order[i] == -1).all())
        assert stats[i].tolist() == [0] * 10 + [-1, 0] and sums[i].tolist() == [0.0, 0.0]
    assert stats[2, 0].item() == int(plus.sum()) and stats[2, 10].item() == (R // 2) * R + R // 2


def test_refusals_return_an_error_and_write_nothing(ngan):
    lib = ngan._C.lib()
    stream = torch.cuda.current_stream().cuda_stream
    R = 32
    mask, centre = TC.family("plus", R)[0], [R // 2, R // 2, 0]
    src = dev(np.stack([mask, mask]))
    ctr = dev(np.array([centre, centre]), torch.int32)
    outs = {"cost": torch.full((2, R, R), GUARD, device=DEV, dtype=torch.int32), "parent": torch.full((2, R, R), GUARD, device=DEV, dtype=torch.int32),
            "order": torch.full((2, R, R), GUARD, device=DEV, dtype=torch.int32), "stats": torch.full((2, 12), GUARD, device=DEV, dtype=torch.int32),
            "sums": torch.full((2, 2), float(GUARD), device=DEV, dtype=torch.float64)}
    ws = torch.zeros(lib.ngtree_workspace_bytes(2, R) + 16, device=DEV, dtype=torch.uint8)
    sentinel = {k: v.clone() for k, v in outs.items()}
    p = dict({k: v.data_ptr() for k, v in outs.items()}, src=src.data_ptr(), centre=ctr.data_ptr(), w=ws.data_ptr())
    ARG, SHAPE = -1, -2                                                 # NGAN_ERR_ARG, NGAN_ERR_SHAPE (include/ngan.h)

    def trace(B=1, R=R, **kw):
        a = dict(p, **kw)
        return lib.ngtree_trace(a["src"], a["centre"], a["cost"], a["parent"], a["order"], a["stats"], a["sums"], a["w"], B, R, stream)
    cases = [({"R": 8}, SHAPE, "R=8"), ({"R": 24}, SHAPE, "R=24"), ({"R": 1024}, SHAPE, "R=1024"), ({"B": 0}, SHAPE, "B=0"),
             ({"B": 65536}, SHAPE, "B=65536"), ({"src": p["src"] + 1}, ARG, "16-byte"), ({"cost": p["cost"] + 4}, ARG, "16-byte"),
             ({"parent": p["parent"] + 8}, ARG, "16-byte"), ({"order": p["order"] + 4}, ARG, "16-byte"), ({"w": p["w"] + 8}, ARG, "16-byte"),
             ({"sums": p["sums"] + 4}, ARG, "8-byte"), ({"centre": p["centre"] + 2}, ARG, "4-byte"), ({"stats": p["stats"] + 1}, ARG, "4-byte"),
             ({"src": None}, ARG, "null"), ({"centre": None}, ARG, "null"), ({"cost": None}, ARG, "null"), ({"parent": None}, ARG, "null"),
             ({"stats": None}, ARG, "null"), ({"sums": None}, ARG, "null"), ({"w": None}, ARG, "null")]
    for kw, code, word in cases:
        assert trace(**kw) == code, kw
        assert word in lib.ngan_last_error().decode(), (kw, lib.ngan_last_error())
    torch.cuda.synchronize()
    for k in outs:
        assert torch.equal(outs[k], sentinel[k]), f"a refused call wrote {k}"
    assert trace() == 0                                                                           # one image of the two
    torch.cuda.synchronize()
    ref = TC.trace_ref(mask, centre)
    assert outs["stats"][0].tolist() == ref["stats"].tolist() and np.array_equal(outs["cost"][0].cpu().numpy(), ref["cost"])
    assert outs["stats"][0, [1, 4, 6, 7]].tolist() == [1, 0, 4, 1]                                # one tree, no cycle, four tips, one fork
    for k in outs:
        assert torch.equal(outs[k][1], sentinel[k][1]), f"{k} of the image that was not asked for changed"


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def close(a, b, slack=0.0):
    return (np.isnan(a) and np.isnan(b)) or abs(a - b) <= RTOL * max(1.0, abs(b)) + slack


def test_arbor_tree_returns_the_abi_outputs(ngan):
    M = ngan.metrics
    masks, centres, refs = TC.case(64)
    t = M.arbor_tree(dev(masks), dev(centres, torch.int32))
    assert set(t) == {"cost", "parent", "order", "stats", "sums"} and t["sums"].dtype == torch.float64 and tuple(t["stats"].shape) == (len(masks), 12)
    base = trace_abi(ngan, masks, centres)
    assert all(torch.equal(t[k], b) for k, b in zip(("cost", "parent", "order", "stats", "sums"), base))
    bare = M.arbor_tree(dev(masks), dev(centres, torch.int32), want_order=False)
    assert bare["order"] is None and torch.equal(bare["stats"], t["stats"]) and torch.equal(bare["sums"], t["sums"])


@pytest.mark.parametrize("size", (32, 64, 128))
def test_tree_statistics_of_mask_images(ngan, size):
    """images whose level is 200 on the mask and 20 off it, cut at the fixed threshold 100: thick and thin families; min_size 1 and 4"""
    M = ngan.metrics
    names = ("thick_arbor", "plus3", "bar3", "frame", "disc", "arbor", "burrs", "loop", "rings", "random41", "empty", "full")
    masks = np.stack([TC.BC.family(f, size) for f in names])
    img = np.where(masks != 0, 200, 20).astype(np.uint8)
    x = dev(MC.from_bytes(img)[..., None])
    for kw in (dict(), dict(min_size=4)):
        st = M.tree_statistics(x, threshold=100, **kw)
        assert set(st) == set(TC.STATISTICS) | {"scored"} and all(st[n].dtype == torch.float64 and st[n].is_cuda for n in TC.STATISTICS)
        for i, name in enumerate(names):
            sk, _, soma, t, kept_area = TC.chain_ref(masks[i], **kw)
            ref = TC.statistics_of(size, kept_area, t["stats"], t["tip_cost"], t["contraction"])
            assert bool(st["scored"][i]) == ref["scored"], (size, kw, name)
            for n in ("trees", "cycles", "tips", "forks", "max_order"):
                assert float(st[n][i]) == ref[n], (size, kw, name, n, float(st[n][i]), ref[n])
            for n in ("path_max", "path_mean"):
                assert close(float(st[n][i]), ref[n]), (size, kw, name, n, float(st[n][i]), ref[n])
            slack = TC.contraction_bound(t["terms"]) / max(1.0, ref["tips"])
            assert close(float(st["contraction"][i]), ref["contraction"], slack), (size, kw, name, float(st["contraction"][i]), ref["contraction"])


class StubGenerator(torch.nn.Module):
    """hands out a fixed set of images, one minibatch per call, in order"""

    def __init__(self, images):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=DEV))
        self.images, self.at = images.to(DEV), 0
        self.image_size, self.latent_dim, self.N_colors = int(images.shape[1]), 8, 1

    def forward(self, z):
        out = self.images[self.at:self.at + z.shape[0]]
        self.at += z.shape[0]
        return out


class StubDataset:
    def __init__(self, images):
        self.images, self.image_size = images.to(DEV), int(images.shape[1])

    def __len__(self):
        return self.images.shape[0]

    def set_image_size(self, size):
        assert size == self.images.shape[1]

    def batch(self, idx):
        return self.images[idx]


def test_cut_trees_separate_through_evaluate_tree(ngan):
    """sixteen dilated random-walk trees at 64 x 64 as the data and the same trees cut along every sixth row and column as the samples,
    through images whose class above t0 is the mask, in uneven minibatches: every expected value is tree_result_ref's, and the cut set
    separates on `trees` and on `path_max` (KS 1)"""
    M = ngan.metrics
    whole, cut = TC.separation_sets()
    xw, xc = (torch.from_numpy(MC.mask_images(m, s)[1]) for m, s in ((whole, 5), (cut, 6)))
    G, data = StubGenerator(xc), StubDataset(xw)
    res, metric = M.evaluate_tree(G, data, n_images=16, batch_size=5, seed=1, return_metric=True)
    print(M.format_tree(res))
    ref = TC.tree_result_ref([TC.tree_statistics_ref(m) for m in whole], [TC.tree_statistics_ref(m) for m in cut])
    assert isinstance(metric, M.Tree) and set(res) == set(ref) and (res["images"], res["skipped_real"], res["skipped_fake"]) == (16, 0, 0)
    for name in TC.STATISTICS:
        for k, v in ref[name].items():
            assert close(res[name][k], v, 1e-13 if name == "contraction" else 0.0), (name, k, res[name][k], v)
    assert res["trees"]["ks"] == 1.0 and res["path_max"]["ks"] == 1.0 and res["trees"]["real"] == 1.0
    assert len(M.format_tree(res).splitlines()) == 2 + 8
    G.at = 0
    assert M.evaluate_tree(G, None, n_images=16, batch_size=5, seed=1, real_from=metric) == res
    with pytest.raises(ValueError):
        M.evaluate_tree(G, None, n_images=16, batch_size=5, seed=1, min_size=2, real_from=metric)


def test_export_arbors_writes_files_that_read_back(ngan, tmp_path):
    M = ngan.metrics
    names = ("thick_arbor", "two_trees", "loop", "ring_tie")
    masks = np.stack([(TC.family(n, 64)[0] if n in TC.NEW_FAMILIES else TC.BC.family(n, 64)) for n in names])
    x = dev(MC.mask_images(masks, 3)[1])
    rows = M.export_arbors(x.permute(0, 3, 1, 2).contiguous(), str(tmp_path), "probe", first=7)
    more = M.export_arbors(x[:1], str(tmp_path), "main", fragments=False)
    assert sorted(os.listdir(tmp_path)) == sorted(["arbors.csv", "main_0000.swc", "main_0000.png"] + [f"probe_{7 + i:04d}.{e}" for i in range(4) for e in ("swc", "png")])
    table = open(tmp_path / "arbors.csv").read().splitlines()
    assert table[0].split(",") == list(M.ARBOR_CSV) and len(table) == 1 + 5 and [r["file"] for r in rows + more] == [l.split(",")[0] for l in table[1:]]
    from PIL import Image
    levels = M.morph_levels(x)[0].cpu().numpy()
    for i, name in enumerate(names):
        sk, dist2, soma, ref, kept_area = TC.chain_ref(masks[i])
        comments, nodes = TC.read_swc(tmp_path / f"probe_{7 + i:04d}.swc")
        assert len(comments) == 4 and np.array_equal(np.asarray(Image.open(tmp_path / f"probe_{7 + i:04d}.png")), levels[i])
        stats = TC.statistics_of(64, kept_area, ref["stats"], ref["tip_cost"], ref["contraction"])
        assert rows[i]["scored"] == int(stats["scored"]) and rows[i]["trees"] == stats["trees"] and rows[i]["cycles"] == stats["cycles"]
        TC.check_swc(nodes, sk, soma)                                    # the rasterised nodes are the oracle's skeleton: the kernel's too
        assert rows[i]["soma"] == float(np.sqrt(np.float64(soma[2])))
    sk, _, soma, ref, _ = TC.chain_ref(masks[0])
    TC.check_swc(TC.read_swc(tmp_path / "main_0000.swc")[1], sk, soma, int(ref["stats"][11]))
    kernel_sk, _ = M.thin(M._kept_mask(x, 1, 1, None)[3])
    for i in range(3):
        nodes = TC.read_swc(tmp_path / f"probe_{7 + i:04d}.swc")[1]
        TC.check_swc(nodes, kernel_sk[i].cpu().numpy(), TC.chain_ref(masks[i])[2])


# ---- eval.py ---------------------------------------------------------------------------------------------------------------------------------
def test_eval_prints_the_tree_table_and_exports_swc(ngan, tmp_path, capsys):
    """--tree prints its table after the others; --swc writes samples of the generator and of the data; without them nothing of either"""
    torch.manual_seed(3)
    G = ngan.models.Generator_PG([32, 16, 16], image_size_init=8, latent_dim=32).to(DEV)
    D = ngan.models.Discriminator_PG([16, 16, 32], image_size_init=8).to(DEV)
    G.set_resolution(32, 1.0)
    D.set_resolution(32, 1.0)
    f = str(tmp_path / "GenDisc_tree.pth")
    ngan.utils.Checkpointer(G, D, 1e-3, f, N_epochs=2, verbose=False, device=torch.device(DEV), trainer=ngan.train.PGGANTrainer(G, D)).save_state(1)
    images = str(tmp_path / "images.pt")
    torch.save(torch.rand(8, 1, 32, 32, generator=torch.Generator().manual_seed(9)) * 2 - 1, images)
    out_dir = tmp_path / "arbors"
    capsys.readouterr()
    assert ngan.eval.main(["-weights", f, "--branches", "8", "--images", images]) == 0
    out = capsys.readouterr().out
    assert "Arbor branches" in out and "Arbor trees" not in out and not out_dir.exists()
    assert ngan.eval.main(["-weights", f, "--tree", "8", "--branches", "8", "--tree_min_size", "2", "--images", images, "--swc", str(out_dir),
                           "--swc_count", "3", "--swc_seed", "4", "--swc_main_only"]) == 0
    out = capsys.readouterr().out
    assert out.count("Arbor trees, training generator of") == 1 and out.index("Arbor branches") < out.index("Arbor trees")
    want = ["arbors.csv"] + [f"{p}_{i:04d}.{e}" for p in ("generated", "data") for i in range(3) for e in ("swc", "png")]
    assert sorted(os.listdir(out_dir)) == sorted(want)
    assert len(open(out_dir / "arbors.csv").read().splitlines()) == 1 + 6
    for name in want[1::2]:
        comments, nodes = TC.read_swc(out_dir / name)
        assert len(comments) == 4 and "main tree alone" in comments[2] and sum(n[6] == -1 for n in nodes) <= 1
        assert [n[0] for n in nodes] == list(range(1, len(nodes) + 1)) and all(n[6] < n[0] for n in nodes)
