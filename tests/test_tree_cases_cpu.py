"""CPU-only checks of the arbor-tree reference (tests/tree_cases.py): the Dijkstra oracle against a naive Bellman-Ford, the invariants
of the definition on every family and size, the separation experiment on two sets of masks, and the SWC writer of metrics.py on the
oracle's arrays (plain host code: no GPU)."""
import numpy as np
import pytest

import branch_cases as BC
import morph_cases as MC
import tree_cases as TC


@pytest.mark.parametrize("size", (16, 32))
def test_dijkstra_agrees_with_bellman_ford(size):
    masks, centres, refs = TC.case(size)
    for name, m, c, ref in zip(TC.FAMILIES, masks, centres, refs):
        if c[0] < 0:
            continue
        adj = TC.graph(m)
        roots = set(TC.roots_of(m, c)[0].values())
        slow = TC.bellman_ford(adj, roots)
        got = {p: int(ref["cost"].ravel()[p]) for p in adj}
        assert slow == got, name


@pytest.mark.parametrize("size", TC.SIZES)
def test_invariants_of_the_definition(size):
    masks, centres, refs = TC.case(size)
    R = size
    for name, m, c, ref in zip(TC.FAMILIES, masks, centres, refs):
        cost, parent, order = (ref[k].ravel() for k in ("cost", "parent", "order"))
        st = dict(zip(TC.STAT_NAMES, ref["stats"].tolist()))
        on = m.ravel() != 0
        if c[0] < 0:                                                     # the soma of an empty mask: nothing set
            assert not on.any() and st == dict(dict.fromkeys(TC.STAT_NAMES, 0), main_root=-1), name
            continue
        assert (cost[on] >= 0).all() and (cost[~on] == -1).all() and (parent[~on] == -2).all() and (order[~on] == -1).all(), name
        weight = {(p, q): w for p, qs in TC.graph(m).items() for q, w in qs}
        for p in np.flatnonzero(on):
            q = int(parent[p])
            if q < 0:
                assert q == -1 and cost[p] == 0 and order[p] == 0, name
            else:
                assert cost[q] + weight[(int(p), q)] == cost[p] and order[q] <= order[p] <= order[q] + 1, (name, p)
        assert st["cycles"] >= 0 and st["trees"] == int((parent == -1).sum()) and st["tips"] <= st["leaves"], name
        assert st["pixels"] == int(on.sum()) and 0 < st["main_pixels"] <= st["pixels"] and parent[st["main_root"]] == -1, name
        assert st["path_max"] == cost.max() and st["max_order"] == order.max(), name
        assert all(0.0 < t <= 1.0 + 2e-6 for t in ref["terms"]), name          # no path is shorter than the straight line
        rev = 0.0
        for t in reversed(ref["terms"]):
            rev += t
        assert abs(rev - ref["contraction"]) <= TC.contraction_bound(ref["terms"]), name
    cycles = {name: int(ref["stats"][4]) for name, ref in zip(TC.FAMILIES, refs)}
    assert cycles["tee"] == 0 and cycles["loop"] == 1 and cycles["rings"] == R // 4 and cycles["ring_tie"] == 1 and cycles["off_centre"] == 1
    assert cycles["plus"] == 0 and cycles["snake"] == 0 and cycles["full"] == (R - 1) ** 2


def test_the_new_families_decide_what_they_claim():
    for R in TC.SIZES:
        c = R // 2
        m, centre = TC.family("ring_tie", R)
        ref = TC.trace_ref(m, centre)
        a, b = R // 4, 3 * R // 4
        meet = b * R + c
        assert ref["cost"][b, c - 1] == ref["cost"][b, c + 1] and ref["parent"].ravel()[meet] == meet - 1          # the smaller index wins
        assert ref["stats"][5] == 2 and ref["stats"][6] == 0 and ref["stats"][10] == a * R + c        # both fronts end in a leaf that is no tip
        m, centre = TC.family("two_trees", R)
        ref = TC.trace_ref(m, centre)
        st = dict(zip(TC.STAT_NAMES, ref["stats"].tolist()))
        assert st["trees"] == 2 and st["main_root"] == (c + 2) * R + c and st["main_pixels"] == R - 2
        assert (c - 5) * R + c < st["main_root"] and 9 < (c - 1) ** 2 + 4                                          # smaller indices, nearer than the far end
        m, centre = TC.family("root_tie", R)
        ref = TC.trace_ref(m, centre)
        st = dict(zip(TC.STAT_NAMES, ref["stats"].tolist()))
        assert st["trees"] == 1 and st["main_root"] == c * R + c - 1 and ref["cost"][c, c + 1] == 6 * 408
        m, centre = TC.family("off_centre", R)
        assert centre[:2] == [R - 1, 0] and not m[R - 1, 0] and TC.trace_ref(m, centre)["stats"][10] >= 0


def _scores(masks):
    return [TC.tree_statistics_ref(m) for m in masks]


def test_cut_trees_separate_from_whole_ones():
    """sixteen dilated random-walk trees at 64 x 64 against the same trees cut along every sixth row and column: the cut ones fall
    apart into many short trees, every one of the whole ones is one tree with a long path"""
    whole, cut = TC.separation_sets()
    a, b = _scores(whole), _scores(cut)
    mean = lambda rows, k: float(np.mean([r[k] for r in rows]))   # noqa: E731
    for name, rows in (("whole", a), ("cut", b)):
        print(name, {k: round(mean(rows, k), 3) for k in TC.STATISTICS})
    assert all(r["scored"] for r in a + b)
    assert all(r["trees"] == 1.0 for r in a) and min(r["trees"] for r in b) > 10
    assert MC.ks_ref([r["trees"] for r in a], [r["trees"] for r in b]) == 1.0
    assert MC.ks_ref([r["path_max"] for r in a], [r["path_max"] for r in b]) == 1.0
    assert mean(a, "path_max") > 3 * mean(b, "path_max") and mean(a, "max_order") > 2 * mean(b, "max_order")
    assert mean(a, "cycles") > mean(b, "cycles") >= 0
    raw = [TC.trace_ref(MC.arbor(64, s), [32, 32, 0])["stats"][4] for s in range(16)]
    assert np.mean(raw) > 4 * mean(a, "cycles")                        # undilated walks cross themselves; dilation and thinning fuse most of it
    res = TC.tree_result_ref(a, b)
    assert res["trees"]["ks"] == 1.0 and res["path_max"]["ks"] == 1.0 and res["images"] == 16


@pytest.mark.parametrize("name", ("thick_arbor", "loop", "two_trees", "random20", "plus3", "disc", "single", "ring_tie"))
def test_swc_round_trip_on_oracle_arrays(ngan, tmp_path, name):
    M = ngan.metrics
    R = 64
    mask = TC.family(name, R)[0]
    sk, dist2, soma, ref, _ = TC.chain_ref(mask)
    assert soma[0] >= 0
    st = dict(zip(TC.STAT_NAMES, ref["stats"].tolist()))
    for fragments in (True, False):
        nodes = M.swc_nodes(sk, dist2, np.array(soma), ref, fragments=fragments)
        path = str(tmp_path / f"{name}_{int(fragments)}.swc")
        M.write_swc(path, nodes, comments=("a test", name))
        comments, back = TC.read_swc(path)
        assert comments[:2] == ["# a test", "# " + name] and len(comments) == 3 and len(back) == len(nodes["id"])
        TC.check_swc(back, sk, soma, None if fragments else st["main_pixels"])
        if fragments:
            assert sum(n[6] == -1 for n in back) == st["trees"]
            radii = {(int(n[3]), int(n[2])): n[5] for n in back[1:]}
            assert all(r == float(np.sqrt(np.float64(dist2[y, x]))) for (y, x), r in radii.items())
    empty = M.swc_nodes(np.zeros((R, R), np.uint8), np.zeros((R, R), np.int32), np.array([-1, -1, 0]), TC.trace_ref(np.zeros((R, R), np.uint8), [-1, -1, 0]))
    assert len(empty["id"]) == 0
