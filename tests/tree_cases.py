"""Reference side of the arbor-tree tests (no test in here, and nothing of the package is imported): the definition of include/ngtree.h
restated in plain Python, and the mask families with their centres.

    graph         branch_cases.edge_list: the orth and diag pairs; an orth edge weighs 408, a diag edge 577.
    components    morph_cases.label_ref (a flood fill; morph_cases.label_runs_ref above 128 x 128, where that takes too long).
    roots         per component the pixel minimising ((y - cy)^2 + (x - cx)^2, index); the main tree has the smallest such key.  A centre
                  outside the image: no root, background values everywhere, zero statistics but main_root = -1.
    cost          Dijkstra with heapq from all roots at once (not the kernel's algorithm: no sweeps).
    parent        the smallest index among the neighbours q with cost[q] + w == cost[p]; -1 on a root, -2 on the background.
    order         pixels in ascending cost: order[parent] + (children(parent) >= 2); 0 on a root, -1 on the background.
    statistics    the twelve integers in the order of STAT_NAMES, tip_cost (an integer), and the contraction terms of the tips with
                  cost > 0 in ascending pixel order, sqrt(d2) / (cost / 408.0) in fp64.

Families: every one of branch_cases.FAMILIES about the soma of the mask itself (sholl_cases.soma_ref of its distance transform), and
    ring_tie      a square ring whose root, the middle of its upper side, is equidistant from the middle of the lower side both ways
                  round: the parent of that pixel is decided by the tie rule, and it is a leaf but no tip
    two_trees     a long bar below the centre and a short fragment above it that has the smaller indices and lies nearer to the centre
                  than the bar's ends, but whose root is farther than the bar's: the main tree is the bar
    root_tie      two arms left and right of the centre, joined by a detour below it: the pixels left and right of the centre are
                  equally near, the smaller index is the root
    off_centre    branch_cases' `loop` about the lower left corner of the image, which is not on the skeleton"""
import heapq
import math

import numpy as np

import branch_cases as BC
import morph_cases as MC
import sholl_cases as GC

f64 = np.float64
ORTH, DIAG = 408, 577
NEW_FAMILIES = ("ring_tie", "two_trees", "root_tie", "off_centre")
FAMILIES = BC.FAMILIES + NEW_FAMILIES
SIZES = (16, 32, 64, 128)
LARGE_FAMILIES = BC.LARGE_FAMILIES
STAT_NAMES = ("pixels", "trees", "orth", "diag", "cycles", "leaves", "tips", "forks", "path_max", "max_order", "main_root", "main_pixels")
STATISTICS = ("trees", "cycles", "tips", "forks", "path_max", "path_mean", "contraction", "max_order")


# ---- definitions ------------------------------------------------------------------------------------------------------------------------
def graph(mask):
    """{p: [(q, w)]} over the set pixels"""
    adj = {int(p): [] for p in np.flatnonzero(np.asarray(mask) != 0)}
    for p, q, diag in BC.edge_list(mask):
        w = DIAG if diag else ORTH
        adj[p].append((q, w))
        adj[q].append((p, w))
    return adj


def labels_of(mask):
    return (MC.label_ref(mask)[0] if mask.shape[0] <= 128 else MC.label_runs_ref(mask)).ravel()


def roots_of(mask, centre, lab=None):
    """{label: root pixel}, main root (or -1)"""
    R = mask.shape[0]
    cy, cx = int(centre[0]), int(centre[1])
    lab = labels_of(mask) if lab is None else lab
    best = {}
    for p in np.flatnonzero(lab >= 0):
        y, x = divmod(int(p), R)
        key = ((y - cy) ** 2 + (x - cx) ** 2, int(p))
        if int(lab[p]) not in best or key < best[int(lab[p])]:
            best[int(lab[p])] = key
    return {l: k[1] for l, k in best.items()}, (min(best.values())[1] if best else -1)


def dijkstra(adj, roots):
    cost = {r: 0 for r in roots}
    heap = [(0, r) for r in roots]
    heapq.heapify(heap)
    while heap:
        c, p = heapq.heappop(heap)
        if c > cost[p]:
            continue
        for q, w in adj[p]:
            if q not in cost or c + w < cost[q]:
                cost[q] = c + w
                heapq.heappush(heap, (c + w, q))
    return cost


def bellman_ford(adj, roots):
    """the same costs the naive way: every edge relaxed in turn until nothing changes"""
    cost = {p: (0 if p in roots else None) for p in adj}
    changed = True
    while changed:
        changed = False
        for p in adj:
            for q, w in adj[p]:
                if cost[q] is not None and (cost[p] is None or cost[q] + w < cost[p]):
                    cost[p] = cost[q] + w
                    changed = True
    return cost


def trace_ref(mask, centre):
    """{cost, parent, order: (R, R) int32; stats: (12) int64; tip_cost: int; terms: [fp64]; contraction: their sum in ascending pixel order}"""
    m = np.asarray(mask) != 0
    R = m.shape[0]
    cost = np.full(R * R, -1, np.int32)
    parent = np.full(R * R, -2, np.int32)
    order = np.full(R * R, -1, np.int32)
    st = dict.fromkeys(STAT_NAMES, 0)
    st["main_root"] = -1
    out = {"cost": cost.reshape(R, R), "parent": parent.reshape(R, R), "order": order.reshape(R, R), "tip_cost": 0, "terms": [], "contraction": 0.0}
    cy, cx = int(centre[0]), int(centre[1])
    if 0 <= cy < R and 0 <= cx < R and m.any():
        adj = graph(m)
        lab = labels_of(m)
        roots, main = roots_of(m, centre, lab)
        rootset = set(roots.values())
        c = dijkstra(adj, rootset)
        assert len(c) == len(adj), "a set pixel was not reached"
        par = {p: -1 if p in rootset else min(q for q, w in adj[p] if c[q] + w == c[p]) for p in adj}
        kids = dict.fromkeys(adj, 0)
        for p, q in par.items():
            if q >= 0:
                kids[q] += 1
        ordr = {}
        for p in sorted(adj, key=lambda p: (c[p], p)):
            ordr[p] = 0 if par[p] < 0 else ordr[par[p]] + (kids[par[p]] >= 2)
        for p in adj:
            cost[p], parent[p], order[p] = c[p], par[p], ordr[p]
        edges = BC.edge_list(m)
        st["pixels"], st["trees"] = len(adj), len(rootset)
        st["diag"] = sum(d for _, _, d in edges)
        st["orth"] = len(edges) - st["diag"]
        st["cycles"] = len(edges) - len(adj) + len(rootset)
        leaves = [p for p in sorted(adj) if kids[p] == 0]             # (a root without a child is an isolated pixel)
        tips = [p for p in leaves if len(adj[p]) <= 1]
        st["leaves"], st["tips"], st["forks"] = len(leaves), len(tips), sum(k >= 2 for k in kids.values())
        st["path_max"], st["max_order"], st["main_root"] = max(c.values()), max(ordr.values()), main
        st["main_pixels"] = sum(roots[int(lab[p])] == main for p in adj)
        out["tip_cost"] = sum(c[p] for p in tips)
        for p in tips:
            if c[p] > 0:
                r = roots[int(lab[p])]
                d2 = (p // R - r // R) ** 2 + (p % R - r % R) ** 2
                out["terms"].append(math.sqrt(float(d2)) / (float(c[p]) / 408.0))
        total = 0.0
        for t in out["terms"]:
            total += t
        out["contraction"] = total
    out["stats"] = np.array([st[k] for k in STAT_NAMES], np.int64)
    return out


def contraction_bound(terms):
    """(n + 4) 2^-52 sum |terms|: one rounding per square root, per division and per addition, in any order of the additions"""
    return (len(terms) + 4) * 2.0 ** -52 * sum(abs(t) for t in terms)


def statistics_of(R, kept_area, stats, tip_cost, contraction):
    """the eight statistics and `scored` from the numbers of one image"""
    s = dict(zip(STAT_NAMES, (int(v) for v in stats)))
    tips = max(1, s["tips"])
    return {"trees": float(s["trees"]), "cycles": float(s["cycles"]), "tips": float(s["tips"]), "forks": float(s["forks"]),
            "path_max": s["path_max"] / 408.0 / R, "path_mean": float(tip_cost) / tips / 408.0 / R, "contraction": contraction / tips,
            "max_order": float(s["max_order"]), "scored": bool(kept_area > 0 and s["pixels"] > 0)}


def chain_ref(mask, min_size=1):
    """(skeleton, dist2, soma, trace_ref's dictionary) of one mask: the kept mask of morph_cases.stats_ref is thinned and
    distance-transformed, and the skeleton is traced from the soma"""
    _, st, kept = MC.stats_ref(mask, min_size)
    sk, _ = BC.SC.thin_ref(kept)
    dist2 = GC.edt2_ref(kept)
    soma = GC.soma_ref(dist2)
    return sk, dist2, soma, trace_ref(sk, soma), st[3]


def tree_statistics_ref(mask, min_size=1):
    sk, _, _, t, kept_area = chain_ref(mask, min_size)
    return statistics_of(mask.shape[0], kept_area, t["stats"], t["tip_cost"], t["contraction"])


def tree_result_ref(real, fake):
    """Tree.result() from two lists of tree_statistics_ref dictionaries"""
    out = {"images": len(real), "skipped_real": sum(not r["scored"] for r in real), "skipped_fake": sum(not r["scored"] for r in fake)}
    sides = {"real": [r for r in real if r["scored"]], "fake": [r for r in fake if r["scored"]]}
    for name in STATISTICS:
        row = {"ks": MC.ks_ref([r[name] for r in sides["real"]], [r[name] for r in sides["fake"]])}
        for which in ("real", "fake"):
            v = np.array([r[name] for r in sides[which]], f64)
            row[which] = float(v.mean())
            row[which + "_sem"] = float(v.std(ddof=1) / np.sqrt(v.size)) if v.size > 1 else None
        out[name] = row
    return out


# ---- SWC files, read back ------------------------------------------------------------------------------------------------------------------
def read_swc(path):
    """(comment lines, [(id, type, x, y, z, radius, parent)]) of an SWC file; the comments must come first"""
    comments, nodes = [], []
    for line in open(path).read().splitlines():
        if line.startswith("#"):
            assert not nodes, "a comment line after the first node"
            comments.append(line)
        elif line.strip():
            f = line.split()
            assert len(f) == 7, line
            nodes.append((int(f[0]), int(f[1]), float(f[2]), float(f[3]), float(f[4]), float(f[5]), int(f[6])))
    return comments, nodes


def check_swc(nodes, skeleton, soma, main_pixels=None):
    """the promises of an SWC file of `skeleton` about `soma` = (y, x, dist2); main_pixels: the file holds the main tree alone"""
    sk = np.asarray(skeleton) != 0
    R = sk.shape[0]
    assert [n[0] for n in nodes] == list(range(1, len(nodes) + 1)), "ids are not 1 .. n"
    assert [n[1] for n in nodes].count(1) == 1 and nodes[0][1] == 1 and nodes[0][6] == -1 and all(n[1] in (1, 3) for n in nodes)
    assert (nodes[0][2], nodes[0][3], nodes[0][4]) == (float(soma[1]), float(soma[0]), 0.0) and nodes[0][5] == math.sqrt(float(soma[2]))
    at = {n[0]: n for n in nodes}
    soma_on = bool(sk[soma[0], soma[1]])                              # then the soma is the main tree's root, and node 1 is both
    for n in nodes[1:]:
        assert n[6] == -1 or 1 <= n[6] < n[0], f"the parent of node {n[0]} does not precede it"
        assert n[4] == 0.0 and n[2] == int(n[2]) and n[3] == int(n[3]) and n[5] >= 1.0
        if n[6] >= 1 and not (n[0] == 2 and not soma_on):             # every edge but the soma link joins neighbours
            p = at[n[6]]
            assert (n[2] - p[2]) ** 2 + (n[3] - p[3]) ** 2 in (1.0, 2.0), f"node {n[0]} is not beside its parent"
    assert soma_on or len(nodes) < 2 or nodes[1][6] == 1
    raster = np.zeros((R, R), bool)
    for n in nodes[(0 if soma_on else 1):]:
        assert not raster[int(n[3]), int(n[2])], "a pixel twice"
        raster[int(n[3]), int(n[2])] = True
    if main_pixels is None:
        assert np.array_equal(raster, sk), "the rasterised nodes are not the skeleton"
    else:
        assert not (raster & ~sk).any() and len(nodes) == main_pixels + (0 if soma_on else 1)
        assert sum(n[6] == -1 for n in nodes) == 1


# ---- families ---------------------------------------------------------------------------------------------------------------------------
def family(name, R, seed=0):
    """(mask (R, R) uint8, centre [y, x, 0])"""
    c = R // 2
    if name not in NEW_FAMILIES:
        m = BC.family(name, R, seed)
        return m, GC.soma_ref(GC.edt2_ref(m))
    m = np.zeros((R, R), np.uint8)
    if name == "ring_tie":
        a, b = R // 4, 3 * R // 4                    # a side of R / 2 edges, an even number
        m[a, a:b + 1] = m[b, a:b + 1] = 1
        m[a:b + 1, a] = m[a:b + 1, b] = 1
        return m, [a, c, 0]
    if name == "two_trees":
        m[c + 2, 1:R - 1] = 1                        # root (c + 2, c), 4 away
        m[c - 5:c - 2, c] = 1                        # root (c - 3, c), 9 away; the bar's ends are (c - 1)^2 + 4 away
        return m, [c, c, 0]
    if name == "root_tie":
        m[c, 2:c] = m[c, c + 1:R - 2] = 1            # (c, c - 1) and (c, c + 1) are both 1 away
        m[c + 1, c - 1] = m[c + 1, c + 1] = 1
        m[c + 2, c - 1:c + 2] = 1
        return m, [c, c, 0]
    return BC.family("loop", R), [R - 1, 0, 0]       # off_centre


_cache = {}


def case(R, families=FAMILIES):
    """(masks (n, R, R) uint8, centres (n, 3) int32, [trace_ref's dictionary]): computed once and shared; treat as read-only"""
    key = (R, tuple(families))
    if key not in _cache:
        pairs = [family(f, R) for f in families]
        masks, centres = np.stack([p[0] for p in pairs]), np.array([p[1] for p in pairs], np.int32)
        _cache[key] = (masks, centres, [trace_ref(m, c) for m, c in zip(masks, centres)])
    return _cache[key]


def separation_sets():
    """sixteen dilated random-walk trees at 64 x 64, and the same trees cut along every sixth row and column: masks, not thinned"""
    whole = np.stack([BC.SC.dilate(MC.arbor(64, seed)) for seed in range(16)]).astype(np.uint8)
    cut = whole.copy()
    cut[:, 0::6, :] = 0
    cut[:, :, 0::6] = 0
    return whole, cut
