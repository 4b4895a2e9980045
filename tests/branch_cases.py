"""Reference side of the arbor-branch tests (no test in here, and nothing of the package is imported): the definitions of
include/ngan.h's "arbor branches" section restated in numpy and plain Python, and the mask families.

    graph         vertices: the set pixels.  Edges: orth (horizontal or vertical neighbours) and diag (diagonal neighbours neither of
                  whose two common 4-neighbours is set), the pairs skeleton_cases.counts_ref counts.  `edge_list` names every edge once
                  in a loop over the set pixels; deg(p) counts the edges at p.
    pixels        node pixel deg >= 3, branch pixel deg <= 2; node edge / branch edge: both ends of that kind; attachment: one of each.
    components    nodes: node pixels under node edges; branches: branch pixels under branch edges -- a union-find in a dictionary, the
                  smaller linear index becoming the root (not the kernel's algorithm: no tiles, no atomics, no arrays).
    per branch    n pixels, a attachments, o / d orth / diag branch edges plus attachments, L = o + isqrt(2 d d) (math.isqrt).
                  free a == 0; spur a == 1 and n < spur; terminal a == 1 and n >= spur; link a == 2.
    per node      strong: attachments whose branch is no spur; fork: strong >= 3.
    statistics    forks, nodes, terminals, spurs; terminal_length = (term_orth + sqrt(2) term_diag) / max(1, terminal) / R, link_length
                  likewise; longest = stats[18] / R.

Families: every one of skeleton_cases.FAMILIES, raw and ("thin:" in front of the name) thinned by skeleton_cases.thin_ref, and
    burrs         `plus` with side stubs of one, two and three pixels, in turn, every 5 pixels along each arm: spur = 1, 2, 3 and 4 class
                  them differently
    loop          a square ring with one tail: a link that starts and ends at the same node
    double_t      two tees sharing a 2-pixel link
    seam          a tee whose node lies on pixel (63, 63) and whose arms run over 64 at R >= 128, a corner of 64-pixel tiles (at smaller
                  sizes on (R / 2 - 1, R / 2 - 1))"""
import hashlib
import math

import numpy as np

import morph_cases as MC
import skeleton_cases as SC

f64 = np.float64
STATS, BINS = 20, 64
NEW_FAMILIES = ("burrs", "loop", "double_t", "seam")
FAMILIES = SC.FAMILIES + tuple("thin:" + f for f in SC.FAMILIES) + NEW_FAMILIES
SIZES = (16, 32, 64, 128)
LARGE_FAMILIES = ("seam", "thick_arbor", "thin:thick_arbor", "checkerboard", "empty")     # what runs at 512
STATISTICS = ("forks", "nodes", "terminals", "spurs", "terminal_length", "link_length", "longest")
STAT_NAMES = ("pixels", "node_pixels", "nodes", "branches", "terminal", "links", "free", "spurs", "term_orth", "term_diag", "link_orth",
              "link_diag", "free_orth", "free_diag", "spur_orth", "spur_diag", "node_orth", "node_diag", "longest", "forks")


def default_spur(R):
    return max(2, R // 32)


# ---- definitions ------------------------------------------------------------------------------------------------------------------------
def edge_list(mask):
    """[(p, q, diag)] with p < q linear indices: every edge once"""
    m = np.asarray(mask) != 0
    R = m.shape[0]
    at = lambda y, x: 0 <= y < R and 0 <= x < R and bool(m[y, x])   # noqa: E731
    edges = []
    for y, x in zip(*np.nonzero(m)):
        y, x = int(y), int(x)
        p = y * R + x
        if at(y, x + 1):
            edges.append((p, p + 1, 0))
        if at(y + 1, x):
            edges.append((p, p + R, 0))
        if at(y + 1, x + 1) and not at(y, x + 1) and not at(y + 1, x):
            edges.append((p, p + R + 1, 1))
        if at(y + 1, x - 1) and not at(y, x - 1) and not at(y + 1, x):
            edges.append((p, p + R - 1, 1))
    return edges


class _Sets:
    def __init__(self, items):
        self.parent = {i: i for i in items}

    def find(self, i):
        while self.parent[i] != i:
            self.parent[i] = self.parent[self.parent[i]]
            i = self.parent[i]
        return i

    def join(self, a, b):
        a, b = self.find(a), self.find(b)
        if a != b:
            self.parent[max(a, b)] = min(a, b)


class Structure:
    """what does not depend on `spur`: pixels, deg {p: n}, node (set of node pixels), root {p: root}, branches {root: {n, a, o, d, edges
    (branch edges), inner {p: branch edges at p}, nodes [the node root of every attachment]}}, nodes {root: pixels}, node_orth,
    node_diag, R"""


_structures = {}


def structure(mask):
    mask = np.ascontiguousarray(np.asarray(mask) != 0)
    key = (mask.shape[0], hashlib.sha1(mask.tobytes()).hexdigest())
    if key in _structures:
        return _structures[key]
    s = Structure()
    s.R = R = mask.shape[0]
    s.pixels = [int(p) for p in np.flatnonzero(mask)]
    edges = edge_list(mask)
    s.deg = {p: 0 for p in s.pixels}
    for p, q, _ in edges:
        s.deg[p] += 1
        s.deg[q] += 1
    s.node = {p for p in s.pixels if s.deg[p] >= 3}
    sets = _Sets(s.pixels)
    for p, q, _ in edges:
        if (p in s.node) == (q in s.node):
            sets.join(p, q)
    s.root = {p: sets.find(p) for p in s.pixels}
    s.nodes, s.branches, s.node_orth, s.node_diag = {}, {}, 0, 0
    for p in s.pixels:
        r = s.root[p]
        if p in s.node:
            s.nodes[r] = s.nodes.get(r, 0) + 1
        else:
            b = s.branches.setdefault(r, {"n": 0, "a": 0, "o": 0, "d": 0, "edges": 0, "inner": {}, "nodes": []})
            b["n"] += 1
            b["inner"][p] = 0
    for p, q, diag in edges:
        pn, qn = p in s.node, q in s.node
        if pn and qn:
            s.node_orth += 1 - diag
            s.node_diag += diag
            continue
        b = s.branches[s.root[q if pn else p]]
        b["d" if diag else "o"] += 1
        if pn or qn:
            b["a"] += 1
            b["nodes"].append(s.root[p if pn else q])
        else:
            b["edges"] += 1
            b["inner"][p] += 1
            b["inner"][q] += 1
    _structures[key] = s
    return s


def floor_length(o, d):
    return o + math.isqrt(2 * d * d)


def branch_class(b, spur):
    return "free" if b["a"] == 0 else "links" if b["a"] == 2 else "spurs" if b["n"] < spur else "terminal"


def graph_ref(mask, spur):
    """(labels (R, R) int32, stats (20) int64, hist (64) int64) of one mask"""
    assert spur >= 1
    s = structure(mask)
    R = s.R
    labels = np.full(R * R, -1, np.int32)
    for p in s.pixels:
        labels[p] = -2 - s.root[p] if p in s.node else s.root[p]
    st = dict.fromkeys(STAT_NAMES, 0)
    hist = np.zeros(BINS, np.int64)
    st["pixels"], st["node_pixels"], st["nodes"], st["branches"] = len(s.pixels), len(s.node), len(s.nodes), len(s.branches)
    st["node_orth"], st["node_diag"] = s.node_orth, s.node_diag
    strong = dict.fromkeys(s.nodes, 0)
    prefix = {"terminal": "term", "links": "link", "free": "free", "spurs": "spur"}
    for b in s.branches.values():
        assert b["a"] <= 2
        cls = branch_class(b, spur)
        st[cls] += 1
        st[prefix[cls] + "_orth"] += b["o"]
        st[prefix[cls] + "_diag"] += b["d"]
        if cls != "spurs":
            L = floor_length(b["o"], b["d"])
            st["longest"] = max(st["longest"], L)
            if cls != "free":
                hist[min(BINS - 1, L // max(1, R // 128))] += 1
            for node in b["nodes"]:
                strong[node] += 1
    st["forks"] = sum(v >= 3 for v in strong.values())
    return labels.reshape(R, R), np.array([st[k] for k in STAT_NAMES], np.int64), hist


def statistics_of(R, kept_area, stats, hist):
    """the seven statistics and `scored` from the integers of one image"""
    s = dict(zip(STAT_NAMES, (int(v) for v in stats)))
    root2 = np.sqrt(f64(2.0))
    return {"forks": float(s["forks"]), "nodes": float(s["nodes"]), "terminals": float(s["terminal"]), "spurs": float(s["spurs"]),
            "terminal_length": float((s["term_orth"] + root2 * s["term_diag"]) / max(1, s["terminal"]) / R),
            "link_length": float((s["link_orth"] + root2 * s["link_diag"]) / max(1, s["links"]) / R),
            "longest": s["longest"] / float(R), "scored": bool(kept_area > 0 and s["pixels"] > 0), "hist": np.asarray(hist, np.int64)}


def branch_statistics_ref(mask, min_size=1, spur=None):
    """{forks, nodes, terminals, spurs, terminal_length, link_length, longest, scored, hist} of one mask: the kept mask of
    morph_cases.stats_ref is thinned and cut into branches"""
    R = mask.shape[0]
    _, st, kept = MC.stats_ref(mask, min_size)
    sk, _ = SC.thin_ref(kept)
    _, stats, hist = graph_ref(sk, default_spur(R) if spur is None else spur)
    return statistics_of(R, st[3], stats, hist)


def branches_ref(real, fake, R):
    """Branches.result() from two lists of branch_statistics_ref dictionaries"""
    out = {"images": len(real), "skipped_real": sum(not r["scored"] for r in real), "skipped_fake": sum(not r["scored"] for r in fake)}
    sides = {"real": [r for r in real if r["scored"]], "fake": [r for r in fake if r["scored"]]}
    for name in STATISTICS:
        row = {"ks": MC.ks_ref([r[name] for r in sides["real"]], [r[name] for r in sides["fake"]])}
        for which in ("real", "fake"):
            v = np.array([r[name] for r in sides[which]], f64)
            row[which] = float(v.mean())
            row[which + "_sem"] = float(v.std(ddof=1) / np.sqrt(v.size)) if v.size > 1 else None
        out[name] = row
    total = {which: np.sum([r["hist"] for r in sides[which]], axis=0, dtype=np.int64) for which in sides}
    hit = np.flatnonzero(total["real"] + total["fake"])
    n = int(hit[-1]) + 1 if hit.size else 0
    out["profile"] = {"length": [k * max(1, R // 128) / float(R) for k in range(n)],
                      "real": [int(v) / float(len(sides["real"])) for v in total["real"][:n]],
                      "fake": [int(v) / float(len(sides["fake"])) for v in total["fake"][:n]]}
    return out


# ---- families ---------------------------------------------------------------------------------------------------------------------------
def add_burrs(m):
    """side stubs of 2 pixels (a thinning leaves them alone; spur = 3 prunes them) on the straight runs of a 0 / 1 mask, as many as
    fit: in raster order, the middle pixel of three in a row gets a stub upwards or else downwards, the middle one of three in a column
    a stub to the right or else to the left, the middle one of three on a diagonal a stub along the other diagonal, where the stub with
    a one-pixel margin round it meets nothing but the run's pixels (earlier stubs included) and stays inside the image"""
    m = (np.asarray(m) != 0).astype(np.uint8)
    R = m.shape[0]
    out = m.copy()
    for y in range(1, R - 1):
        for x in range(1, R - 1):
            if not m[y, x]:
                continue
            if m[y, x - 1] and m[y, x + 1]:
                ways, run = ((-1, 0), (1, 0)), 3
            elif m[y - 1, x] and m[y + 1, x]:
                ways, run = ((0, 1), (0, -1)), 3
            elif m[y - 1, x - 1] and m[y + 1, x + 1]:
                ways, run = ((-1, 1), (1, -1)), 1
            elif m[y - 1, x + 1] and m[y + 1, x - 1]:
                ways, run = ((-1, -1), (1, 1)), 1
            else:
                continue
            for dy, dx in ways:
                y1, x1 = y + 3 * dy, x + 3 * dx
                if not (0 <= y1 < R and 0 <= x1 < R):
                    continue
                ys, xs = sorted((y + dy, y1 if dy else y)), sorted((x + dx, x1 if dx else x))
                if out[max(0, ys[0] - 1):ys[1] + 2, max(0, xs[0] - 1):xs[1] + 2].sum() > run:
                    continue
                out[y + dy, x + dx] = out[y + 2 * dy, x + 2 * dx] = 1
                break
    return out


def family(name, R, seed=0):
    if name.startswith("thin:"):
        return SC.thin_ref(SC.family(name[5:], R, seed))[0]
    if name not in NEW_FAMILIES:
        return SC.family(name, R, seed)
    m = np.zeros((R, R), np.uint8)
    c = R // 2
    if name == "burrs":
        m = SC.family("plus", R)
        k = 0
        for t in range(4, R - 4, 5):                 # along the arms, away from the centre and the ends
            if abs(t - c) < 3:
                continue
            n = 1 + k % 3
            m[c - n:c, t] = 1                        # up from the horizontal arm
            m[t, c + 1:c + 1 + n] = 1                # right from the vertical arm
            k += 1
    elif name == "loop":
        a, b = R // 4, 3 * R // 4 - 1
        m[a, a:b + 1] = m[b, a:b + 1] = 1
        m[a:b + 1, a] = m[a:b + 1, b] = 1
        m[b, b:R - 2] = 1                            # the tail leaves the lower right corner
    elif name == "double_t":
        m[4, 2:R - 2] = 1
        m[4:8, c] = 1                                # node (4, c), link (5, c), (6, c), node (7, c)
        m[7, 2:R - 2] = 1
    elif name == "seam":
        j = 63 if R >= 128 else c - 1
        m[j, 2:R - 2] = 1
        m[j:R - 2, j] = 1
    return m


_cache = {}


def case(R, families=FAMILIES):
    """masks (n, R, R) uint8: computed once and shared; treat as read-only"""
    key = (R, tuple(families))
    if key not in _cache:
        _cache[key] = np.stack([family(f, R) for f in families])
    return _cache[key]


def reference(R, spur, families=FAMILIES):
    """[(labels, stats, hist)] of case(R, families) at that spur: computed once and shared"""
    key = (R, spur, tuple(families))
    if key not in _cache:
        _cache[key] = [graph_ref(m, spur) for m in case(R, families)]
    return _cache[key]


def separation_sets():
    """W: the skeletons of the 16 `thick_arbor` trees of seeds 0 .. 15 at 64 x 64; the same skeletons with burrs"""
    W = np.stack([SC.thin_ref(SC.family("thick_arbor", 64, seed))[0] for seed in range(16)])
    return W, np.stack([add_burrs(m) for m in W])
