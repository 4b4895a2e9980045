"""Reference side of the skeleton tests (no test in here, and nothing of the package is imported): the definitions of include/ngan.h's
"arbor skeleton" section restated in numpy, and the mask families.

    thinning      Guo and Hall 1989, algorithm A1, on a 0 / 1 mask padded with background.  Neighbours clockwise from north: P2 N,
                  P3 NE, P4 E, P5 SE, P6 S, P7 SW, P8 W, P9 NW.
                      C  = [!P2 & (P3|P4)] + [!P4 & (P5|P6)] + [!P6 & (P7|P8)] + [!P8 & (P9|P2)]
                      N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8),  N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9),  N = min(N1, N2)
                  a set pixel goes in a sub-iteration when C == 1, 2 <= N <= 3 and (P2|P3|!P5) & P4 == 0 (sub-iteration 0) or
                  (P6|P7|!P9) & P8 == 0 (sub-iteration 1), all decided on the state before the sub-iteration.  0 and 1 alternate; the
                  loop ends after the first pair that deleted nothing; `passes` counts the sub-iterations run, that pair included.
    counts        B set neighbours, X the 0 -> 1 steps round the ring P2 .. P9, P2.  pixels; tips X == 1 and B <= 2; junctions X >= 3;
                  isolated B == 0; orth pairs of horizontal or vertical neighbours; diag pairs of diagonal neighbours neither of whose
                  two common 4-neighbours is set.
    statistics    length = (orth + sqrt(2) diag) / R, tips, junctions, width = kept pixels / skeleton pixels.

Families: every one of morph_cases.FAMILIES, `row` and `disc`, and
    bars_v / bars_h   bars 3 wide along the whole side, centred on column (row) 31 in the first half of the rows (columns) and on 32 in
                      the second, from 128 up also on 63 and 64, cut to the image (nothing at 16, the border columns at 32): neighbour
                      bits cross every word boundary of 32- and of 64-bit words
    frame             a 3-pixel frame on the image border: "outside is background" on all four sides
    block2            one 2 x 2 block
    plus, plus3       a row and a column through (R / 2, R / 2) from 2 to R - 3, one pixel and three pixels thick
    tee               row 4 from 2 to R - 3 with a stem in column R / 2 down to R - 3
    cross_x           both diagonals
    bar3              rows R / 2 - 1 .. R / 2 + 1 over columns 2 .. R - 3
    thick_arbor       morph_cases.arbor dilated by a 3 x 3 square: the workload's own shape"""
import numpy as np

import morph_cases as MC

f64 = np.float64
NEW_FAMILIES = ("bars_v", "bars_h", "frame", "block2", "plus", "plus3", "tee", "cross_x", "bar3", "thick_arbor")
FAMILIES = MC.FAMILIES + ("row", "disc") + NEW_FAMILIES
SIZES = (16, 32, 64, 128)
STATISTICS = ("length", "tips", "junctions", "width")
STAT_NAMES = ("pixels", "tips", "junctions", "isolated", "orth", "diag", "passes", "area")


# ---- definitions ------------------------------------------------------------------------------------------------------------------------
def neighbours(m):
    """the eight neighbour planes P2 .. P9 of a boolean (R, R) mask, background outside"""
    R = m.shape[0]
    p = np.zeros((R + 2, R + 2), bool)
    p[1:-1, 1:-1] = m
    at = lambda dy, dx: p[1 + dy:1 + dy + R, 1 + dx:1 + dx + R]   # noqa: E731
    return at(-1, 0), at(-1, 1), at(0, 1), at(1, 1), at(1, 0), at(1, -1), at(0, -1), at(-1, -1)


def deletable(m, sub):
    P2, P3, P4, P5, P6, P7, P8, P9 = neighbours(m)
    i = lambda b: b.astype(np.int32)   # noqa: E731
    C = i(~P2 & (P3 | P4)) + i(~P4 & (P5 | P6)) + i(~P6 & (P7 | P8)) + i(~P8 & (P9 | P2))
    N1 = i(P9 | P2) + i(P3 | P4) + i(P5 | P6) + i(P7 | P8)
    N2 = i(P2 | P3) + i(P4 | P5) + i(P6 | P7) + i(P8 | P9)
    N = np.minimum(N1, N2)
    side = ((P2 | P3 | ~P5) & P4) if sub == 0 else ((P6 | P7 | ~P9) & P8)
    return m & (C == 1) & (N >= 2) & (N <= 3) & ~side


def thin_ref(mask):
    """(skeleton uint8 0 / 1, passes) of one (R, R) mask"""
    m = np.asarray(mask) != 0
    passes = 0
    while True:
        changed = False
        for sub in (0, 1):
            d = deletable(m, sub)
            changed |= bool(d.any())
            m = m & ~d
            passes += 1
        if not changed:
            return m.astype(np.uint8), passes


def counts_ref(mask):
    """[pixels, tips, junctions, isolated, orth, diag] of one (R, R) mask"""
    m = np.asarray(mask) != 0
    ring = neighbours(m)
    P2, P3, P4, P5, P6, P7, P8, P9 = ring
    B = sum(r.astype(np.int32) for r in ring)
    X = sum((~ring[k] & ring[(k + 1) % 8]).astype(np.int32) for k in range(8))
    orth = int((m & P4).sum() + (m & P6).sum())
    diag = int((m & P5 & ~P4 & ~P6).sum() + (m & P7 & ~P8 & ~P6).sum())
    return [int(m.sum()), int((m & (X == 1) & (B <= 2)).sum()), int((m & (X >= 3)).sum()), int((m & (B == 0)).sum()), orth, diag]


def stats_ref(mask):
    """(skeleton, the eight integers of ngan_skel_thin's stats row)"""
    sk, passes = thin_ref(mask)
    return sk, counts_ref(sk) + [passes, int((np.asarray(mask) != 0).sum())]


def skeleton_statistics_ref(mask, min_size=1):
    """{length, tips, junctions, width, scored} of one mask (the kept mask of morph_cases.stats_ref is thinned)"""
    R = mask.shape[0]
    _, st, kept = MC.stats_ref(mask, min_size)
    sk, s = stats_ref(kept)
    if st[3] == 0 or s[0] == 0:
        return {"length": 0.0, "tips": float(s[1]), "junctions": float(s[2]), "width": float("nan"), "scored": False, "pixels": s[0]}
    return {"length": (s[4] + np.sqrt(f64(2.0)) * s[5]) / float(R), "tips": float(s[1]), "junctions": float(s[2]),
            "width": st[3] / float(s[0]), "scored": True, "pixels": s[0]}


def skeleton_ref(real, fake):
    """Skeleton.result() from two lists of skeleton_statistics_ref dictionaries"""
    out = {"images": len(real), "skipped_real": sum(not r["scored"] for r in real), "skipped_fake": sum(not r["scored"] for r in fake)}
    for name in STATISTICS:
        a = np.array([r[name] for r in real if r["scored"]], f64)
        b = np.array([r[name] for r in fake if r["scored"]], f64)
        row = {"ks": MC.ks_ref(a, b)}
        for which, v in (("real", a), ("fake", b)):
            row[which] = float(v.mean())
            row[which + "_sem"] = float(v.std(ddof=1) / np.sqrt(v.size)) if v.size > 1 else None
        out[name] = row
    return out


# ---- families ---------------------------------------------------------------------------------------------------------------------------
def dilate(m):
    """one dilation by a 3 x 3 square, background outside"""
    m = np.asarray(m) != 0
    out = m.copy()
    for r in neighbours(m):
        out |= r
    return out.astype(np.uint8)


def family(name, R, seed=0):
    if name not in NEW_FAMILIES:
        return MC.family(name, R, seed)
    m = np.zeros((R, R), np.uint8)
    c = R // 2
    if name in ("bars_v", "bars_h"):
        for first, second in ((31, 32),) + (((63, 64),) if R >= 128 else ()):
            if first - 1 < R:
                m[1:c - 1, first - 1:min(first + 2, R)] = 1
            if second - 1 < R:
                m[c + 1:R - 1, second - 1:min(second + 2, R)] = 1
        if name == "bars_h":
            m = m.T.copy()
    elif name == "frame":
        m[:] = 1
        m[3:R - 3, 3:R - 3] = 0
    elif name == "block2":
        m[c - 1:c + 1, c - 1:c + 1] = 1
    elif name == "plus":
        m[c, 2:R - 2] = 1
        m[2:R - 2, c] = 1
    elif name == "plus3":
        m[c - 1:c + 2, 2:R - 2] = 1
        m[2:R - 2, c - 1:c + 2] = 1
    elif name == "tee":
        m[4, 2:R - 2] = 1
        m[4:R - 2, c] = 1
    elif name == "cross_x":
        m = (MC.family("diagonal", R) | MC.family("antidiagonal", R)).astype(np.uint8)
    elif name == "bar3":
        m[c - 1:c + 2, 2:R - 2] = 1
    elif name == "thick_arbor":
        m = dilate(MC.arbor(R, 77 + seed))
    return m


_cache = {}


def case(R, families=FAMILIES):
    """(masks (n, R, R) uint8, [(skeleton, stats row)]): computed once and shared; treat as read-only"""
    key = (R, tuple(families))
    if key not in _cache:
        masks = np.stack([family(f, R) for f in families])
        _cache[key] = (masks, [stats_ref(m) for m in masks])
    return _cache[key]
