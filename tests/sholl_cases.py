"""Reference side of the arbor-geometry tests (no test in here, and nothing of the package is imported): the definitions of
include/ngan.h's "arbor geometry" section restated in numpy, and the mask families.

    dist2         0 on the background; on a foreground pixel the smallest squared Euclidean distance to a background pixel, the ring of
                  pixels just outside the image (rows and columns -1 and R) counting as background.  `edt2_ref`: the mask is padded with
                  that ring, g is the distance to the nearest background pixel of the same column (two scans), and dist2(y, x) =
                  min over x' of g(y, x')^2 + (x - x')^2, row by row.  `edt2_brute`: the search over all background pixels, R <= 32.
    soma          {y, x, dist2} of the largest dist2, the smallest linear index among equals; {-1, -1, 0} for an empty mask.
    crossings     ring step s = max(2, R / 64); ring index k(p) = the largest k with (k s)^2 <= |p - c|^2 = isqrt(|p - c|^2) // s; the
                  edges are the orth and diag planes of skeleton_cases.counts_ref; an edge whose ends differ in k adds one to bin
                  max(k(p), k(q)) of 91.  roots = sum over the set pixels of sqrt(dist2).
    statistics    with n the skeleton pixels: calibre = 2 roots / n - 1, soma = sqrt(soma dist2), sholl_peak = max crossings,
                  sholl_radius = k s / R for the smallest k at the peak (0 without a crossing), reach = k s / R for the largest k with
                  a crossing (0 without one).

Families: every one of skeleton_cases.FAMILIES, and
    hole          the full image but for the one background pixel (R / 4, 3 R / 8 + 1): dist2 = min(min(y + 1, R - y, x + 1, R - x)^2,
                  (y - hy)^2 + (x - hx)^2)
    wedge         foreground where x > y: the nearest background lies diagonally
    two_discs     equal discs of radius R / 8 about (R / 4, R / 4) and (3 R / 4, 3 R / 4): the soma tie goes to the smaller index
    soma_arbor    thick_arbor with a disc of radius R / 8 at the centre: the soma falls inside the disc"""
import numpy as np

import morph_cases as MC
import skeleton_cases as SC

f64 = np.float64
SHOLL_BINS = 91
NEW_FAMILIES = ("hole", "wedge", "two_discs", "soma_arbor")
FAMILIES = SC.FAMILIES + NEW_FAMILIES
SIZES = (16, 32, 64, 128)
STATISTICS = ("calibre", "soma", "sholl_peak", "sholl_radius", "reach")


def sholl_step(R):
    return max(2, R // 64)


# ---- definitions ------------------------------------------------------------------------------------------------------------------------
def column_distance(mask):
    """g of the mask padded with one ring of background: (R + 2, R + 2) int64"""
    R = mask.shape[0]
    p = np.zeros((R + 2, R + 2), bool)
    p[1:-1, 1:-1] = np.asarray(mask) != 0
    down = np.zeros(p.shape, np.int64)
    for y in range(1, R + 2):
        down[y] = (down[y - 1] + 1) * p[y]
    up = np.zeros(p.shape, np.int64)
    for y in range(R, -1, -1):
        up[y] = (up[y + 1] + 1) * p[y]
    return np.minimum(down, up)


def edt2_ref(mask):
    """(R, R) int64 squared distances"""
    R = mask.shape[0]
    g2 = column_distance(mask) ** 2
    xs = np.arange(R + 2, dtype=np.int64)
    apart = (xs[:, None] - xs[None, :]) ** 2                   # [x, x']
    out = np.empty((R, R), np.int64)
    for y in range(R):
        out[y] = (apart + g2[y + 1][None, :]).min(axis=1)[1:-1]
    return out


def edt2_brute(mask):
    R = mask.shape[0]
    assert R <= 32
    p = np.zeros((R + 2, R + 2), bool)
    p[1:-1, 1:-1] = np.asarray(mask) != 0
    by, bx = np.nonzero(~p)
    out = np.zeros((R, R), np.int64)
    for y, x in zip(*np.nonzero(p)):
        out[y - 1, x - 1] = ((by - y) ** 2 + (bx - x) ** 2).min()
    return out


def full_ref(R):
    yy, xx = np.mgrid[0:R, 0:R]
    return np.minimum(np.minimum(yy + 1, R - yy), np.minimum(xx + 1, R - xx)).astype(np.int64) ** 2


def hole_at(R):
    return R // 4, 3 * R // 8 + 1


def hole_ref(R):
    yy, xx = np.mgrid[0:R, 0:R]
    hy, hx = hole_at(R)
    return np.minimum(full_ref(R), ((yy - hy) ** 2 + (xx - hx) ** 2).astype(np.int64))


def soma_ref(dist2):
    i = int(np.argmax(dist2))                                  # the first of the largest: the smallest linear index
    d = int(dist2.ravel()[i])
    return [i // dist2.shape[1], i % dist2.shape[1], d] if d > 0 else [-1, -1, 0]


def ring_index(d2, s):
    r = np.floor(np.sqrt(np.asarray(d2, np.int64).astype(f64))).astype(np.int64)
    r = r - (r * r > d2) + ((r + 1) * (r + 1) <= d2)           # (the float root of an integer below 2^52 needs neither)
    return r // s


def sholl_ref(skeleton, dist2, centre):
    """(crossings (91) int64, roots) of one image; centre = (y, x[, ...])"""
    m = np.asarray(skeleton) != 0
    R = m.shape[0]
    crossings = np.zeros(SHOLL_BINS, np.int64)
    cy, cx = int(centre[0]), int(centre[1])
    if cy < 0:
        return crossings, 0.0
    yy, xx = np.mgrid[-1:R + 1, -1:R + 1]
    k = ring_index((yy - cy) ** 2 + (xx - cx) ** 2, sholl_step(R))
    at = lambda dy, dx: k[1 + dy:1 + dy + R, 1 + dx:1 + dx + R]   # noqa: E731
    P2, P3, P4, P5, P6, P7, P8, P9 = SC.neighbours(m)
    planes = ((m & P4, (0, 1)), (m & P6, (1, 0)), (m & P5 & ~P4 & ~P6, (1, 1)), (m & P7 & ~P8 & ~P6, (1, -1)))      # orth, orth, diag, diag
    for edge, (dy, dx) in planes:
        a, b = at(0, 0)[edge], at(dy, dx)[edge]
        np.add.at(crossings, np.maximum(a, b)[a != b], 1)
    return crossings, float(np.sqrt(np.asarray(dist2)[m].astype(f64)).sum())


def statistics_of(R, kept_area, pixels, soma, crossings, roots):
    """the five statistics and `scored` from the integers of one image"""
    s = sholl_step(R)
    scored = bool(kept_area > 0 and pixels > 0)
    peak = int(crossings.max())
    hit = np.flatnonzero(crossings)
    return {"calibre": 2.0 * roots / pixels - 1.0 if pixels else float("nan"), "soma": float(np.sqrt(f64(soma[2]))), "sholl_peak": float(peak),
            "sholl_radius": int(np.argmax(crossings)) * s / float(R) if peak else 0.0, "reach": int(hit[-1]) * s / float(R) if hit.size else 0.0,
            "scored": scored, "crossings": np.asarray(crossings, np.int64)}


def sholl_statistics_ref(mask, min_size=1):
    """{calibre, soma, sholl_peak, sholl_radius, reach, scored, crossings} of one mask: the kept mask of morph_cases.stats_ref is thinned
    and measured, the crossings are counted about its soma"""
    R = mask.shape[0]
    _, st, kept = MC.stats_ref(mask, min_size)
    sk, _ = SC.thin_ref(kept)
    dist2 = edt2_ref(kept)
    soma = soma_ref(dist2)
    crossings, roots = sholl_ref(sk, dist2, soma)
    return statistics_of(R, st[3], int(sk.sum()), soma, crossings, roots)


def sholl_result_ref(real, fake, R):
    """Sholl.result() from two lists of sholl_statistics_ref dictionaries"""
    out = {"images": len(real), "skipped_real": sum(not r["scored"] for r in real), "skipped_fake": sum(not r["scored"] for r in fake)}
    sides = {"real": [r for r in real if r["scored"]], "fake": [r for r in fake if r["scored"]]}
    for name in STATISTICS:
        row = {"ks": MC.ks_ref([r[name] for r in sides["real"]], [r[name] for r in sides["fake"]])}
        for which in ("real", "fake"):
            v = np.array([r[name] for r in sides[which]], f64)
            row[which] = float(v.mean())
            row[which + "_sem"] = float(v.std(ddof=1) / np.sqrt(v.size)) if v.size > 1 else None
        out[name] = row
    total = {which: np.sum([r["crossings"] for r in sides[which]], axis=0, dtype=np.int64) for which in sides}
    hit = np.flatnonzero(total["real"] + total["fake"])
    n = int(hit[-1]) + 1 if hit.size else 0
    out["profile"] = {"radius": [k * sholl_step(R) / float(R) for k in range(n)],
                      "real": [int(v) / float(len(sides["real"])) for v in total["real"][:n]],
                      "fake": [int(v) / float(len(sides["fake"])) for v in total["fake"][:n]]}
    return out


# ---- families ---------------------------------------------------------------------------------------------------------------------------
def disc(R, cy, cx, radius):
    yy, xx = np.mgrid[0:R, 0:R]
    return ((yy - cy) ** 2 + (xx - cx) ** 2 <= radius * radius).astype(np.uint8)


def family(name, R, seed=0):
    if name not in NEW_FAMILIES:
        return SC.family(name, R, seed)
    if name == "hole":
        m = np.ones((R, R), np.uint8)
        m[hole_at(R)] = 0
        return m
    if name == "wedge":
        yy, xx = np.mgrid[0:R, 0:R]
        return (xx > yy).astype(np.uint8)
    if name == "two_discs":
        return disc(R, R // 4, R // 4, R // 8) | disc(R, 3 * R // 4, 3 * R // 4, R // 8)
    return SC.family("thick_arbor", R, seed) | disc(R, R // 2, R // 2, R // 8)


def crop(masks, R, radius):
    """the masks inside the disc of that radius about (R / 2, R / 2)"""
    return np.asarray(masks) * disc(R, R // 2, R // 2, radius)[None]


def known_sets():
    """W: 16 dilated random-walk trees at 64 x 64; its own dilation; W cropped to the disc of radius 16 about the centre"""
    W = np.stack([SC.dilate(m) for m in MC.arbor_set(64, 16, 1)])
    return W, np.stack([SC.dilate(m) for m in W]), crop(W, 64, 16)


_cache = {}


def case(R, families=FAMILIES):
    """(masks (n, R, R) uint8, [(dist2, soma)]): computed once and shared; treat as read-only"""
    key = (R, tuple(families))
    if key not in _cache:
        masks = np.stack([family(f, R) for f in families])
        d = [edt2_ref(m) for m in masks]
        _cache[key] = (masks, [(x, soma_ref(x)) for x in d])
    return _cache[key]


def known(which):
    """the sholl_statistics_ref dictionaries of one of the known sets ('W', 'fat', 'cropped'): computed once and shared"""
    if "known" not in _cache:
        _cache["known"] = {k: [sholl_statistics_ref(m) for m in s] for k, s in zip(("W", "fat", "cropped"), known_sets())}
    return _cache["known"][which]
