"""Reference side of the morphology tests (no test in here, and nothing of the package is imported): the definitions of include/ngan.h's
"arbor morphology" section restated in numpy, and the mask families.

    levels        np.float32(np.float64(x) * 127.5 + 128.0), clamped to [0, 255] and truncated.  The fp64 product of an fp32 value with
                  127.5 is exact (24 + 8 bits) and so is the sum for |x| >= 2^-21 or x = 0 (it fits 53 bits), so the one rounding to
                  fp32 is the fused form's single rounding; the test images have no other values.  For three channels the mean is
                  (x0 + x1) + x2 in fp32, times fp32(1 / 3).
    labels        flood fill under 8-connectivity, scanning the pixels in ascending linear index: the pixel a fill starts from is the
                  smallest index of its component, which is the canonical label.
    box counts    reshape to (R / s, s, R / s, s) and any() over the box axes.
    dimension     least-squares slope of ln N(s) against ln(1 / s) over s = 1, 2, ..., R / 4.
    ks            sup |F_a - F_b| over the pooled values, F the empirical distribution function (<=).

Families (each for a mistake it catches; tests/test_morph_cpu.py checks that they do what is claimed):
    empty, full, single (one pixel in the last corner)
    checkerboard   one component under 8-connectivity, R^2 / 2 under 4
    diagonal, antidiagonal   a missing diagonal direction
    snake          even rows full, joined alternately at the right and left end in the odd rows: one component R^2 / 2 pixels long
                   (R / 2 full rows and R / 2 - 1 joints, the last odd row is empty), crossing every tile border; the canonical
                   minimum has to travel its whole length
    comb, comb_flip, comb_t   teeth in every other column joined only in the last row (flipped: the first; transposed: the last
                   column): labels must travel against scan order
    corners        at every pair of multiples of 8 (my, mx) inside the image two pixels touch only diagonally across that point:
                   (my-1, mx-1), (my, mx) where (my + mx) / 8 is even and (my-1, mx), (my, mx-1) otherwise: (R / 8 - 1)^2 components
                   of size 2, pinning the corner neighbour of the border merge for tiles of 8, 16, 32 and 64
    gaps           everything but the first column of every 64-pixel tile: runs that start in bit 1 and end in the last bit of a row mask
    rings          concentric square outlines two pixels apart, nested and not touching: R / 4 components
    random20 / random41 / random60   densities 0.2, 0.41 (near the 8-connected percolation point), 0.6
    arbor          a seeded random-walk tree"""
import numpy as np

f64 = np.float64
FAMILIES = ("empty", "full", "single", "checkerboard", "diagonal", "antidiagonal", "snake", "comb", "comb_flip", "comb_t", "corners",
            "gaps", "rings", "random20", "random41", "random60", "arbor")
SIZES = (16, 32, 64, 128)
STATISTICS = ("fill", "components", "largest_share", "dimension")


# ---- definitions ------------------------------------------------------------------------------------------------------------------------
def channel_mean(x):
    """(B, R, R, C) fp32 -> (B, R, R) fp32: the pixel, or ((x0 + x1) + x2) * fp32(1 / 3) in fp32"""
    x = np.asarray(x, np.float32)
    if x.shape[3] == 1:
        return x[..., 0]
    return ((x[..., 0] + x[..., 1]) + x[..., 2]) * np.float32(1.0 / 3.0)


def levels_ref(x):
    g = channel_mean(x)
    v = np.float32(g.astype(f64) * 127.5 + 128.0)
    return np.clip(v, np.float32(0), np.float32(255)).astype(np.int64).astype(np.uint8)


def from_bytes(img):
    """uint8 -> the fp32 value whose level is that byte: v / 127.5 - 1 in fp64, rounded"""
    return (np.asarray(img).astype(f64) / 127.5 - 1.0).astype(np.float32)


def label_ref(mask, connectivity=8):
    """(R, R) -> (labels int32 with -1 on the background and the smallest linear index of the component elsewhere, sizes by root)"""
    m = np.asarray(mask) != 0
    R = m.shape[0]
    lab = np.full(R * R, -1, np.int32)
    flat = m.ravel()
    sizes = {}
    if connectivity == 8:
        steps = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx]
    else:
        steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    for s in np.flatnonzero(flat):
        if lab[s] >= 0:
            continue
        lab[s] = s
        stack, n = [int(s)], 0
        while stack:
            p = stack.pop()
            n += 1
            y, x = divmod(p, R)
            for dy, dx in steps:
                yy, xx = y + dy, x + dx
                if 0 <= yy < R and 0 <= xx < R:
                    q = yy * R + xx
                    if flat[q] and lab[q] < 0:
                        lab[q] = s
                        stack.append(q)
        sizes[int(s)] = n
    return lab.reshape(R, R), sizes


def label_runs_ref(mask):
    """label_ref's labels by another route, for sizes where a flood fill in Python takes too long: the runs of every row, joined with
    the runs of the row above that they touch (columns overlapping or diagonal), the smaller first pixel becoming the root"""
    m = np.asarray(mask) != 0
    R = m.shape[0]
    parent, start, rows = [], [], []

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for y in range(R):
        d = np.diff(np.concatenate([[0], m[y].astype(np.int8), [0]]))
        s, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1)            # runs [s, e)
        ids = list(range(len(parent), len(parent) + s.size))
        parent.extend(ids)
        start.extend((y * R + s).tolist())
        if y and rows[-1][0].size and s.size:
            ps, pe, pid = rows[-1]
            j = 0
            for k in range(s.size):
                while j < ps.size and pe[j] < s[k]:                      # the run above ends left of column s - 1
                    j += 1
                i = j
                while i < ps.size and ps[i] <= e[k]:                     # and starts no further right than column e
                    a, b = find(ids[k]), find(pid[i])
                    if a != b:
                        if start[a] < start[b]:
                            parent[b] = a
                        else:
                            parent[a] = b
                    i += 1
        rows.append((s, e, ids))
    lab = np.full((R, R), -1, np.int32)
    for y, (s, e, ids) in enumerate(rows):
        for a, b, i in zip(s, e, ids):
            lab[y, a:b] = start[find(i)]
    return lab


def stats_of_labels(lab, min_size=1):
    """[area, components, largest, kept_area] and the kept mask from canonical labels"""
    roots, n = np.unique(lab[lab >= 0], return_counts=True)
    counted = roots[n >= min_size]
    kept = np.isin(lab, counted)
    return [int(n.sum()), int(counted.size), int(n.max()) if n.size else 0, int(n[n >= min_size].sum())], kept.astype(np.uint8)


def stats_ref(mask, min_size=1):
    """(labels, [area, components, largest, kept_area], kept mask uint8)"""
    lab, sizes = label_ref(mask)
    counted = {r for r, n in sizes.items() if n >= min_size}
    kept = np.isin(lab, sorted(counted)) if counted else np.zeros(lab.shape, bool)
    stats = [int(sum(sizes.values())), len(counted), max(sizes.values()) if sizes else 0, int(sum(sizes[r] for r in counted))]
    return lab, stats, kept.astype(np.uint8)


def box_counts_ref(mask):
    m = np.asarray(mask) != 0
    R = m.shape[0]
    out = []
    s = 1
    while s <= R:
        out.append(int(m.reshape(R // s, s, R // s, s).any(axis=(1, 3)).sum()))
        s *= 2
    return out


def dimension_ref(counts, R):
    n = int(R).bit_length() - 2
    c = np.asarray(counts, f64)[:n]
    if (c <= 0).any():
        return float("nan")
    x = -np.log(2.0) * np.arange(n, dtype=f64)
    y = np.log(c)
    xc = x - x.mean()
    return float((y * xc).sum() / (xc * xc).sum())


def ks_ref(a, b):
    a, b = np.sort(np.asarray(a, f64)), np.sort(np.asarray(b, f64))
    at = np.concatenate([a, b])
    return float(np.abs(np.searchsorted(a, at, side="right") / a.size - np.searchsorted(b, at, side="right") / b.size).max())


def arbor_statistics_ref(mask, min_size=1):
    """{fill, components, largest_share, dimension, scored} of one mask"""
    R = mask.shape[0]
    _, st, kept = stats_ref(mask, min_size)
    if st[3] == 0:
        return {"fill": 0.0, "components": float(st[1]), "largest_share": float("nan"), "dimension": float("nan"), "scored": False}
    return {"fill": st[3] / float(R * R), "components": float(st[1]), "largest_share": st[2] / float(st[3]),
            "dimension": dimension_ref(box_counts_ref(kept), R), "scored": True}


def morphology_ref(real, fake):
    """Morphology.result() from two lists of arbor_statistics_ref dictionaries"""
    out = {"images": len(real), "skipped_real": sum(not r["scored"] for r in real), "skipped_fake": sum(not r["scored"] for r in fake)}
    for name in STATISTICS:
        a = np.array([r[name] for r in real if r["scored"]], f64)
        b = np.array([r[name] for r in fake if r["scored"]], f64)
        row = {"ks": ks_ref(a, b)}
        for which, v in (("real", a), ("fake", b)):
            row[which] = float(v.mean())
            row[which + "_sem"] = float(v.std(ddof=1) / np.sqrt(v.size)) if v.size > 1 else None
        out[name] = row
    return out


# ---- families ---------------------------------------------------------------------------------------------------------------------------
def arbor(R, seed):
    """a tree grown by random walks that start on the tree: one 8-connected component through the centre"""
    rng = np.random.default_rng(seed)
    m = np.zeros((R, R), np.uint8)
    m[R // 2, R // 2] = 1
    for _ in range(8 + R // 4):
        ys, xs = np.nonzero(m)
        i = int(rng.integers(ys.size))
        y, x = int(ys[i]), int(xs[i])
        dy, dx = rng.integers(-1, 2, 2)
        for _ in range(int(rng.integers(R // 2, R))):
            if rng.random() < 0.3:
                dy, dx = rng.integers(-1, 2, 2)
            y, x = y + int(dy), x + int(dx)
            if not (1 <= y < R - 1 and 1 <= x < R - 1):
                break
            m[y, x] = 1
    return m


def family(name, R, seed=0):
    m = np.zeros((R, R), np.uint8)
    yy, xx = np.mgrid[0:R, 0:R]
    if name == "empty":
        pass
    elif name == "full":
        m[:] = 1
    elif name == "single":
        m[R - 1, R - 1] = 1
    elif name == "checkerboard":
        m[(yy + xx) % 2 == 0] = 1
    elif name == "diagonal":
        m[yy == xx] = 1
    elif name == "antidiagonal":
        m[yy + xx == R - 1] = 1
    elif name == "snake":
        m[0::2, :] = 1
        m[1:R - 1:4, R - 1] = 1
        m[3:R - 1:4, 0] = 1
    elif name in ("comb", "comb_flip", "comb_t"):
        m[:, 0::2] = 1
        m[R - 1, :] = 1
        m[:R - 1, 1::2] = 0
        if name == "comb_flip":
            m = m[::-1].copy()
        if name == "comb_t":
            m = m.T.copy()
    elif name == "corners":
        for my in range(8, R, 8):
            for mx in range(8, R, 8):
                if ((my + mx) // 8) % 2 == 0:
                    m[my - 1, mx - 1] = m[my, mx] = 1
                else:
                    m[my - 1, mx] = m[my, mx - 1] = 1
    elif name == "gaps":
        m[:] = 1
        m[:, 0::64] = 0
    elif name == "rings":
        d = np.minimum(np.minimum(yy, xx), np.minimum(R - 1 - yy, R - 1 - xx))
        m[d % 2 == 0] = 1
    elif name.startswith("random"):
        rng = np.random.default_rng(1000 + seed + int(name[6:]))
        m[rng.random((R, R)) < int(name[6:]) / 100.0] = 1
    elif name == "arbor":
        m = arbor(R, 77 + seed)
    elif name == "row":
        m[R // 2, :] = 1
    elif name == "disc":
        c = 0.5 * (R - 1)
        m[np.hypot(yy - c, xx - c) <= 0.4 * R] = 1
    elif name == "corner_boxes":                      # one pixel in each corner box of every level
        m[0, 0] = m[0, R - 1] = m[R - 1, 0] = m[R - 1, R - 1] = 1
    else:
        raise ValueError(name)
    return m


_cache = {}


def case(R, families=FAMILIES):
    """(masks (n, R, R) uint8, [(labels, stats, kept)] at min_size 1): computed once and shared; treat as read-only"""
    key = (R, tuple(families))
    if key not in _cache:
        masks = np.stack([family(f, R) for f in families])
        _cache[key] = (masks, [stats_ref(m) for m in masks])
    return _cache[key]


def arbor_set(R, n, seed, cut=False):
    """n arbor masks; cut: every sixth row and column cleared, which takes the trees apart"""
    out = np.stack([arbor(R, 1000 * seed + i) for i in range(n)])
    if cut:
        out[:, 0::6, :] = 0
        out[:, :, 0::6] = 0
    return out


def mask_images(masks, seed):
    """(n, R, R) masks -> (n, R, R, 1) fp32 images in [-1, 1] whose multi-Otsu class above t0 is the mask: a noise floor of levels
    16 .. 20 on the background, levels 90 .. 98, 150 .. 158 and 215 .. 223 (by pixel) on the foreground, so that t0 falls between 20
    and 89 (tests/test_morph_cpu.py checks it for the sets the GPU test uses)"""
    rng = np.random.default_rng(seed)
    masks = np.asarray(masks)
    img = rng.integers(16, 21, masks.shape)
    fg = np.array([90, 150, 215])[rng.integers(0, 3, masks.shape)] + rng.integers(0, 9, masks.shape)
    img = np.where(masks != 0, fg, img).astype(np.uint8)
    return img, from_bytes(img)[..., None]
