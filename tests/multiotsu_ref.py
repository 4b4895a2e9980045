"""Reference side of the data-set tests (no test in here, and nothing of the package is imported): the 4-class multi-Otsu
definition of include/ngan.h's "data set" section restated in numpy fp64, and a seeded generator of micrograph-like bytes.

Definition.  h is a 256-bin histogram, lo / hi its lowest / highest occupied level, P(a, b) = sum h[v] and S(a, b) = sum v h[v] over
the levels a..b inclusive, both exact int64 from prefix sums.  A candidate is a triplet of levels lo <= t0 < t1 < t2 <= hi - 1; its
classes are lo..t0, t0+1..t1, t1+1..t2, t2+1..hi; its score is the sum over the classes of S^2 / P in fp64 (0 for an empty class),
added as ((c0 + c1) + c2) + c3.  The answer is the first maximum in C order of (t0, t1, t2), i.e. the lexicographically smallest
triplet of the largest score.  Two triplets cut the occupied levels into the same four sets exactly when their cumulative counts
P(lo, t0), P(lo, t1), P(lo, t2) agree; `second` below is the best score over the candidates that cut them differently from the winner.
"""
import numpy as np


def prefix_sums(hist):
    """pp[v] = sum h[0..v-1], sp[v] = sum u h[u] over the same levels: int64, 257 entries each"""
    h = np.asarray(hist).astype(np.int64)
    assert h.shape == (256,) and (h >= 0).all()
    pp = np.concatenate([[0], np.cumsum(h)])
    sp = np.concatenate([[0], np.cumsum(h * np.arange(256, dtype=np.int64))])
    return pp, sp


def class_scores(pp, sp):
    """c[a, b] = S(a, b)^2 / P(a, b) in fp64 for a <= b, 0 where the class is empty (or a > b)"""
    p = pp[None, 1:] - pp[:256, None]
    s = (sp[None, 1:] - sp[:256, None]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(p > 0, s * s / p.astype(np.float64), 0.0)
    return c


def multiotsu4(hist):
    """(triplet, best score, best score among the candidates that cut the occupied levels differently or None if there is none).
    ValueError when fewer than four levels are occupied (skimage raises there too)."""
    pp, sp = prefix_sums(hist)
    occupied = np.flatnonzero(np.asarray(hist))
    if occupied.size < 4:
        raise ValueError("fewer than four occupied levels")
    lo, hi = int(occupied[0]), int(occupied[-1])
    c = class_scores(pp, sp)
    levels = np.arange(256)
    best, triplet = -1.0, None
    per_t0 = []
    for t0 in range(lo, hi - 2):
        t1 = levels[t0 + 1:hi - 1]                                   # t0 < t1 <= hi - 2
        t2 = levels[t0 + 2:hi]                                       # t1 < t2 <= hi - 1
        c01 = c[lo, t0] + c[t0 + 1, t1]                              # (c0 + c1), by t1
        score = (c01[:, None] + c[t1[:, None] + 1, t2[None, :]]) + c[t2 + 1, hi][None, :]
        score = np.where(t2[None, :] > t1[:, None], score, -1.0)
        per_t0.append((t0, t1, t2, score))
        k = int(np.argmax(score))                                    # first maximum in C order of (t1, t2)
        i, j = divmod(k, t2.size)
        if score[i, j] > best:                                       # strict: the smallest t0 keeps a tie
            best, triplet = float(score[i, j]), (t0, int(t1[i]), int(t2[j]))
    cut = (pp[triplet[0] + 1], pp[triplet[1] + 1], pp[triplet[2] + 1])
    second = None
    for t0, t1, t2, score in per_t0:
        same = (pp[t0 + 1] == cut[0]) & (pp[t1 + 1] == cut[1])[:, None] & (pp[t2 + 1] == cut[2])[None, :]
        other = np.where(same | (score < 0), -1.0, score)
        m = float(other.max()) if other.size else -1.0
        if m >= 0 and (second is None or m > second):
            second = m
    return triplet, best, second


def relative_gap(best, second):
    return np.inf if second is None else (best - second) / best


def noise_record(image, t0):
    """(count, mean, std) of the pixels 0 < v < t0 the way the reference takes them (NeuronDataset.py:94-97): float64 numpy"""
    img = np.asarray(image)
    sel = img[np.logical_and(img > 0, img < t0)].astype(np.float64)
    return sel.size, float(np.mean(sel)), float(np.std(sel))


def micrograph(seed, size):
    """(size, size) uint8: a zero background outside a disc, inside it a Gaussian noise floor around level 18 and line-shaped
    structures of three brightness classes (about 60, 120 and 200)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    centre = 0.5 * (size - 1)
    img = np.clip(np.rint(rng.normal(18.0, 4.0, (size, size))), 1, 255)
    for level, spread, n_lines, width in ((60.0, 7.0, 7, 0.030), (120.0, 9.0, 5, 0.024), (200.0, 11.0, 4, 0.018)):
        for _ in range(n_lines):
            p0, p1 = rng.uniform(0.1 * size, 0.9 * size, 2), rng.uniform(0.1 * size, 0.9 * size, 2)
            d = p1 - p0
            t = np.clip(((xx - p0[0]) * d[0] + (yy - p0[1]) * d[1]) / max(float(d @ d), 1e-9), 0.0, 1.0)
            dist = np.hypot(xx - (p0[0] + t * d[0]), yy - (p0[1] + t * d[1]))
            on = dist <= max(0.5 * width * size, 0.75)
            img = np.where(on, np.clip(np.rint(rng.normal(level, spread, (size, size))), 1, 255), img)
    img = np.where(np.hypot(xx - centre, yy - centre) <= 0.47 * size, img, 0.0)
    return img.astype(np.uint8)


def pad_noise_fill(images, normals, mean, std):
    """numpy restatement of NeuronDataset.py:13-19, 70-71, 100-107 with given draws: pad by R // 4 with zeros, every zero pixel
    <- trunc(clamp(std * draw + mean, 0, 255)) (the reference's uint8 assignment wraps where this clamps), ToTensor's / 255."""
    images = np.asarray(images)
    n, r, _ = images.shape
    pad = r // 4
    padded = np.zeros((n, r + 2 * pad, r + 2 * pad), dtype=np.uint8)
    padded[:, pad:pad + r, pad:pad + r] = images
    noise = np.asarray(std, np.float64)[:, None, None] * np.asarray(normals).astype(np.float64) + np.asarray(mean, np.float64)[:, None, None]
    noise = np.clip(noise, 0.0, 255.0).astype(np.uint8)              # truncation toward zero
    filled = np.where(padded == 0, noise, padded)
    return filled.astype(np.float32) / np.float32(255.0)
