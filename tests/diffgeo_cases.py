"""Geometric differentiable augmentation (csrc/diffgeo.hip, ops.DiffGeometry): the operator restated in fp64 with its absolute-value
twin, the per-element bound, an emulation of the kernels' arithmetic, ngan_diffgeo_params in numpy, and the inputs and affine
tables of the tests.  Shared by tests/test_diffgeo_cpu.py (restatement against grid_sample, emulation against restatement) and
tests/test_gpu_diffgeo.py (the kernels against the restatement).

The operator (include/ngan_geoaug.h), per sample with row {a00, a01, a02, a10, a11, a12}:
    si = a00 i + a01 j + a02,  sj = a10 i + a11 j + a12                                  source position of output pixel (i, j)
    y[i, j] = sum over the taps (floor si + di, floor sj + dj), di, dj in {0, 1}, of w . tap,  (ti, tj) = (si - floor si, sj - floor sj),
              w = (di ? ti : 1 - ti)(dj ? tj : 1 - tj);  a tap outside the image holds `fill`;  ti = tj = 0: the tap (floor si, floor sj)
    adjoint:  gx[q] = sum over p of w_p(q) gy[p]
The restatement evaluates si and sj from the fp32 entries in double (the products are exact there, the two additions round at 2^-53)
and blends in double.  The kernels do the same and round the result to fp32 once.

Bound, per element:   |got - ref| <= N_ROUND 2^-24 absref + coordinate term,   N_ROUND = 2
  absref   forward  sum w |tap| (|fill| for a tap outside), 0 where the source position is a cell or more off the image
           adjoint  sum w_p(q) |gy[p]|
  N_ROUND  the kernels carry coordinates, fractions, weights and the sum in double and round to fp32 once on the way to an element:
           1 rounding, at most 2^-24 of |result| <= 2^-24 absref (the double arithmetic errs at a few 2^-53: no further unit).
           Doubled, as everywhere in this suite, so that the bound is one the reference alone meets: 2.
           tests/test_diffgeo_cpu.py holds the fp32 emulation to half the bound.
  coordinate term
           An implementation may evaluate the two coordinates in fp32, si = fmaf(a00, i, fmaf(a01, j, a02)).  A fused multiply-add
           errs by at most 2^-24 of its result, so each coordinate is then off by at most d = 2^-24 (|inner fmaf| + |outer fmaf|),
           evaluated per pixel, and the fraction si - floor si, exact for si >= 0, rounds once more, by at most 2^-25, for
           -1 < si < 0 (the difference 1 + si has a coarser grid than si), added to d there.  The kernels of csrc/diffgeo.hip
           evaluate the coordinates in double and use none of this term: an fp32 evaluation takes 0.5 .. 1 of it (a rounding costs
           between 2^-25 and 2^-24 of the value) and so cannot stay within half the bound where the term dominates.
           forward: the blend is continuous and piecewise bilinear in (si, sj), also across a cell boundary, with a slope of at most
             the largest absolute difference between adjacent pixels around the position; a floor that flips therefore costs no more.
             The term is (d_i + d_j) times the largest absolute difference between horizontally or vertically adjacent pixels (fill
             included) in the 4 x 4 neighbourhood of the cell (rows floor si - 1 .. floor si + 2, columns likewise).
           adjoint: w_p(q) is continuous in p's source position with slope at most 1 per coordinate and vanishes where the cell stops
             touching q, so p's weight on q is off by at most d_i(p) + d_j(p), for every p whose cell touches q or would after a
             flipped floor: q in the 4 x 4 neighbourhood of p's cell.  The term is the sum of (d_i(p) + d_j(p)) |gy[p]| over those p.
A row whose six entries are integers (the identity and the eight blits: entries in {0, +-1}, offsets in {0, R - 1}) has exact
coordinates and zero fractions everywhere: bound 0, the kernels copy bit for bit.  So does every position whose 4 x 4 neighbourhood
is all fill.

Which tests need the product: restatement, emulation, grid_sample transcription and parameter arithmetic here are checked against
each other in tests/test_diffgeo_cpu.py without touching the package -- self-checks of the reference, which pass on any commit; the
tests that fail without the feature are those that call the library, the operators, the trainer or the flags with a new group."""
import functools
import math

import numpy as np

f32, f64 = np.float32, np.float64
N_ROUND = 2.0
EPS = 2.0 ** -24
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
GROUPS = {"color": 1, "translation": 2, "cutout": 4, "blit": 8, "geometry": 16}
LOG2_SCALE = 0.35
PAD = 4                                    # padding of the neighbourhood search: cells are clipped to [-3, R + 1]

# (B, C, R): one-row float4 tiles;  several channels at the smallest size;  several workgroups per sample and an odd batch;  full-length rows
SHAPES = [(3, 1, 16), (2, 3, 4), (5, 1, 64), (2, 1, 512)]
FILLS = (0.0, -1.0)


def policy_mask(policy):
    return sum(GROUPS[s.strip()] for s in policy.split(",") if s.strip())


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def affine_row(R, flip=False, k=0, s=1.0, theta=None, inv=None):
    """the row of include/ngan_geoaug.h in double, each entry rounded to fp32 once: A = Flip . Quarter^k . (1 / s) . Rot(theta) about
    the centre; theta None: the rotation gate is closed; inv: 1 / s given directly"""
    B = np.eye(2)
    Q = np.array([[0.0, 1.0], [-1.0, 0.0]])
    for _ in range(k):
        B = B @ Q
    if flip:
        B = np.array([[1.0, 0.0], [0.0, -1.0]]) @ B
    co, sn = (1.0, 0.0) if theta is None else (math.cos(theta), math.sin(theta))
    if inv is None:
        inv = 1.0 / s
    G = np.array([[inv * co, -(inv * sn)], [inv * sn, inv * co]])
    if sn == 0.0:
        G[0, 1] = G[1, 0] = 0.0
    A = B @ G + 0.0
    c = 0.5 * (R - 1)
    row = (A[0, 0], A[0, 1], c - (A[0, 0] + A[0, 1]) * c, A[1, 0], A[1, 1], c - (A[1, 0] + A[1, 1]) * c)
    return tuple(float(f32(v)) for v in row)


def blit_rows(R):
    """the eight blits, (flip, k) in row-major order: rot90(flip(x), k)"""
    return [affine_row(R, flip=bool(f), k=k) for f in (0, 1) for k in range(4)]


def master_rows(R):
    """identity; the eight blits; theta = +-pi/2 and +-pi through the general path (cos or sin a rounding away from 0: coordinates a
    rounding away from integers, the floor-flip stress); theta = pi/4 at both ends of the scale range (largest window, most fill);
    the scale alone at both ends; theta = 1e-3; a flip composed with theta = 2.0 and s = 1.1"""
    lo, hi = 2.0 ** -LOG2_SCALE, 2.0 ** LOG2_SCALE
    return ([IDENTITY] + blit_rows(R)
            + [affine_row(R, theta=t) for t in (math.pi / 2, -math.pi / 2, math.pi, -math.pi)]
            + [affine_row(R, s=hi, theta=math.pi / 4), affine_row(R, s=lo, theta=math.pi / 4)]
            + [affine_row(R, s=hi), affine_row(R, s=lo)]
            + [affine_row(R, theta=1e-3), affine_row(R, flip=True, s=1.1, theta=2.0)])


def tables(B, R):
    """[(name, B rows)]: the master rows dealt out B at a time until each has been used"""
    rows = master_rows(R)
    return [(f"t{t}", [rows[(t * B + n) % len(rows)] for n in range(B)]) for t in range((len(rows) + B - 1) // B)]


def is_exact(row):
    """integer entries: exact coordinates, zero fractions"""
    return all(float(v) == round(float(v)) for v in row)


def seed_of(tag, *shape):
    s = tag
    for v in shape:
        s = (s * 131 + int(v)) % (2 ** 31 - 1)
    return s


def inputs(B, C, R):
    """images in [-1, 1] with a mean away from zero and an incoming gradient, a -0.0 in each"""
    g = np.random.default_rng(seed_of(11, B, C, R))
    x = (g.uniform(-1, 1, (B, C, R, R)) * 0.8 + 0.2).astype(f32)
    gy = g.standard_normal((B, C, R, R)).astype(f32)
    x[0, 0, 1, 2] = -0.0
    x[-1, -1, R - 1, 0] = -0.0
    gy[0, 0, 2, 1] = -0.0
    gy[-1, -1, 0, R - 1] = -0.0
    return x, gy


# ---- the geometry of one row: cells, fractions, coordinate errors ---------------------------------------------------------------------
def _grid(R):
    return np.meshgrid(np.arange(R, dtype=f64), np.arange(R, dtype=f64), indexing="ij")


@functools.lru_cache(maxsize=64)
def plan(row, R):
    """per output pixel, from the fp32 entries in double: cell (i0, j0) clipped to [-3, R + 1], fractions, `near` (some tap can lie
    inside), and the coordinate errors d_i + d_j of the bound"""
    a = [f64(f32(v)) for v in row]
    ii, jj = _grid(R)
    out = {}
    d = np.zeros((R, R))
    for name, (p, q, t) in (("i", a[0:3]), ("j", a[3:6])):
        inner = q * jj + t
        s = p * ii + inner
        fl = np.floor(s)
        out["s" + name], out["t" + name] = s, s - fl
        out["c" + name] = np.clip(fl, -3, R + 1).astype(np.int64)
        d += EPS * (np.abs(inner) + np.abs(s)) + np.where(s < 0, 2.0 ** -25, 0.0)
    out["near"] = (out["si"] > -1) & (out["si"] < R) & (out["sj"] > -1) & (out["sj"] < R)
    out["d"] = np.zeros((R, R)) if is_exact(row) else d
    out["exact"] = is_exact(row)
    return out


def _taps(pl):
    """[(di, dj, weight)] of the four taps, weights in double"""
    ti, tj = pl["ti"], pl["tj"]
    return [(0, 0, (1 - ti) * (1 - tj)), (0, 1, (1 - ti) * tj), (1, 0, ti * (1 - tj)), (1, 1, ti * tj)]


def _padded(img, fill):
    R = img.shape[-1]
    xp = np.full(img.shape[:-2] + (R + 2 * PAD, R + 2 * PAD), f64(f32(fill)))
    xp[..., PAD:PAD + R, PAD:PAD + R] = img
    return xp


def _neighbourhood_slope(xp):
    """M[r, c]: the largest |difference| between adjacent entries of the 4 x 4 block of xp with top left corner (r, c)"""
    n = xp.shape[-1]
    dh = np.abs(np.diff(xp, axis=-1))      # (.., n, n - 1)
    dv = np.abs(np.diff(xp, axis=-2))      # (.., n - 1, n)
    m = np.zeros(xp.shape[:-2] + (n - 3, n - 3))
    for r in range(4):
        for c in range(3):
            m = np.maximum(m, dh[..., r:r + n - 3, c:c + n - 3])
            m = np.maximum(m, dv[..., c:c + n - 3, r:r + n - 3])
    return m


def fwd_ref(x, rows, fill=0.0):
    """(ref, bound) in fp64"""
    B, C, R, _ = x.shape
    x = x.astype(f64)
    fv = f64(f32(fill))
    ref, bd = np.empty_like(x), np.empty_like(x)
    for n, row in enumerate(rows):
        pl = plan(tuple(row), R)
        xp = _padded(x[n], fill)
        ci, cj = pl["ci"], pl["cj"]
        y, a = np.zeros((C, R, R)), np.zeros((C, R, R))
        for di, dj, w in _taps(pl):
            v = xp[:, ci + di + PAD, cj + dj + PAD]
            y += w * v
            a += w * np.abs(v)
        near = pl["near"]
        ref[n] = np.where(near, y, fv)
        slope = _neighbourhood_slope(xp)[:, ci - 1 + PAD, cj - 1 + PAD]
        bd[n] = 0.0 if pl["exact"] else N_ROUND * EPS * np.where(near, a, 0.0) + pl["d"] * slope
    return ref, bd


def bwd_ref(gy, rows):
    """(ref, bound) in fp64: the scatter form of the adjoint"""
    B, C, R, _ = gy.shape
    gy = gy.astype(f64)
    ref, bd = np.empty_like(gy), np.empty_like(gy)
    for n, row in enumerate(rows):
        pl = plan(tuple(row), R)
        ci, cj, near = pl["ci"], pl["cj"], pl["near"]
        for ch in range(C):
            g = gy[n, ch]
            acc, aab, win = np.zeros(R * R), np.zeros(R * R), np.zeros(R * R)
            for di, dj, w in _taps(pl):
                qi, qj = ci + di, cj + dj
                ok = near & (qi >= 0) & (qi < R) & (qj >= 0) & (qj < R)
                idx = (qi * R + qj)[ok]
                acc += np.bincount(idx, weights=(w * g)[ok], minlength=R * R)
                aab += np.bincount(idx, weights=(w * np.abs(g))[ok], minlength=R * R)
            if not pl["exact"]:
                e = pl["d"] * np.abs(g)
                for di in range(-1, 3):
                    for dj in range(-1, 3):
                        qi, qj = ci + di, cj + dj
                        ok = (qi >= 0) & (qi < R) & (qj >= 0) & (qj < R)
                        win += np.bincount((qi * R + qj)[ok], weights=e[ok], minlength=R * R)
            ref[n, ch] = acc.reshape(R, R)
            bd[n, ch] = 0.0 if pl["exact"] else (N_ROUND * EPS * aab + win).reshape(R, R)
    return ref, bd


def ratio(got, ref, bd):
    """worst |got - ref| / bound; a position with bound 0 must hold the reference exactly (inf otherwise)"""
    err = np.abs(np.asarray(got, f64) - ref)
    if (err[bd == 0] != 0).any():
        return float("inf")
    return float((err[bd > 0] / bd[bd > 0]).max()) if (bd > 0).any() else 0.0


def pairing_defect(x, g, y, y0, gx):
    """|<T x - T 0, g> - <x, T^T g>| in fp64: T is affine (the fill adds a constant), its linear part is what the adjoint transposes"""
    lhs = ((y.astype(f64) - y0.astype(f64)) * g).sum()
    return abs(lhs - (x.astype(f64) * gx).sum())


def pairing_slack(x, g, rows, fill=0.0):
    """the per-element bounds of T x, T 0 and T^T g, summed against the other factor, plus what the two double sums of pairing_defect
    round themselves: n 2^-53 of their sums of absolute values"""
    r, b = fwd_ref(x, rows, fill)
    r0, b0 = fwd_ref(np.zeros_like(x), rows, fill)
    rg, bg = bwd_ref(g, rows)
    sums = ((np.abs(r) + np.abs(r0)) * np.abs(g)).sum() + (np.abs(x) * np.abs(rg)).sum()
    return ((b + b0) * np.abs(g)).sum() + (np.abs(x) * bg).sum() + x.size * 2.0 ** -53 * sums


# ---- the kernels' arithmetic in numpy: double throughout, one rounding to fp32 -------------------------------------------------------------------------------------------------
def _fma(a, x, c):
    """double fused multiply-add of an fp32 entry (as double), an integer and a double: the product is exact, one rounding"""
    return f64(f32(a)) * np.asarray(x, f64) + np.asarray(c, f64)


def _emulated_cells(row, R):
    """cells, fractions and weights as the kernels form them: all in double from the fp32 entries"""
    ii, jj = _grid(R)
    out = []
    for p, q, t in (row[0:3], row[3:6]):
        s = _fma(p, ii, _fma(q, jj, f64(f32(t))))
        fl = np.floor(s)
        out.append((s, np.clip(fl, -3, R + 1).astype(np.int64), s - fl))
    (si, ci, ti), (sj, cj, tj) = out
    near = (si > -1) & (si < R) & (sj > -1) & (sj < R)
    w = [(1.0 - ti) * (1.0 - tj), (1.0 - ti) * tj, ti * (1.0 - tj), ti * tj]
    return ci, cj, near, (ti == 0) & (tj == 0), w


def fwd_emulate(x, rows, fill=0.0):
    B, C, R, _ = x.shape
    out = np.empty_like(x)
    for n, row in enumerate(rows):
        ci, cj, near, zero, w = _emulated_cells(row, R)
        xp = _padded(x[n].astype(f64), fill)
        s = np.zeros((C, R, R))
        for t, (di, dj) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            s += w[t] * xp[:, ci + di + PAD, cj + dj + PAD]
        y = np.where(zero, xp[:, ci + PAD, cj + PAD], s).astype(f32)
        out[n] = np.where(near, y, f32(fill))
    return out


def bwd_emulate(gy, rows):
    B, C, R, _ = gy.shape
    out = np.empty_like(gy)
    for n, row in enumerate(rows):
        ci, cj, near, zero, w = _emulated_cells(row, R)
        for ch in range(C):
            g = gy[n, ch].astype(f64)
            acc = np.zeros(R * R)
            for t, (di, dj) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
                qi, qj = ci + di, cj + dj
                ok = near & (qi >= 0) & (qi < R) & (qj >= 0) & (qj < R) & (~zero if t else True)
                term = np.where(zero, g, w[t] * g)
                acc += np.bincount((qi * R + qj)[ok], weights=term[ok], minlength=R * R)
            out[n, ch] = acc.reshape(R, R).astype(f32)
    return out


# ---- the same operator through torch's grid_sample (fp64, differentiable by torch.autograd) ------------------------------------------
def grid_theta(rows, R):
    """(B, 2, 3) matrices of F.affine_grid(align_corners=True) for the rows: normalised (x, y) = (column, row) / c - 1, c = (R - 1) / 2"""
    c = 0.5 * (R - 1)
    th = np.zeros((len(rows), 2, 3))
    for n, row in enumerate(rows):
        a00, a01, a02, a10, a11, a12 = (f64(f32(v)) for v in row)
        th[n] = [[a11, a10, a10 + a11 + a12 / c - 1.0], [a01, a00, a00 + a01 + a02 / c - 1.0]]
    return th


def transcription(x, rows, fill=0.0):
    """x: (B, C, R, R) double tensor -> T(x) by affine_grid + grid_sample (bilinear, zero padding, align_corners=True); the fill
    constant by shifting the values so that it becomes the padding's zero"""
    import torch
    import torch.nn.functional as F
    grid = F.affine_grid(torch.from_numpy(grid_theta(rows, x.shape[-1])), list(x.shape), align_corners=True)
    return F.grid_sample(x - float(fill), grid, mode="bilinear", padding_mode="zeros", align_corners=True) + float(fill)


# ---- ngan_diffgeo_params in numpy -----------------------------------------------------------------------------------------------------
def draw_int(u, n):
    """min(n - 1, floor(u n)) with the product in fp32"""
    return int(min(n - 1, np.floor(f32(u) * f32(n))))


def params_ref(U, R, mask, p):
    """(B, 8) uniforms -> list of rows; mask: bits 1 blit, 2 geometry (GROUPS' bits >> 3).  u0 / u1 the flip's gate and coin, u2 / u3
    the quarter turns' gate and count, u4 / u5 the scale's gate and exponent, u6 / u7 the rotation's gate and angle"""
    U = np.asarray(U, f32)
    p = f32(p)
    rows = []
    for u in U:
        flip, k, inv, theta = False, 0, 1.0, None
        if mask & 1:
            flip = bool(u[0] < p and u[1] < f32(0.5))
            if u[2] < p:
                k = draw_int(u[3], 4)
        if mask & 2:
            if u[4] < p:
                inv = float(np.exp2(-((2.0 * f64(u[5]) - 1.0) * LOG2_SCALE)))      # 1 / s, as the kernel forms it
            if u[6] < p:
                theta = float((2.0 * f64(u[7]) - 1.0) * math.pi)
        rows.append(affine_row(R, flip, k, theta=theta, inv=inv))
    return rows


def params_close(got, ref, R):
    """linear entries within 4 2^-24 max(1, |ref|), offsets within that times R (the device's exp2, cos and sin against numpy's: a few
    units of 2^-53, then one rounding to fp32 each -- a unit of 2^-24 apart at most; 4 with the factor everything here carries)"""
    for g, r in zip(got, ref):
        for k in range(6):
            tol = 4 * EPS * max(1.0, abs(r[k])) * (R if k in (2, 5) else 1)
            if not abs(g[k] - r[k]) <= tol:
                return False
    return len(got) == len(ref)


def chosen_uniforms(p=0.5):
    """every pairing of 0, 0.5 and 1 - 2^-24 in the value columns with each gate column below p (open), at p exactly (closed: the
    comparison is strict) and above it"""
    vals = [0.0, 0.25, 0.5, 1.0 - 2.0 ** -24]
    rows = []
    for gate in (0.5 * p, p, 0.5 * (1 + p)):
        for a in vals:
            for b in vals:
                rows.append([gate, a, gate, b, gate, a, gate, b])
                rows.append([p - gate if gate < p else gate, b, gate, a, 0.5 * p, b, gate, a])
    return np.asarray(rows, f32)
