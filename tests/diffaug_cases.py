"""Differentiable augmentation (csrc/diffaug.hip, ops.DiffAugment): the operator restated in fp64 with its absolute-value twin, the
per-element bound, an fp32 emulation of the kernels' arithmetic, the integer arithmetic of ngan_diffaug_params in numpy, and the
inputs and parameter tables of the tests.  Shared by tests/test_diffaug_cpu.py (restatement against a literal transcription of the
DiffAugment steps, emulation against restatement) and tests/test_gpu_diffaug.py (the kernels against the restatement).

The operator (include/ngan.h), per sample with row {b, c, tx, ty, i0, i1, j0, j1} and N = C R R:
    m = (sum x) / N;  k = fp32(c b + (1 - c)(m + b));  u = fmaf(c, x, k)
    y[ch, i, j] = u[ch, i + tx, j + ty] if (i + tx, j + ty) is inside the image and (i, j) outside [i0, i1) x [j0, j1), else 0
    adjoint: gu[q] = gy[q - t] where q - t is inside the image and outside the cutout, else 0;
             r = fp32((1 - c) / N sum gu);  gx = fmaf(c, gu, r)

Bound, per element:   |got - ref| <= N_ROUND 2^-24 absref,   N_ROUND = 4
  absref   forward  |c| |x| + |c| |b| + |1 - c| (mean|x| + |b|) at the source position, 0 where the output is 0 by definition
           adjoint  |c| |gu| + |1 - c| / N sum|gu|
  N_ROUND  the kernel rounds twice on the way to an element: k (or r) from its double value, at most 2^-24 |k| <= 2^-24 absref, and the
           fused multiply-add, at most 2^-24 |y| <= 2^-24 absref: 2.  The fp64 sum behind k and r errs by at most N 2^-53 of the sum of
           absolute values, under 2^-25 absref for N < 2^28, and the double arithmetic that forms k and r by a few 2^-53: no further
           unit.  Doubled, as everywhere in this suite, so that a correct implementation in another legitimate order (k formed in
           fp32, the product rounded before the addition) has a factor two in hand: 4.  tests/test_diffaug_cpu.py holds the fp32
           emulation to half the bound.
A position that the definition sets to the fill constant (0 in DiffAugment's own form, -1 in the trainer's) has absref 0: the kernels
must store exactly that constant there.

Which tests need the product: the restatement, transcription, emulation and parameter arithmetic here are checked against each other
in tests/test_diffaug_cpu.py without touching the package -- self-checks of the reference, which pass on any commit; the tests that
fail without the feature are those that call the library, the operators, the trainers or the flags."""
import numpy as np
import torch

f32, f64 = np.float32, np.float64
N_ROUND = 4.0
IDENTITY = (0.0, 1.0, 0, 0, 0, 0, 0, 0)
GROUPS = {"color": 1, "translation": 2, "cutout": 4}

# (B, C, R): S = 2, K = 8;  S = 1, K = 2 and one workgroup per sample;  several workgroups per sample and an odd batch;  the sum
# pass's 32 workgroups per sample at full length
SHAPES = [(3, 1, 16), (2, 3, 4), (5, 1, 64), (2, 1, 512)]


def shift_size(R):
    return int(R * 0.125 + 0.5)


def cutout_size(R):
    return int(R * 0.5 + 0.5)


def cutout_box(oi, oj, R):
    K = cutout_size(R)
    return (max(oi - K // 2, 0), min(oi - K // 2 + K, R), max(oj - K // 2, 0), min(oj - K // 2 + K, R))


def master_rows(R):
    """ten rows: shifts at +-S in all four sign pairs, one-step and zero shifts, a column shift that is / is not a multiple of 4;
    cutouts over each corner and each edge, and inside; c in {0.5, 1.5} and b = +-0.5 among the colour values; one identity"""
    S, K = shift_size(R), cutout_size(R)
    last = R - (K & 1)                   # the largest centre offset
    mid = R // 2
    odd = min(S, 3) if S >= 3 else 1     # a column shift that is no multiple of 4
    return [
        (0.5, 1.5, S, -S) + cutout_box(mid, mid, R),            # inside
        (-0.5, 0.5, -S, S) + cutout_box(0, 0, R),               # top left corner
        IDENTITY,
        (0.5, 0.5, S, S) + cutout_box(last, last, R),           # bottom right corner
        (-0.5, 1.5, -S, -S) + cutout_box(0, mid, R),            # top edge
        (0.25, 1.25, 1, 0) + cutout_box(last, mid, R),          # bottom edge
        (-0.125, 0.75, 0, -odd) + cutout_box(mid, 0, R),        # left edge
        (0.0, 1.0, 0, odd) + cutout_box(mid, last, R),          # right edge, colour closed
        (0.375, 1.5, -1, min(S, 4)) + cutout_box(0, last, R),   # top right corner
        (-0.5, 0.5, S, -1) + cutout_box(last, 0, R),            # bottom left corner
    ]


def tables(B, R):
    """[(name, B rows)]: the master rows dealt out B at a time until each has been used, then a whole identity table"""
    rows = master_rows(R)
    out = []
    for t in range((len(rows) + B - 1) // B):
        out.append((f"t{t}", [rows[(t * B + n) % len(rows)] for n in range(B)]))
    out.append(("identity", [IDENTITY] * B))
    return out


def colourless(rows):
    return [(0.0, 1.0) + tuple(r[2:]) for r in rows]


def seed_of(tag, *shape):
    s = tag
    for v in shape:
        s = (s * 131 + int(v)) % (2 ** 31 - 1)
    return s


def inputs(B, C, R):
    """images in [-1, 1] with a mean away from zero, and an incoming gradient"""
    g = np.random.default_rng(seed_of(7, B, C, R))
    x = (g.uniform(-1, 1, (B, C, R, R)) * 0.8 + 0.2).astype(f32)
    gy = g.standard_normal((B, C, R, R)).astype(f32)
    return x, gy


def _windows(R, t):
    """destination and source slices of a shift by t along one axis: dst[i] = src[i + t]"""
    lo, hi = max(0, -t), min(R, R - t)
    return slice(lo, max(lo, hi)), slice(lo + t, max(lo, hi) + t)


def _shift(u, tx, ty):
    R = u.shape[-1]
    y = np.zeros_like(u)
    di, si = _windows(R, tx)
    dj, sj = _windows(R, ty)
    y[..., di, dj] = u[..., si, sj]
    return y


def _live(R, row):
    """(R, R) bool: the output positions that receive a source value (the others hold the fill)"""
    b, c, tx, ty, i0, i1, j0, j1 = row
    live = _shift(np.ones((1, R, R)), tx, ty)[0] > 0
    live[i0:i1, j0:j1] = False
    return live


def fwd_ref(x, rows, fill=0.0):
    """(ref, absref) in fp64; fill: the constant of the positions the shift or the cutout leaves empty (absref 0: exact)"""
    x = x.astype(f64)
    ref, absref = np.zeros_like(x), np.zeros_like(x)
    for n, (b, c, tx, ty, i0, i1, j0, j1) in enumerate(rows):
        b, c = f64(f32(b)), f64(f32(c))
        m, ma = x[n].mean(), np.abs(x[n]).mean()
        k = c * b + (1 - c) * (m + b)
        y = _shift(c * x[n] + k, tx, ty)
        a = _shift(abs(c) * np.abs(x[n]) + abs(c) * abs(b) + abs(1 - c) * (ma + abs(b)), tx, ty)
        live = _live(x.shape[-1], rows[n])
        ref[n], absref[n] = np.where(live, y, f64(f32(fill))), np.where(live, a, 0.0)
    return ref, absref


def _adjoint_gather(g, tx, ty, box):
    i0, i1, j0, j1 = box
    g = g.copy()
    g[:, i0:i1, j0:j1] = 0
    return _shift(g, -tx, -ty)          # gu[q] = masked gy[q - t]


def bwd_ref(gy, rows):
    gy = gy.astype(f64)
    ref, absref = np.zeros_like(gy), np.zeros_like(gy)
    N = gy[0].size
    for n, (b, c, tx, ty, i0, i1, j0, j1) in enumerate(rows):
        c = f64(f32(c))
        gu = _adjoint_gather(gy[n], tx, ty, (i0, i1, j0, j1))
        ref[n] = c * gu + (1 - c) / N * gu.sum()
        absref[n] = abs(c) * np.abs(gu) + abs(1 - c) / N * np.abs(gu).sum()
    return ref, absref


def _fmaf(c, x, k):
    """fp32 fused multiply-add of fp32 operands: the product is exact in double, the sum rounds to double and then to fp32"""
    return (f64(c) * x.astype(f64) + f64(k)).astype(f32)


def fwd_emulate(x, rows, fill=0.0):
    """the forward kernels' arithmetic in numpy: fp64 sum, k rounded once from double, one fp32 fused multiply-add per element"""
    out = np.zeros_like(x)
    for n, (b, c, tx, ty, i0, i1, j0, j1) in enumerate(rows):
        b, c = f32(b), f32(c)
        m = x[n].astype(f64).sum() / x[n].size
        k = f32(f64(c) * f64(b) + (1.0 - f64(c)) * (m + f64(b)))
        out[n] = np.where(_live(x.shape[-1], rows[n]), _shift(_fmaf(c, x[n], k), tx, ty), f32(fill))
    return out


def bwd_emulate(gy, rows):
    out = np.zeros_like(gy)
    for n, (b, c, tx, ty, i0, i1, j0, j1) in enumerate(rows):
        c = f32(c)
        gu = _adjoint_gather(gy[n], tx, ty, (i0, i1, j0, j1))
        r = f32((1.0 - f64(c)) / gy[n].size * gu.astype(f64).sum())
        out[n] = _fmaf(c, gu, r)
    return out


def bound(absref):
    return N_ROUND * 2.0 ** -24 * absref


def ratio(got, ref, absref):
    """worst |got - ref| / bound; a position with bound 0 must hold the reference exactly (inf otherwise)"""
    err = np.abs(np.asarray(got, f64) - ref)
    bd = bound(absref)
    if (err[bd == 0] != 0).any():
        return float("inf")
    return float((err[bd > 0] / bd[bd > 0]).max()) if (bd > 0).any() else 0.0


def pairing_defect(x, g, y, y0, gx):
    """|<T x - T 0, g> - <x, T^T g>| in fp64: T is affine (brightness adds a constant), its linear part is what the adjoint transposes"""
    lhs = ((y.astype(f64) - y0.astype(f64)) * g).sum()
    return abs(lhs - (x.astype(f64) * gx).sum())


def pairing_slack(x, g, rows):     # (the fill is part of T 0 and has bound 0)
    """the per-element bounds of T x, T 0 and T^T g, summed against the other factor"""
    _, a = fwd_ref(x, rows)
    _, a0 = fwd_ref(np.zeros_like(x), rows)
    _, ag = bwd_ref(g, rows)
    return ((bound(a) + bound(a0)) * np.abs(g)).sum() + (np.abs(x) * bound(ag)).sum()


# ---- a literal transcription of the DiffAugment steps in torch operators (fp64, differentiable by torch.autograd) -------------------
def transcription(x, rows, fill=0.0):
    """x: (B, C, R, R) double tensor.  brightness x + b; contrast (x - mean) c + mean; translation: padding by S on every side (with
    `fill`; DiffAugment pads with 0) and the shifted window; cutout: the fill where a 0/1 mask is 0."""
    import torch.nn.functional as F
    R = x.shape[-1]
    S = max(shift_size(R), max(max(abs(r[2]), abs(r[3])) for r in rows))
    out = []
    for n, (b, c, tx, ty, i0, i1, j0, j1) in enumerate(rows):
        b, c = float(f32(b)), float(f32(c))
        v = x[n] + b
        mean = v.mean()
        v = (v - mean) * c + mean
        v = F.pad(v, (S, S, S, S), value=float(fill))[:, S + tx:S + tx + R, S + ty:S + ty + R]
        mask = torch.ones(R, R, dtype=torch.bool)
        mask[i0:i1, j0:j1] = False
        out.append(v * mask + float(fill) * (~mask))
    return torch.stack(out)


# ---- ngan_diffaug_params in numpy --------------------------------------------------------------------------------------------------
def draw_int(u, n):
    """min(n - 1, floor(u n)) with the product in fp32"""
    return np.minimum(n - 1, np.floor(u.astype(f32) * f32(n)).astype(np.int64))


def policy_mask(policy):
    return sum(GROUPS[s.strip()] for s in policy.split(",") if s.strip())


def params_ref(U, R, mask, p):
    """(B, 8) uniforms -> list of rows; the scheme of include/ngan.h: u0 colour gate, u1 brightness, u2 contrast, u3 translation gate,
    u4 the shift pair, u5 cutout gate, u6 / u7 the cutout's centre offsets"""
    U = np.asarray(U, f32)
    S, K = shift_size(R), cutout_size(R)
    side, span = 2 * S + 1, R + 1 - K % 2
    cell = draw_int(U[:, 4], side * side)
    oi, oj = draw_int(U[:, 6], span), draw_int(U[:, 7], span)
    p = f32(p)
    rows = []
    for n in range(U.shape[0]):
        row = list(IDENTITY)
        if mask & 1 and U[n, 0] < p:
            row[0], row[1] = float(U[n, 1] - f32(0.5)), float(U[n, 2] + f32(0.5))
        if mask & 2 and U[n, 3] < p:
            row[2], row[3] = int(cell[n] // side - S), int(cell[n] % side - S)
        if mask & 4 and U[n, 5] < p:
            row[4:8] = cutout_box(int(oi[n]), int(oj[n]), R)
        rows.append(tuple(row))
    return rows


def chosen_uniforms():
    """every combination of 0, 0.5 and 1 - 2^-24 in the value columns, with the three gate columns at 0.25 (open at p = 0.5) and at
    0.75 (closed at p = 0.5), dealt out so that each value meets each gate state"""
    vals = [0.0, 0.5, 1.0 - 2.0 ** -24]
    rows = []
    for gate in (0.25, 0.75):
        for a in vals:
            for b in vals:
                rows.append([gate, a, b, gate, a, gate, b, a])
                rows.append([1.0 - gate, b, a, gate, b, 1.0 - gate, a, b])
    return np.asarray(rows, f32)
