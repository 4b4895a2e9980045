"""The input pipeline's augmentation kernels (csrc/augment.hip: `ngan_augment_batch`, two launches) pinned pass by pass: shared cases,
the fp64 definition, the per-element bounds and an fp32 emulation in the kernels' own order.  Shared by tests/test_gpu_augment.py (the
kernels against the definition) and tests/test_augment_bounds_cpu.py (the emulation against the definition: it settles the constants
on the CPU before any kernel is looked at, and shows that fifteen wrong emulations miss their checks).  No test in here, and nothing
of the package is imported: `pack` restates `NeuronDataset.pack_params`, and the CPU test holds the two together bit for bit.

Pass 1 (augment_affine_kernel) is compared BIT FOR BIT.  Its arithmetic on pixel values is a gather followed by at most one fp32
multiply and a clamp, which numpy fp32 reproduces exactly; what can differ legitimately is which source pixel a coordinate next to a
rounding boundary picks.  `pass1_definition` takes the fp32 cos / sin / tx / ty of the packed record, as the kernel receives them,
evaluates the kernel's coordinate expression
    xs = cos xd + sin yd + c0,  ys = -sin xd + cos yd + c0,   xd = xo - c0 - tx,  yd = (flip ? P - 1 - yo : yo) - c0 - ty,  c0 = (P - 1) / 2
in fp64, and calls a pixel AMBIGUOUS when either coordinate lies within MARGIN = 2^-20 P of k + 1/2.  Why that margin: the fp32
evaluation has five roundings of quantities below 2 P (two products, two sums below P sqrt 2, the subtractions of c0 and t are exact
for integers and half-integers below 2^23), each at most 2^-24 of its value: at most 5 * 2 P * 2^-24 = 0.625 * 2^-20 P in the worst
case, and a contracted multiply-add only removes roundings.  The emulation below (no contraction) stays under 0.13 of the margin on
every case (printed by the CPU test).  An unambiguous pixel has one admissible value; an ambiguous one admits the values of its up to
four neighbouring sources (floor and ceiling of each ambiguous coordinate), each zero where that source lies outside the canvas.  The
flip acts on the affine's OUTPUT row, brightness (clamped) is applied in pass 1 only when contrast_first == 0.  The share of ambiguous
pixels of any sample is capped at AMBIGUOUS_CAP = 5 %: a condition on the case table, asserted on the CPU from the definition alone,
not a tolerance.  Exact ties are there on purpose: at 45 degrees both diagonals of an even canvas (2 / P of the pixels), at 30 degrees
(sin = 0.5 exactly in fp32) every other pixel of the centre row and column of an odd canvas (1 / P).  Those two rows are left out at
P = 3 and P = 6, where the same ties are 44 % and 33 % of the canvas.

Pass 2 (augment_finish_kernel) is defined from the KERNEL'S OWN canvas, read back from the workspace, so that a nearest-neighbour
choice of pass 1 cannot dilute it.  In fp64 (`pass2_definition`): the mean over the whole P x P canvas; the remaining colour operations,
blend-and-clamp, brightness after contrast iff contrast_first; the crop at offset R // 4; 2 v - 1; and Wy @ img @ Wx^T with dense S x R
weight matrices from aten's antialias definition (`aa_matrix`: window [int(c - scale + .5), int(c + scale + .5)) clipped to [0, R),
c = scale (i + .5), weight 1 - |j - c + .5| / scale, rows normalised by their own sum).  S = R skips the resize.  The partial sums
of pass 1 are compared with fp64 tile sums of the kernel's canvas (`tile_sums`); the tile size is read from the library's workspace
formula (`tile_pixels`), not written down here.

Bounds, per element:  |got - ref| <= C_ACC 2^-24 absref.
  partial (b, t)   absref = the tile's sum of absolute values
  out              absref = sum_j w~_j |colour_j| over the window (w~ the normalised weights) + |1 - contrast| mean, the mean's
                   contribution.  At S = R the window is the pixel itself.
  out at S = R     also: absform = the formula on absolute values, a = 2 min(contrast v + |1 - contrast| mean, 1) [* brightness,
                   clamped at 1, if it comes second] + 1
C_ACC is not fixed in advance: per output class it is the smallest power of two at which the emulation stays at or below 0.5 of the
bound on every case (`C_ACC` below; tests/test_augment_bounds_cpu.py asserts each is needed and minimal, and prints the table that
DESIGN.md quotes).  Measured against the emulation, never against the kernel.  Why S = R has a second bound: the roundings of the
blend, of the brightness product and of the mean are relative to v and to |1 - contrast| mean, which the renormalisation 2 v - 1
cancels, so a pixel at mid grey (colour = 0) carries an error of 2^-24 whatever |colour| is.  With nothing to average over, the first
form needs C_ACC = 2^18 at S = R (emulated worst 1.1e5 at R = 33) and says little there; `absform` is |colour| plus what was
cancelled, needs C_ACC = 4, and is asserted next to it.  At S < R absref <= absform element by element, so the first form is the
tighter one at any common constant, and it alone is asserted.

Emulation (class Emulator), numpy fp32 in the kernels' order: pass 1 -- a thread adds its 8 pixels of the tile (stride 256) one after
the other, the butterfly of group_sum<64> per wave, (red0 + red1) + (red2 + red3); pass 2 -- lane l adds partials l, l + 64, ...,
the same butterfly, one division by float(P) float(P); colour per tap without contraction; r = fma(wx, colour, r) along the row,
acc = fma(wy, r, acc) down the window, one division by wys * wxs (the weight sums added serially).  An fma is emulated as the fp64
product and sum rounded once more to fp32 (the product is exact in fp64; the double rounding differs from a true fma in about one
case in 2^29).  `Emulator(wrong)` commits one named mistake; WRONG lists the case each must fail on."""
import functools
import math
import types

import numpy as np

f32, f64 = np.float32, np.float64

MARGIN_PER_PIXEL = 2.0 ** -20      # x P: how near a rounding boundary a source coordinate may lie before both neighbours are admitted
AMBIGUOUS_CAP = 0.05               # largest share of ambiguous pixels in any sample of the table
N_IMAGES = 5
EMULATED_TILE = 2048               # 256 threads x 8 pixels: the only tile the emulation's order describes

# R -> stage sizes S.  P = R + 2 (R // 4).  The smallest shapes at which each mechanism can still go wrong:
#   3    no padding (P = 3), crop 0, fewer pixels than a wave           4    36 pixels, one ragged tile
#   33   odd canvas (P = 49, integer centre), 2 tiles, ragged last      40   even canvas (P = 60), scales 2 / 5 / 8
#   64   P = 96, 4.5 tiles                                              256  P = 384, 72 tiles > the 64 lanes of the partial-sum loop,
#                                                                            128-tap windows at S = 4; two samples only
GEOMETRY = {3: (3, 1), 4: (4, 2, 1), 33: (33, 11, 3, 1), 40: (40, 20, 8, 5), 64: (64, 16, 4), 256: (256, 4)}
CASES = [(R, S) for R, sizes in GEOMETRY.items() for S in sizes]

# per output class: the smallest power of two at which the emulation stays <= 0.5 of the bound on every case (the CPU test pins it)
C_ACC = {"partials": 4.0, "out_full": 2.0 ** 18, "out_full_abs": 4.0, "out_resized": 16.0}


def canvas_of(R):
    return R + 2 * (R // 4)


def out_class(R, S):
    return "out_full" if S == R else "out_resized"


# ---- the parameter table: named rows, no seed ---------------------------------------------------------------------------------------
def rows_of(R):
    """[(name, angle in degrees, tx, ty, flip, brightness, contrast, contrast_first)] of the canvas of stage R"""
    P = canvas_of(R)
    d = float(round(0.1 * P))
    rows = [
        ("identity", 0.0, 0, 0, 0, 1.0, 1.0, 0),
        ("rot90_t", 90.0, 2, -1, 0, 1.1, 0.9, 0),
        ("rot180_t", 180.0, -1, 2, 0, 0.9, 1.1, 1),
        ("rot-90_t", -90.0, 1, 1, 1, 1.0, 1.2, 0),
        ("rot45_t", 45.0, 1, -2, 0, 1.1, 1.1, 0),             # exact ties on both diagonals of an even canvas
        ("rot30_ties", 30.0, 0, 0, 0, 0.9, 0.9, 1),             # sin = 0.5: exact ties on the centre row / column of an odd canvas
        ("rot179.9", 179.9, 0, 1, 0, 1.0, 0.8, 0),
        ("rot0.01", 0.01, -1, 0, 1, 1.2, 1.0, 1),
        ("odd_f0_c0", 17.3, 1, 0, 0, 1.1, 0.9, 0),               # four fixed odd angles: every combination of flip and contrast_first
        ("odd_f1_c0", -63.7, 0, -1, 1, 0.9, 1.1, 0),
        ("odd_f0_c1", 101.9, -1, 1, 0, 1.2, 0.8, 1),
        ("odd_f1_c1", -148.1, 0, 0, 1, 0.8, 1.2, 1),
        ("bright_both_clamps", 7.0, 0, 0, 0, 1.25, 1.25, 0),     # brightness clamps the saturated patch, contrast clamps it again
        ("bright_both_clamps_c1", -7.0, 0, 0, 0, 1.25, 1.25, 1),
        ("dim_0.75", 23.0, 0, 0, 1, 0.75, 0.75, 0),
        ("contrast_one", 23.0, 0, 0, 0, 1.1, 1.0, 1),            # the mean must drop out exactly
        ("t+x", 0.0, d, 0, 0, 1.0, 0.9, 0),                      # the largest translation draw_params makes, on each axis
        ("t-x", 0.0, -d, 0, 1, 1.0, 1.1, 1),
        ("t+y", 0.0, 0, d, 1, 1.1, 1.0, 0),
        ("t-y", 0.0, 0, -d, 0, 0.9, 1.0, 1),
        ("all_outside", 0.0, float(P), 0, 0, 1.1, 0.9, 0),       # canvas all zeros, output all -1
    ]
    if P < 40:                                                   # the tie rows would be 44 % (P = 3) and 33 % (P = 6) ambiguous
        rows = [r for r in rows if r[0] not in ("rot45_t", "rot30_ties")]
    if R == 256:                                                 # two samples: every flag set, both factors off 1; and the ties
        rows = [r for r in rows if r[0] in ("odd_f1_c1", "rot45_t")]
    return rows


# which image each sample reads: repeats, permutes, B > N, and idx[b] != b % N wherever a sample's content matters
IDX = [2, 0, 4, 1, 3, 3, 2, 0, 4, 1, 4, 2, 1, 0, 3, 1, 3, 0, 2, 2, 4]


def pack(rows):
    """the (B, 8) fp32 record array of include/ngan.h: cos and sin of the fp32 angle taken in double, then rounded"""
    rec = np.zeros((len(rows), 8), dtype=f32)
    for b, (_, angle, tx, ty, flip, brightness, contrast, cfirst) in enumerate(rows):
        rad = float(f32(angle)) * (math.pi / 180.0)
        rec[b, :6] = [math.cos(rad), math.sin(rad), tx, ty, brightness, contrast]
        rec[b, 6:].view(np.int32)[:] = [flip, cfirst]
    return rec


def flags(rec):
    return np.ascontiguousarray(rec[:, 6:8]).view(np.int32)


def images(P, n_images=N_IMAGES):
    """(N, P, P) fp32 in (0, 1): a stratified rand ** 2 (so that all values of an image are distinct and a wrong neighbour can never
    match by accident) scaled to below 0.85, a saturated patch with values above 0.85 and a dark patch holding the lowest values"""
    rng = np.random.default_rng(1000 + P)
    side = max(1, P // 5)
    out = np.zeros((n_images, P, P), dtype=f64)
    for i in range(n_images):
        bright, dark = np.zeros((P, P), bool), np.zeros((P, P), bool)
        a, d = P // 4, P - side - P // 4
        bright[a:a + side, a + i % 2:a + i % 2 + side] = True
        dark[d:d + side, d - i % 2:d - i % 2 + side] = True
        assert not (bright & dark).any()
        k, kd = int(bright.sum()), int(dark.sum())
        m = P * P - k
        out[i][bright] = 0.85 + 0.15 * (rng.permutation(k) + rng.uniform(0.25, 0.75, k)) / k
        rank = np.empty((P, P))
        rank[dark] = rng.permutation(kd)
        rank[~dark & ~bright] = kd + rng.permutation(m - kd)
        rest = ~bright
        out[i][rest] = 0.85 * ((rank[rest] + rng.uniform(0.25, 0.75, m)) / m) ** 2
    out = out.astype(f32)
    for i in range(n_images):
        assert np.unique(out[i]).size == P * P and out[i].min() > 0 and out[i].max() < 1
        assert out[i][out[i] > 0.85].size == side * side
    return out


class Case:
    def __init__(self, R):
        self.R, self.P = R, canvas_of(R)
        self.rows = rows_of(R)
        self.names = [r[0] for r in self.rows]
        self.B = len(self.rows)
        self.rec = pack(self.rows)
        self.idx = np.array(IDX[:self.B] if R != 256 else [4, 1], dtype=np.int32)
        self.src = images(self.P)
        self.src.setflags(write=False)
        self.rec.setflags(write=False)
        assert self.idx.size == self.B and self.idx.max() < N_IMAGES

    def row(self, name):
        return self.names.index(name)

    def params(self):
        """the dictionary `NeuronDataset.batch(idx, params)` takes (torch tensors, angles in degrees)"""
        import torch
        col = lambda k, dt: torch.tensor([r[k] for r in self.rows], dtype=dt)
        return dict(angle=col(1, torch.float32), tx=col(2, torch.float32), ty=col(3, torch.float32), flip=col(4, torch.int32),
                    brightness=col(5, torch.float32), contrast=col(6, torch.float32), contrast_first=col(7, torch.int32))


@functools.lru_cache(maxsize=None)
def case(R):
    return Case(R)


# ---- pass 1 ----------------------------------------------------------------------------------------------------------------------------
def source_coords(q, flip, P, dt, wrong=None):
    """(xs, ys), each (P, P) in dtype dt: the kernel's coordinate expression for one record, every operation in dt (no contraction)"""
    c0 = dt(0.5) * dt(P - 1)
    cosv, sinv, tx, ty = (dt(q[k]) for k in range(4))
    if wrong == "sin_reversed":
        sinv = -sinv
    if wrong == "translation_wrong_sign":
        tx, ty = -tx, -ty
    yo, xo = np.mgrid[0:P, 0:P]
    if flip and wrong != "flip_source_rows":
        yo = P - 1 - yo                                            # RandomVerticalFlip acts on the affine's output
    xo, yo = xo.astype(dt), yo.astype(dt)
    if wrong == "translation_after_rotation":
        xd, yd = xo - c0, yo - c0
        return (cosv * xd + sinv * yd) + c0 - tx, (-sinv * xd + cosv * yd) + c0 - ty
    xd, yd = (xo - c0) - tx, (yo - c0) - ty
    return (cosv * xd + sinv * yd) + c0, (-sinv * xd + cosv * yd) + c0


def gather(im, xi, yi):
    """im[yi, xi], zero outside"""
    P = im.shape[0]
    inside = (xi >= 0) & (xi < P) & (yi >= 0) & (yi < P)
    return np.where(inside, im[np.clip(yi, 0, P - 1), np.clip(xi, 0, P - 1)], f32(0))


def clamp01(v):
    return np.minimum(np.maximum(v, f32(0)), f32(1))


def first_colour(v, q, cfirst):
    """what pass 1 does to a gathered value: brightness, clamped, when it comes first -- exact in numpy fp32"""
    return v if cfirst else clamp01(v * f32(q[4]))


def pass1_definition(src, idx, rec):
    """.cand (B, 4, P, P) fp32 admissible values, .amb (B, P, P) ambiguous pixels, .xs / .ys (B, P, P) fp64 source coordinates"""
    B, P = len(idx), src.shape[-1]
    margin = MARGIN_PER_PIXEL * P
    d = types.SimpleNamespace()
    d.cand, d.amb = np.zeros((B, 4, P, P), dtype=f32), np.zeros((B, P, P), dtype=bool)
    d.xs, d.ys = np.zeros((B, P, P)), np.zeros((B, P, P))
    fl = flags(rec)
    for b in range(B):
        xs, ys = source_coords(rec[b], fl[b, 0], P, f64)
        lo_hi = []
        for s in (xs, ys):
            fs = np.floor(s)
            amb = np.abs(s - (fs + 0.5)) < margin
            near = np.rint(s)
            lo_hi.append((np.where(amb, fs, near).astype(np.int64), np.where(amb, fs + 1, near).astype(np.int64), amb))
        (x0, x1, ax), (y0, y1, ay) = lo_hi
        im = src[idx[b]]
        for k, (xi, yi) in enumerate(((x0, y0), (x1, y0), (x0, y1), (x1, y1))):
            d.cand[b, k] = first_colour(gather(im, xi, yi), rec[b], fl[b, 1])
        d.amb[b], d.xs[b], d.ys[b] = ax | ay, xs, ys
    return d


@functools.lru_cache(maxsize=None)
def definition_of(R):
    c = case(R)
    return pass1_definition(c.src, c.idx, c.rec)


def pass1_violations(canvas, d):
    """per sample: (unambiguous pixels that are not bit-equal to their one value, ambiguous pixels outside their admissible set)"""
    canvas = np.ascontiguousarray(canvas, dtype=f32)
    ok = (canvas.view(np.int32)[:, None] == d.cand.view(np.int32)).any(axis=1)
    return [(int((~ok[b] & ~d.amb[b]).sum()), int((~ok[b] & d.amb[b]).sum())) for b in range(len(canvas))]


# ---- partial sums ----------------------------------------------------------------------------------------------------------------------
def nblk_of(lib, B, P):
    """tiles per canvas from the workspace layout of include/ngan.h: B canvases of P x P floats, then B x nblk partials"""
    floats, rem = divmod(int(lib.ngan_augment_workspace_bytes(B, P)), 4 * B)
    assert rem == 0 and floats > P * P
    return floats - P * P


def tile_pixels(lib):
    """the one tile size T with nblk = ceil(P P / T) at every P the entry point takes a query for"""
    lo, hi = 1, 1 << 40                                            # T in [lo, hi)
    for P in range(1, 2049):
        n = nblk_of(lib, 1, P)
        lo = max(lo, -(-P * P // n))
        if n > 1:
            hi = min(hi, -(-P * P // (n - 1)))
    assert hi == lo + 1, (lo, hi)
    return lo


def tile_sums(canvas, T):
    """fp64 (ref, absref), each (B, nblk): tile t is elements [t T, (t + 1) T) of the row-major canvas"""
    B, n = canvas.shape[0], canvas.shape[1] * canvas.shape[2]
    nblk = -(-n // T)
    flat = np.zeros((B, nblk * T))
    flat[:, :n] = canvas.reshape(B, n)
    t = flat.reshape(B, nblk, T)
    return t.sum(axis=2), np.abs(t).sum(axis=2)


# ---- pass 2 ----------------------------------------------------------------------------------------------------------------------------
def aa_matrix(R, S):
    """(S, R) fp64: aten's antialiased (triangle) down-sampling weights, rows normalised by their own sum"""
    scale = R / S
    W = np.zeros((S, R))
    for i in range(S):
        c = scale * (i + 0.5)
        lo, hi = max(int(c - scale + 0.5), 0), min(int(c + scale + 0.5), R)
        for j in range(lo, hi):
            W[i, j] = max(0.0, 1.0 - abs(j - c + 0.5) / scale)
        W[i] /= W[i].sum()
    return W


def pass2_definition(canvas, rec, R, S):
    """fp64 (ref, absref, absform), each (B, S, S), of the finish pass on the canvas given (the kernel's own, or the emulation's)"""
    canvas = np.asarray(canvas, dtype=f64)
    B, P = canvas.shape[0], canvas.shape[-1]
    crop = R // 4
    fl = flags(rec)
    ref, absref, absform = np.zeros((B, S, S)), np.zeros((B, S, S)), np.zeros((B, S, S))
    Wm = np.eye(R) if S == R else aa_matrix(R, S)
    for b in range(B):
        brightness, contrast = f64(rec[b, 4]), f64(rec[b, 5])
        mean = canvas[b].sum() / (P * P)
        v = canvas[b, crop:crop + R, crop:crop + R]
        a = np.minimum(contrast * v + abs(1.0 - contrast) * mean, 1.0)
        v = np.clip(contrast * v + (1.0 - contrast) * mean, 0.0, 1.0)
        if fl[b, 1]:
            v, a = np.clip(v * brightness, 0.0, 1.0), np.minimum(a * brightness, 1.0)
        col = 2.0 * v - 1.0
        ref[b] = col if S == R else Wm @ col @ Wm.T
        absref[b] = Wm @ np.abs(col) @ Wm.T + abs(1.0 - contrast) * mean
        absform[b] = Wm @ (2.0 * a + 1.0) @ Wm.T
    return ref, absref, absform


def out_ratios(got, definition, R, S):
    """per sample: worst err / bound of the output over the bounds asserted for its class"""
    ref, absref, absform = definition
    r = row_ratios(got, ref, absref, C_ACC[out_class(R, S)])
    if S == R:
        r = [max(x, y) for x, y in zip(r, row_ratios(got, ref, absform, C_ACC["out_full_abs"]))]
    return r


def ratio(got, ref, absref, c_acc):
    """worst err / bound over the elements; 0 / 0 counts as 0 (an all-zero tile), a NaN or x / 0 as infinite"""
    got = np.asarray(got, dtype=f64)
    assert got.shape == ref.shape == absref.shape, (got.shape, ref.shape, absref.shape)
    err, bound = np.abs(got - ref), c_acc * 2.0 ** -24 * absref
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where((err == 0) & (bound == 0), 0.0, err / bound)
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def row_ratios(got, ref, absref, c_acc):
    return [ratio(got[b], ref[b], absref[b], c_acc) for b in range(len(got))]


# ---- the emulation ---------------------------------------------------------------------------------------------------------------------
def fma(a, b, c):
    return (np.asarray(a, dtype=f64) * np.asarray(b, dtype=f64) + np.asarray(c, dtype=f64)).astype(f32)


def butterfly64(v):
    """group_sum<64> along the last axis (64 lanes): v += shfl_xor(v, o) for o = 32 ... 1"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v


WRONGS = ("flip_source_rows", "sin_reversed", "translation_after_rotation", "translation_wrong_sign", "image_b_not_idx",
          "brightness_clamp_omitted", "colour_ops_swapped", "mean_over_crop", "mean_before_brightness", "renormalise_first",
          "crop_off_by_one", "centre_without_half", "window_over_scale2", "last_tile_left_out", "first_64_partials_only")


class Emulator:
    def __init__(self, wrong=None):
        assert wrong is None or wrong in WRONGS, wrong
        self.wrong = wrong

    def cfirst(self, flag):
        return 1 - flag if self.wrong == "colour_ops_swapped" else flag

    def pass1(self, src, idx, rec, T):
        """(canvas (B, P, P), partial (B, nblk)) fp32, and the fp32 source coordinates for the margin statistics"""
        assert T == EMULATED_TILE, T
        B, P, n = len(idx), src.shape[-1], src.shape[-1] ** 2
        nblk = -(-n // T)
        fl = flags(rec)
        canvas, summed = np.zeros((B, P, P), dtype=f32), np.zeros((B, P, P), dtype=f32)
        self.coords = []
        for b in range(B):
            xs, ys = source_coords(rec[b], fl[b, 0], P, f32, self.wrong)
            assert xs.dtype == f32 and ys.dtype == f32
            self.coords.append((xs, ys))
            xi, yi = np.rint(xs).astype(np.int64), np.rint(ys).astype(np.int64)      # nearbyintf: half to even
            if fl[b, 0] and self.wrong == "flip_source_rows":
                yi = P - 1 - yi
            im = src[b % src.shape[0]] if self.wrong == "image_b_not_idx" else src[idx[b]]
            raw = gather(im, xi, yi)
            if self.cfirst(fl[b, 1]):
                v = raw
            else:
                v = raw * f32(rec[b, 4])
                v = v if self.wrong == "brightness_clamp_omitted" else clamp01(v)
            canvas[b], summed[b] = v, raw if self.wrong == "mean_before_brightness" else v
        flat = np.zeros((B, nblk * T), dtype=f32)
        flat[:, :n] = summed.reshape(B, n)
        t = flat.reshape(B, nblk, T // 256, 256)
        s = np.zeros((B, nblk, 256), dtype=f32)
        for k in range(T // 256):
            s = s + t[:, :, k]
        red = butterfly64(s.reshape(B, nblk, 4, 64))[..., 0]
        partial = (red[..., 0] + red[..., 1]) + (red[..., 2] + red[..., 3])
        assert canvas.dtype == f32 and partial.dtype == f32
        return canvas, partial

    def mean(self, canvas_b, partial_b, R):
        P, nblk = canvas_b.shape[-1], partial_b.size
        if self.wrong == "mean_over_crop":
            crop = R // 4
            return f32(canvas_b[crop:crop + R, crop:crop + R].astype(f64).mean())
        use = partial_b[:nblk - 1] if self.wrong == "last_tile_left_out" else partial_b
        s = np.zeros(64, dtype=f32)
        for i0 in range(0, use.size, 64):
            chunk = use[i0:i0 + 64]
            s[:chunk.size] = s[:chunk.size] + chunk
            if self.wrong == "first_64_partials_only":
                break
        return butterfly64(s)[0] / (f32(P) * f32(P))

    def colour(self, v, q, cfirst, mean):
        brightness, contrast = f32(q[4]), f32(q[5])
        if self.wrong == "renormalise_first":
            v = f32(2) * v - f32(1)
        v = clamp01(contrast * v + (f32(1) - contrast) * mean)
        if cfirst:
            v = clamp01(v * brightness)
        return v if self.wrong == "renormalise_first" else f32(2) * v - f32(1)

    def window(self, R, S):
        """per output index: centre, first tap, end of the window, the serial sum of the weights; and inv_scale"""
        scale = f32(R) / f32(S)
        inv = f32(1) / scale
        i = np.arange(S).astype(f32)
        c = scale * i if self.wrong == "centre_without_half" else scale * (i + f32(0.5))
        lo = np.maximum(np.trunc(c - scale + f32(0.5)).astype(np.int64), 0)
        hi = np.minimum(np.trunc(c + scale + f32(0.5)).astype(np.int64), R)
        wsum = np.zeros(S, dtype=f32)
        for t in range(int((hi - lo).max())):
            j = lo + t
            wsum = np.where(j < hi, wsum + self.weight(j, c, inv), wsum)
        return c, lo, hi, wsum, inv

    @staticmethod
    def weight(j, c, inv):
        t = np.abs(((j.astype(f32) - c) + f32(0.5)) * inv)
        return np.where(t < f32(1), f32(1) - t, f32(0)).astype(f32)

    def pass2(self, canvas, partial, rec, R, S):
        canvas = np.ascontiguousarray(canvas, dtype=f32)
        B, P = canvas.shape[0], canvas.shape[-1]
        crop = int(np.rint(f32(0.5) * f32(P - R)))
        if self.wrong == "crop_off_by_one":
            crop -= 1
        fl = flags(rec)
        out = np.zeros((B, S, S), dtype=f32)
        if S != R:
            c, lo, hi, wsum, inv = self.window(R, S)
            taps = int((hi - lo).max())
        for b in range(B):
            mean = self.mean(canvas[b], partial[b], R)
            assert mean.dtype == f32
            col = self.colour(canvas[b, crop:crop + R, crop:crop + R], rec[b], self.cfirst(fl[b, 1]), mean)
            assert col.dtype == f32 and col.shape == (R, R)
            if S == R:
                out[b] = col
                continue
            r = np.zeros((R, S), dtype=f32)                        # r[jy, xo]: the row sums do not depend on yo
            for t in range(taps):
                j = lo + t
                valid = j < hi
                r = np.where(valid[None, :], fma(self.weight(j, c, inv)[None, :], col[:, np.minimum(j, R - 1)], r), r)
            acc = np.zeros((S, S), dtype=f32)
            for t in range(taps):
                j = lo + t
                valid = j < hi
                acc = np.where(valid[:, None], fma(self.weight(j, c, inv)[:, None], r[np.minimum(j, R - 1), :], acc), acc)
            scale = f32(R) / f32(S)
            out[b] = acc / (scale * scale if self.wrong == "window_over_scale2" else wsum[:, None] * wsum[None, :])
        return out


# ---- the named case each wrong emulation must fail on: (wrong, R, S, row, what fails) ---------------------------------------------------
# "pass1": the bit comparison of the canvas; "partials" / "out": that output of the row exceeds its bound.  first_64_partials_only can
# only show where a canvas has more than 64 tiles: R = 256.
WRONG = [
    ("flip_source_rows", 33, 33, "odd_f1_c0", "pass1"),
    ("sin_reversed", 40, 40, "rot90_t", "pass1"),
    ("translation_after_rotation", 64, 64, "rot90_t", "pass1"),
    ("translation_wrong_sign", 4, 4, "t+x", "pass1"),
    ("image_b_not_idx", 3, 3, "identity", "pass1"),
    ("brightness_clamp_omitted", 40, 40, "bright_both_clamps", "pass1"),
    ("colour_ops_swapped", 33, 33, "odd_f0_c1", "pass1"),
    ("mean_over_crop", 33, 11, "odd_f1_c1", "out"),
    ("mean_before_brightness", 40, 8, "odd_f0_c0", "partials"),
    ("mean_before_brightness", 40, 8, "odd_f0_c0", "out"),
    ("renormalise_first", 4, 2, "odd_f1_c0", "out"),
    ("crop_off_by_one", 64, 16, "identity", "out"),
    ("centre_without_half", 33, 3, "identity", "out"),
    ("window_over_scale2", 40, 5, "identity", "out"),
    ("last_tile_left_out", 4, 1, "dim_0.75", "out"),
    ("last_tile_left_out", 33, 33, "odd_f1_c1", "out"),
    ("first_64_partials_only", 256, 4, "odd_f1_c1", "out"),
    ("first_64_partials_only", 256, 256, "rot45_t", "out"),
]
