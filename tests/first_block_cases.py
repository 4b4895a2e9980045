"""The folded critic first block (csrc/first_block.hip: FromImage folded into the block's first 3x3 conv, LeakyReLU and PixelNorm) at
the smallest shapes that reach every special case of its kernels: a replica of the launch plan, case lists, inputs, fp64 references with
their absolute-value twins, the per-element bound and fp32 emulations in the kernels' own summation order.  Shared by
tests/test_gpu_first_block.py (the kernels, through the C ABI, against the references) and tests/test_first_block_bounds_cpu.py (the
emulations against the references: the constants are settled on the CPU, before any kernel is looked at).  `ratio`, `draws` and C_ACC
are those of tests/wide_f32_cases.py.

Bound, per element:   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref + carried,   C_ACC = 8
  absref   the output's own (last-level) sum with absolute values
  n_round  the fp32 roundings applied to the element AFTER its last addition (each relative to |ref|); the rounding of a last
           addition itself counts as one
  carried  the bound of the operands that are themselves computed sums (the folded tables A and Bv in y, rnorm and gx; the pixel sums
           S1 and S0 in the parameter gradients), propagated to first order in fp64 through the output's formula with absolute values.
           It is 0 for an output computed from the inputs alone (tables, S).
A reference is a tuple (ref, absref, n_round, carried); `worst` evaluates err / bound with `ratio` (carried enters as absref +
carried / (C_ACC 2^-24), which is the same bound).

n_round per output, line by line from csrc/first_block.hip:
  tables   first_block_tables_kernel: a = fmaf(w, wf[c], a) over c, then `a * scale`: the product after the chain                   1
           absref scale sum_c |W| |wf| (Bv: |bf|)
  pre      first_block_fwd_kernel, the pre-activation (not an output; its bound e_c is carried into y and rnorm): acc = bias + Bcol[1]
           (+ Bcol[0], + Bcol[2]), then nine f4fma: the last fma is the last addition                                               1
           absref |bias| + sum_{taps inside} (|A| |p| + |Bv|) with the fp64 tables;  carried sum_{taps inside} (e_A |p| + e_Bv)
  y        `acc > 0 ? acc : slope * acc` 1;  `ss / N + eps` reach y through the root, halved: together 1;  sqrtf 1;  `1.0f / r` 1;
           f4scale 1                                                                                                                5
           absref |y| (the N positive squares of ss);  carried m e_c / r + |y| mean_j(|l_j| m_j e_c,j) / r^2  (m the LeakyReLU
           pattern, l = m pre, r = sqrt(mean l^2 + eps): epilogue 1 of tests/conv_fwd_cases.py)
  rnorm    `ss / N + eps` halved by the root: together 1;  sqrtf 1                                                                  2
           absref r;  carried mean_j(|l_j| m_j e_c,j) / r
  S        first_block_sums_kernel + reduce_partials (the reduced S1 / S0 the backward leaves behind its slabs): fma chain over the
           rows of a chunk, DPP scan, four-wave add, slab reduction `s * 1.0f` (exact): the butterfly's last addition               1
           absref sum |gc| |p(x + t)| (S0: sum |gc| over the pixels whose tap t is inside)
  gW       first_block_finish_kernel: `scale * (wf[c] * S1 + bf[c] * S0)` compiles to scale * fma(wf, S1, bf * S0): the product
           with scale after the addition                                                                                            1
           absref scale (|wf| |S1| + |bf| |S0|);  carried scale (|wf| e_S1 + |bf| e_S0)
  gwf gbf  a = fmaf(w, S1[..], a) over every 16th of the N*9 products, group_sum<16>, `a * scale`                                     1
           absref scale sum_{n,t} |W| |S1| (gbf: |S0|);  carried scale sum |W| e_S
  gbc      S0 at the centre tap, copied: S's own bound                                                                              1
  accumulate bit set: the addition of the buffer, one more (tests/stem_head_cases.py `plus`); gwf / gbf accumulate with one
           fma(a, scale, old), which is within the same count
  gx       first_block_dx_kernel: three f4dot per kx, `s += d1 + d2 + d3`, group_sum<Q>: the butterfly's last addition; the
           pooled store's 0.25f * s is exact                                                                                        1
           absref sum_{n,t} |A| |gc(x - t)|;  carried sum e_A |gc(x - t)|
LeakyReLU masks are those of the stored output, with a condition, not a tolerance: wherever the fp64 pre-activation has |pre| > e_c
the stored sign must be the fp64 sign (sign_violations).  The inputs leave far fewer than 1e-2 of a case's elements inside
|pre| <= e_c (tests/test_first_block_bounds_cpu.py asserts the cap on the reference alone).

Emulations (numpy fp32, fma as one rounding of the fp64 product-sum), in the order the compiled kernels take -- where the source
leaves the contraction to the compiler (f4dot, the finish kernel's expressions) the order is the one the gfx950 code object has:
  tables_emulate  sequential fma over c, then * scale
  fwd_emulate     Bcol[ky] = ((0 + Bv[ky][0] if x > 0) + Bv[ky][1]) + Bv[ky][2] if x < W - 1;  acc = bias + Bcol[1], + Bcol[0] below
                  the first image row, + Bcol[2] above the last;  the fmas kx-outer, ky-inner;  f4dot(acc, acc) as four rounded squares
                  added in order, ((x^2 + y^2) + z^2) + w^2;  butterfly over the Q lanes of a pixel
  sums_emulate    per thread the rows of its chunk in order (S1 fma, S0 add; padding rows and lanes add 0, which is exact), the column
                  masks, the Hillis-Steele scan of row_tail_sum over the PW pixels of a DPP row segment (shifts 1, 2, 4 and for
                  PW = 16 also 8, zeros shifted in), (w0 + w1) + (w2 + w3) over the four waves, then reduce_partials: lane l adds slabs
                  l, l + 64, ... into four accumulators while four fit and the rest into the first, (s0 + s1) + (s2 + s3), 64-lane
                  butterfly
  finish_emulate  as listed under gW / gwf above; the 16-lane butterfly
  dx_emulate      f4dot(a, b) = fma(a.w, b.w, fma(a.z, b.z, fma(a.x, b.x, a.y b.y)));  per lane the three f4dot of a kx as
                  (d1 + d2) + d3 added to s (0 + first exactly), butterfly over Q, 0.25 s
Each emulation takes `defect=`: one of DEFECTS, a planted mistake that tests/test_first_block_bounds_cpu.py shows to be caught.

RAISED lists the outputs whose emulated worst err / bound exceeds 0.5 with C_ACC = 8, with the next power of two that brings it to 0.5
or below and the emulated ratio at that constant; tests/test_first_block_bounds_cpu.py pins both.  One entry: the folded tables, whose
raised constant reaches y, rnorm and gx through the carried term only."""
import functools

import numpy as np

import wide_f32_cases as W
from wide_f32_cases import C_ACC, draws, ratio  # noqa: F401  (re-exported)

f32, f64 = np.float32, np.float64
SLOPE, EPS = W.SLOPE, W.EPS
U23, U24 = 2.0 ** -23, 2.0 ** -24
FB_ROWS, FB_MAX_C, MAX_SLABS = 8, 64, 1024
NGAN_ERR_SHAPE = -2
# output name -> (raised C_ACC, emulated worst err / bound at that constant)
RAISED = {
    # 0.526 with C_ACC = 8 at C = 16 (N = 32: 576 table entries to find the worst among): a 16-term sum whose leading terms cancel, so
    # that one rounding of a partial sum is a large share of absref; C = 20 and 64 stay below 0.5
    "tables": (16.0, 0.291),
}
DEFECTS = ("bv_left", "bv_right", "row_mask_chunk", "no_reprime", "pad_lanes", "tail_pw8", "dx_noflip", "dx_pool_no_quarter",
           "gbc_tap", "acc_bits_swapped", "scale_twice", "skip_c16")


def c_acc(name):
    return float(RAISED.get(name, (C_ACC, None))[0])


def seed_of(tag, *shape):
    s = tag
    for v in shape:
        s = (s * 131 + int(v)) % (2 ** 31 - 1)
    return s


def worst(got, entry, name):
    """worst err / bound of one output; nan where an element was left unwritten (NaN)"""
    ref, absref, n_round, carried = entry
    c = c_acc(name)
    return ratio(got, ref, absref + carried / (c * U24), n_round, c)


def plus(entry, buf):
    """reference of an accumulating form that starts from `buf`: one more rounding, the addition"""
    r, a, n, e = entry
    return r + buf.astype(f64), a + np.abs(buf.astype(f64)), n + 1, e


# ---- the launch plan (fb_plan of csrc/first_block.hip; checked against ngan_first_block_plan in tests/test_first_block_bounds_cpu.py) ----
def _cd(a, b):
    return -(-a // b)


def shape_ok(B, H, Wd, C, N):
    return (B > 0 and H > 0 and Wd > 0 and 0 < C <= FB_MAX_C and N in (16, 32) and B * _cd(H, FB_ROWS) < 65536
            and B * H * Wd * N < 2 ** 31)


def plan(B, H, Wd, C, N):
    """(grid.x, R, nchunk, slabs), or None where the library refuses the shape"""
    if not shape_ok(B, H, Wd, C, N):
        return None
    gx = _cd(Wd * (N // 4), 256)
    R = FB_ROWS
    while gx * B * _cd(H, R) > MAX_SLABS and _cd(H, R) > 1:
        R *= 2
    nchunk = _cd(H, R)
    slabs = gx * B * nchunk
    return (gx, R, nchunk, slabs) if slabs <= MAX_SLABS else None


# the shapes at which the unbounded doubling of R could not end (gx * B > 1024), smallest last
HANGING = [(65, 8, 1024, 16, 16), (33, 1024, 1024, 16, 32), (1025, 1, 1, 16, 16)]
SMALLEST_REFUSED = (1025, 1, 1)        # B, H, W: 1025 slabs of one pixel each


# ---- case lists: (B, H, W, C, N) ---------------------------------------------------------------------------------------------------------
def span(N):
    """pixels of a row per workgroup: 256 threads / Q lanes per pixel (forward, dx) = 4 waves x PW (sums)"""
    return 1024 // N


NS = (16, 32)
HS = (1, 2, 7, 8, 9, 17)            # one-row images, a full chunk, a halo row owned by the neighbouring chunk on either side
CS = (1, 16, 20, 64)                # 20: the `c < C` guard of the finish kernel's second 16-channel pass; 64: FB_MAX_C


def widths(N):
    """1: both column masks on one pixel; the workgroup span - 1, the span, the span + 1 (a second x-block whose padding lanes share
    a DPP row with live ones)"""
    return (1, 2, 3, span(N) - 1, span(N), span(N) + 1)


# every W x H edge pair for both N; B and C cycle through their sets so that each value meets each edge
EDGE = [((1, 3)[(iw + ih) % 2], H, Wd, CS[(iw + 2 * ih) % 4], N)
        for N in NS for iw, Wd in enumerate(widths(N)) for ih, H in enumerate(HS)]
CHANNELS = [(B, 9, span(N) + 1, C, N) for N in NS for C in CS for B in (1, 3)]
FULL = EDGE + CHANNELS
NULL_SHAPES = [(3, 9, span(N) + 1, 20, N) for N in NS]
NULLS = ("bf", "bc", "gbf", "gbc")
# (accumulate mask, gbf null, gb_conv null): none, each bit alone, all, and bits set for outputs passed as null
ACCUMULATE = [(0, False, False), (1, False, False), (2, False, False), (4, False, False), (8, False, False), (15, False, False),
              (15, True, True), (4, True, False), (8, False, True)]
# the sums plan: R = 8 with exactly 1024 slabs, R = 16, R = 32, two x-blocks together with R = 16
PLAN_CASES = [(1, 8192, 1, 16, 16), (1, 8200, 1, 16, 32), (5, 3300, 3, 16, 16), (1, 4104, 33, 16, 32)]
PLAN_EXPECT = {(1, 8192, 1, 16, 16): (1, 8, 1024, 1024), (1, 8200, 1, 16, 32): (1, 16, 513, 513),
               (5, 3300, 3, 16, 16): (1, 32, 104, 520), (1, 4104, 33, 16, 32): (2, 16, 257, 514)}


def scale_of(C):
    """the equalised-learning-rate scale of a 3x3 conv over C channels, as the C ABI passes it: rounded to fp32"""
    return float(f32(1.3868 / np.sqrt(9 * C)))


@functools.lru_cache(maxsize=4)
def inputs(B, H, Wd, C, N):
    """p (B, H, W) image, standard normal: non-zero on every border pixel;  w (N, C, 3, 3), wf, bf (C): no symmetry between taps or
    channels, bf of the size of wf * p;  bc (N);  gc (B, H, W, N);  buffers of the size of the gradient they are added to"""
    d = draws(seed_of(41, B, H, Wd, C, N), p=(B, H, Wd), w=(N, C, 3, 3), wf=(C,), bf=(C,), bc=(N,), gc=(B, H, Wd, N),
              bufW=(N, C, 3, 3), bufwf=(C,), bufbf=(C,), bufbc=(N,))
    sc, npix = scale_of(C), B * H * Wd
    d["bc"] = (d["bc"] * f32(0.3)).astype(f32)
    d["bufW"] = (d["bufW"] * f32(sc * np.sqrt(npix))).astype(f32)
    d["bufwf"] = (d["bufwf"] * f32(sc * np.sqrt(9.0 * N * npix))).astype(f32)
    d["bufbf"] = (d["bufbf"] * f32(sc * np.sqrt(9.0 * N * npix))).astype(f32)
    d["bufbc"] = (d["bufbc"] * f32(np.sqrt(npix))).astype(f32)
    d["scale"] = sc
    return d


# ---- fp64 references -----------------------------------------------------------------------------------------------------------------
def _padded(a, rows=0):
    """zero border of one pixel around axes 1 and 2 (and `rows` more rows below)"""
    out = np.zeros((a.shape[0], a.shape[1] + 2 + rows, a.shape[2] + 2) + a.shape[3:], a.dtype)
    out[:, 1:a.shape[1] + 1, 1:a.shape[2] + 1] = a
    return out


def _e(entry, name):
    ref, absref, n_round, carried = entry
    return n_round * U23 * np.abs(ref) + c_acc(name) * U24 * absref + carried


def tables_ref(w, wf, bf, scale):
    """{"tables": (2, 9, N)}: A then Bv"""
    N, C = w.shape[:2]
    w9 = w.astype(f64).reshape(N, C, 9)
    b64 = bf.astype(f64) if bf is not None else np.zeros(C)
    ref = scale * np.stack([np.einsum("nct,c->tn", w9, wf.astype(f64)), np.einsum("nct,c->tn", w9, b64)])
    absref = scale * np.stack([np.einsum("nct,c->tn", np.abs(w9), np.abs(wf.astype(f64))), np.einsum("nct,c->tn", np.abs(w9), np.abs(b64))])
    return {"tables": (ref, absref, 1, 0.0)}


def pre_ref(p, w, wf, bf, bc, scale):
    """(pre, e_c): the fp64 pre-activation (B, H, W, N) and its bound"""
    B, H, Wd = p.shape
    tab = tables_ref(w, wf, bf, scale)["tables"]
    (A, Bv), (eA, eB) = tab[0], _e(tab, "tables")
    Pz, Iz = _padded(p.astype(f64)), _padded(np.ones(p.shape))
    b64 = bc.astype(f64) if bc is not None else np.zeros(A.shape[1])
    pre = np.zeros(p.shape + (A.shape[1],)) + b64
    absref, carried = np.zeros_like(pre) + np.abs(b64), np.zeros_like(pre)
    for t in range(9):
        ky, kx = divmod(t, 3)
        pv, iv = Pz[:, ky:ky + H, kx:kx + Wd, None], Iz[:, ky:ky + H, kx:kx + Wd, None]
        pre += pv * A[t] + iv * Bv[t]
        absref += np.abs(pv) * np.abs(A[t]) + iv * np.abs(Bv[t])
        carried += np.abs(pv) * eA[t] + iv * eB[t]
    return pre, _e((pre, absref, 1, carried), "pre")


def fwd_ref(p, w, wf, bf, bc, scale, y_stored):
    """{"y", "rnorm"} and "_pre": (pre, e_c); the LeakyReLU pattern is the stored output's"""
    pre, e_c = pre_ref(p, w, wf, bf, bc, scale)
    m = W.mask_of(y_stored)
    l, e_l = m * pre, m * e_c
    r = np.sqrt((l * l).mean(-1, keepdims=True) + EPS)
    y = l / r
    dr = (np.abs(l) * e_l).mean(-1, keepdims=True) / r
    return {"y": (y, np.abs(y), 5, e_l / r + np.abs(y) * dr / r), "rnorm": (r[..., 0], r[..., 0], 2, dr[..., 0]), "_pre": (pre, e_c)}


def sign_violations(pre, e_c, y_stored):
    """elements whose fp64 pre-activation is outside |pre| <= e_c and whose stored sign is not the fp64 sign"""
    return int(((np.abs(pre) > e_c) & ((np.asarray(y_stored) > 0) != (pre > 0))).sum())


def undecided_fraction(pre, e_c):
    return float((np.abs(pre) <= e_c).mean())


def sums_ref(p, gc):
    """{"S": (2, 9, N)}: S1 then S0"""
    B, H, Wd = p.shape
    g = gc.astype(f64)
    Pz, Iz = _padded(p.astype(f64)), _padded(np.ones(p.shape))
    ref, absref = np.zeros((2, 9, gc.shape[-1])), np.zeros((2, 9, gc.shape[-1]))
    for t in range(9):
        ky, kx = divmod(t, 3)
        pv, iv = Pz[:, ky:ky + H, kx:kx + Wd], Iz[:, ky:ky + H, kx:kx + Wd]
        ref[0, t], ref[1, t] = np.einsum("bhwn,bhw->n", g, pv), np.einsum("bhwn,bhw->n", g, iv)
        absref[0, t], absref[1, t] = np.einsum("bhwn,bhw->n", np.abs(g), np.abs(pv)), np.einsum("bhwn,bhw->n", np.abs(g), iv)
    return {"S": (ref, absref, 1, 0.0)}


def bwd_ref(p, gc, w, wf, bf, scale):
    """{"S", "gW", "gwf", "gbf", "gbc"}: written forms; an accumulating form is plus(entry, buffer)"""
    N, C = w.shape[:2]
    S = sums_ref(p, gc)["S"]
    (S1, S0), (a1, a0), (e1, e0) = S[0], S[1], _e(S, "S")
    w9, wf64 = w.astype(f64).reshape(N, C, 9), wf.astype(f64)
    b64 = bf.astype(f64) if bf is not None else np.zeros(C)
    out = {"S": S}
    nct = lambda v, s: v[None, :, None] * s.T[:, None, :]          # (C,), (9, N) -> (N, C, 9)
    out["gW"] = ((scale * (nct(wf64, S1) + nct(b64, S0))).reshape(w.shape),
                 (scale * (nct(np.abs(wf64), np.abs(S1)) + nct(np.abs(b64), np.abs(S0)))).reshape(w.shape), 1,
                 (scale * (nct(np.abs(wf64), e1) + nct(np.abs(b64), e0))).reshape(w.shape))
    for name, s, e in (("gwf", S1, e1), ("gbf", S0, e0)):
        out[name] = (scale * np.einsum("nct,tn->c", w9, s), scale * np.einsum("nct,tn->c", np.abs(w9), np.abs(s)), 1,
                     scale * np.einsum("nct,tn->c", np.abs(w9), e))
    out["gbc"] = (S0[4], a0[4], 1, 0.0)
    return out


def dx_ref(gc, w, wf, scale, pool):
    """{"gx"}: (B, H, W), or the (B, 2H, 2W) image of four copies of 0.25 s"""
    B, H, Wd, N = gc.shape
    tab = tables_ref(w, wf, None, scale)["tables"]
    A, eA = tab[0][0], _e(tab, "tables")[0]
    Gz = _padded(gc.astype(f64))
    ref, absref, carried = np.zeros((B, H, Wd)), np.zeros((B, H, Wd)), np.zeros((B, H, Wd))
    for t in range(9):
        ky, kx = divmod(t, 3)
        gv = Gz[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + Wd]
        ref += gv @ A[t]
        absref += np.abs(gv) @ np.abs(A[t])
        carried += np.abs(gv) @ eA[t]
    if pool:
        up = lambda v: 0.25 * v.repeat(2, axis=1).repeat(2, axis=2)
        ref, absref, carried = up(ref), up(absref), up(carried)
    return {"gx": (ref, absref, 1, carried)}


# ---- fp32 emulations -------------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _butterfly(v, width):
    """group_sum<width> over the last axis"""
    idx = np.arange(width)
    o = width // 2
    while o:
        v = v + v[..., idx ^ o]
        o //= 2
    return v[..., 0]


def _f4dot(a, b):
    """f4dot as compiled: fma(a.w, b.w, fma(a.z, b.z, fma(a.x, b.x, a.y * b.y))); the last axis holds x, y, z, w"""
    t = a[..., 1] * b[..., 1]
    t = _fma(a[..., 0], b[..., 0], t)
    t = _fma(a[..., 2], b[..., 2], t)
    return _fma(a[..., 3], b[..., 3], t)


def tables_emulate(w, wf, bf, scale):
    N, C = w.shape[:2]
    w9 = w.reshape(N, C, 9)
    a, b = np.zeros((N, 9), f32), np.zeros((N, 9), f32)
    for c in range(C):
        a = _fma(w9[:, c], wf[c], a)
        b = _fma(w9[:, c], bf[c] if bf is not None else f32(0), b)
    return {"tables": np.stack([a.T, b.T]) * f32(scale)}


def fwd_emulate(p, tables, bc, defect=None):
    """first_block_fwd_kernel on the fp32 tables (2, 9, N): {"y", "rnorm"}"""
    B, H, Wd = p.shape
    A, Bv = tables
    N = A.shape[1]
    Q = N // 4
    x, yy = np.arange(Wd), np.arange(H)
    mx0 = (x > 0) | (defect == "bv_left")
    mx2 = (x < Wd - 1) | (defect == "bv_right")
    Bcol = []
    for ky in range(3):
        t = np.where(mx0[:, None], Bv[3 * ky][None], f32(0))
        t = t + Bv[3 * ky + 1][None]
        Bcol.append(np.where(mx2[:, None], t + Bv[3 * ky + 2][None], t))              # (W, N)
    bias = bc if bc is not None else np.zeros(N, f32)
    top = (yy % FB_ROWS != 0) if defect == "row_mask_chunk" else (yy > 0)
    acc = np.broadcast_to(bias[None] + Bcol[1], (H, Wd, N))
    acc = np.where(top[:, None, None], acc + Bcol[0][None], acc)
    acc = np.where((yy < H - 1)[:, None, None], acc + Bcol[2][None], acc)
    acc = np.broadcast_to(acc[None], (B, H, Wd, N)).astype(f32)
    Pz = _padded(p)
    for kx in range(3):
        for ky in range(3):
            pv = Pz[:, ky:ky + H, kx:kx + Wd]
            if defect == "no_reprime" and ky == 0:
                pv = pv * (yy % FB_ROWS != 0)[None, :, None].astype(f32)
            acc = _fma(A[3 * ky + kx], pv[..., None], acc)
    acc = np.where(acc > 0, acc, f32(SLOPE) * acc).astype(f32)
    a4 = acc.reshape(B, H, Wd, Q, 4)
    sq = a4 * a4                                             # the squares are rounded on their own here (two packed multiplies)
    ss = _butterfly(((sq[..., 0] + sq[..., 1]) + sq[..., 2]) + sq[..., 3], Q)
    r = np.sqrt(ss / f32(N) + f32(EPS)).astype(f32)
    return {"y": acc * (f32(1) / r)[..., None], "rnorm": r}


def reduce_partials_emulate(parts):
    """reduce_partials_kernel with scale 1: parts (nparts, M) -> (M,)"""
    nparts, M = parts.shape
    acc = np.zeros((4, 64, M), f32)
    for lane in range(64):
        j = lane
        while j + 192 < nparts:
            for u in range(4):
                acc[u, lane] = acc[u, lane] + parts[j + 64 * u]
            j += 256
        while j < nparts:
            acc[0, lane] = acc[0, lane] + parts[j]
            j += 64
    s = (acc[0] + acc[1]) + (acc[2] + acc[3])
    return _butterfly(np.ascontiguousarray(s.T), 64)


def sums_emulate(p, gc, defect=None):
    """first_block_sums_kernel + reduce_partials: {"S": (2, 9, N)}, the chunks of R rows side by side"""
    B, H, Wd = p.shape
    N = gc.shape[-1]
    gx, R, nchunk, slabs = plan(B, H, Wd, 1, N)
    Q = N // 4
    PW = 64 // Q
    wpad, hp = gx * 4 * PW, nchunk * R
    xs = np.minimum(np.arange(wpad), Wd - 1)              # the padding lanes are clamped to the last column
    Pz = _padded(p, hp - H)
    G = np.zeros((B, hp, wpad, N), f32)
    G[:, :H, :Wd] = gc
    if defect == "pad_lanes":
        G[:, :H, Wd:] = gc[:, :, Wd - 1:Wd]
    G = G.reshape(B, nchunk, R, wpad, N)
    y0 = np.arange(nchunk) * R
    s1 = [np.zeros((B, nchunk, wpad, N), f32) for _ in range(9)]
    r0 = [np.zeros((B, nchunk, wpad, N), f32) for _ in range(3)]
    for r in range(R):
        yy, g = y0 + r, G[:, :, r]
        for ky in range(3):
            rows = Pz[:, yy + ky]                          # (B, nchunk, W + 2): image row yy + ky - 1
            if defect == "no_reprime" and r == 0 and ky == 0:
                rows = np.zeros_like(rows)
            for kx in range(3):
                s1[3 * ky + kx] = _fma(g, rows[:, :, xs + kx, None], s1[3 * ky + kx])
        top = np.full(nchunk, r > 0) if defect == "row_mask_chunk" else yy > 0
        r0[1] = r0[1] + g
        r0[0] = np.where(top[None, :, None, None], r0[0] + g, r0[0])
        r0[2] = np.where((yy < H - 1)[None, :, None, None], r0[2] + g, r0[2])
    mx = (xs > 0, np.ones(wpad, bool), xs < Wd - 1)
    v = np.stack(s1 + [np.where(mx[kx][:, None], r0[ky], f32(0)) for ky in range(3) for kx in range(3)])
    v = v.reshape(18, B, nchunk, gx, 4, PW, N)
    for s in (1, 2, 4, 8)[:3 if PW == 8 else 4]:          # row_tail_sum<PW>: the last lane of the segment holds the total
        sh = np.zeros_like(v)
        sh[..., s:, :] = v[..., :-s, :]
        v = v + sh
    tot = v[..., PW - 1, :]                                # (18, B, nchunk, gx, 4 waves, N)
    if defect == "tail_pw8" and PW == 8:                   # row_shr:8 as well: the odd channel quad's total takes the even one's
        t4 = tot.reshape(tot.shape[:-1] + (Q, 4)).copy()
        t4[..., 1::2, :] = t4[..., 1::2, :] + t4[..., 0::2, :]
        tot = t4.reshape(tot.shape)
    slab = (tot[..., 0, :] + tot[..., 1, :]) + (tot[..., 2, :] + tot[..., 3, :])       # (18, B, nchunk, gx, N)
    parts = np.ascontiguousarray(slab.transpose(1, 2, 3, 0, 4)).reshape(slabs, 18 * N)
    return {"S": reduce_partials_emulate(parts).reshape(2, 9, N)}


def finish_emulate(S, w, wf, bf, scale, start, mask, defect=None):
    """first_block_finish_kernel.  start: {"gW", "gwf", "gbf", "gbc"} initial buffers (None: a null pointer); an output whose bit is
    clear is overwritten; returns the same keys (None for a null output; NaN where the kernel would leave an element unwritten)"""
    N, C = w.shape[:2]
    S1, S0 = S
    sc = f32(scale)
    if defect == "acc_bits_swapped":
        mask = (mask & ~6) | ((mask & 2) << 1) | ((mask & 4) >> 1)
    bfv = bf if bf is not None else np.zeros(C, f32)
    t = bfv[None, :, None] * S0.T[:, None, :]
    v = (sc * _fma(wf[None, :, None], S1.T[:, None, :], t)).reshape(w.shape)
    out = {"gW": start["gW"] + v if mask & 1 else v}
    wflat = np.ascontiguousarray(w.transpose(1, 0, 2, 3)).reshape(C, N * 9)
    for name, s, bit in (("gwf", S1, 2), ("gbf", S0, 4)):
        if start.get(name) is None:
            out[name] = None
            continue
        sflat = np.ascontiguousarray(s.T).reshape(N * 9)
        a = np.zeros((C, 16), f32)
        for i in range(N * 9 // 16):
            idx = 16 * i + np.arange(16)
            a = _fma(wflat[:, idx], sflat[idx][None], a)
        a = _butterfly(a, 16)
        if defect == "scale_twice" and name == "gwf":
            a = a * sc
        res = _fma(a, sc, start[name]) if mask & bit else a * sc
        if defect == "skip_c16":
            res = np.where(np.arange(C) < 16, res, start[name] if mask & bit else f32(np.nan)).astype(f32)
        out[name] = res
    tap = 3 if defect == "gbc_tap" else 4
    out["gbc"] = None if start.get("gbc") is None else (start["gbc"] + S0[tap] if mask & 8 else S0[tap].copy())
    return out


def dx_emulate(gc, tables, pool, defect=None):
    """first_block_dx_kernel on the fp32 tables: {"gx"}"""
    B, H, Wd, N = gc.shape
    Q = N // 4
    A4 = tables[0].reshape(9, Q, 4)
    Gz = _padded(gc).reshape(B, H + 2, Wd + 2, Q, 4)
    yy = np.arange(H)
    s = None
    for kx in range(3):
        d = []
        for ky in range(3):
            col = kx if defect == "dx_noflip" else 2 - kx
            gv = Gz[:, 2 - ky:2 - ky + H, col:col + Wd]
            if defect == "no_reprime" and ky == 2:
                gv = gv * (yy % FB_ROWS != 0)[None, :, None, None, None].astype(f32)
            d.append(_f4dot(A4[3 * ky + kx][None, None, None], gv))
        grp = (d[0] + d[1]) + d[2]
        s = grp if s is None else s + grp
    s = _butterfly(s, Q)
    if pool:
        q4 = s if defect == "dx_pool_no_quarter" else f32(0.25) * s
        return {"gx": q4.repeat(2, axis=1).repeat(2, axis=2)}
    return {"gx": s}
