"""The 3x3 weight-gradient kernels and the slab reductions behind them (csrc/conv3x3_wgrad.hip) at every template instance and every
edge of their tiling: the case list, fp64 references with their absolute-value twins, the per-element bound and numpy emulations in
the kernels' own order.  Shared by tests/test_gpu_wgrad.py (the kernels against the references) and tests/test_wgrad_bounds_cpu.py
(the emulations against the references: the constants are settled on the CPU, before any kernel is looked at; the plan replica below
is checked against the built library there).  Nothing of the package is imported here.

A case is (B, H, W, Cin, Cout, resample); H, W are those of the output gradient g (B, H, W, Cout); the input x is (B, H, W, Cin) for
resample 0, (B, 2H, 2W, Cin) for 1 (2x2 average on load) and (B, H/2, W/2, Cin) for 2 (bilinear x2 on load).  Every case runs at the
three precision codes: 0 (fp32, Winograd form), 1 (split-bf16 arithmetic on fp32 tensors), 5 (bf16 tensors, plain bf16 products).

Instances.  launch_wgrad picks (COT, CIT) = (co_s, ci_s) / 16 from the plan, the tile width TW (16 for W <= 16, else 32), the
resample code, and the XF staging form (resample 0, TW = 32, W % 32 == 0).  EXPECTED_NAMES is that product written out: 4 slice
shapes x (3 resample codes x 2 tile widths + XF) x 3 kernel families = 84.

Bound, per element:   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref (+ 2^-15 absref for the split-bf16 form),   C_ACC = 8
  absref, direct forms (precision 1 and 5)   |scale| sum_pixels |g| |resample(x)|: the fp64 reference's own sum with absolute values
  absref, fp32 Winograd form                 the error of that form is not relative to the direct sum but to the magnitudes that its
             transformed operands reach: |scale| |G|^T [ sum_tiles (|A| |dY| |A|^T) . (|B|^T |d| |B|) ] |G| over the kernel's 2x2 output
             tiles (even coordinates, zeros outside the image), with the entries of A, B, G replaced by their absolute values
  n_round    the fp32 roundings applied to an element after its last addition, the rounding of that addition counting as one:
             direct path (wgrad_reduce_kernel)   written: s * scale                                                           1
                                                 accumulated: fmaf(s, scale, *o), the product's share and the addition          2
             deferred path (wgrad_reduce_many_kernel)   total = fma(t, scale[s], total) per source: with one source that is
                                                 round(t * scale), with several the last fma is the last addition (the earlier
                                                 ones round partial totals, which absref bounds: accumulation term); written    1
                                                 accumulated: *o + total, one more                                             2
  split-bf16 term   hi = rne_bf16(v), lo = rne_bf16(v - hi) (v - hi is exact in fp32).  bf16 has an 8-bit significand: for v = m 2^e,
             1 <= m < 2, |lo| <= |v - hi| <= 2^-8 2^e (half an ulp of hi); lo then lies below 2^(e-8), where an ulp is at most 2^(e-16), so the
             residual |v - hi - lo| <= 2^-17 2^e.  The kernel adds lo.hi + hi.lo + hi.hi, exact products; against g x it lacks lo.lo
             (<= 2^-16 |g x|) and the two residual cross terms (<= 2^-17 |g x| each; second order dropped): 2^-15 per product, a power
             of two already, and attained in the limit m -> 1 -- so SPLIT_TERM = 2^-15 of the direct absref, not the 2^-16 that a count
             with a 9-bit significand (|lo| <= 2^-9 |v|) would give: the emulation of the 1 x 1 image, one product per element, reaches
             1.05 of that.  Being a deterministic, attainable worst case and not a summation-order effect, this term cannot be held
             to "half the bound": tests/test_wgrad_bounds_cpu.py settles the two parts apart.  Part A: the emulation against
             split_reference() -- the fp64 sum of the three products the kernel forms -- within n_round 2^-23 |ref| + C_ACC 2^-24 absref at
             <= 0.5.  Part B: split_reference() against the fp64 reference within (SPLIT_TERM + C_ACC / 2 2^-24) absref (the second term: the fp32
             roundings of a resampled input's blend, half the accumulation term) at <= 1.  A at 0.5 plus B is the whole bound.  A truncating split has |lo| < 2^-7 2^e and lacks up
             to 2^-14 |g x|: it misses the bound on the smallest images.  In bf16 storage (precision 5) the operands are bf16 values,
             the products are exact and no such term applies; a resampled input is blended in fp32 and rounded to bf16 once, and the
             reference rounds its fp64 blend once in the same way.
Nothing here was fitted to a kernel's result.

Emulations (numpy, fp32 where the kernel is fp32).  Tiles per workgroup wx: t = wx, wx + nwx, ... in that order.  fp32 Winograd
form: the transforms B^T d B and A dY A^T in the kernel's operation order with its sign trick (A's last row without the minus; the
back-transform negates the positions u = 3 xor v = 3); a wave step contracts four Winograd tiles per MFMA (lane quarter q, tile
4 q + j of a row of 16; with 16-pixel tiles q selects the row pair and the half row), j = 0..3 in order; the four products of an MFMA
are summed exactly and rounded once ("exact") or one fma after the other ("seq") -- the rounding inside v_mfma_f32_16x16x4_f32 is not
documented, both are held to the bound; per row-group wave the back-transform G^T [.] G in the kernel's order, then the waves summed
in index order.  bf16 forms: a k-step is 32 pixels (one row of a 32-wide tile, two of a 16-wide one); per k-step and tap the MFMAs
lo.hi, hi.lo, hi.hi (plain bf16: hi.hi alone), each summed exactly and rounded once into the wave's accumulator (the 32 products of
v_mfma_f32_16x16x32_bf16 are exact in fp32 and their sum is formed in fp64 here: the "exact" form only); the k-steps split over the
row-group waves, which are summed in index order.  The numerics of an element do not depend on which slice or wave owns it, only on
the number of row groups, so the emulations run all channels at once (or a prefix of the output channels: `co_limit`, used for the
128-channel cases, whose elements are computed independently of one another).  Then the slabs go through wgrad_reduce_kernel (16
part-lanes, four accumulators per lane with a 16-stride tail, (a0 + a1) + (a2 + a3), the lanes in order) or wgrad_reduce_many_kernel
(NG groups from the largest nparts, eight accumulators with an NG-stride tail, folded 4 + 4, (a0 + a1) + (a2 + a3), the groups in order,
fma per source).

Wrong variants (`defect=`), each of which tests/test_wgrad_bounds_cpu.py shows to miss the bound: "halo" (the left halo column of the
last tile dropped), "slab_twice", "slab_skipped", "swap" ((co_l, ci_l) transposed in the second slice), "no_lohi" (the lo.hi product
dropped), "trunc" (a truncating instead of a rounding bf16 split).

RAISED: (form, output) whose emulated worst err / bound exceeds 0.5 with C_ACC = 8, with the next power of two that brings it to 0.5
or below and the emulated ratio there; tests/test_wgrad_bounds_cpu.py pins it.  It is empty: no form needed a raise."""
import functools
import struct

import numpy as np
import torch

import fp64_conv

f32, f64 = np.float32, np.float64
C_ACC = 8.0
SPLIT_TERM = 2.0 ** -15
SCALE = 0.0417
PRECISIONS = (0, 1, 5)
FORM = {0: "f32_winograd", 1: "bf16x3", 5: "bf16"}
# (form, output) -> (raised C_ACC, emulated worst err / bound at that constant)
RAISED = {}


def c_acc(form, output="gw"):
    return float(RAISED.get((form, output), (C_ACC, None))[0])


# ---- the case list ------------------------------------------------------------------------------------------------------------------
# Channel pairs (Cin, Cout) by the slice shape (COT, CIT) they give.  (16,16) (1,1), (64,64) (2,2), (16,64) (2,1) and (64,16) (1,2) give
# the same shape at every precision and tile width; the small rule of precision 0 (32-wide tiles, both sides <= 32 channels: 16 x 16
# slices) acts on (32,32), (16,32), (32,16).
NARROW = [   # TW = 16: W in {1, 12, 16} (ragged right column), H in {1, 18} (ragged bottom row, two tile rows)
    (1, 1, 1, 16, 16, 0), (2, 18, 12, 64, 64, 0), (2, 18, 16, 16, 64, 0), (3, 1, 16, 64, 16, 0),
    (2, 18, 16, 32, 32, 0),          # 32 -> 32 at W = 16: no small rule, one 32 x 32 slice at precision 0
    (1, 18, 12, 32, 16, 0), (1, 18, 1, 16, 32, 0),
    (2, 18, 12, 16, 16, 1), (1, 1, 16, 64, 64, 1), (2, 8, 12, 16, 64, 1), (1, 18, 16, 64, 16, 1),
    (2, 2, 2, 16, 16, 2), (1, 18, 12, 64, 64, 2), (2, 2, 16, 16, 64, 2), (1, 18, 2, 64, 16, 2),       # H = 2 / W = 2: every tap clamped
]
WIDE = [     # TW = 32, generic staging: W in {17, 40}; H in {1, 8, 12, 20}: top-only tile, exact tile, ragged bottom; B >= 2
    (2, 1, 17, 16, 16, 0), (2, 12, 40, 64, 64, 0), (2, 8, 17, 16, 64, 0), (2, 20, 40, 64, 16, 0),
    (2, 12, 17, 32, 32, 0),          # 32 -> 32 at W = 17: the small rule, four 16 x 16 slices at precision 0
    (2, 8, 40, 16, 32, 0), (2, 12, 40, 32, 16, 0), (2, 20, 17, 48, 32, 0), (2, 12, 40, 48, 80, 0), (2, 8, 17, 32, 48, 0),
    (2, 12, 17, 16, 16, 1), (2, 8, 64, 64, 64, 1), (2, 20, 40, 16, 64, 1), (2, 1, 40, 64, 16, 1),
    (2, 12, 40, 16, 16, 2), (2, 8, 64, 64, 64, 2), (2, 2, 40, 16, 64, 2), (2, 12, 18, 64, 16, 2),     # bilinear on ragged tiles
]
XF = [       # resample 0, W in {64, 96}: W = 96 has a first, an interior and a last tile column, H = 20 a first, an interior and a last
             # (ragged) tile row; (2, 20, 96) has all nine positions, (2, 8, 96) the columns alone, (2, 20, 64) the rows alone
    (2, 20, 96, 16, 16, 0), (2, 8, 96, 16, 16, 0), (2, 20, 64, 32, 32, 0), (2, 8, 64, 64, 64, 0), (2, 1, 64, 16, 64, 0),
    (2, 12, 96, 64, 16, 0), (2, 12, 64, 48, 80, 0),
]
WALK = [     # several tiles per workgroup.  Precision 0, 128 -> 128: 16 slices, 16 workgroups per slice; (8, 24, 64): 48 tiles of a
             # 2 x 3 grid, step 16 = (dx 0, dy 2, db 2); (5, 20, 96): 45 tiles of a 3 x 3 grid, step 16 = (dx 1, dy 2, db 1): carries in x,
             # y and b.  (5, 128, 256): 640 tiles of 16 -> 16 on 512 workgroups, the largest tensor of this file
    (8, 24, 64, 128, 128, 0), (5, 20, 96, 128, 128, 0), (5, 128, 256, 16, 16, 0),
]
# single-tile images, 16 -> 16: nparts = B across the 64-stride loop of wgrad_reduce_kernel and its 16-stride tail
TAILS = [(1, 8, 32, 16, 16, 0), (15, 5, 20, 16, 16, 0), (16, 8, 16, 16, 16, 0), (17, 8, 32, 16, 16, 0), (49, 3, 9, 16, 16, 0),
         (64, 8, 32, 16, 16, 0), (65, 8, 16, 16, 16, 0), (113, 4, 32, 16, 16, 0)]
CASES = NARROW + WIDE + XF + WALK + TAILS
CO_LIMIT = {128: 32}        # output channels emulated on the CPU for a case with that many (a prefix: the elements are independent)

EXPECTED_NAMES = set()
for _cot in (1, 2):
    for _cit in (1, 2):
        _forms = [(res, tw, 0) for res in (0, 1, 2) for tw in (16, 32)] + [(0, 32, 1)]
        for _res, _tw, _xf in _forms:
            _nw = 8 if _cot * _cit == 4 else 4
            EXPECTED_NAMES.add(f"wgrad_f32_kernel<{_cot}, {_cit}, {_res}, {_tw}, {_nw}, {_xf}, 1>")
            for _plain in ("false", "true"):
                EXPECTED_NAMES.add(f"wgrad_bf16x3_kernel<{_cot}, {_cit}, {_res}, {_tw}, {_plain}, {'true' if _xf else 'false'}>")
assert len(EXPECTED_NAMES) == 84

# ---- synthetic slab sets for ngan_conv3x3_wgrad_reduce_many --------------------------------------------------------------------------
REDUCE_NPARTS = [1, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 512]
REDUCE_SLICES = [(16, 16), (16, 32), (32, 16), (32, 32)]          # (co_s, ci_s)
# sources of one entry: (nparts, scale) each; NG follows the largest nparts
REDUCE_MULTI = [[(17, 0.5), (128, -1.25)], [(1, 1.0), (64, 0.3), (7, 2.0)], [(33, 0.7), (16, -0.2), (129, 1.5), (15, 0.9)],
                [(512, 0.01), (31, 1.0)], [(1, -0.6), (1, 0.4), (1, 1.1), (1, 2.2)]]
ENTRY_FMT = "<4QQ4i8i4f"           # include/ngan.h: 4 slab pointers, gw, nparts[4], nsrc, nslices, n_ci_slices, co_s, ci_s, K, accumulate, first_block, scale[4]


def reduce_shape(co_s, ci_s, n_co=2, n_ci=2):
    """a layer of n_co x n_ci slices: dict(nslices, n_ci_slices, co_s, ci_s, K = Cin, Cout, M)"""
    return dict(nslices=n_co * n_ci, n_ci_slices=n_ci, co_s=co_s, ci_s=ci_s, K=n_ci * ci_s, Cout=n_co * co_s,
                M=n_co * n_ci * 9 * co_s * ci_s)


def many_entries():
    """the mixed call: 26 entries, every NG, every slice shape, 1 - 4 sources, both accumulate codes: [(shape, sources, accumulate)]"""
    out = []
    for i, np_ in enumerate(REDUCE_NPARTS + [3, 20, 40, 100, 200, 2, 1, 130, 66, 18, 5]):
        co_s, ci_s = REDUCE_SLICES[i % 4]
        src = [(np_, 0.25 + 0.125 * i)] + [(1 + (7 * i + 3 * s) % 40, -0.5 + 0.3 * s) for s in range(i % 4)]
        out.append((reduce_shape(co_s, ci_s, 1 + i % 2, 1 + (i // 2) % 3), src, i % 2))
    assert len(out) == 26
    return out


def pack_entry(ptrs, gw_ptr, sources, shape, accumulate):
    n = len(sources)
    return struct.pack(ENTRY_FMT, *(list(ptrs) + [0] * (4 - n)), gw_ptr, *([s[0] for s in sources] + [0] * (4 - n)), n, shape["nslices"],
                       shape["n_ci_slices"], shape["co_s"], shape["ci_s"], shape["K"], accumulate, 0,
                       *([float(s[1]) for s in sources] + [0.0] * (4 - n)))


# ---- plan replica (plan_wgrad; checked against ngan_conv3x3_wgrad_plan in tests/test_wgrad_bounds_cpu.py) -----------------------------
def plan(B, H, W, Cin, Cout, precision):
    tw = 16 if W <= 16 else 32
    th = 256 // tw
    tiles_x, tiles_y = -(-W // tw), -(-H // th)
    n_tiles = B * tiles_x * tiles_y
    small = precision == 0 and Cin <= 32 and Cout <= 32 and tw == 32
    co_s = 32 if Cout % 32 == 0 and not small else 16
    ci_s = 32 if Cin % 32 == 0 and not small else 16
    n_ci = Cin // ci_s
    nslices = (Cout // co_s) * n_ci
    total = 256 if precision == 0 and co_s == 32 and ci_s == 32 else 512
    nwx = min(n_tiles, max(total // nslices, 1))
    return dict(tw=tw, th=th, tiles_x=tiles_x, tiles_y=tiles_y, n_tiles=n_tiles, co_s=co_s, ci_s=ci_s, n_ci_slices=n_ci, nslices=nslices,
                nwx=nwx, slab_floats=nwx * nslices * 9 * co_s * ci_s)


def row_groups(p, precision, res):
    """waves that split a tile's rows and are summed through LDS"""
    cc = (p["co_s"] // 16) * (p["ci_s"] // 16)
    if precision != 0:
        return 4 // cc
    if cc == 4:
        return 4 if res != 2 else 2         # 8 waves; SHARE (two output groups per wave) unless the input is bilinear
    return 4 // cc


def kernel_name(case, precision):
    B, H, W, Cin, Cout, res = case
    p = plan(B, H, W, Cin, Cout, precision)
    xf = res == 0 and p["tw"] == 32 and W % 32 == 0
    cot, cit = p["co_s"] // 16, p["ci_s"] // 16
    if precision == 0:
        return f"wgrad_f32_kernel<{cot}, {cit}, {res}, {p['tw']}, {8 if cot * cit == 4 else 4}, {int(xf)}, 1>"
    return f"wgrad_bf16x3_kernel<{cot}, {cit}, {res}, {p['tw']}, {'true' if precision == 5 else 'false'}, {'true' if xf else 'false'}>"


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def bf16(a):
    """round-to-nearest-even to bf16, returned as fp32"""
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).float().numpy()


def bf16_trunc(a):
    return (np.ascontiguousarray(a, f32).view(np.uint32) & np.uint32(0xFFFF0000)).view(f32)


def x_shape(case):
    B, H, W, Cin, Cout, res = case
    return (B, 2 * H, 2 * W, Cin) if res == 1 else (B, H // 2, W // 2, Cin) if res == 2 else (B, H, W, Cin)


@functools.lru_cache(maxsize=2)
def inputs(case, storage):
    """x, g, buf (the gradient buffer an accumulating call starts from); storage "bf16": x and g hold bf16 values"""
    B, H, W, Cin, Cout, res = case
    seed = 7
    for v in case:
        seed = (seed * 131 + v) % (2 ** 31 - 1)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(*x_shape(case), generator=gen).numpy()
    g = torch.randn(B, H, W, Cout, generator=gen).numpy()
    buf = torch.randn(Cout, Cin, 3, 3, generator=gen).numpy()
    if storage == "bf16":
        x, g = bf16(x), bf16(g)
    return dict(x=x, g=g, buf=buf)


def storage_of(precision):
    return "bf16" if precision == 5 else "f32"


# ---- references -------------------------------------------------------------------------------------------------------------------------
_A = np.array([[1, 0], [1, 1], [1, 1], [0, 1]], f64)                                   # |A|, A = [1 0; 1 1; 1 -1; 0 -1]
_BT = np.array([[1, 0, 1, 0], [0, 1, 1, 0], [0, 1, 1, 0], [0, 1, 0, 1]], f64)            # |B^T|
_G = np.array([[1, 0, 0], [.5, .5, .5], [.5, .5, .5], [0, 0, 1]], f64)                  # |G|


def resampled64(x, res, storage):
    xr = fp64_conv.resample(torch.from_numpy(x).double(), res)
    if res and storage == "bf16":
        xr = xr.float().to(torch.bfloat16).double()          # the staging rounds the blended value once
    return xr


def winograd_absref(xr, g):
    """[ sum over 2x2 output tiles of (|A| |dY| |A|^T) . (|B|^T |d| |B|) ] back through |G|: (Cout, Cin, 3, 3), fp64"""
    B, H, W, Cin = xr.shape
    Cout = g.shape[3]
    He, We = H + H % 2, W + W % 2
    d = np.zeros((B, He + 2, We + 2, Cin), f64)
    d[:, 1:H + 1, 1:W + 1] = np.abs(xr)
    y = np.zeros((B, He, We, Cout), f64)
    y[:, :H, :W] = np.abs(g)
    T = B * (He // 2) * (We // 2)
    rows = [d[:, r:r + He:2] for r in range(4)]                                        # halo rows 2i + r
    tr = [sum(_BT[u, r] * rows[r] for r in range(4)) for u in range(4)]
    V = np.stack([sum(_BT[v, c] * tr[u][:, :, c:c + We:2] for c in range(4)) for u in range(4) for v in range(4)]).reshape(16, T, Cin)
    yr = [sum(_A[u, r] * y[:, r::2] for r in range(2)) for u in range(4)]
    M = np.stack([sum(_A[v, c] * yr[u][:, :, c::2] for c in range(2)) for u in range(4) for v in range(4)]).reshape(16, T, Cout)
    S = np.matmul(M.transpose(0, 2, 1), V).reshape(4, 4, Cout, Cin)
    return np.einsum("ur,uvoi,vs->oirs", _G, S, _G)


@functools.lru_cache(maxsize=4)
def reference(case, storage, winograd=False):
    """(ref, absref, 1) of the written gradient, (Cout, Cin, 3, 3) fp64; winograd: the fp32 Winograd form's absolute twin"""
    d = inputs(case, storage)
    sc = float(f32(SCALE))
    xr = resampled64(d["x"], case[5], storage)
    g = torch.from_numpy(d["g"]).double()
    ref = fp64_conv.conv3x3_wgrad(xr, g, sc).numpy()
    if winograd:
        absref = abs(sc) * winograd_absref(xr.numpy(), d["g"].astype(f64))
    else:
        absref = fp64_conv.conv3x3_wgrad(xr.abs(), g.abs(), abs(sc)).numpy()
    return ref, absref, 1


def plus(ref, buf):
    """reference of the accumulating form that starts from `buf`: one more rounding, the addition"""
    r, a, n = ref
    return r + buf.astype(f64), a + np.abs(buf.astype(f64)), n + 1


def ratio(got, ref, absref, n_round, c=C_ACC, split_absref=None):
    """worst err / bound over the elements; split_absref: the direct absref of the split-bf16 term"""
    got = np.asarray(got, dtype=f64)
    bound = n_round * 2.0 ** -23 * np.abs(ref) + c * 2.0 ** -24 * absref + 1e-30
    if split_absref is not None:
        bound = bound + SPLIT_TERM * split_absref
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    return float((np.abs(got - ref) / bound).max())


@functools.lru_cache(maxsize=2)
def split_reference(case):
    """the fp64 sum of the three products that the split-bf16 kernel forms (lo.hi + hi.lo + hi.hi), on the input as the staging blends it
    in fp32 (a last-bit difference in a blended value can flip the rounding of hi and with it the sign of lo, which moves lo.lo by
    2^-15 |g x|: the operands must be the emulation's own): what an exact accumulation of the kernel's operands gives, (Cout, Cin, 3, 3)"""
    d = inputs(case, "f32")
    sc = float(f32(SCALE))
    x32 = np.ascontiguousarray(resample_f32(d["x"], case[5], case[1], case[2]))
    xh, gh = bf16(x32), bf16(d["g"])
    xl, gl = bf16(x32 - xh), bf16(d["g"] - gh)
    t = lambda a: torch.from_numpy(a).double()
    w = fp64_conv.conv3x3_wgrad
    return (w(t(xh), t(gl), sc) + w(t(xl), t(gh), sc) + w(t(xh), t(gh), sc)).numpy()


def split_part_b(case):
    """worst |split_reference - ref| / ((SPLIT_TERM + C_ACC / 2 2^-24) absref): the derivation of the split term, checked on the operands"""
    ref, absref, _ = reference(case, "f32", False)
    return float((np.abs(split_reference(case) - ref) / ((SPLIT_TERM + C_ACC / 2 * 2.0 ** -24) * absref + 1e-30)).max())


def check(case, precision, got, accumulate, co_limit=None, part_a=False):
    """worst err / bound of a (Cout, Cin, 3, 3) result of `case` at `precision`, written (accumulate 0) or added to inputs()["buf"].
    part_a (precision 1): against split_reference() and without the split term (see the module docstring)"""
    st = storage_of(precision)
    ref = reference(case, st, precision == 0)
    buf = inputs(case, st)["buf"]
    split = reference(case, st, False)[1] if precision == 1 and not part_a else None
    if part_a:
        assert precision == 1
        ref = (split_reference(case),) + ref[1:]
    if accumulate:
        ref = plus(ref, buf)
    r, a, n = ref
    if co_limit:
        r, a, split = r[:co_limit], a[:co_limit], (split[:co_limit] if split is not None else None)
    return ratio(got, r, a, n, c_acc(FORM[precision]), split)


# ---- emulation: staging -------------------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def resample_f32(x, res, H, W):
    """the resampled input as the kernels' staging computes it, fp32: 0.25 ((a + b) + (c + d)); bilinear: per axis the taps (i0, i0 + 1),
    i0 = floor((Y - 1) / 2), clamped, with weights (.75, .25) for odd Y and (.25, .75) for even Y: top / bot = fma(x1, 1 - wx0, x0 wx0) along x,
    then fma(bot, 1 - wy0, top wy0)"""
    x = np.asarray(x, f32)
    if res == 0:
        return x
    if res == 1:
        return ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2])) * f32(0.25)
    h, w = H // 2, W // 2
    Y, X = np.arange(H), np.arange(W)
    y0, x0 = np.clip((Y - 1) >> 1, 0, h - 1), np.clip((X - 1) >> 1, 0, w - 1)
    y1, x1 = np.clip(((Y - 1) >> 1) + 1, 0, h - 1), np.clip(((X - 1) >> 1) + 1, 0, w - 1)
    wy0 = np.where(Y & 1, f32(0.75), f32(0.25)).astype(f32)[None, :, None, None]
    wx0 = np.where(X & 1, f32(0.75), f32(0.25)).astype(f32)[None, None, :, None]
    rows0, rows1 = x[:, y0], x[:, y1]
    top = _fma(rows0[:, :, x1], f32(1) - wx0, rows0[:, :, x0] * wx0)
    bot = _fma(rows1[:, :, x1], f32(1) - wx0, rows1[:, :, x0] * wx0)
    return _fma(bot, f32(1) - wy0, top * wy0)


def _tile_arrays(xr, g, p, B, H, W, defect=None):
    """g tiles (n_tiles, TH, TW, Cout) and x halo tiles (n_tiles, TH + 2, TW + 2, Cin), zeros outside the image, tile t = (b, ty, tx)"""
    th, tw, ty_n, tx_n = p["th"], p["tw"], p["tiles_y"], p["tiles_x"]
    Cin, Cout = xr.shape[3], g.shape[3]
    gp = np.zeros((B, ty_n * th, tx_n * tw, Cout), f32)
    gp[:, :H, :W] = g
    xp = np.zeros((B, ty_n * th + 2, tx_n * tw + 2, Cin), f32)
    xp[:, 1:H + 1, 1:W + 1] = xr
    gt = gp.reshape(B, ty_n, th, tx_n, tw, Cout).transpose(0, 1, 3, 2, 4, 5).reshape(-1, th, tw, Cout)
    t = np.arange(p["n_tiles"])
    b, ty, tx = t // (tx_n * ty_n), (t // tx_n) % ty_n, t % tx_n
    rows = ty[:, None] * th + np.arange(th + 2)[None, :]
    cols = tx[:, None] * tw + np.arange(tw + 2)[None, :]
    xt = xp[b[:, None, None], rows[:, :, None], cols[:, None, :]]
    if defect == "halo":
        xt[-1, :, 0] = 0
    return np.ascontiguousarray(gt), np.ascontiguousarray(xt)


def _walk(a, nwx):
    """(n_tiles, ...) -> (steps, nwx, ...): workgroup wx takes tiles wx, wx + nwx, ...; a missing tile is zeros (adds nothing)"""
    n = a.shape[0]
    steps = -(-n // nwx)
    if steps * nwx != n:
        a = np.concatenate([a, np.zeros((steps * nwx - n,) + a.shape[1:], a.dtype)])
    return a.reshape((steps, nwx) + a.shape[1:])


# ---- emulation: fp32 Winograd form ----------------------------------------------------------------------------------------------------
def _winograd_operands(gt, xt, tw):
    """per pixel tile the transformed operands in MFMA order: M (n, 4 steps, 4 j, 4 q, 16, Cout), V (.., Cin); position = 4 u + v"""
    th = gt.shape[1]
    r = [xt[:, k:k + th:2] for k in range(4)]                                          # halo rows 2 i + k
    t = [r[0] - r[2], r[1] + r[2], r[2] - r[1], r[1] - r[3]]
    V = []
    for u in range(4):
        c = [t[u][:, :, k:k + tw:2] for k in range(4)]
        V += [c[0] - c[2], c[1] + c[2], c[2] - c[1], c[1] - c[3]]
    g0, g1 = gt[:, 0::2], gt[:, 1::2]
    sg = [g0, g0 + g1, g0 - g1, g1]
    M = []
    for u in range(4):
        c0, c1 = sg[u][:, :, 0::2], sg[u][:, :, 1::2]
        M += [c0, c0 + c1, c0 - c1, c1]

    def order(ops):
        a = np.stack(ops, 3)                                                           # (n, I, J, 16, C)
        n, C = a.shape[0], a.shape[4]
        if tw == 32:                                                                   # I = 4 steps, J = 16 = (q, j)
            return a.reshape(n, 4, 4, 4, 16, C).transpose(0, 1, 3, 2, 4, 5)
        a = a.reshape(n, 4, 2, 2, 4, 16, C)                                            # I = (step, q >> 1), J = (q & 1, j)
        return a.transpose(0, 1, 4, 2, 3, 5, 6).reshape(n, 4, 4, 4, 16, C)
    return np.ascontiguousarray(order(M)), np.ascontiguousarray(order(V))


def _back_transform(acc):
    """acc (..., 16, Cout, Cin) fp32 -> the 9 taps (..., 9, Cout, Cin), in the kernel's order of operations"""
    a = lambda u, v: acc[..., 4 * u + v, :, :]
    h = f32(0.5)
    out = [None] * 9
    for j in range(3):
        Z = []
        for u in range(4):
            d1, d2 = a(u, 1), a(u, 2)
            z = (a(u, 0) + (d1 + d2) * h) if j == 0 else ((d1 - d2) * h) if j == 1 else ((d1 + d2) * h - a(u, 3))
            Z.append(-z if u == 3 else z)
        p12, m12 = (Z[1] + Z[2]) * h, (Z[1] - Z[2]) * h
        out[0 + j], out[3 + j], out[6 + j] = Z[0] + p12, m12, p12 + Z[3]
    return np.stack(out, -3)


def emulate_slabs_f32(case, mode, defect=None, co_limit=None):
    """wgrad_f32_kernel: the slabs (nwx, 9, Cout, Cin) of every workgroup column; mode "exact" / "seq" (the MFMA's four products)"""
    B, H, W, Cin, Cout, res = case
    d = inputs(case, "f32")
    p = plan(B, H, W, Cin, Cout, 0)
    g = d["g"][..., :co_limit] if co_limit else d["g"]
    gt, xt = _tile_arrays(resample_f32(d["x"], res, H, W), g, p, B, H, W, defect)
    M, V = _winograd_operands(gt, xt, p["tw"])
    M, V = _walk(M, p["nwx"]), _walk(V, p["nwx"])
    wrw = row_groups(p, 0, res)
    spw = 4 // wrw
    nwx, co = p["nwx"], g.shape[3]
    acc = np.zeros((nwx, wrw, 16, co, Cin), f32)
    for k in range(M.shape[0]):
        Mk = M[k].reshape(nwx, wrw, spw, 4, 4, 16, co)
        Vk = V[k].reshape(nwx, wrw, spw, 4, 4, 16, Cin)
        for s in range(spw):
            for j in range(4):
                if mode == "exact":
                    t = acc.astype(f64)
                    for q in range(4):
                        t += Mk[:, :, s, j, q, :, :, None].astype(f64) * Vk[:, :, s, j, q, :, None, :].astype(f64)
                    acc = t.astype(f32)
                else:
                    for q in range(4):
                        acc = _fma(Mk[:, :, s, j, q, :, :, None], Vk[:, :, s, j, q, :, None, :], acc)
    taps = _back_transform(acc)                                                        # (nwx, wrw, 9, co, Cin)
    v = taps[:, 0]
    for w in range(1, wrw):
        v = v + taps[:, w]
    return v


# ---- emulation: split-bf16 and plain bf16 forms -----------------------------------------------------------------------------------------
def emulate_slabs_bf16(case, precision, defect=None, co_limit=None):
    """wgrad_bf16x3_kernel: the slabs (nwx, 9, Cout, Cin).  precision 1: hi / lo planes, MFMAs lo.hi, hi.lo, hi.hi; 5: one plane"""
    B, H, W, Cin, Cout, res = case
    d = inputs(case, storage_of(precision))
    p = plan(B, H, W, Cin, Cout, precision)
    g = d["g"][..., :co_limit] if co_limit else d["g"]
    gt, xt = _tile_arrays(resample_f32(d["x"], res, H, W), g, p, B, H, W, defect)
    rnd = bf16_trunc if defect == "trunc" else bf16
    gh, xh = rnd(gt), rnd(xt)
    planes = [(gh, xh)]
    if precision == 1:
        gl, xl = bf16(gt - gh), bf16(xt - xh)
        planes = ([] if defect == "no_lohi" else [(gl, xh)]) + [(gh, xl), (gh, xh)]
    planes = [(_walk(a, p["nwx"]).astype(f64), _walk(b, p["nwx"]).astype(f64)) for a, b in planes]
    th, tw, nwx, co = p["th"], p["tw"], p["nwx"], g.shape[3]
    wr_n = row_groups(p, precision, res)
    kpw, rpk = 8 // wr_n, 32 // tw                                                     # k-steps per wave, tile rows per k-step
    acc = np.zeros((nwx, wr_n, 9, co, Cin), f32)
    for k in range(planes[0][0].shape[0]):
        for ks in range(8):
            wr = ks // kpw
            r0 = ks * rpk
            for tap in range(9):
                dy, dx = tap // 3, tap % 3
                a = acc[:, wr, tap]
                for ga, xa in planes:
                    gm = ga[k][:, r0:r0 + rpk].reshape(nwx, 32, co)
                    xm = xa[k][:, r0 + dy:r0 + dy + rpk, dx:dx + tw].reshape(nwx, 32, Cin)
                    a = (a.astype(f64) + np.matmul(gm.transpose(0, 2, 1), xm)).astype(f32)
                acc[:, wr, tap] = a
    v = acc[:, 0]
    for w in range(1, wr_n):
        v = v + acc[:, w]
    return v


def emulate_slabs(case, precision, mode="exact", defect=None, co_limit=None):
    if precision == 0:
        return emulate_slabs_f32(case, mode, defect, co_limit)
    return emulate_slabs_bf16(case, precision, defect, co_limit)


# ---- emulation: slab layout and the reductions ------------------------------------------------------------------------------------------
def to_workspace(slabs, co_s, ci_s):
    """(nparts, 9, Cout, Cin) -> the workspace layout (nparts, M): [slice = (co / co_s) n_ci + ci / ci_s][tap][co_l][ci_l]"""
    n, _, Cout, Cin = slabs.shape
    a = slabs.reshape(n, 9, Cout // co_s, co_s, Cin // ci_s, ci_s).transpose(0, 2, 4, 1, 3, 5)
    return np.ascontiguousarray(a).reshape(n, -1)


def from_workspace(v, Cout, Cin, co_s, ci_s, defect=None):
    """the reductions' output index map: (M,) in slab order -> gw (Cout, Cin, 3, 3)"""
    a = v.reshape(Cout // co_s, Cin // ci_s, 9, co_s, ci_s)
    if defect == "swap":
        assert co_s == ci_s and a.shape[0] * a.shape[1] > 1
        a = a.copy()
        s = 1
        a[s // a.shape[1], s % a.shape[1]] = a[s // a.shape[1], s % a.shape[1]].transpose(0, 2, 1)
    return np.ascontiguousarray(a.transpose(0, 3, 1, 4, 2)).reshape(Cout, Cin, 3, 3)


def _defective(ws, defect):
    if defect == "slab_twice":
        return np.concatenate([ws, ws[-1:]])
    if defect == "slab_skipped":
        return ws[:-1]
    return ws


def reduce_emulate(ws, scale, buf=None):
    """wgrad_reduce_kernel on ws (nparts, M): (M,) in slab order; buf (M,) in slab order: the accumulating form"""
    nparts, M = ws.shape
    s = np.zeros(M, f32)
    for lane in range(16):
        a = [np.zeros(M, f32) for _ in range(4)]
        j = lane
        while j + 48 < nparts:
            for k in range(4):
                a[k] = a[k] + ws[j + 16 * k]
            j += 64
        while j < nparts:
            a[0] = a[0] + ws[j]
            j += 16
        s = s + ((a[0] + a[1]) + (a[2] + a[3]))
    return _fma(s, f32(scale), buf) if buf is not None else s * f32(scale)


def reduce_groups(nparts):
    np_ = max(nparts)
    return 16 if np_ >= 128 else 8 if np_ >= 64 else 4 if np_ >= 32 else 2 if np_ >= 16 else 1


def reduce_many_emulate(sources, scales, buf=None):
    """wgrad_reduce_many_kernel on one entry: sources = [ws (nparts_s, M)], scales; (M,) in slab order; buf: accumulate = 1"""
    ng = reduce_groups([w.shape[0] for w in sources])
    M = sources[0].shape[1]
    total = np.zeros(M, f32)
    for ws, sc in zip(sources, scales):
        np_ = ws.shape[0]
        t = np.zeros(M, f32)
        for grp in range(ng):
            a = [np.zeros(M, f32) for _ in range(8)]
            j = grp
            while j + 7 * ng < np_:
                for k in range(8):
                    a[k] = a[k] + ws[j + k * ng]
                j += 8 * ng
            while j < np_:
                a[0] = a[0] + ws[j]
                j += ng
            for k in range(4):
                a[k] = a[k] + a[k + 4]
            t = t + ((a[0] + a[1]) + (a[2] + a[3]))
        total = _fma(t, f32(sc), total)
    return buf + total if buf is not None else total


def reduce_many_ref(sources, scales):
    """(ref, absref, 1) in slab order, fp64"""
    r = sum(float(f32(sc)) * w.astype(f64).sum(0) for w, sc in zip(sources, scales))
    a = sum(abs(float(f32(sc))) * np.abs(w.astype(f64)).sum(0) for w, sc in zip(sources, scales))
    return r, a, 1


@functools.lru_cache(maxsize=64)
def synthetic_slabs(nparts, M, tag):
    gen = torch.Generator().manual_seed((tag * 7919 + nparts * 131 + M) % (2 ** 31 - 1))
    return torch.randn(nparts, M, generator=gen).numpy()


def emulate(case, precision, mode="exact", accumulate=0, path="direct", defect=None, co_limit=None):
    """the whole call: slabs, then wgrad_reduce_kernel (path "direct") or wgrad_reduce_many_kernel with one source ("deferred"):
    (Cout or co_limit, Cin, 3, 3) fp32"""
    B, H, W, Cin, Cout, res = case
    p = plan(B, H, W, Cin, Cout, precision)
    slabs = emulate_slabs(case, precision, mode, defect, co_limit)
    co = slabs.shape[2]
    co_s = min(p["co_s"], co)
    ws = _defective(to_workspace(slabs, co_s, p["ci_s"]), defect)
    buf = None
    if accumulate:
        b = inputs(case, storage_of(precision))["buf"][:co]
        buf = to_workspace(np.ascontiguousarray(b.reshape(co, Cin, 9).transpose(2, 0, 1))[None], co_s, p["ci_s"])[0]
    out = reduce_emulate(ws, SCALE, buf) if path == "direct" else reduce_many_emulate([ws], [SCALE], buf)
    return from_workspace(out, co, Cin, co_s, p["ci_s"], defect)
