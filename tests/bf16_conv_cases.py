"""The bf16-storage 3x3 convolution behind ngan_bf16_conv3x3_fwd (precision code 5: csrc/conv3x3_bf16.hip, conv3x3_bf16_impl.h,
conv3x3_bf16_k{16,32,64,128}.hip, conv3x3_bf16_wide.hip, packed by bf16_weight), forward and -- with the flipped packing -- input
gradient, at every one of its 80 template instances and at the edges of their tilings: the instance table, a replica of pick_tile, the
per-instance facts that decide code paths, the case list, fp64 references on the operands as stored, the per-element bounds, the
exact-rounding pin of the bf16 store, a numpy emulation in the kernel's order and planted defects.  Shared by
tests/test_gpu_bf16_conv.py (the kernels against the references) and tests/test_bf16_conv_bounds_cpu.py (the emulation against the
references: the constants are settled on the CPU, before any kernel is looked at; the replica is checked against the built library
there).  Nothing of the package is imported here.  The epilogue propagation, the sign condition and undecided_fraction are those of
tests/conv_fwd_cases.py; rbf / trunc_bf16 and the bf16-output rule those of tests/lane_group_cases.py; a resampled operand is rounded
once, as tests/wgrad_cases.py treats precision 5.

A case is Case(B, H, W, K, N, res, epi, om, var) with the meanings of tests/conv_fwd_cases.py (H, W the convolution's own size; res 1:
x is (B, 2H, 2W, K), 2: (B, H/2, W/2, K); epi 0 none, 1 LeakyReLU -> PixelNorm, 2 PixelNorm backward, 3 epilogue 1 + ToImage; om 1 the
pool-adjoint store); var "" / "noy" (epilogue 3 without a stored y) / "onehot" (one product per output element).  Every case runs with
the weight in both orientations ops._packed offers (mode 0: (N, K, 3, 3); mode 1: (K, N, 3, 3), taps flipped).

Instances.  EXPECTED_NAMES in the text ngan_conv3x3_kernel_name(..., precision 5) prints:
  conv3x3_bf16_kernel<K, N, PGT, NS, NARROW>     K, N in {16, 32, 64, 128} x 4 tile shapes (N <= 32, pixel split: PGT 16 / 8 / 4 of 32
                                                 columns and 4 narrow; N >= 64, output-tile split: PGT 4 / 2, each wide and narrow)    64
  conv3x3_bf16_wide_kernel<N, PGT, NS, NARROW>   any other contraction width, a multiple of 16 up to 1024, in 128-channel slices       16
facts() derives from conv3x3_bf16_body what decides an instance's code paths: S contraction steps (per slice), NTW output tiles per
wave, WREG (S * NTW <= 18: all weight fragments in registers) or a register ring RD = min(S, 8) steps ahead (wide: 9), the slice count,
and the tile TH x TW (TW 16 narrow / 32; TH = PGT / (TW / 16): 8, 4, 2 rows, 1 for the wide-tile PGT 2 of the output split).

Operands as stored: x, ay (and the g of an input gradient, which is x here) hold bf16 values; the weight is rne_bf16(fp32(w) * fp32(scale))
(stored_weight; tests/test_gpu_bf16_conv.py checks the packing bit for bit against pack_replica); a resampled input is the blend rounded
to bf16 once.  inputs() keeps |x| in [2^-6, 8): bf16 values there are multiples of 2^-13 below 2^16 of them, a 2x2 sum stays below
2^18 and a bilinear blend (weights 9, 3, 3, 1 sixteenths) below 2^20 in units of 2^-17 -- every fp32 operation of either staging is
exact, so the kernel's association and the fp64 blend round the same number and the reference does not depend on which one it takes
(test_bf16_conv_bounds_cpu.py shows it for every resampled case).  The fp64 reference convolves those stored operands.

Inputs.  Seven eighths of the x values and of the weight magnitudes are positive, the weight's sign follows its output channel
(n odd: negative) and the bias (3 +- 0.5, sign changing every two channels) adds to it: both LeakyReLU branches occur in every pixel
and the sums cancel little, |c| ~ 0.5 absref.  That is what keeps the fp32 bound e small against the spacing of the bf16 values (the
exact-rounding pin below decides all but about 1e-3 of the elements; zero-centred sums leave several percent undecided at K >= 128)
and the pre-activations off the LeakyReLU kink.

Bounds, per element; nothing here was fitted to a kernel.
  convolution result c = conv + bias before the store   e_c = 2^-23 |c| + C_ACC 2^-24 absref,  C_ACC = 8  (absref: the reference's own
                          sum with absolute values, plus |bias|); RAISED lists the contraction widths whose emulation exceeds 0.5
  fp32 outputs (rnorm of epilogues 1 and 3, the ToImage result): conv_fwd_cases.reference with e_c propagated to first order
  bf16 outputs            |got - ref| <= 2^-8 |ref| + (1 + 2^-8) e,  e the fp32 bound of the same output
  exact-rounding pin      wherever ref lies farther than e from every midpoint between neighbouring bf16 values the stored bits must be
                          rne_bf16(ref); at most 1e-2 of a case's elements may be left undecided (checked on the reference alone)
  LeakyReLU pattern       the stored output's; the stored sign must be the fp64 sign wherever |c| > e_c; at most 1e-4 undecided
  out_mode 1              the factor 0.25 is exact; epilogue 2 is evaluated at the four pixels of each window

Emulation (emulate): a k-step is 32 contraction indices -- K = 16: a pair of taps (the tenth tap zero); 32 / 64 / 128: tap-major with
32-channel sub-blocks; wide: 128-channel slices outermost -- whose 32 products are exact in fp32; their sum is formed in fp64 and
rounded once into the fp32 accumulator (the model of v_mfma_f32_16x16x32_bf16 in tests/wgrad_cases.py).  The bias is added last.  A
per-pixel sum goes over a lane's channels ((a + b) + c) + d per output tile, the tiles in order, then the four k-group rows pairwise
(sum_rows4) and, in the output split, the four waves as (s0 + s1) + (s2 + s3); rsq and rnorm = m * rsq(m).

Planted defects (`defect=`), each of which test_bf16_conv_bounds_cpu.py shows to miss a bound or the pin: trunc_store, trunc_weight,
halo (the left halo column of the last tile column dropped), chunk_swap (channel chunks 0 and 2 exchanged in the columns of one
swizzle class), tap10 (the padding tap of K = 16 carrying tap 8's weights), ring_stale (step RD uses step 0's weights), slice_pad,
norm_wave (the PixelNorm sum over one wave's channels), rn_group (the norm of pixel group 1 stored at group 0's pixels), clamp (a
bilinear edge tap one pixel off), double_round (the bilinear blend rounded after the horizontal pass too), pool_twice, flip (mode 1
without the tap flip).  slice_pad: the staging zero-pads the last slice and so does the packing, and either alone multiplies by the
other's zeros and changes no result; the planted defect loses both (x reads on into the next pixel's channels, the weight into the
next rows of the (N, K, 9) array), which is the form that can be seen.

RAISED: contraction width -> (raised C_ACC, emulated worst err / bound of c there), for the widths whose emulation exceeds 0.5 at
C_ACC = 8: the next power of two that brings it to 0.5 or below.  With sums that do not cancel the partial sums grow linearly, and each
of the S k-steps rounds at the partial sum's magnitude: the accumulated rounding grows like sqrt(S) |c| while C_ACC absref does not."""
import collections
import functools

import numpy as np
import torch

import conv_fwd_cases as F
import fp64_conv
from conv_fwd_cases import C_ACC, EPS, SLOPE, _cdiv, _chan_sum, _np, pool_adjoint_f32, scale_of, w_eff, x_shape, y_shape      # noqa: F401
from lane_group_cases import rbf, trunc_bf16
from wgrad_cases import _fma, resample_f32

f32, f64 = np.float32, np.float64
PREC = 5
UNDECIDED_CAP = 1e-2
# contraction width -> (raised C_ACC, emulated worst err / bound of c at that constant)
RAISED = {144: (16.0, 0.301), 256: (16.0, 0.289), 1024: (32.0, 0.278)}

Case = collections.namedtuple("Case", "B H W K N res epi om var", defaults=("",))
Facts = collections.namedtuple("Facts", "wide S NTW WREG RD NSL TH TW NS path")


def c_acc(K):
    return float(RAISED.get(K, (C_ACC, None))[0])


def case_id(c):
    return "x".join(map(str, c[:8])) + (("-" + c.var) if c.var else "")


# ---- the instance table and the routing (conv3x3_bf16.hip: pick_tile, conv3x3_bf16_kernel_name) ---------------------------------------
TUNED_K = (16, 32, 64, 128)
CHANNELS = (16, 32, 64, 128)
SMALL_TILES = [(16, False), (8, False), (4, False), (4, True)]           # N <= 32: (PGT, NARROW)
BIG_TILES = [(4, False), (2, False), (4, True), (2, True)]               # N >= 64


def _b(v):
    return "true" if v else "false"


def name_of(K, N, pgt, narrow):
    if K in TUNED_K:
        return "conv3x3_bf16_kernel<%d, %d, %d, %s, %s>" % (K, N, pgt, _b(N >= 64), _b(narrow))
    return "conv3x3_bf16_wide_kernel<%d, %d, %s, %s>" % (N, pgt, _b(N >= 64), _b(narrow))


EXPECTED_NAMES = {name_of(K, N, pgt, narrow) for K in TUNED_K + (48,) for N in CHANNELS for pgt, narrow in (SMALL_TILES if N <= 32 else BIG_TILES)}
assert len(EXPECTED_NAMES) == 64 + 16


def wide_ok(K):
    return 0 < K <= 1024 and K % 16 == 0 and K not in TUNED_K


def pick_tile(B, H, W, N):
    """(PGT, NARROW) as pick_tile counts tiles"""
    narrow = W <= 16
    if N <= 32:
        t8, t4 = B * _cdiv(H, 8) * _cdiv(W, 32), B * _cdiv(H, 4) * _cdiv(W, 32)
        return (4 if narrow else 16 if t8 >= 512 else 8 if t4 >= 384 else 4), narrow
    t64 = B * _cdiv(H, 4) * _cdiv(W, 16) if narrow else B * _cdiv(H, 2) * _cdiv(W, 32)
    return (4 if t64 >= 256 else 2), narrow


def facts(K, N, pgt, narrow):
    """what decides the code paths of conv3x3_bf16_body<K, N, PGT, NS, NARROW, WIDE>"""
    wide = K not in TUNED_K
    kt = 128 if wide else K
    S = 5 if kt == 16 else 9 * (kt // 32)
    ns = N >= 64
    ntw = N // 64 if ns else N // 16
    wreg = not wide and S * ntw <= 18
    tw = 16 if narrow else 32
    return Facts(wide, S, ntw, wreg, 9 if wide else min(S, 8), _cdiv(K, 128) if wide else 1, pgt // (tw // 16), tw, ns,
                 "wide" if wide else "wreg" if wreg else "ring")


def facts_of(c):
    return facts(c.K, c.N, *pick_tile(c.B, c.H, c.W, c.N))


def kernel_name(c):
    return name_of(c.K, c.N, *pick_tile(c.B, c.H, c.W, c.N))


def pack_elements(K, N):
    """ngan::conv3x3_bf16_elements"""
    if N not in CHANNELS:
        return 0
    if wide_ok(K):
        return 36 * _cdiv(K, 128) * (N // 16) * 512
    return (5 if K == 16 else 9 * (K // 32)) * (N // 16) * 512 if K in TUNED_K else 0


def pack_replica(w, mode, scale):
    """bf16_weight for every index of the packed array: fp32 numpy holding the bf16 values; w the fp32 master (Cout, Cin, 3, 3)"""
    Cout, Cin = w.shape[:2]
    K, N = (Cin, Cout) if mode == 0 else (Cout, Cin)
    idx = np.arange(pack_elements(K, N), dtype=np.int64)
    e, lane, r = idx & 7, (idx >> 3) & 63, idx >> 9
    j, step = r % (N // 16), r // (N // 16)
    n, kk = j * 16 + (lane & 15), 8 * (lane >> 4) + e
    if K == 16:
        tap, k = 2 * step + (kk >> 4), kk & 15
    elif K in TUNED_K:
        tap, k = step // (K // 32), (step % (K // 32)) * 32 + kk
    else:
        tap, k = (step % 36) >> 2, (step // 36) * 128 + ((step % 36) & 3) * 32 + kk
    ok = (tap < 9) & (k < K)
    tap, k = np.where(ok, tap, 0), np.where(ok, k, 0)
    flat = np.ascontiguousarray(w, dtype=f32).reshape(-1)
    v = flat[(n * Cin + k) * 9 + tap] if mode == 0 else flat[(k * Cin + n) * 9 + (8 - tap)]
    return rbf(np.where(ok, v, f32(0)).astype(f32) * f32(scale))


# ---- the case list -----------------------------------------------------------------------------------------------------------------
# (N <= 32, PGT, NARROW) -> the smallest shapes that reach the tile: [ragged right column and bottom row, ...extras: an image of exactly
# one tile per image, smaller ones]; EVEN: the bilinear input's (even sides; H = 2 / W = 2: every tap clamped)
SHAPES = {
    (True, 4, True): [(2, 5, 12), (16, 1, 1), (1, 4, 16)],
    (True, 4, False): [(2, 3, 40), (1, 2, 32), (2, 5, 70)],           # (2, 5, 70): a first, an interior and a last tile in both directions
    (True, 8, False): [(96, 6, 40), (384, 4, 32)],                     # t4 = 384, t8 = 192 / 384 < 512
    (True, 16, False): [(128, 12, 40), (512, 8, 32)],                  # t8 = 512
    (False, 2, False): [(2, 3, 40), (1, 1, 32), (2, 5, 70)],           # one-row tiles, odd tile origins
    (False, 4, False): [(32, 7, 40), (256, 2, 32)],                    # t64 = 256
    (False, 2, True): [(2, 5, 12), (16, 1, 1), (1, 2, 16)],
    (False, 4, True): [(128, 5, 12), (256, 4, 16)],                    # t64 = 256
}
EVEN = {
    (True, 4, True): [(2, 6, 12), (8, 2, 2)], (True, 4, False): [(2, 4, 40), (2, 2, 40)], (True, 8, False): [(96, 6, 40)],
    (True, 16, False): [(128, 12, 40)], (False, 2, False): [(2, 4, 40), (2, 2, 40)], (False, 4, False): [(43, 6, 40)],
    (False, 2, True): [(2, 6, 12), (8, 2, 2)], (False, 4, True): [(128, 6, 12)],
}
BIG_BATCH = {(True, 8, False), (True, 16, False), (False, 4, False), (False, 4, True)}
WIDE_K = (48, 144, 256)            # one padded slice; two slices, the last 16 channels wide; two whole slices; 1024 once (below)
# the legal forms other than resample 0 with epilogues 0 and 1: (res, epi, om, var)
OTHER_FORMS = [(1, 0, 0, ""), (1, 1, 0, ""), (2, 0, 0, ""), (2, 1, 0, ""), (0, 2, 0, ""), (0, 2, 1, ""), (0, 0, 1, "")]
TO_IMAGE_FORMS = [(0, 3, 0, ""), (0, 3, 0, "noy")]                        # N <= 32
# one (K, N) per split kind and weight path
REPRESENTATIVE = {(True, "wreg"): (16, 16), (True, "ring"): (64, 32), (True, "wide"): (144, 16),
                  (False, "wreg"): (16, 64), (False, "ring"): (64, 128), (False, "wide"): (144, 64)}


def _tiles(N):
    return SMALL_TILES if N <= 32 else BIG_TILES


def _instance_cases():
    out = []
    for ni, N in enumerate(CHANNELS):
        for ti, (pgt, narrow) in enumerate(_tiles(N)):
            key = (N <= 32, pgt, narrow)
            for ki, K in enumerate(TUNED_K + (None,)):
                if K is None:
                    K = 48 if key in BIG_BATCH else WIDE_K[(ni + ti) % 3]
                shapes = SHAPES[key][:1] + (SHAPES[key][1:] if (K == 16 and N in (16, 64)) else [])
                for shape in shapes:
                    for epi in (0, 1):
                        out.append(Case(*shape, K, N, 0, epi, 0))
    return out


def _form_cases():
    out = []
    for (small, path), (K, N) in REPRESENTATIVE.items():
        for pgt, narrow in _tiles(N):
            key = (small, pgt, narrow)
            kk = 48 if (path == "wide" and key in BIG_BATCH) else K
            for res, epi, om, var in OTHER_FORMS + (TO_IMAGE_FORMS if small else []):
                for shape in (EVEN[key] if res == 2 else SHAPES[key][:1]):
                    out.append(Case(*shape, kk, N, res, epi, om, var))
    return out


# one product per output element, per split kind; the widest contraction once, on the smallest ragged image
ONE_PRODUCT = [Case(2, 5, 12, 32, 32, 0, 0, 0, "onehot"), Case(2, 3, 40, 32, 64, 0, 0, 0, "onehot")]
WIDEST = [Case(2, 5, 12, 1024, 16, 0, 0, 0), Case(2, 5, 12, 1024, 16, 0, 1, 0)]
INSTANCE, FORMS = _instance_cases(), _form_cases()
CASES = list(dict.fromkeys(INSTANCE + FORMS + ONE_PRODUCT + WIDEST))
# two launches of these must be bit-equal: one per split kind and weight path
REPEAT = [Case(*SHAPES[(small, 4, False)][0], K, N, 0, 1, 0) for (small, path), (K, N) in REPRESENTATIVE.items()]


def covering(cases):
    """{(form, split kind, narrow, TH, weight path)} of the cases, form = (res, epi, om, var)"""
    out = set()
    for c in cases:
        f = facts_of(c)
        out.add(((c.res, c.epi, c.om, c.var), "tile" if f.NS else "pixel", f.TW == 16, f.TH, f.path))
    return out


def required_covering():
    out = set()
    for small in (True, False):
        for pgt, narrow in (SMALL_TILES if small else BIG_TILES):
            th = pgt // (1 if narrow else 2)
            for path in ("wreg", "ring", "wide"):
                for form in OTHER_FORMS + (TO_IMAGE_FORMS if small else []):
                    out.add((form, "pixel" if small else "tile", narrow, th, path))
    return out


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def has_bias(c):
    return c.epi != 2 and c.var != "onehot"


def _mostly_positive(shape, gen, floor=0.0):
    mag = torch.randn(*shape, generator=gen).abs().clamp_(min=floor)
    return torch.where(torch.rand(*shape, generator=gen) < 0.125, -mag, mag)


def _bf(t):
    return t.to(torch.bfloat16).float()


@functools.lru_cache(maxsize=2)
def inputs(c, mode):
    """fp32 torch tensors on the CPU; x and ay hold bf16 values.  x, w: the same for every (epi, om, var) of a (shape, K, N, res, mode)"""
    seed = 17
    for v in c[:6]:
        seed = (seed * 131 + v) % (2 ** 31 - 1)
    x = _bf(_mostly_positive(x_shape(c), torch.Generator().manual_seed(seed), 2.0 ** -6))          # (the same in both orientations)
    gen = torch.Generator().manual_seed(seed + 1 + mode)
    sign = torch.tensor([1.0 if n % 2 == 0 else -1.0 for n in range(c.N)]).view(-1, 1, 1, 1)
    weff = _mostly_positive((c.N, c.K, 3, 3), gen) * sign
    if c.var == "onehot":
        # x in channel 0 only, the weight in the centre tap only, no bias: every output element is one exact product
        # (the last significand bit of x set: the 16-bit product is then a tie between two bf16 values, which the pin leaves undecided,
        # only where the stored weight is a power of two)
        x0 = torch.zeros_like(x)
        x0[..., 0] = (x[..., 0].contiguous().view(torch.int32) | 0x10000).view(torch.float32)
        w0 = torch.zeros_like(weff)
        w0[:, :, 1, 1] = weff[:, :, 1, 1]
        x, weff = x0, w0
    d = dict(x=x, w=(weff if mode == 0 else weff.flip(2, 3).transpose(0, 1)).contiguous(), bias=None)
    gen = torch.Generator().manual_seed(seed + 3)
    if has_bias(c):
        bsign = torch.tensor([1.0 if (ch // 2) % 2 == 0 else -1.0 for ch in range(c.N)])
        d["bias"] = 3.0 * bsign + 0.5 * torch.randn(c.N, generator=gen)
    if c.epi == 2:
        d["ay"] = _bf(torch.randn(*y_shape(c), generator=gen))
        d["arn"] = torch.rand(*y_shape(c)[:3], generator=gen) + 0.5
    if c.epi == 3:
        d["wimg"] = torch.randn(c.N, generator=gen) / c.N ** 0.5
    return d


def stored_weight(c, mode, d, defect=None):
    """rne_bf16(fp32(w) * fp32(scale)) in the convolution's own orientation: (N, K, 3, 3) fp32 numpy holding bf16 values"""
    w = d["w"] if (mode == 0 or defect != "flip") else d["w"].flip(2, 3)
    v = (_np(w_eff(w, mode)) * f32(scale_of(c))).astype(f32)
    return trunc_bf16(v) if defect == "trunc_weight" else rbf(v)


def staged64(c, d, dev="cpu"):
    """the operand the MFMAs read: the fp64 blend of x rounded to bf16 once; (B, H, W, K) fp64 torch"""
    xr = fp64_conv.resample(d["x"].to(dev).double(), c.res)
    return xr.float().to(torch.bfloat16).double() if c.res else xr


def _bilinear_f32(x, H, W, defect=None):
    """resample_f32's bilinear with the planted defects: fp32 (B, H, W, K)"""
    if defect == "clamp":
        good = resample_f32(x, 2, H, W)
        bad = resample_f32(np.concatenate([x[:, :-1], x[:, -2:-1]], 1), 2, H, W)
        return np.concatenate([good[:, :-1], bad[:, -1:]], 1)
    if defect != "double_round":
        return resample_f32(x, 2, H, W)
    h, w = H // 2, W // 2
    Y, X = np.arange(H), np.arange(W)
    y0, x0 = np.clip((Y - 1) >> 1, 0, h - 1), np.clip((X - 1) >> 1, 0, w - 1)
    y1, x1 = np.clip(((Y - 1) >> 1) + 1, 0, h - 1), np.clip(((X - 1) >> 1) + 1, 0, w - 1)
    wy0 = np.where(Y & 1, f32(0.75), f32(0.25)).astype(f32)[None, :, None, None]
    wx0 = np.where(X & 1, f32(0.75), f32(0.25)).astype(f32)[None, None, :, None]
    rows0, rows1 = x[:, y0], x[:, y1]
    top = rbf(_fma(rows0[:, :, x1], f32(1) - wx0, rows0[:, :, x0] * wx0))
    bot = rbf(_fma(rows1[:, :, x1], f32(1) - wx0, rows1[:, :, x0] * wx0))
    return _fma(bot, f32(1) - wy0, top * wy0)


def staged32(c, d, defect=None):
    """the same operand by the kernel's own fp32 association (0.25 * ((a + b) + (c + d)); the staging's fmaf chain), rounded once"""
    x = _np(d["x"])
    if c.res == 0:
        return x
    return rbf(_bilinear_f32(x, c.H, c.W, defect) if c.res == 2 else resample_f32(x, 1, c.H, c.W))


# ---- references -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _conv_reference(key, mode, dev):
    c = Case(*key[:6], 0, 0, "onehot" if key[-1] else "")
    d = inputs(c, mode)
    t = lambda a: torch.from_numpy(a).to(dev).double()
    xr, wq = staged64(c, d, dev), t(stored_weight(c, mode, d))
    return fp64_conv.conv3x3(xr, wq), fp64_conv.conv3x3(xr.abs(), wq.abs())


def conv_reference(c, mode, d, dev="cpu"):
    """(c64, e_c, absref) of conv + bias on the stored operands, (B, H, W, N) fp64 on `dev` (the convolution itself is shared by the
    epilogues and stores of one (shape, K, N, res, mode))"""
    c64, absref = _conv_reference(tuple(c[:6]) + (c.var == "onehot",), mode, str(dev))
    if d.get("bias") is not None:
        bias = d["bias"].to(dev).double()
        c64, absref = c64 + bias, absref + bias.abs()
    return c64, 2.0 ** -23 * c64.abs() + c_acc(c.K) * 2.0 ** -24 * absref, absref


def reference(c, mode, d, stored_y=None, dev="cpu"):
    """{output: (ref, bound)} for y (the bf16 bound; "y32": its fp32 bound e) / rn / img, plus "_c": (c64, e_c)"""
    c64, e_c, _ = conv_reference(c, mode, d, dev)
    out = F.reference(c, mode, d, stored_y=stored_y, dev=dev, pre=(c64, e_c))
    r, e = out["y"]
    out["y32"] = (r, e)
    out["y"] = (r, 2.0 ** -8 * r.abs() + (1 + 2.0 ** -8) * e)
    return out


def midpoint_distance(r):
    """distance of the fp64 values r from the nearest midpoint between two neighbouring bf16 values"""
    a = r.abs()
    _, ex = torch.frexp(a)                                        # a = m 2^ex, m in [0.5, 1): bf16 values are 2^(ex - 8) apart there
    ulp = torch.ldexp(torch.ones_like(a), ex - 8)
    t = a / ulp
    inside = ((t - torch.floor(t)) - 0.5).abs() * ulp
    below = a - (torch.ldexp(torch.ones_like(a), ex - 1) - ulp / 4)      # the last midpoint of the binade below (half the spacing)
    return torch.where(a > 0, torch.minimum(inside, below), inside)


def exact_pin(stored, r, e):
    """(stored elements that differ from rne_bf16(ref) although ref is farther than e from every midpoint, share of undecided elements)"""
    decided = midpoint_distance(r) > e
    want = r.float().to(torch.bfloat16)
    got = stored.to(r.device).to(torch.bfloat16)
    miss = decided & (got.view(torch.int16) != want.view(torch.int16)) & ~((got == 0) & (want == 0))
    return int(miss.sum()), float((~decided).double().mean())


def check(c, mode, d, got, dev="cpu"):
    """got: {"y": the stored bf16 output (any float dtype holding it), "rn", "img"} torch -> {"y", "rn", "img": worst err / bound,
    "exact_miss", "undecided", "sign", "kink"}"""
    stored = got.get("y")
    ref = reference(c, mode, d, stored_y=stored if c.epi in (1, 3) else None, dev=dev)
    out = {k: F.ratio(got[k].float(), *ref[k]) for k in ("y", "rn", "img") if k in got}
    out["exact_miss"], out["undecided"] = exact_pin(stored, *ref["y32"]) if stored is not None else (0, 0.0)
    out["kink"] = F.undecided_fraction(*ref["_c"]) if c.epi in (1, 3) else 0.0
    out["sign"] = F.sign_violations(*ref["_c"], stored.float()) if (c.epi in (1, 3) and stored is not None) else 0
    return out


def failures(st):
    """what of a check() result breaks the contract"""
    bad = [(k, st[k]) for k in ("y", "rn", "img") if k in st and not st[k] <= 1.0]
    bad += [(k, st[k]) for k in ("exact_miss", "sign") if st[k]]
    bad += [("undecided", st["undecided"])] if st["undecided"] > UNDECIDED_CAP else []
    return bad + ([("kink", st["kink"])] if st["kink"] > 1e-4 else [])


# ---- emulation ------------------------------------------------------------------------------------------------------------------------
def k_steps(K):
    """[[(tap, first channel, end channel)]] per k-step of 32 contraction indices"""
    if K == 16:
        return [[(t, 0, 16) for t in (2 * s, 2 * s + 1) if t < 9] for s in range(5)]
    if K in TUNED_K:
        return [[(t, 32 * ks, 32 * ks + 32)] for t in range(9) for ks in range(K // 32)]
    return [[(t, 128 * sl + 32 * ks, min(128 * sl + 32 * ks + 32, K))] for sl in range(_cdiv(K, 128)) for t in range(9) for ks in range(4)]


def conv_emulate(xr, wq, bias, fa, defect=None):
    """the fp32 accumulators + bias: xr (B, H, W, K) and wq (N, K, 3, 3) hold bf16 values"""
    B, H, W, K = xr.shape
    N = wq.shape[0]
    xp = np.pad(xr, ((0, 0), (1, 1), (1, 2), (0, 0))).astype(f64)
    w64 = wq.astype(f64)
    acc = np.zeros((B * H * W, N), f32)
    steps = k_steps(K)
    wstep = list(range(len(steps)))
    if defect == "ring_stale":
        assert not fa.WREG and len(steps) > fa.RD, "the defect needs the ring"
        wstep[fa.RD] = 0
    win = lambda dy, dx, lo, hi: xp[:, dy:dy + H, dx:dx + W, lo:hi].reshape(B * H * W, hi - lo)
    for s, step in enumerate(steps):
        tot = acc.astype(f64)
        for (t, lo, hi), (tw, lw, hw) in zip(step, steps[wstep[s]]):
            if lo < hi:
                tot = tot + win(t // 3, t % 3, lo, hi) @ w64[:, lw:hw, tw // 3, tw % 3].T
        if defect == "tap10" and K == 16 and s == 4:
            tot = tot + win(2, 2, 0, 16) @ w64[:, :, 2, 2].T
        if defect == "slice_pad" and s == len(steps) - 1:
            assert K % 128, "the defect needs a padded slice"
            flat = np.concatenate([w64.reshape(-1), np.zeros(9 * 128 * N)])
            k = np.arange(K, _cdiv(K, 128) * 128)
            for t in range(9):
                tot = tot + win(t // 3, t % 3 + 1, 0, K)[:, (k - K) % K] @ flat[(np.arange(N)[:, None] * K + k[None, :]) * 9 + t].T
        acc = tot.astype(f32)
    return (acc + bias).reshape(B, H, W, N)


def _pix_sum(p, ns, one_wave=False):
    """per-pixel sum of per-channel terms (.., N); one_wave: every wave keeps its own partial (returned per channel)"""
    if not ns:
        return _chan_sum(p)
    w = p.shape[-1] // 4
    s = [_chan_sum(p[..., i * w:(i + 1) * w]) for i in range(4)]
    if one_wave:
        return np.repeat(np.stack(s, -1), w, axis=-1)
    return (s[0] + s[1]) + (s[2] + s[3])


def _pn_bwd(g, ay, arn, ns):
    s = _pix_sum(g * ay, ns) * (f32(1) / f32(g.shape[-1]))
    inv_r = (1.0 / arn.astype(f64)).astype(f32)
    return (g - ay * s[..., None]) * inv_r[..., None] * np.where(ay > 0, f32(1), f32(SLOPE)).astype(f32)


def _swap_chunks(c, xr, fa):
    """chunks 0 and 2 (channels 0-7 and 16-23) exchanged in the staged columns of swizzle class 1"""
    P = min(c.K, 128) // 8
    assert P > 2, "the defect needs a swizzled width"
    hx = np.arange(c.W) % fa.TW + 1
    cols = ((hx // (16 // P)) & (P // 2 - 1)) == 1
    out = xr.copy()
    out[:, :, cols, 0:8], out[:, :, cols, 16:24] = xr[:, :, cols, 16:24], xr[:, :, cols, 0:8]
    return out


def emulate(c, mode, defect=None, fa=None):
    """the outputs of the case in the kernel's order: {"c": fp32 pre-epilogue result, "y32": the output before its store, "y": the stored
    bf16 values as fp32, "rn", "img"} numpy.  fa: the facts of another case's instance (a small image evaluated as a large one's kernel would)"""
    d = inputs(c, mode)
    fa = fa or facts_of(c)
    bias = _np(d["bias"]).astype(f32) if d.get("bias") is not None else np.zeros(c.N, f32)
    wq = stored_weight(c, mode, d, defect)
    xr = staged32(c, d, defect)
    if defect == "chunk_swap":
        xr = _swap_chunks(c, xr, fa)
    cc = conv_emulate(xr, wq, bias, fa, defect)
    if defect == "halo":
        x0 = (_cdiv(c.W, fa.TW) - 1) * fa.TW
        assert x0 > 0, "the defect needs a second tile column"
        z = xr.copy()
        z[:, :, x0 - 1] = 0
        cc[:, :, x0] = conv_emulate(z, wq, bias, fa)[:, :, x0]
    store = trunc_bf16 if defect == "trunc_store" else rbf
    out = {"c": cc}
    if c.epi == 0:
        out["y32"] = pool_adjoint_f32(cc, defect) if c.om else cc
    elif c.epi in (1, 3):
        a = np.maximum(cc, f32(SLOPE) * cc)
        ss = _pix_sum(a * a, fa.NS, defect == "norm_wave")
        m = ss * (f32(1) / f32(c.N)) + f32(EPS)
        inv = (1.0 / np.sqrt(m.astype(f64))).astype(f32)
        y = a * (inv if defect == "norm_wave" else inv[..., None])
        rn = (m * inv)[..., 0] if defect == "norm_wave" else m * inv
        if defect == "rn_group":
            rn = rn.copy()
            assert c.W >= fa.TW and (fa.TW == 32 or c.H >= 2), "the defect needs two pixel groups"
            rn[:, 0, 0:16] = rn[:, 0, 16:32] if fa.TW == 32 else rn[:, 1, 0:16]
        out["y32"], out["rn"] = y, rn
        if c.epi == 3:
            out["img"] = np.tanh(_chan_sum(y * _np(d["wimg"])).astype(f64)).astype(f32)
    else:
        g = pool_adjoint_f32(cc, defect) if c.om else cc
        out["y32"] = _pn_bwd(g, _np(d["ay"]), _np(d["arn"]), fa.NS)
    out["y"] = store(out["y32"])
    if c.var == "noy":
        del out["y"], out["rn"]
    return out
