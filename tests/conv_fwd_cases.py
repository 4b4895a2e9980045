"""The forward / input-gradient 3x3 convolutions behind ngan_conv3x3_fwd_ex and ngan_conv3x3_up2_border (csrc/conv3x3_generic.hip, _mid,
_persist, _tile, _wino, _up2f, packed by _pack) at every template instance the launch switches can produce and at the edges of their
tilings: the instance table, a replica of the routing, the case list, fp64 references with their absolute-value twins, the per-element
bound through every epilogue, numpy emulations of the four arithmetic forms and planted defects.  Shared by tests/test_gpu_conv_fwd.py
(the kernels against the references) and tests/test_conv_fwd_bounds_cpu.py (the emulations against the references: the constants are
settled on the CPU, before any kernel is looked at; the replica is checked against the built library there).  Nothing of the package
is imported here.

A case is Case(B, H, W, K, N, res, epi, om, prec, var): H, W are the convolution's own size (its input after resampling); the input x is
(B, H, W, K) for res 0, (B, 2H, 2W, K) for 1 (2x2 average on load), (B, H/2, W/2, K) for 2 (bilinear x2 on load); epi is the epilogue
(0 none, 1 LeakyReLU -> PixelNorm, 2 PixelNorm backward, 3 epilogue 1 + ToImage), om the store (1: pool adjoint, 0.25 c to the 2x2 block
of a (2H, 2W) tensor), prec the precision code of ngan_conv3x3_algorithm (0 exact fp32 direct, 1 split-bf16, 2 split-bf16 with K = 16
padded to 32, 3 bilinear folded into the weights, 4 fp32 Winograd F(2x2, 3x3)), var "" / "noy" (epilogue 3 without a stored y) /
"split" (precision 3 with NGAN_CONV_SKIP_BORDER, then ngan_conv3x3_up2_border) / "onehot" (one product per output element, see inputs()).  Every case runs with the weight in both orientations
ops._packed offers (mode 0: (N, K, 3, 3) forward; mode 1: (K, N, 3, 3), the weight of the convolution being differentiated, taps
flipped; precision 3 packs mode 0 only), with a bias wherever the entry point takes one (not with epilogue 2, nor in the one-product cases), and with the pooled side
output of epilogue 1 wherever ngan_conv3x3_pooled_output says 1.

Instances.  EXPECTED_NAMES is written out from the launch switches, in the text ngan_conv3x3_kernel_name prints:
  conv3x3_kernel<MTW, WN, PGW, PCG, RES, EPI, OUTMODE>   kCfg: 11 distinct tile configurations (N = 16 has one 4x16 entry twice) x the 7
        forms of dispatch_conv2 ((res, epi) in 3 x 2, and the pool-adjoint store)                                                   77
  conv3x3_mid_kernel<KG, PGW, MTW, WN, EPI, OUTMODE, 1, PREC>   mid_launch_kg: KG in {1, 2, 4} x the slice configurations of 32 / 64 /
        128 channels x PREC in {0, 1} x the 5 forms of mid_launch_cfg                                                              90
  conv3x3_persist_kernel<MTW, KG, RES, EPI, OUTMODE, PREC>   (MTW, KG) in {1, 2}^2 x PREC in {0, 1}, and (1, 1) at PREC 2: 9 x the 8
        forms of dispatch_persist2                                                                                                 72
  conv3x3_tile_kernel<MTW, KG, EPI, OUTMODE, PREC>   the same 9 x the 6 forms of dispatch_tile2                                     54
  conv3x3_wino_kernel<KG, MT, ROWS, NWAVES, RES, EPI, OUTMODE>   4 shapes x 2 bilinear forms + 3 shapes x 6 plain forms             26
  conv3x3_up2f_kernel<KG, EPI>                                                                                                       4
together 323.  UNREACHABLE lists what is instantiated and cannot be reached through the two entry points: nothing -- every switch
argument is reachable (the persistent kernel's PREC 0 instances by a precision-0 call, which ops never makes but the C ABI accepts).
Two launches have no name in ngan_conv3x3_kernel_name and are recorded by second_launch(): the border kernel of precision 3 and the
in-place PixelNorm pass behind a channel-split mid launch or behind the generic kernel's epilogue 2.

Bound of the convolution result c = conv + bias, per element:
      e_c = n_round 2^-23 |c| + C_ACC 2^-24 absref (+ SPLIT_TERM absref_direct for the precision codes 1, 2, 3),   C_ACC = 8
  absref_direct   the reference's own sum with absolute values (|scale| sum |x| |w|, a resampled input from |x|), plus |bias|
  absref, direct forms (0, 1, 2)   absref_direct
  absref, Winograd form (4)   |A|^T [ sum_cin (|G| |w| |G|^T) . (|B|^T |d| |B|) ] |A| per 2x2 output tile (even coordinates, zeros outside
        the image, d the resampled input), plus |bias|: the magnitudes its transformed operands reach
  absref, folded bilinear (3)   the four parity weight sets' own terms: W_eff is a sum of W[ky][kx] E[ky][dr] E[kx][dc] with blend
        coefficients E >= 0, which the packing rounds once per fma; the sum of those terms' magnitudes against |x| is, term by term,
        absref_direct with the bilinear resample of |x|.  The border ring is exact fp32 from the unfolded weights: no split term there.
  SPLIT_TERM = 2^-15: derived in tests/wgrad_cases.py (hi / lo by round-to-nearest-even, lo.lo and the two residual cross terms dropped);
        here both operands are split in the same way (the weight by the packing, the input while it is staged)
  n_round (the fp32 roundings applied to an element after its last addition, the rounding of that addition counting as one), from the
  kernel text:
      conv3x3_kernel, conv3x3_mid_kernel, conv3x3_persist_kernel (every PREC), conv3x3_up2f_kernel   acc + bias is the last addition    1
      conv3x3_tile_kernel, conv3x3_wino_kernel   the bias is the accumulators' initial value (Winograd: position (1, 1)); the last
                                                 MFMA (Winograd: the last subtraction of A^T [.] A) is the last addition                 1
      conv3x3_up2_border_kernel                  (c0 + c1) + (c2 + c3) over four fma chains, the bias the start of c0                      1
  The weight's own rounding (w * scale once in fp32; the Winograd packing's G g G^T; the folding's fma chain) and a resampled input's
  blend are per-term roundings of at most 2^-24 of the term each: they belong to the accumulation term, which absref bounds.
Bound through an epilogue: the epilogue's own rounding term (n_round and absref of the same operator in tests/wide_f32_cases.py) plus the
first-order propagation of e_c, in fp64.  m is the LeakyReLU pattern (1 or slope), l = m c, r = sqrt(mean l^2 + eps), y = l / r:
      epilogue 1   y:   4 2^-23 |y| + C_ACC 2^-24 |y| + m e_c / r + |y| sum_j |l_j| m_j e_c,j / (N r^2)
                   rnorm: 4 2^-23 r + C_ACC 2^-24 r + sum_j |l_j| m_j e_c,j / (N r)
      epilogue 2   4 2^-23 |ref| + C_ACC 2^-24 P(|g|) + P(e_c),   P(v) = m_ay (v + |ay| mean(v |ay|)) / arn: pixelnorm_bwd's linear map with
                   absolute values; with out_mode 1, g = 0.25 c on the 2x2 block first (exact) and ay, arn at (2H, 2W)
      epilogue 3   2 2^-23 |t| + C_ACC 2^-24 sum |y| |w| + (1 - t^2) sum_c |w_c| (bound of y_c): tanh within 2 ulp
      out_mode 1   the exact factor 0.25 on every term
      pooled side output of epilogue 1: bit-equal to ngan_pool2_fwd of the stored y (no bound)
LeakyReLU masks are those of the kernel's stored output (tests/lane_group_cases.py), with a condition, not a tolerance: wherever the
fp64 pre-activation has |c| > e_c the stored sign must be the fp64 sign.  The inputs (bias 3 +- 0.5 with the sign changing every two
channels, on pre-activations of standard deviation ~1.4) leave at most 1e-4 of the elements inside |c| <= e_c
(tests/test_conv_fwd_bounds_cpu.py checks it on the fp64 reference alone).  Epilogue 3 without a stored y takes the fp64 pattern.

Emulations (numpy, fp32 where the kernel is fp32), one per arithmetic form -- an element's numerics depend on the form and the contraction
order, not on which tile owns it -- each with the orders the families use:
  direct fp32    v_mfma_f32_16x16x4_f32 steps: per (tap, 16-channel group g) four MFMAs i = 0..3, MFMA i contracting the channels
                 16 g + 4 q + i, q = 0..3; "g_tap" (conv3x3_kernel, conv3x3_mid_kernel: groups outside) or "tap_g" (persist / tile: taps
                 outside); the four products summed exactly and rounded once ("exact") or one fma after the other ("seq"): the rounding
                 inside the MFMA is not documented, both are held to the bound; bias last or first
  split-bf16     hi = rne_bf16(v), lo = rne_bf16(v - hi) of the packed weight w * scale and of the staged (fp32-blended) input; a k-step is
                 32 contraction indices: "pair" (K = 16: two taps per step, the tenth tap zero), "tap" (K = 32, persist / tile) or
                 "kg_tap" (mid: 32-channel groups outside, taps inside; K = 16 padded: 16 real channels per step); per step lo.hi, hi.lo,
                 hi.hi, each summed exactly (the products are exact in fp32, the sum is formed in fp64) and rounded once
  Winograd       G g G^T and * scale as pack_weights_wino_kernel rounds them, B^T d B rows then columns, per position (u, v) the MFMA
                 steps of the direct form over the input channels, A^T [.] A as (m0 + m1) + m2 and (m1 - m2) - m3 on rows then columns;
                 bias at position (1, 1) first (tile, wino) or added last (persist)
  folded         W_eff by the packing's fma chain over (ky, kx), * scale, split; the low-resolution input split once per value, taps
                 clamped; steps as the persistent kernel's; the border ring by conv3x3_up2_border_kernel's four fma chains on the
                 fp32-blended window from the unfolded weights
and the epilogues in fp32 ("sqrt": r = sqrtf, 1 / r, as conv3x3_kernel and conv3x3_mid_kernel; "rsq": the reciprocal square root and
rnorm = m * rsq(m), as the persistent kernels).

Planted defects (`defect=`), each of which tests/test_conv_fwd_bounds_cpu.py shows to miss the bound: "halo" (the left halo column of the
last tile column dropped), "strip" (the last row of the last tile left as the zero it was), "misstore" (one tile's components of one
channel stored at the next tile's offset), "no_lohi" (the lo.hi product dropped; "no_lohi_step": in the last k-step only), "trunc" (a
truncating split: like the rounding one it lacks lo.lo, but its lo reaches 2^-7 of the value, not 2^-8; the sum over a contraction hides
that, one product per element shows it: the ONE_PRODUCT cases), "bias_slice" (bias on the first 32-channel slice only),
"norm_slice" (the PixelNorm sum over the first 32 channels), "clamp" (a bilinear edge tap clamped one pixel off), "border_folded" (the
border ring computed like the interior: clamped taps instead of the convolution's zero padding), "pool_twice" (0.25 applied twice).

RAISED: (form, output) whose emulated worst err / bound exceeds 0.5 with C_ACC = 8, with the next power of two that brings it to 0.5
or below and the emulated ratio there; tests/test_conv_fwd_bounds_cpu.py pins it.  The key's output is "c", the convolution result, whose
constant every output of the case inherits through e_c.  One entry: the direct fp32 form with the MFMA's four products added one fma
after the other ("seq") -- 9 K roundings in sequence, up to 1152, each at the magnitude of the partial sum, which carries the bias from
the start where the bias is the accumulators' initial value -- reaches 1.08 at C_ACC = 8 (32 -> 16, taps outside, bias first) and 0.56 at
16; the "exact" MFMA stays at 0.49 with 8.  Nothing here was fitted to a kernel's result."""
import collections
import functools
import math

import numpy as np
import torch

import fp64_conv
from wgrad_cases import _fma, bf16, bf16_trunc, resample_f32

f32, f64 = np.float32, np.float64
C_ACC = 8.0
SPLIT_TERM = 2.0 ** -15
SLOPE = 0.2
EPS = 1e-8
EPI_NONE, EPI_LRELU_PN, EPI_PN_BWD, EPI_TO_IMAGE = 0, 1, 2, 3
SKIP_BORDER = 1                                        # NGAN_CONV_SKIP_BORDER (include/ngan.h)
FORM = {0: "f32_direct", 1: "bf16x3", 2: "bf16x3", 3: "folded", 4: "f32_winograd"}
# (form, output) -> (raised C_ACC, emulated worst err / bound at that constant)
RAISED = {("f32_direct", "c"): (32.0, 0.285)}

Case = collections.namedtuple("Case", "B H W K N res epi om prec var", defaults=("",))


def c_acc(form, output="c"):
    return float(RAISED.get((form, output), (C_ACC, None))[0])


def case_id(c):
    return "x".join(map(str, c[:9])) + (("-" + c.var) if c.var else "")


def modes(case):
    return (0,) if case.prec == 3 else (0, 1)


# ---- the instance table, written out from the launch switches ----------------------------------------------------------------------
K_CFG = [   # kCfg[mti][ci] = (MTW, WN, PGW, PCG), conv3x3_internal.h
    [(1, 1, 4, 2), (1, 1, 1, 1), (1, 1, 1, 1)],
    [(2, 1, 4, 2), (2, 1, 1, 1), (1, 2, 1, 1)],
    [(4, 1, 4, 2), (2, 2, 2, 1), (1, 4, 1, 1)],
    [(8, 1, 4, 2), (2, 4, 4, 1), (2, 4, 1, 1)],
]
GENERIC_FORMS = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (2, 0, 0), (2, 1, 0), (0, 0, 1)]                 # dispatch_conv2: (RES, EPI, OUTMODE)
MID_FORMS = [(2, 1), (2, 0), (0, 1), (1, 0), (0, 0)]                                                         # mid_launch_cfg: (EPI, OUTMODE)
MID_SLICE_CFG = {32: (2, 1, 2), 64: (2, 2, 2), 128: (4, 2, 4)}                                               # mid_launch_kg: ns -> (PGW, MTW, WN)
PERSIST_FORMS = [(0, 2, 1), (0, 2, 0), (0, 3, 0), (0, 0, 1), (0, 1, 0), (0, 0, 0), (2, 1, 0), (2, 0, 0)]     # dispatch_persist2: (RES, EPI, OUTMODE)
TILE_FORMS = [(2, 1), (2, 0), (3, 0), (0, 1), (1, 0), (0, 0)]                                                # dispatch_tile2: (EPI, OUTMODE)
PERSIST_SHAPES = [(mtw, kg, prec) for mtw in (1, 2) for kg in (1, 2) for prec in (0, 1)] + [(1, 1, 2)]       # dispatch_*_prec
WINO_SHAPES = [(2, 2, 8, 8), (2, 1, 16, 8), (1, 2, 8, 4), (1, 1, 8, 4)]                                     # conv3x3_wino_launch: (KG, MT, ROWS, NWAVES)

EXPECTED_NAMES = set()
for _row in K_CFG:
    for _cfg in set(_row):
        for _f in GENERIC_FORMS:
            EXPECTED_NAMES.add("conv3x3_kernel<%d, %d, %d, %d, %d, %d, %d>" % (_cfg + _f))
for _kg in (1, 2, 4):
    for _ns, _s in MID_SLICE_CFG.items():
        for _prec in (0, 1):
            for _f in MID_FORMS:
                EXPECTED_NAMES.add("conv3x3_mid_kernel<%d, %d, %d, %d, %d, %d, 1, %d>" % ((_kg,) + _s + _f + (_prec,)))
for _mtw, _kg, _prec in PERSIST_SHAPES:
    for _f in PERSIST_FORMS:
        EXPECTED_NAMES.add("conv3x3_persist_kernel<%d, %d, %d, %d, %d, %d>" % ((_mtw, _kg) + _f + (_prec,)))
    for _f in TILE_FORMS:
        EXPECTED_NAMES.add("conv3x3_tile_kernel<%d, %d, %d, %d, %d>" % ((_mtw, _kg) + _f + (_prec,)))
for _s in WINO_SHAPES:
    for _epi in (0, 1):
        EXPECTED_NAMES.add("conv3x3_wino_kernel<%d, %d, %d, %d, 2, %d, 0>" % (_s + (_epi,)))
    if _s[0] * _s[1] > 1:
        for _f in TILE_FORMS:
            EXPECTED_NAMES.add("conv3x3_wino_kernel<%d, %d, %d, %d, 0, %d, %d>" % (_s + _f))
for _kg in (1, 2):
    for _epi in (0, 1):
        EXPECTED_NAMES.add("conv3x3_up2f_kernel<%d, %d>" % (_kg, _epi))
assert len(EXPECTED_NAMES) == 77 + 90 + 72 + 54 + 26 + 4 == 323
# (name, the line that makes it unreachable through ngan_conv3x3_fwd_ex / ngan_conv3x3_up2_border)
UNREACHABLE = []


# ---- replica of the routing (conv3x3_internal.h, conv3x3_mid.hip, conv3x3_api.hip) ----------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def cfg_tile(cfg):
    mtw, wn, pgw, pcg = cfg
    npg = (4 // wn) * pgw
    return npg // pcg, pcg * 16            # (th, tw)


def pick_cfg(mti, B, H, W):
    for i in range(3):
        th, tw = cfg_tile(K_CFG[mti][i])
        nwg = B * _cdiv(H, th) * _cdiv(W, tw)
        if nwg >= 256 and nwg * th * tw / (B * H * W) <= 1.3:
            return i
    return 2


def persist_eligible(B, H, W, K, N, res):
    return N <= 32 and K <= 32 and res != 1 and pick_cfg(N // 16 - 1, B, H, W) == 0


def up2f_eligible(B, H, W, K, N, res):
    return res == 2 and N == 16 and K in (16, 32) and H % 2 == 0 and W % 2 == 0 and H >= 16 and W >= 32 and persist_eligible(B, H, W, K, N, res)


def wino_eligible(B, H, W, K, N, res):
    if res == 1 or not persist_eligible(B, H, W, K, N, res):
        return False
    return (K == 16 and N == 16) or W % 32 == 0


def mid_eligible(K, N):
    return K in (32, 64, 128) and N in (32, 64, 128)


def mid_tiles(B, H, W):
    return B * _cdiv(W, 16) * _cdiv(H, 4)


def mid_slice(n_tiles, N):
    for ns in (N, 64, 32):
        if ns > N or N % ns or ns not in (32, 64, 128):
            continue
        if n_tiles * (N // ns) >= 256:
            return ns
    return 32


def algorithm(B, H, W, K, N, res, precision):
    """ngan_conv3x3_algorithm for the requested arithmetic (0 exact fp32, 1 split-bf16)"""
    if precision == 0:
        return 4 if wino_eligible(B, H, W, K, N, res) else 0
    if precision != 1:
        return 0
    if up2f_eligible(B, H, W, K, N, res):
        return 3
    if persist_eligible(B, H, W, K, N, res) or mid_eligible(K, N):
        return 1
    return 2 if K == 16 and mid_eligible(32, N) else 0


def available(c):
    """the precision test at the head of ngan_conv3x3_fwd_ex"""
    a = (c.B, c.H, c.W, c.K, c.N, c.res)
    return c.prec == 0 or (c.prec == 4 and algorithm(*a, 0) == 4) or (c.prec in (1, 2, 3) and algorithm(*a, 1) == c.prec)


def pooled_output(c):
    return c.prec == 4 and c.H % 2 == 0 and c.W % 32 == 0 and algorithm(c.B, c.H, c.W, c.K, c.N, c.res, 0) == 4


def epilogue_fused(c):
    if c.epi in (0, 1):
        return True
    persist = persist_eligible(c.B, c.H, c.W, c.K, c.N, c.res)
    if c.epi == 3:
        return persist and c.res == 0 and c.om == 0
    k = 32 if c.prec == 2 else c.K
    return c.res == 0 and (persist or (mid_eligible(k, c.N) and mid_slice(mid_tiles(c.B, c.H, c.W), c.N) == c.N))


def route(c):
    """(family, kernel name, second launch or None) as ngan_conv3x3_fwd_ex routes the call"""
    B, H, W, K, N, res, epi, om, prec = c[:9]
    assert available(c), c
    if persist_eligible(B, H, W, K, N, res):
        if prec == 3:
            assert epi in (0, 1) and om == 0
            return "up2f", "conv3x3_up2f_kernel<%d, %d>" % (K // 16, epi), "conv3x3_up2_border_kernel<%d, %d>" % (epi, K)
        tprec = 2 if prec == 4 else prec
        if tprec == 2 and W % 32 == 0 and (K == 32 or N == 32 or res == 2):
            kg, mt = K // 16, N // 16
            rows = 16 if (kg == 2 and mt == 1) else 8
            return "wino", "conv3x3_wino_kernel<%d, %d, %d, %d, %d, %d, %d>" % (kg, mt, rows, 8 if kg == 2 else 4, res, epi, om), None
        if res == 0 and W % 32 == 0:
            return "tile", "conv3x3_tile_kernel<%d, %d, %d, %d, %d>" % (N // 16, K // 16, epi, om, tprec), None
        return "persist", "conv3x3_persist_kernel<%d, %d, %d, %d, %d, %d>" % (N // 16, K // 16, res, epi, om, tprec), None
    if prec >= 1 or (res != 1 and mid_eligible(K, N)):
        k = 32 if prec == 2 else K
        ns = mid_slice(mid_tiles(B, H, W), N)
        fused = epi == 0 or ns == N
        e = epi if fused else 0
        second = None if fused else ("ngan_lrelu_pixelnorm_fwd" if epi == 1 else "ngan_lrelu_pixelnorm_bwd")
        return "mid", "conv3x3_mid_kernel<%d, %d, %d, %d, %d, %d, 1, %d>" % ((k // 32,) + MID_SLICE_CFG[ns] + (e, om, 1 if prec else 0)), second
    cfg = K_CFG[{16: 0, 32: 1, 64: 2, 128: 3}[N]][pick_cfg({16: 0, 32: 1, 64: 2, 128: 3}[N], B, H, W)]
    e = 0 if epi == 2 else epi
    return "generic", "conv3x3_kernel<%d, %d, %d, %d, %d, %d, %d>" % (cfg + (res, e, om)), ("ngan_lrelu_pixelnorm_bwd" if epi == 2 else None)


def kernel_name(c):
    return route(c)[1]


def second_launch(c):
    return route(c)[2]


def tile_of(c):
    """(th, tw) of the tiling the case's kernel walks"""
    fam, name, _ = route(c)
    if fam == "generic":
        return cfg_tile(K_CFG[{16: 0, 32: 1, 64: 2, 128: 3}[c.N]][pick_cfg({16: 0, 32: 1, 64: 2, 128: 3}[c.N], c.B, c.H, c.W)])
    if fam == "mid":
        return 4, 16
    if fam == "wino":
        return (16 if (c.K == 32 and c.N == 16) else 8), 32
    if fam == "up2f":
        return 8, 32
    mtw, kg = c.N // 16, c.K // 16              # persist_tile_h
    return (4 if (mtw * kg == 4 or (kg == 2 and c.res == 2 and fam == "persist")) else 8), 32


def n_tiles(c):
    th, tw = tile_of(c)
    return c.B * _cdiv(c.H, th) * _cdiv(c.W, tw)


# ---- the case list -----------------------------------------------------------------------------------------------------------------
BIG_RAGGED = (2, 60, 500)        # 2 x 8 x 16 = 256 tiles of 8x32, ragged right (500 = 15 x 32 + 20) and bottom (60 = 7 x 8 + 4)
BIG_WHOLE = (2, 60, 512)         # W % 32 == 0 (tile / Winograd kernels), ragged bottom
BIG_SQUARE = (4, 64, 256)        # whole tiles both ways
ONE_TILE = (256, 8, 32)          # an image of exactly one 8x32 tile
SUB_TILE = (256, 7, 30)          # an image smaller than a tile both ways (the 8x32 configurations are chosen only up to 1.3 waste)
SUB_TILE_EVEN = (256, 8, 26)     # ... with even sides, for a bilinear input
NO_UP2F = (16, 14, 500)          # H < 16: bilinear input at N = 16 stays on the persistent kernel in split-bf16
WALK_RAGGED = (5, 110, 470)      # 5 x 14 x 15 = 1050 tiles of 8x32 > the 1024 workgroups that can be resident: several tiles per workgroup
WALK_WHOLE = (5, 110, 480)
WALK_ROWS16 = (70, 8, 480)       # 70 x 1 x 15 = 1050 tiles of the 16-row Winograd instance too (each half empty)
MEDIUM = (4, 30, 140)            # 4 x 8 x 9 = 288 tiles of 4x16 (ragged both ways), 80 of 8x32: the 4x16 configurations, whole-N mid slices
HALF = (2, 30, 140)              # 144 tiles of 4x16: N = 128 in two slices of 64
MID_FULL = [MEDIUM, (64, 5, 20), (256, 4, 16), (256, 1, 1), (256, 2, 2)]      # >= 256 tiles of 4x16: ragged, one tile, sub-tile, every tap clamped
SMALL = [(1, 1, 1), (2, 5, 20), (3, 7, 33), (1, 4, 16), (2, 1, 16), (2, 2, 2), (1, 2, 16), (2, 6, 2), (2, 4, 34)]
SMALL_EVEN = [s for s in SMALL if s[1] % 2 == 0 and s[2] % 2 == 0]
_MTI = {16: 0, 32: 1, 64: 2, 128: 3}


def _cyc(seq, i):
    return seq[i % len(seq)]


def _generic_cases():
    out, i = [], 0
    for N in (16, 32, 64, 128):
        for ci in (0, 1, 2):
            for res, epi, om in GENERIC_FORMS + [(0, 2, 0), (0, 2, 1)]:
                i += 1
                if ci == 0:
                    shape = _cyc([BIG_RAGGED, BIG_WHOLE, ONE_TILE, SUB_TILE_EVEN if res == 2 else SUB_TILE], i)
                    K = 16 if res == 1 else _cyc([48, 80], i)          # K <= 32 with a plain or bilinear input is the persistent family's
                elif ci == 1:
                    shape, K = MEDIUM, _cyc([16, 48, 80], i)
                else:
                    shape, K = _cyc(SMALL_EVEN if res == 2 else SMALL, i), _cyc([16, 48, 80], i)
                out.append(Case(*shape, K, N, res, epi, om, 0))
    return out


def _mid_cases():
    out, i = [], 0
    for prec in (0, 1, 2):
        for K in ((16,) if prec == 2 else (32, 64, 128)):
            for ns in (32, 64, 128):
                for epi, om in MID_FORMS:              # all channels in one workgroup: N = ns
                    i += 1
                    plain = epi == 2 or om == 1
                    res = 0 if plain else _cyc((0, 2) if prec == 0 else (0, 1, 2), i)
                    pool = [s for s in (SMALL + MID_FULL if ns == 32 else MID_FULL) if res != 2 or (s[1] % 2 == 0 and s[2] % 2 == 0)]
                    out.append(Case(*_cyc(pool, i), K, ns, res, epi, om, prec))
            for N, shape in ((64, SMALL[1]), (128, SMALL[2]), (128, HALF)):      # channels split over workgroups: slices of 32, 32, 64
                for epi, om in ((0, 0), (1, 0), (2, 0), (2, 1)):
                    out.append(Case(*shape, K, N, 0, epi, om, prec))
    return out


def _persist_cases():
    out, i = [], 0
    for mtw, kg, tprec in PERSIST_SHAPES:
        K, N, prec = kg * 16, mtw * 16, (4 if tprec == 2 else tprec)
        for res, epi, om in PERSIST_FORMS:
            i += 1
            if res == 2:
                shape = NO_UP2F if (prec == 1 and N == 16) else _cyc([BIG_RAGGED, BIG_WHOLE] if prec == 0 else [BIG_RAGGED], i)
            else:
                shape = _cyc([BIG_RAGGED, SUB_TILE], i)
            out.append(Case(*shape, K, N, res, epi, om, prec))
        out.append(Case(*BIG_RAGGED, K, N, 0, 3, 0, prec, "noy"))
        for epi, om in TILE_FORMS:
            i += 1
            out.append(Case(*_cyc([BIG_WHOLE, ONE_TILE, BIG_SQUARE], i), K, N, 0, epi, om, prec))
    return out


def _wino_cases():
    out, i = [], 0
    for kg, mt, rows, nw in WINO_SHAPES:
        for epi in (0, 1):
            i += 1
            out.append(Case(*_cyc([BIG_WHOLE, BIG_SQUARE, ONE_TILE], i), kg * 16, mt * 16, 2, epi, 0, 4))
        if kg * mt > 1:
            for epi, om in TILE_FORMS:
                i += 1
                out.append(Case(*_cyc([BIG_WHOLE, BIG_SQUARE, ONE_TILE], i), kg * 16, mt * 16, 0, epi, om, 4))
    return out


def _up2f_cases():
    out = []
    for K in (16, 32):
        for epi in (0, 1):
            for j, shape in enumerate([BIG_RAGGED, (2, 64, 512), (16, 16, 256)]):
                out.append(Case(*shape, K, 16, 2, epi, 0, 3, "split" if (j + epi) % 2 else ""))
            out.append(Case(*BIG_RAGGED, K, 16, 2, epi, 0, 3, "" if epi else "split"))
    return list(dict.fromkeys(out))


# several tiles per workgroup, one per persistent family and arithmetic; the step of the walk (grid / 8) is no multiple of tiles_x = 15
WALK = [Case(*WALK_RAGGED, 16, 16, 0, 1, 0, 0), Case(*WALK_RAGGED, 16, 16, 0, 0, 0, 1), Case(*WALK_RAGGED, 16, 16, 2, 1, 0, 4),
        Case(*WALK_RAGGED, 32, 32, 0, 0, 0, 1),
        Case(*WALK_WHOLE, 16, 16, 0, 0, 0, 0), Case(*WALK_WHOLE, 16, 16, 0, 1, 0, 1), Case(*WALK_WHOLE, 16, 16, 0, 1, 0, 4),
        Case(*WALK_WHOLE, 32, 32, 0, 1, 0, 4), Case(*WALK_ROWS16, 32, 16, 0, 0, 0, 4),
        Case(*WALK_RAGGED, 16, 16, 2, 1, 0, 3), Case(*WALK_RAGGED, 32, 16, 2, 0, 0, 3)]
# one product per output element (var "onehot", see inputs()): where a truncating hi / lo split shows.  One per split-bf16 family and
# k-step layout that the entry point reaches: mid at K = 32, 64 and the padded K = 16 on 1 x 1 images, persist and tile at K = 16 and 32,
# the persistent kernel's bilinear input, the folded kernel at K = 16 and 32
ONE_PRODUCT = [Case(256, 1, 1, 32, 32, 0, 0, 0, 1, "onehot"), Case(256, 1, 1, 64, 64, 0, 0, 0, 1, "onehot"), Case(256, 1, 1, 16, 32, 0, 0, 0, 2, "onehot"),
               Case(*BIG_RAGGED, 16, 16, 0, 0, 0, 1, "onehot"), Case(*BIG_RAGGED, 32, 32, 0, 0, 0, 1, "onehot"),
               Case(*BIG_WHOLE, 16, 16, 0, 0, 0, 1, "onehot"), Case(*BIG_WHOLE, 32, 16, 0, 0, 0, 1, "onehot"),
               Case(*NO_UP2F, 16, 16, 2, 0, 0, 1, "onehot"),
               Case(*BIG_RAGGED, 16, 16, 2, 0, 0, 3, "onehot"), Case(*BIG_RAGGED, 32, 16, 2, 0, 0, 3, "onehot")]
GENERIC, MID, PERSIST, WINO, UP2F = _generic_cases(), _mid_cases(), _persist_cases(), _wino_cases(), _up2f_cases()
CASES = list(dict.fromkeys(GENERIC + MID + PERSIST + WINO + UP2F + WALK + ONE_PRODUCT))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def x_shape(c):
    return (c.B, 2 * c.H, 2 * c.W, c.K) if c.res == 1 else (c.B, c.H // 2, c.W // 2, c.K) if c.res == 2 else (c.B, c.H, c.W, c.K)


def y_shape(c):
    return (c.B, 2 * c.H, 2 * c.W, c.N) if c.om else (c.B, c.H, c.W, c.N)


def scale_of(c):
    return float(f32(1.3868 / math.sqrt(9 * c.K)))


def has_bias(c):
    return c.epi != 2 and c.var != "onehot"


@functools.lru_cache(maxsize=2)
def inputs(c, mode):
    """fp32 torch tensors on the CPU: x, w (mode 0: (N, K, 3, 3); mode 1: (K, N, 3, 3)), bias or None, and per epilogue ay / arn (2) or
    wimg (3)"""
    seed = 11 + mode
    for v in c[:9]:
        seed = (seed * 131 + v) % (2 ** 31 - 1)
    gen = torch.Generator().manual_seed(seed)
    d = dict(x=torch.randn(*x_shape(c), generator=gen), w=torch.randn(*((c.N, c.K) if mode == 0 else (c.K, c.N)), 3, 3, generator=gen), bias=None)
    if has_bias(c):
        sign = torch.tensor([1.0 if (ch // 2) % 2 == 0 else -1.0 for ch in range(c.N)])
        d["bias"] = 3.0 * sign + 0.5 * torch.randn(c.N, generator=gen)
    if c.epi == 2:
        d["ay"] = torch.randn(*y_shape(c), generator=gen)
        d["arn"] = torch.rand(*y_shape(c)[:3], generator=gen) + 0.5
    if c.epi == 3:
        d["wimg"] = torch.randn(c.N, generator=gen)
    if c.var == "onehot":
        # one product per output element: x lives in channel 0 with values over (1, 1 + 2^-7) -- every remainder a bf16 split can
        # leave, up to the 2^-7 of a truncating one -- the weight in the centre tap, no bias.  Bilinear input: x on the even-even
        # lattice only, so that the 2 x 2 low-resolution taps of an output pixel hold one non-zero value
        x = torch.zeros(*x_shape(c))
        x[..., 0] = 1 + 2.0 ** -7 * torch.rand(*x_shape(c)[:3], generator=gen)
        if c.res == 2:
            lattice = torch.zeros(x.shape[1], x.shape[2])
            lattice[0::2, 0::2] = 1
            x = x * lattice[None, :, :, None]
        w = torch.zeros_like(d["w"])
        w[:, :, 1, 1] = d["w"][:, :, 1, 1]
        d["x"], d["w"] = x, w
    return d


def w_eff(w, mode):
    """(N, K, 3, 3): the weight the convolution applies"""
    return w if mode == 0 else w.flip(2, 3).transpose(0, 1)


# ---- references -----------------------------------------------------------------------------------------------------------------------
_AT = [[1, 1, 1, 0], [0, 1, 1, 1]]                                       # |A^T|, A^T = [1 1 1 0; 0 1 -1 -1]
_BT = [[1, 0, 1, 0], [0, 1, 1, 0], [0, 1, 1, 0], [0, 1, 0, 1]]           # |B^T|
_G = [[1, 0, 0], [.5, .5, .5], [.5, .5, .5], [0, 0, 1]]                  # |G|


def winograd_absref(xr_abs, w_abs):
    """|A|^T [ sum_cin (|G| |w| |G|^T) . (|B|^T |d| |B|) ] |A| per 2x2 output tile: xr_abs (B, H, W, K) >= 0 the resampled input's
    magnitudes, w_abs (N, K, 3, 3) >= 0 (scale included) -> (B, H, W, N), fp64 torch on the operands' device"""
    B, H, W, K = xr_abs.shape
    N = w_abs.shape[0]
    dev, dt = xr_abs.device, xr_abs.dtype
    He, We = H + H % 2, W + W % 2
    d = torch.zeros(B, He + 2, We + 2, K, dtype=dt, device=dev)
    d[:, 1:H + 1, 1:W + 1] = xr_abs
    G = torch.tensor(_G, dtype=dt, device=dev)
    U = torch.einsum("ur,nkrs,vs->uvnk", G, w_abs, G)
    rows = [d[:, r:r + He:2] for r in range(4)]
    tr = [sum(_BT[u][r] * rows[r] for r in range(4) if _BT[u][r]) for u in range(4)]
    out = torch.zeros(B, He, We, N, dtype=dt, device=dev)
    M = [[None] * 4 for _ in range(4)]
    for u in range(4):
        for v in range(4):
            V = sum(_BT[v][c] * tr[u][:, :, c:c + We:2] for c in range(4) if _BT[v][c])
            M[u][v] = V @ U[u, v].t()
    for a in range(2):
        for b in range(2):
            out[:, a::2, b::2] = sum(M[u][v] for u in range(4) for v in range(4) if _AT[a][u] and _AT[b][v])
    return out[:, :H, :W]


def interior_mask(c, dev="cpu"):
    m = torch.zeros(c.H, c.W, dtype=torch.bool, device=dev)
    m[1:-1, 1:-1] = True
    return m


def conv_reference(c, mode, d, dev="cpu"):
    """(c64, e_c, absref) of the pre-epilogue result conv + bias, (B, H, W, N) fp64 on `dev`"""
    x, w = d["x"].to(dev).double(), w_eff(d["w"], mode).to(dev).double()
    bias = d["bias"].to(dev).double() if d.get("bias") is not None else None
    sc = scale_of(c)
    xr = fp64_conv.resample(x, c.res)
    c64 = fp64_conv.conv3x3(xr, w, sc, 0, bias)
    xa = fp64_conv.resample(x.abs(), c.res)
    direct = fp64_conv.conv3x3(xa, w.abs(), abs(sc), 0, bias.abs() if bias is not None else None)
    form = FORM[c.prec]
    if form == "f32_winograd":
        absref = winograd_absref(xa, w.abs() * abs(sc))
        if bias is not None:
            absref = absref + bias.abs()
    else:
        absref = direct
    e_c = 2.0 ** -23 * c64.abs() + c_acc(form) * 2.0 ** -24 * absref
    if c.prec in (1, 2):
        e_c = e_c + SPLIT_TERM * direct
    elif c.prec == 3:
        e_c = e_c + SPLIT_TERM * direct * interior_mask(c, dev)[None, :, :, None]
    return c64, e_c, absref


def _pn_bwd_map(v, ay_abs, m, arn):
    return m * (v + ay_abs * (v * ay_abs).mean(-1, keepdim=True)) / arn.unsqueeze(-1)


def reference(c, mode, d, stored_y=None, dev="cpu", pre=None):
    """{output: (ref, bound)} fp64 torch on `dev` for the outputs y / rn / img of the case, plus "_c": (c64, e_c) of the pre-activation.
    stored_y: the output under test (its LeakyReLU pattern is used, epilogues 1 and 3); None: the fp64 pattern.  pre: (c64, e_c) in
    place of conv_reference's (part A of the split-bf16 settlement: the three products' exact sum and the bound without the split term)"""
    c64, e_c = pre if pre is not None else conv_reference(c, mode, d, dev)[:2]
    ca, u23, u24 = C_ACC, 2.0 ** -23, 2.0 ** -24          # the epilogue's own terms keep C_ACC = 8: a raise of "c" reaches them through e_c only
    out = {"_c": (c64, e_c)}
    if c.epi == 0:
        ref, bound = c64, e_c
        if c.om:
            ref, bound = fp64_conv.pool_adjoint(ref), fp64_conv.pool_adjoint(bound)
        out["y"] = (ref, bound)
    elif c.epi in (1, 3):
        pos = (stored_y.to(dev) > 0) if stored_y is not None else (c64 > 0)
        m = torch.where(pos, torch.ones_like(c64), torch.full_like(c64, SLOPE))
        l = m * c64
        r = torch.sqrt((l * l).mean(-1, keepdim=True) + EPS)
        y = l / r
        e_l = m * e_c
        dr = (l.abs() * e_l).mean(-1, keepdim=True) / r
        by = 4 * u23 * y.abs() + ca * u24 * y.abs() + e_l / r + y.abs() * dr / r
        out["y"] = (y, by)
        out["rn"] = (r[..., 0], (4 * u23 * r + ca * u24 * r + dr)[..., 0])
        if c.epi == 3:
            wimg = d["wimg"].to(dev).double()
            t, ta = fp64_conv.to_image(y, wimg)
            out["img"] = (t, 2 * u23 * t.abs() + ca * u24 * ta + (1 - t * t) * (by * wimg.abs()).sum(-1))
    else:
        g, e_g = (fp64_conv.pool_adjoint(c64), fp64_conv.pool_adjoint(e_c)) if c.om else (c64, e_c)
        ay, arn = d["ay"].to(dev).double(), d["arn"].to(dev).double()
        m = torch.where(ay > 0, torch.ones_like(ay), torch.full_like(ay, SLOPE))
        ref = fp64_conv.pixelnorm_bwd(g, ay, arn, SLOPE)
        out["y"] = (ref, 4 * u23 * ref.abs() + ca * u24 * _pn_bwd_map(g.abs(), ay.abs(), m, arn) + _pn_bwd_map(e_g, ay.abs(), m, arn))
    return out


def ratio(got, ref, bound):
    """worst |got - ref| / bound over the elements (nan if an element is NaN)"""
    got = got.to(ref.device).double()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    r = (got - ref).abs() / (bound + 1e-30)
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


def sign_violations(c64, e_c, stored_y):
    """elements whose fp64 pre-activation is outside |c| <= e_c and whose stored sign is not the fp64 sign"""
    sure = c64.abs() > e_c
    return int((sure & ((stored_y.to(c64.device) > 0) != (c64 > 0))).sum())


def undecided_fraction(c64, e_c):
    return float((c64.abs() <= e_c).double().mean())


# ---- emulation: operands --------------------------------------------------------------------------------------------------------------
def _np(t):
    return np.ascontiguousarray(t.detach().cpu().numpy())


def _w32(c, mode, d):
    """the packed weight's value: fp32(w * scale), (N, K, 3, 3)"""
    return (_np(w_eff(d["w"], mode)) * f32(scale_of(c))).astype(f32)


def _xr32(c, d, defect=None):
    """the staged input: resampled in fp32 as the kernels blend it, (B, H, W, K)"""
    x = _np(d["x"])
    if defect == "clamp" and c.res == 2:
        good = resample_f32(x, 2, c.H, c.W)
        bad = resample_f32(np.concatenate([x[:, :-1], x[:, -2:-1]], 1), 2, c.H, c.W)
        return np.concatenate([good[:, :-1], bad[:, -1:]], 1)
    return resample_f32(x, c.res, c.H, c.W)


def _pad(xr):
    return np.pad(xr, ((0, 0), (1, 1), (1, 1), (0, 0)))


def _bias32(c, d, defect=None):
    if d.get("bias") is None:
        return np.zeros(c.N, f32)
    b = _np(d["bias"]).astype(f32)
    if defect == "bias_slice":
        b = b.copy()
        b[32:] = 0
    return b


# ---- emulation: the four arithmetic forms -----------------------------------------------------------------------------------------------
def conv_direct_f32(xr, w32, bias, order="g_tap", mfma="exact", bias_first=False):
    """direct fp32 on v_mfma_f32_16x16x4_f32: (B, H, W, N) fp32"""
    B, H, W, K = xr.shape
    N = w32.shape[0]
    xp = _pad(xr)
    acc = np.broadcast_to(bias if bias_first else np.zeros(N, f32), (B * H * W, N)).astype(f32)
    G = K // 16
    steps = [(g, t) for g in range(G) for t in range(9)] if order == "g_tap" else [(g, t) for t in range(9) for g in range(G)]
    for g, tap in steps:
        dy, dx = divmod(tap, 3)
        xs = xp[:, dy:dy + H, dx:dx + W, 16 * g:16 * g + 16].reshape(-1, 16)
        ws = w32[:, 16 * g:16 * g + 16, dy, dx]                            # (N, 16)
        for i in range(4):
            idx = [4 * q + i for q in range(4)]
            if mfma == "exact":
                acc = (acc.astype(f64) + xs[:, idx].astype(f64) @ ws[:, idx].astype(f64).T).astype(f32)
            else:
                for k in idx:
                    acc = _fma(xs[:, k:k + 1], ws[None, :, k], acc)
    return (acc if bias_first else acc + bias).reshape(B, H, W, N)


def _split(a, defect=None):
    hi = (bf16_trunc if defect == "trunc" else bf16)(a)
    return hi, bf16((a - hi).astype(f32))


def _bf16x3_steps(K, layout):
    """[(tap, channel slice)] per k-step"""
    if layout == "pair":
        assert K == 16
        return [[(t, slice(0, 16)) for t in (2 * s, 2 * s + 1) if t < 9] for s in range(5)]
    if layout == "tap":
        return [[(t, slice(0, K))] for t in range(9)]
    return [[(t, slice(32 * kg, min(32 * kg + 32, K)))] for kg in range(_cdiv(K, 32)) for t in range(9)]


def conv_bf16x3(xp_hi, xp_lo, w_hi, w_lo, bias, H, W, layout, defect=None):
    """split-bf16 accumulation over padded operand planes (B, H + 2, W + 2, K): lo.hi, hi.lo, hi.hi per k-step, each an exact sum
    rounded once into the fp32 accumulator; weights (N, K, 3, 3) planes; bias added last"""
    B, K, N = xp_hi.shape[0], xp_hi.shape[3], w_hi.shape[0]
    acc = np.zeros((B * H * W, N), f32)
    products = [(w_lo, xp_hi), (w_hi, xp_lo), (w_hi, xp_hi)]
    if defect == "no_lohi":
        products = products[1:]
    steps = _bf16x3_steps(K, layout)
    for step in steps:
        for wpl, xpl in (products[1:] if (defect == "no_lohi_step" and step is steps[-1]) else products):
            s = acc.astype(f64)
            for tap, ch in step:
                dy, dx = divmod(tap, 3)
                s = s + xpl[:, dy:dy + H, dx:dx + W, ch].reshape(B * H * W, -1).astype(f64) @ wpl[:, ch, dy, dx].astype(f64).T
            acc = s.astype(f32)
    return (acc + bias).reshape(B, H, W, N)


def conv_split_bf16(xr, w32, bias, layout, defect=None):
    xh, xl = _split(_pad(xr), defect)
    wh, wl = _split(w32, defect)
    return conv_bf16x3(xh, xl, wh, wl, bias, xr.shape[1], xr.shape[2], layout, defect)


def wino_weights(w_eff32, scale):
    """G g G^T * scale as pack_weights_wino_kernel rounds it: (4, 4, N, K) fp32 from the unscaled (N, K, 3, 3)"""
    g = w_eff32.astype(f32)
    h = f32(0.5)
    row = [g[:, :, 0], h * ((g[:, :, 0] + g[:, :, 1]) + g[:, :, 2]), h * ((g[:, :, 0] - g[:, :, 1]) + g[:, :, 2]), g[:, :, 2]]       # (N, K, 3) each
    U = np.empty((4, 4) + g.shape[:2], f32)
    for u in range(4):
        r = row[u]
        vals = [r[:, :, 0], h * ((r[:, :, 0] + r[:, :, 1]) + r[:, :, 2]), h * ((r[:, :, 0] - r[:, :, 1]) + r[:, :, 2]), r[:, :, 2]]
        for v in range(4):
            U[u, v] = vals[v] * f32(scale)
    return U


def conv_winograd_f32(xr, U, bias, mfma="exact", bias_first=True):
    """fp32 Winograd F(2x2, 3x3) forward in the kernels' operation order: (B, H, W, N) fp32"""
    B, H, W, K = xr.shape
    N = U.shape[2]
    He, We = H + H % 2, W + W % 2
    d = np.zeros((B, He + 2, We + 2, K), f32)
    d[:, 1:H + 1, 1:W + 1] = xr
    r = [d[:, k:k + He:2] for k in range(4)]
    bd = [r[0] - r[2], r[1] + r[2], r[2] - r[1], r[1] - r[3]]
    T = B * (He // 2) * (We // 2)
    ta = [[None] * 4 for _ in range(2)]
    for v in range(4):
        m = []
        for u in range(4):
            cc = [bd[u][:, :, k:k + We:2] for k in range(4)]
            vv = (cc[0] - cc[2], cc[1] + cc[2], cc[2] - cc[1], cc[1] - cc[3])[v].reshape(T, K)
            acc = np.broadcast_to(bias if (bias_first and u == 1 and v == 1) else np.zeros(N, f32), (T, N)).astype(f32)
            for g in range(K // 16):
                for i in range(4):
                    idx = [16 * g + 4 * q + i for q in range(4)]
                    if mfma == "exact":
                        acc = (acc.astype(f64) + vv[:, idx].astype(f64) @ U[u, v][:, idx].astype(f64).T).astype(f32)
                    else:
                        for k in idx:
                            acc = _fma(vv[:, k:k + 1], U[u, v][None, :, k], acc)
            m.append(acc)
        ta[0][v] = (m[0] + m[1]) + m[2]
        ta[1][v] = (m[1] - m[2]) - m[3]
    out = np.empty((B, He, We, N), f32)
    for a in range(2):
        out[:, a::2, 0::2] = ((ta[a][0] + ta[a][1]) + ta[a][2]).reshape(B, He // 2, We // 2, N)
        out[:, a::2, 1::2] = ((ta[a][1] - ta[a][2]) - ta[a][3]).reshape(B, He // 2, We // 2, N)
    out = out[:, :H, :W]
    return out if bias_first else out + bias


_E = np.array([[.75, .25, 0], [.25, .75, 0], [0, .75, .25], [0, .25, .75]], f32)       # up2_blend: [parity + k][d]


def folded_weights(w_eff32, scale):
    """W_eff[set] * scale by the packing's fma chain: (4, N, K, 3, 3) fp32 from the unscaled (N, K, 3, 3); set = 2 py + px, taps (dr, dc)"""
    out = np.zeros((4,) + w_eff32.shape, f32)
    for s in range(4):
        py, px = s >> 1, s & 1
        for dr in range(3):
            for dc in range(3):
                v = np.zeros(w_eff32.shape[:2], f32)
                for ky in range(3):
                    for kx in range(3):
                        v = _fma(w_eff32[:, :, ky, kx], np.full(v.shape, _E[py + ky, dr] * _E[px + kx, dc], f32), v)
                out[s, :, :, dr, dc] = v * f32(scale)
    return out


def conv_folded(c, mode, d, defect=None):
    """precision 3: the interior by the folded split-bf16 form, the border ring by conv3x3_up2_border_kernel's fma chains: (B, H, W, N)"""
    x = _np(d["x"])
    B, h, w, K = x.shape
    H, W, N = c.H, c.W, c.N
    bias = _bias32(c, d)
    wf = folded_weights(_np(w_eff(d["w"], mode)).astype(f32), scale_of(c))
    xe = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")                     # clamped taps
    xh, xl = _split(xe, defect)
    out = np.empty((B, H, W, N), f32)
    for s in range(4):
        wh, wl = _split(wf[s], defect)
        out[:, (s >> 1)::2, (s & 1)::2] = conv_bf16x3(xh, xl, wh, wl, bias, h, w, "pair" if K == 16 else "tap", defect)
    if defect == "border_folded":
        return out
    # border ring: u = the 3x3 window of the fp32-blended input (zeros outside), t = tap * K + k in four interleaved fma chains
    up = _pad(resample_f32(x, 2, H, W))
    w32 = _w32(c, mode, d)
    ring = np.zeros((H, W), bool)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
    ys, xs = np.nonzero(ring)
    cs = [np.broadcast_to(bias, (B, len(ys), N)).astype(f32)] + [np.zeros((B, len(ys), N), f32) for _ in range(3)]
    for tap in range(9):
        dy, dx = divmod(tap, 3)
        win = up[:, ys + dy, xs + dx]                                                  # (B, P, K)
        for k in range(K):
            j = (tap * K + k) % 4
            cs[j] = _fma(win[:, :, k:k + 1], w32[None, None, :, k, dy, dx], cs[j])
    out[:, ys, xs] = (cs[0] + cs[1]) + (cs[2] + cs[3])
    return out


# ---- emulation: epilogues -------------------------------------------------------------------------------------------------------------
def _chan_sum(p):
    """sum over the channels of per-channel terms (.., N): per 16-channel tile and lane quad ((a + b) + c) + d, the tiles of a lane in
    order, then the four quads pairwise (two shuffles)"""
    sh = p.shape[:-1]
    t = p.reshape(sh + (-1, 4, 4))                                                    # (mt, q, 4)
    f4 = ((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]                            # (mt, q)
    s = np.zeros(sh + (4,), f32)
    for mt in range(f4.shape[-2]):
        s = s + f4[..., mt, :]
    return (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])


def epilogue_lrelu_pn(cc, variant="sqrt", defect=None):
    """(y, rn) fp32 of epilogue 1 on the pre-activation cc (.., N)"""
    N = cc.shape[-1]
    a = np.where(cc > 0, cc, f32(SLOPE) * cc).astype(f32)
    sq = a * a
    if defect == "norm_slice":
        ss, inv_n = _chan_sum(sq[..., :32]), f32(1) / f32(32)
    else:
        ss, inv_n = _chan_sum(sq), f32(1) / f32(N)
    m = ss * inv_n + f32(EPS)
    if variant == "sqrt":
        r = np.sqrt(m)
        inv = f32(1) / r
    else:
        inv = (1.0 / np.sqrt(m.astype(f64))).astype(f32)
        r = m * inv
    return a * inv[..., None], r


def epilogue_pn_bwd(g, ay, arn):
    N = g.shape[-1]
    s = _chan_sum(g * ay) * (f32(1) / f32(N))
    inv_r = f32(1) / arn
    return (g - ay * s[..., None]) * inv_r[..., None] * np.where(ay > 0, f32(1), f32(SLOPE)).astype(f32)


def pool_adjoint_f32(v, defect=None):
    q = v * f32(0.25)
    if defect == "pool_twice":
        q = q * f32(0.25)
    return q.repeat(2, axis=1).repeat(2, axis=2)


# ---- emulation: a whole case ----------------------------------------------------------------------------------------------------------
def family_orders(c):
    """the (order / layout, bias_first, epilogue variant) the case's kernel family uses"""
    fam = route(c)[0]
    if fam == "generic":
        return "g_tap", False, "sqrt"
    if fam == "mid":
        return ("g_tap" if c.prec == 0 else "kg_tap"), False, "sqrt"
    if fam == "up2f":
        return ("pair" if c.K == 16 else "tap"), False, "rsq"
    first = fam in ("tile", "wino")
    if c.prec == 0:
        return "tap_g", first, "rsq"
    if c.prec == 1:
        return ("pair" if c.K == 16 else "tap"), first, "rsq"
    return "wino", first, "rsq"


def _tile_defects(c, out, defect, recompute, tile):
    """the store / staging defects on the pre-epilogue result out (B, H, W, N); recompute(zero_col) gives the result with one input column zeroed"""
    if defect not in ("halo", "strip", "misstore"):
        return out
    th, tw = tile
    x0 = (_cdiv(c.W, tw) - 1) * tw
    y0 = (_cdiv(c.H, th) - 1) * th
    if defect == "halo":
        assert x0 > 0, "the defect needs a second tile column"
        out = out.copy()
        out[:, :, x0] = recompute(x0 - 1)[:, :, x0]
    elif defect == "strip":
        out = out.copy()
        out[-1, c.H - 1, x0:] = 0
    elif defect == "misstore":
        assert x0 >= tw, "the defect needs two tiles in a row"
        out = out.copy()
        n = min(tw, c.W - x0)
        out[-1, y0, x0:x0 + n, 3] = out[-1, y0, x0 - tw:x0 - tw + n, 3]
    return out


def emulate(c, mode, mfma="exact", defect=None, orders=None, tile=None):
    """the outputs of the case as its kernel family computes them: {"c": pre-epilogue result, "y", "rn", "img"} fp32 numpy.  orders, tile:
    those of another case's family (family_orders, tile_of) -- a small image evaluated in the order a large one's kernel uses"""
    d = inputs(c, mode)
    order, bias_first, variant = orders or family_orders(c)
    bias = _bias32(c, d, defect)

    def conv(zero_col=None):
        if c.prec == 3:
            assert zero_col is None
            return conv_folded(c, mode, d, defect)
        xr = _xr32(c, d, defect)
        if zero_col is not None:
            xr = xr.copy()
            xr[:, :, zero_col] = 0
        if c.prec == 0:
            return conv_direct_f32(xr, _w32(c, mode, d), bias, order, mfma, bias_first)
        if c.prec in (1, 2):
            return conv_split_bf16(xr, _w32(c, mode, d), bias, order, defect)
        return conv_winograd_f32(xr, wino_weights(_np(w_eff(d["w"], mode)), scale_of(c)), bias, mfma, bias_first)

    cc = _tile_defects(c, conv(), defect, conv, tile or (tile_of(c) if defect in ("halo", "strip", "misstore") else None))
    out = {"c": cc}
    if c.epi == 0:
        out["y"] = pool_adjoint_f32(cc, defect) if c.om else cc
    elif c.epi in (1, 3):
        out["y"], out["rn"] = epilogue_lrelu_pn(cc, variant, defect)
        if c.epi == 3:
            out["img"] = np.tanh(_chan_sum(out["y"] * _np(d["wimg"])).astype(f64)).astype(f32)
    else:
        g = pool_adjoint_f32(cc, defect) if c.om else cc
        out["y"] = epilogue_pn_bwd(g, _np(d["ay"]), _np(d["arn"]))
    return out


def split_reference(c, mode, d):
    """the fp64 sum of the three products the split-bf16 forms add (lo.hi + hi.lo + hi.hi) on the emulation's own operands, plus the
    bias: what an exact accumulation gives (part A of the two-part settlement of tests/wgrad_cases.py); (B, H, W, N) fp64 numpy"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    bias = t(_bias32(c, d))
    if c.prec == 3:
        x = _np(d["x"])
        xh, xl = _split(np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge"))
        wf = folded_weights(_np(w_eff(d["w"], mode)).astype(f32), scale_of(c))
        out = torch.empty(c.B, c.H, c.W, c.N, dtype=torch.float64)
        for s in range(4):
            wh, wl = _split(wf[s])
            full = sum(fp64_conv.conv3x3(t(a), t(b)) for a, b in ((xh, wl), (xl, wh), (xh, wh)))[:, 1:-1, 1:-1]
            out[:, (s >> 1)::2, (s & 1)::2] = full + bias
        return out.numpy()
    xh, xl = _split(_xr32(c, d))
    wh, wl = _split(_w32(c, mode, d))
    return (sum(fp64_conv.conv3x3(t(a), t(b)) for a, b in ((xh, wl), (xl, wh), (xh, wh))) + bias).numpy()
