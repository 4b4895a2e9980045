"""Index widths of the training step's kernels: the table of DESIGN.md section 2 ("Index widths") as data, the shapes that cross the
32-bit boundaries, and the fp64 references of the per-pixel operators the crossing tests need.

Two tests read this module.  tests/test_index_limits_cpu.py calls every limited entry point of ROWS with the first shape past its
limit (dummy pointers: every check comes before the launch) and expects NGAN_ERR_SHAPE with the limit named; it also holds ROWS
against the headers: every in-scope symbol has a row, no row names a symbol that does not exist.  tests/test_gpu_large_offsets.py
runs the accepted crossing shapes on the GPU.

The thresholds.  T1 = 2^31 BYTES (a signed 32-bit byte offset), T2 = 2^32 bytes (an unsigned one), T3 = 2^31 ELEMENTS (a signed
32-bit element index).  Before this module the largest tensor of the suite was the (32, 512, 512, 16) of FULL_SIZE_LAYERS: 2^27
elements, 2^29 bytes -- a factor of four below the first threshold.

Scope: every entry point a PGGAN or WGAN training step launches on an activation-sized tensor (IN_SCOPE).  Out of scope: the
image-sized and metric entry points (diffaug, diffgeo, augment, swd, msssim, spectrum, morphology, specloss, simloss, ada, data
set), the stem / head / scalar heads (one latent or one score per sample) and the optimiser steps (the flat parameter buffers: a few
hundred MB at the widest preset) -- none of their tensors comes near 2^31 bytes in a step.

What the audit changed, and the wrong variant each change stands against (the CPU test would show it as a launch, i.e. a status
other than NGAN_ERR_SHAPE, at the first bad shape; the GPU checks (b) and (c) as wrong pixels):
  * ngan_conv3x3_wgrad, precision 0: the one-image-below-1-GiB guard applied to precisions 1 and 5 only, from the time the exact
    kernel walked pixels with 64-bit addresses; wgrad_f32_kernel has since moved to per-image buffer descriptors.  Variant: "byte
    offset inside an image formed in int, no guard" -- above 2^31 bytes per image the offset is negative, the descriptor's range
    check returns zeros, and the gradient silently loses those pixels.
  * ngan_conv3x3_fwd(_ex), the many-channel kernel (conv3x3_mid.hip): the same descriptor form, no guard at all.  Variant as above.
  * ngan_conv3x3_up2_border and precision 3 of ngan_conv3x3_fwd(_ex): one grid row per image, no guard.  Variant: "B on gridDim.y
    unchecked" -- a launch error at B = 65536 instead of a refusal.
  * one thread (or lane group) per item with the block count narrowed to int (PixelNorm, ToImage forward, the wide.hip twins,
    s2_conv, bn_act_apply, bn_act_bwd(_merged), tanh_bwd, stdfield_add): the runtime refuses 2^32 threads along x.  Variant:
    "block count narrowed to int / thread count unchecked" -- a launch error (or, past 2^39 items, a wrapped block count and an
    unwritten tail) instead of a refusal.
  * the wide.hip pixel reductions (channel_sum, ToImage's colour-weight gradient, FromImage's parameter sums at channel counts outside the
    lane-group kernels): the one value defect the GPU run found, an accuracy one -- a single sequential fp32 accumulator per channel was
    1.3e-4 off at 4.5e7 pixels; they sum in three levels now.  Variant: "one accumulator over all pixels"; check (c) of the reductions
    (fp64 over the whole batch) is what shows it.
wrapped_index() below restates the index variants as arithmetic only (the fixes to the index paths were refusals, so there is no operator
emulation to plant a defect in): test_index_limits_cpu.py shows that at the crossing shapes of this module an index formed in 32 bits
first goes wrong in an image that checks (b) and (c) look at, next to one that is still right.
"""
import re

NGAN_ERR_SHAPE = -2
T1, T2, T3 = 1 << 31, 1 << 32, 1 << 31          # bytes, bytes, elements
MAX_THREADS = (1 << 32) - 256                   # NGAN_REQUIRE_THREADS (csrc/ngan_common.h): items of a one-thread-per-item launch
MEMORY_CAP = 64 << 30                           # torch.cuda.max_memory_allocated() of every GPU test
SENTINEL = 7.25                                 # guard images around every output (exact in bf16 too)


# ---- scope ------------------------------------------------------------------------------------------------------------------------
IN_SCOPE = [re.compile(p) for p in (
    r"ngan_conv3x3_(fwd|fwd_ex|up2_border|wgrad)", r"ngan_bf16_conv3x3_(fwd|wgrad)",
    r"ngan_(bf16_)?lrelu_pixelnorm_(fwd|bwd|bwd2|bwdbwd)", r"ngan_(bf16_)?channel_sum(_acc)?",
    r"ngan_(bf16_)?from_image_(fwd|dx|dw|dw_acc)", r"ngan_(bf16_)?to_image_(fwd|bwd|bwd_pnbwd|bwd_pnbwd_acc)",
    r"ngan_(bf16_)?(up2_fwd|up2_adjoint|up2_adjoint_pnbwd|pool2_fwd|pool2_adjoint)", r"ngan_(bf16_)?(lerp|fade_bwd)",
    r"ngan_first_block_(fwd|bwd|dx)", r"ngan_mbstd_(fwd|bwd|bwdbwd)", r"ngan_stdfield_(add|ds|dw)",
    r"ngan_(s2_conv|s2_wgrad|bn_stats|bn_moments|bn_act_apply|bn_act_bwd|bn_act_bwd_partial|bn_act_bwd_merged|chan_sum|tanh_bwd)",
)]


def in_scope(symbol):
    return any(p.fullmatch(symbol) for p in IN_SCOPE)


# ---- the table --------------------------------------------------------------------------------------------------------------------
class Limit:
    """`text` is the formula as DESIGN.md prints it; the shape is accepted while value(d) < bound.  first_bad() grows `vary` from 1
    over `base` until the formula refuses: the limit under test comes from the formula, never from the library's message."""

    def __init__(self, text, value, bound, vary, base, token, variants=({},)):
        self.text, self.value, self.bound, self.vary, self.base, self.token, self.variants = text, value, bound, vary, dict(base), token, variants

    def first_bad(self, variant=None):
        """the named arguments of the first refused shape (and of the last accepted one) for one of `variants`"""
        base = dict(self.base, **(variant or {}))
        at = lambda v: self.value(dict(base, **{self.vary: v}))      # noqa: E731
        lo, hi = 0, 1                                    # at(lo) < bound <= at(hi): the formulas are monotone in `vary`
        while at(hi) < self.bound:
            lo, hi = hi, 2 * hi
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if at(mid) < self.bound else (lo, mid)
        assert lo >= 1, (self.text, "no accepted shape below the first refused one")
        return dict(base, **{self.vary: hi}), dict(base, **{self.vary: lo})


class Row:
    def __init__(self, symbols, widest, limits=()):
        self.symbols, self.widest, self.limits = tuple(symbols), widest, tuple(limits)


def _twins(*names):
    """ngan_<op> and ngan_bf16_<op>"""
    return tuple(n for name in names for n in ("ngan_" + name, "ngan_bf16_" + name))


def _ceil(a, b):
    return -(-a // b)


_CONV = dict(B=1, resample=0, epilogue=0, out_mode=0, flags=0)
_LONG = "long element index, grid-stride or capped grid"
NONE = "none below the allocation"

ROWS = [
    Row(("ngan_conv3x3_fwd", "ngan_conv3x3_fwd_ex"),
        "persist / tile / wino / up2f (K, N <= 32 on large images): unsigned 32-bit byte offset inside ONE image (buffer descriptor), "
        "long image base, int tile count (>= 8 KB per tile).  mid (K, N in 32..128): the same with the offset formed in int.  generic: "
        "long throughout",
        [Limit("H*W*max(K,N)*16 < 2^32 (K, N <= 32, large image)", lambda d: d["H"] * d["W"] * max(d["K"], d["N"]) * 16, 1 << 32, "H",
               dict(_CONV, W=4096, K=16, N=16, precision=0), b"one image must stay below 1 GiB"),
         Limit("H*W*K*4 < 2^31 (many channels)", lambda d: d["H"] * d["W"] * d["K"] * 4, 1 << 31, "H",
               dict(_CONV, W=2048, K=128, N=128, precision=0), b"one input image must stay below 2 GiB"),
         Limit("B < 65536 (precision 3: the border ring)", lambda d: d["B"], 65536, "B",
               dict(_CONV, H=16, W=32, K=16, N=16, resample=2, precision=3), b"border-ring kernel takes at most 65535 images")]),
    Row(("ngan_conv3x3_up2_border",), "long pixel index; one grid row (gridDim.y) per image",
        [Limit("B < 65536", lambda d: d["B"], 65536, "B", dict(H=16, W=32, K=16, N=16, epilogue=0), b"at most 65535 images per call")]),
    Row(("ngan_bf16_conv3x3_fwd",), "32-bit byte offset inside one image (buffer descriptor), long image base, int tile count",
        [Limit("H*W*(4 if pooled input or pool-adjoint store else 1)*max(K,N)*2 < 2^31",
               lambda d: d["H"] * d["W"] * (4 if d["out_mode"] or d["resample"] == 1 else 1) * max(d["K"], d["N"]) * 2, 1 << 31, "H",
               dict(_CONV, W=8192, K=16, N=16), b"one image must stay below 2 GiB", variants=({}, dict(resample=1)))]),
    Row(("ngan_conv3x3_wgrad", "ngan_bf16_conv3x3_wgrad"),
        "32-bit byte offset inside one image (buffer descriptor, formed in int) in every precision; long image base; slabs: long",
        [Limit("H*W*max(Cin,Cout)*16 < 2^32", lambda d: d["H"] * d["W"] * max(d["Cin"], d["Cout"]) * 16, 1 << 32, "H",
               dict(B=1, W=4096, Cin=16, Cout=16, resample=0, accumulate=0), b"one image must stay below 1 GiB", variants=(dict(precision=0), dict(precision=1)))]),
    Row(("ngan_lrelu_pixelnorm_fwd", "ngan_lrelu_pixelnorm_bwd", "ngan_lrelu_pixelnorm_bwd2", "ngan_lrelu_pixelnorm_bwdbwd"),
        "long pixel and element index; C/4 lanes per pixel, one launch: npix*C/4 threads (C/4 a power of two <= 64), npix threads else",
        [Limit("npix*C/4 <= 2^32 - 256", lambda d: d["npix"] * (d["C"] // 4), MAX_THREADS + 1, "npix", dict(C=256), b"threads in one launch: must stay below 2^32"),
         Limit("npix <= 2^32 - 256 (other C: wide.hip)", lambda d: d["npix"], MAX_THREADS + 1, "npix", dict(C=48), b"threads in one launch: must stay below 2^32")]),
    Row(("ngan_bf16_lrelu_pixelnorm_fwd", "ngan_bf16_lrelu_pixelnorm_bwd", "ngan_bf16_lrelu_pixelnorm_bwd2", "ngan_bf16_lrelu_pixelnorm_bwdbwd"),
        "as fp32, C/8 lanes per pixel where C % 8 == 0",
        [Limit("npix*C/8 <= 2^32 - 256", lambda d: d["npix"] * (d["C"] // 8), MAX_THREADS + 1, "npix", dict(C=256), b"threads in one launch: must stay below 2^32"),
         Limit("npix <= 2^32 - 256 (other C: wide.hip)", lambda d: d["npix"], MAX_THREADS + 1, "npix", dict(C=48), b"threads in one launch: must stay below 2^32")]),
    Row(_twins("channel_sum", "channel_sum_acc"), _LONG + " (at most 1024 workgroups); workspace 1024*C floats"),
    Row(_twins("from_image_fwd"), "unsigned item index inside one image row, long pixel index; one grid row (gridDim.y) per image row",
        [Limit("B*H*W*C/4 < 2^31", lambda d: d["B"] * d["H"] * d["W"] * (d["C"] // 4), 1 << 31, "B", dict(H=512, W=512, C=256, Ncol=1, pool=0), b"B*H*W*C/4 must be below 2^31"),
         Limit("B*H < 65536", lambda d: d["B"] * d["H"], 65536, "B", dict(H=512, W=32, C=16, Ncol=1, pool=0), b"B*H must be below 65536")]),
    Row(_twins("from_image_dx"), "unsigned pixel count and lane index ((unsigned)B*H*W), long addresses; other C (wide.hip): long pixel index, "
                                 "one launch of B*H*W threads",
        [Limit("B*H*W <= 2^32 - 256 (other C: wide.hip)", lambda d: d["B"] * d["H"] * d["W"], MAX_THREADS + 1, "B", dict(H=256, W=256, C=48, Ncol=1, pool=0),
               b"threads in one launch: must stay below 2^32"),
         Limit("B*H*W*C/4 < 2^31", lambda d: d["B"] * d["H"] * d["W"] * (d["C"] // 4), 1 << 31, "B", dict(H=512, W=512, C=256, Ncol=1, pool=0), b"B*H*W*C/4 must be below 2^31")]),
    Row(_twins("from_image_dw", "from_image_dw_acc"), "int image-row index B*H, long addresses; at most 1024 slabs",
        [Limit("B*H*W*C/4 < 2^31", lambda d: d["B"] * d["H"] * d["W"] * (d["C"] // 4), 1 << 31, "B",
               dict(H=512, W=512, C=256, Ncol=1, pool=0, accumulate=0), b"B*H*W*C/4 must be below 2^31")]),
    Row(_twins("to_image_fwd"), "long lane and pixel index; one launch of npix*C/4 threads (npix threads for other C: wide.hip)",
        [Limit("npix*C/4 <= 2^32 - 256", lambda d: d["npix"] * (d["C"] // 4), MAX_THREADS + 1, "npix", dict(C=256, Ncol=1), b"threads in one launch: must stay below 2^32"),
         Limit("npix <= 2^32 - 256 (other C: wide.hip)", lambda d: d["npix"], MAX_THREADS + 1, "npix", dict(C=48, Ncol=1), b"threads in one launch: must stay below 2^32")]),
    Row(_twins("to_image_bwd", "to_image_bwd_pnbwd", "to_image_bwd_pnbwd_acc"), _LONG + " (at most 1024 workgroups = slabs); other C (wide.hip): "
                                                                             "long pixel index, one launch of npix threads",
        [Limit("npix <= 2^32 - 256 (other C: wide.hip)", lambda d: d["npix"], MAX_THREADS + 1, "npix", dict(C=48, Ncol=1, accumulate=0),
               b"threads in one launch: must stay below 2^32")]),
    Row(_twins("up2_fwd", "pool2_adjoint", "lerp", "fade_bwd"), _LONG + " (4096 workgroups)"),
    Row(_twins("up2_adjoint"), "strip kernel: long image base, int offsets inside two image rows, one grid layer (gridDim.z) per image; "
                               "B >= 65536 or other C: the long grid-stride kernels"),
    Row(_twins("up2_adjoint_pnbwd"), "the strip kernel of up2_adjoint: one grid layer (gridDim.z) per image; other C (wide.hip): long pixel "
                                     "index, one launch of B*h*w threads",
        [Limit("B < 65536", lambda d: d["B"], 65536, "B", dict(h=1, w=1, C=16), b"at most 65535 images per call"),
         Limit("B*h*w <= 2^32 - 256 (other C: wide.hip)", lambda d: d["B"] * d["h"] * d["w"], MAX_THREADS + 1, "h", dict(B=1024, w=2048, C=48),
               b"threads in one launch: must stay below 2^32")]),
    Row(_twins("pool2_fwd"), "int item index where B*h*w*C/4 < 2^31 - 256 (the vector kernels), else the long grid-stride kernel"),
    Row(("ngan_first_block_fwd", "ngan_first_block_bwd", "ngan_first_block_dx"),
        "int element index inside the output; one grid row per 8 image rows; at most 1024 slabs (the Python layer falls back to the "
        "unfused pair: ops.first_block_fusable)",
        [Limit("B*H*W*N < 2^31", lambda d: d["B"] * d["H"] * d["W"] * d["N"], 1 << 31, "B", dict(H=512, W=512, C=16, N=16, pool=0, accumulate=0), b"< 2^31 output elements"),
         Limit("B*ceil(H/8) < 65536", lambda d: d["B"] * _ceil(d["H"], 8), 65536, "B", dict(H=512, W=64, C=16, N=16, pool=0, accumulate=0), b"must stay below 65536 (one grid row per"),
         Limit("B*ceil(W*(N/4)/256) <= 1024 (slabs)", lambda d: d["B"] * _ceil(d["W"] * (d["N"] // 4), 256), 1025, "B",
               dict(H=1, W=1, C=16, N=16, pool=0, accumulate=0), b"slabs (max 1024)")]),
    Row(("ngan_mbstd_fwd", "ngan_mbstd_bwd", "ngan_mbstd_bwdbwd"), "long feature index; one grid row (gridDim.y) per group",
        [Limit("B < 65536", lambda d: d["B"], 65536, "B", dict(H=4, W=4, C=16, segments=1, G_eff=1), b"1 .. 65535 samples per call"),
         Limit("H*W*C <= 2^31", lambda d: d["H"] * d["W"] * d["C"], (1 << 31) + 1, "H", dict(B=1, W=1 << 15, C=16, segments=1, G_eff=1), b"more than 2^31 features per sample")]),
    Row(("ngan_stdfield_add", "ngan_stdfield_ds", "ngan_stdfield_dw"), "long element index; stdfield_add: one launch of B*H*W*C/4 threads",
        [Limit("B < 65536", lambda d: d["B"], 65536, "B", dict(H=4, W=4, C=16), b"1 .. 65535 samples per call"),
         Limit("B*H*W*C < 2^34 - 1024", lambda d: d["B"] * d["H"] * d["W"] * d["C"], (1 << 34) - 1024, "H", dict(B=1 << 15, W=1024, C=16), b"too large (2^34 elements)")]),
    Row(("ngan_stdfield_ds",), "int element index inside one sample (one workgroup per sample)",
        [Limit("H*W*C < 2^29", lambda d: d["H"] * d["W"] * d["C"], 1 << 29, "H", dict(B=1, W=1 << 13, C=16), b"H*W*C below 2^29")]),
    Row(("ngan_s2_conv",), "long pixel index; four threads per output pixel (of one parity when up) in one launch",
        [Limit("4*B*Hq*Wq <= 2^32 - 256 (Hq, Wq: Hin/2, Win/2 down; Hin, Win up)", lambda d: 4 * d["B"] * (d["Hin"] // 2) * (d["Win"] // 2),
               MAX_THREADS + 1, "B", dict(Hin=1024, Win=1024, C=16, M=16, up=0, in_act=0, tanh_out=0), b"threads in one launch: must stay below 2^32"),
         Limit("4*B*Hin*Win <= 2^32 - 256 (up)", lambda d: 4 * d["B"] * d["Hin"] * d["Win"], MAX_THREADS + 1, "B",
               dict(Hin=512, Win=512, C=16, M=16, up=1, in_act=0, tanh_out=0), b"threads in one launch: must stay below 2^32")]),
    Row(("ngan_bn_act_apply", "ngan_bn_act_bwd", "ngan_bn_act_bwd_merged"), "long element index; one thread per element in one launch",
        [Limit("npix*C <= 2^32 - 256", lambda d: d["npix"] * d["C"], MAX_THREADS + 1, "npix", dict(C=64, act=1, world=1, rank=0), b"threads in one launch: must stay below 2^32")]),
    Row(("ngan_tanh_bwd",), "long element index; one thread per element in one launch",
        [Limit("n <= 2^32 - 256", lambda d: d["n"], MAX_THREADS + 1, "n", {}, b"threads in one launch: must stay below 2^32")]),
    Row(("ngan_s2_wgrad", "ngan_bn_stats", "ngan_bn_moments", "ngan_bn_act_bwd_partial", "ngan_chan_sum"),
        "long pixel index; at most 1024 chunks (4096 work items for s2_wgrad)"),
]


def rows_of(symbol):
    return [r for r in ROWS if symbol in r.symbols]


def design_table():
    """the table as DESIGN.md section 2 prints it: one line per row and limit"""
    lines = ["| entry points | widest index | limit |", "|---|---|---|"]
    for r in ROWS:
        names = ", ".join("`" + s.replace("ngan_", "", 1) + "`" for s in r.symbols)
        limit = "; ".join("`" + lim.text + "`" for lim in r.limits) or NONE
        lines.append(f"| {names} | {r.widest} | {limit} |")
    return "\n".join(lines)


# ---- the crossing shapes ----------------------------------------------------------------------------------------------------------
# The large-image family needs 2^26 elements per image for "image 8 starts at T1, image 16 at T2, image 32 at T3" (fp32; bf16 storage:
# image 16 at T1, image 32 at T2 = T3) with B = 33 the smallest crossing batch.  That is 2048 x 2048 x 16 -- the training step's kernel
# families at sixteen times the pixels of the 512^2 stage, whose own (33, 512, 512, 16) tensor has 33 * 2^22 elements and crosses nothing
# (the 512^2 stage first reaches 2^31 bytes in one tensor at batch 128, and 2^31 elements at batch 512).
LARGE = (33, 2048, 2048, 16)
LARGE_32 = (33, 2048, 1024, 32)     # the 32-channel variants: the same elements per image
LARGE_LOW = (33, 1024, 1024, 16)    # the smaller side of a resampling operator whose larger side is LARGE
FROM_IMAGE = (33, 1024, 4096, 16)   # FromImage: the same 2^26 elements per image on B*H = 33792 grid rows (LARGE has 67584: refused, CPU test)
FROM_IMAGE_WIDE = (683, 64, 1024, 48)   # FromImage at a wide.hip channel count: 2^31 + 0.7 M elements on B*H = 43712 grid rows
RAGGED = (33, 2048, 2056, 16)       # a width that is no multiple of the 32-pixel tile: the persistent kernel's ragged path
SMALL = (8193, 64, 64, 64)          # 2^18 elements per image: image 2048 / 4096 / 8192 starts at T1 / T2 / T3 (fp32)
SMALL_WIDE = (10923, 64, 64, 48)    # C = 48 (wide.hip, conv3x3_bf16_wide): 196608 elements per image, 2^31 + 65536 in all
BOTH_SIDES_B = 129                  # resampling operators, fp32: the SMALLER side (129, 1024, 1024, 16) crosses T3 as well (larger: 34.6 GB)
GRID_EDGE = (255, 257, 32, 16)      # from_image_fwd: B*H = 65535 grid rows, the last accepted count; 257 rows per image
LARGE_CHUNK, SMALL_CHUNK = 4, 1024  # images per launch of the chunked twin: 2^24 / 2^28 elements, below every threshold


def boundary_images(B, elems_per_image, itemsize):
    """the images check (b) looks at: the first, the last, and for each threshold the image before and the image that contains it --
    and, where the threshold falls inside an image, the next one too: the first whose BASE lies beyond the threshold"""
    out = {0, B - 1}
    for t in (T1 // itemsize, T2 // itemsize, T3):
        i = t // elems_per_image                      # the image holding element t
        if 0 < i < B:
            out |= {i - 1, i}
            if t % elems_per_image and i + 1 < B:
                out.add(i + 1)
    return sorted(out)


def crosses(B, elems_per_image, itemsize):
    """which of (T1, T2, T3) the tensor's last element lies at or beyond"""
    last = B * elems_per_image - 1
    return last * itemsize >= T1, last * itemsize >= T2, last >= T3


def wrapped_index(index, itemsize, variant):
    """an element index as a WRONG kernel would form it.  variant: "int_elements" (the element index in int32), "int_bytes" (the byte
    offset in int32), "unsigned_bytes" (the byte offset in uint32)"""
    if variant == "int_elements":
        return (index + (1 << 31)) % (1 << 32) - (1 << 31)
    byte = index * itemsize
    if variant == "int_bytes":
        byte = (byte + (1 << 31)) % (1 << 32) - (1 << 31)
    elif variant == "unsigned_bytes":
        byte %= 1 << 32
    else:
        raise ValueError(variant)
    return byte // itemsize


def images_a_variant_gets_wrong(B, elems_per_image, itemsize, variant):
    """the images in which a kernel with that variant reads or writes a wrong address: its first or its last element is misplaced"""
    ends = lambda b: (b * elems_per_image, (b + 1) * elems_per_image - 1)       # noqa: E731
    return [b for b in range(B) if any(wrapped_index(i, itemsize, variant) != i for i in ends(b))]


# ---- fp64 references of the per-pixel operators (torch, any device; the 3x3 and stride-2 ones are tests/fp64_conv.py) ---------------
def pn_bwd_ref(gy, gy2, gr, y, r, slope):
    """ngan_lrelu_pixelnorm_bwd2: gc = m ((g - y mean_c(g y)) / r + gr y / C), g = gy + gy2"""
    import torch
    g = gy if gy2 is None else gy + gy2
    c = y.shape[-1]
    m = torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
    out = (g - y * (g * y).mean(-1, keepdim=True)) / r.unsqueeze(-1)
    if gr is not None:
        out = out + gr.unsqueeze(-1) * y / c
    return m * out


def pn_bwdbwd_ref(h, gy, y, r, slope):
    """ngan_lrelu_pixelnorm_bwdbwd (include/ngan.h): ggy, gy_out, gr_out"""
    import torch
    c = y.shape[-1]
    m = torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
    hp = m * h
    s, t, u = (gy * y).mean(-1, keepdim=True), (hp * y).mean(-1, keepdim=True), (hp * gy).mean(-1, keepdim=True)
    rr = r.unsqueeze(-1)
    return (hp - y * t) / rr, -(s * hp + t * gy) / rr, (-c * (u - s * t) / (rr * rr))[..., 0]


def from_image_ref(x, w, b, pool):
    """x (B, H', W', Ncol) -> (B, H, W, C): y = x_pooled @ w^T + b"""
    if pool:
        bb, h2, w2, k = x.shape
        x = x.reshape(bb, h2 // 2, 2, w2 // 2, 2, k).mean(dim=(2, 4))
    return x @ w.t() + b


def from_image_dx_ref(g, w, pool):
    gx = g @ w
    if pool:
        gx = gx.repeat_interleave(2, 1).repeat_interleave(2, 2) * 0.25
    return gx


def to_image_ref(x, w):
    import torch
    return torch.tanh(x @ w.t())


def to_image_bwd_ref(g, t, x, w):
    """(gx, q) with q = g (1 - t^2): gx = q w; the colour weights' gradient is sum_p q[p]^T x[p]"""
    q = g * (1 - t * t)
    return q @ w, q


def conv3x3_wgrad_ref(x, g, scale=1.0, res=0):
    """fp64_conv.conv3x3_wgrad with the contraction over the pixels split per image row: one batched (N x W)(W x K) product per tap and a
    sum over the B*H rows, instead of one N x (B H W) x K product -- which a BLAS gives to a handful of workgroups (minutes in fp64 at
    2^28 pixels).  The same sum in another order; tests/test_index_limits_cpu.py holds the two together."""
    import torch
    import fp64_conv as R
    x = R.resample(x, res)
    b, h, w, k = x.shape
    n = g.shape[3]
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    gt = g.reshape(b * h, w, n).transpose(1, 2)
    gw = torch.empty(n, k, 3, 3, dtype=x.dtype, device=x.device)
    for dy in range(3):
        for dx in range(3):
            gw[:, :, dy, dx] = scale * torch.bmm(gt, xp[:, dy:dy + h, dx:dx + w, :].reshape(b * h, w, k)).sum(0)
    return gw


def s2_wgrad_ref(half, full):
    """fp64_conv.s2_wgrad (dW[h][f][ky][kx] = sum_{b,i,j} half[b,i,j,h] full[b, 2i-1+ky, 2j-1+kx, f], zero padding) split per image row
    in the same way"""
    import torch
    b, hh, wh, ch = half.shape
    cf = full.shape[3]
    fp = torch.nn.functional.pad(full, (0, 0, 1, 1, 1, 1))
    ht = half.reshape(b * hh, wh, ch).transpose(1, 2)
    dw = torch.empty(ch, cf, 4, 4, dtype=half.dtype, device=half.device)
    for ky in range(4):
        for kx in range(4):
            dw[:, :, ky, kx] = torch.bmm(ht, fp[:, ky:ky + 2 * hh:2, kx:kx + 2 * wh:2, :].reshape(b * hh, wh, cf)).sum(0)
    return dw


def message_is_of(symbol, err):
    """the refusal is the entry point's own: the message's prefix (the text before the first colon, without `ngan_`, `bf16_` and the
    `(wide)` mark of a wide.hip twin) is the entry point's name or the head of it (`conv3x3_fwd` for `ngan_conv3x3_fwd_ex`,
    `lrelu_pixelnorm` for the four PixelNorm entry points, `from_image_dw` for its `_acc` form)"""
    norm = lambda t: t.replace("ngan_", "").replace("bf16_", "").replace("(wide)", "").strip()      # noqa: E731
    return norm(symbol).startswith(norm(err.decode().split(":")[0]))


def pooled_operand_bf16(x):
    """the 2x2-averaged input as the bf16-storage kernels stage it (csrc/conv3x3_bf16_impl.h, the weight-gradient kernel likewise):
    0.25 * ((a + b) + (c + d)) in fp32 from the bf16 sources, then ONE rounding to bf16.  An fp64 average rounded to bf16 differs from it
    where an fp32 addition of two sources of very different magnitude is inexact and the sum lies next to a bf16 midpoint: about one
    staged element in 10^8, i.e. never at 512^2 and a few times in a tensor of 2^31 elements -- where it moves one pixel's norm by 4e-5."""
    import torch
    xf = x.float()
    a, b, c, d = xf[:, 0::2, 0::2], xf[:, 0::2, 1::2], xf[:, 1::2, 0::2], xf[:, 1::2, 1::2]
    return (0.25 * ((a + b) + (c + d))).to(torch.bfloat16).double()
