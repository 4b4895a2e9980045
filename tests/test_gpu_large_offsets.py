"""The training step's kernels on tensors that cross the 32-bit boundaries: T1 = 2^31 bytes, T2 = 2^32 bytes, T3 = 2^31 elements
(tests/large_offset_cases.py: the shapes, the boundary images, the table of limits whose refusals tests/test_index_limits_cpu.py checks).

Every case fills its outputs with NaN between two sentinel images inside the same allocation, draws its inputs from a seeded device
generator, launches the entry point ONCE on the crossing tensor, and checks
  (a) nothing unwritten, nothing out of range: no NaN in the output, both sentinel images bit-identical afterwards;
  (b) per element against fp64 on the boundary images -- the first, the last, and for each threshold the image before it and the image
      that contains it ({0, 7, 8, 15, 16, 31, 32} for the large fp32 shapes) -- with the bounds of tests/test_gpu_full_size.py, unchanged:
      exact fp32 relative L2 <= 1e-6 and max <= 2e-5 of max|ref|, split-bf16 max <= 2e-4, bf16 storage the bf16 neighbour of the fp64 value
      (+ 2e-5 of the maximum, 3e-5 for an input gradient, 1e-4 behind a PixelNorm backward), norms 2e-5, stride 2 / BatchNorm 5e-5;
  (c) the whole tensor: torch.equal with the same entry point run on chunks of the batch (4 images of the large shapes, 1024 of the
      small ones: every chunk below every threshold), after checking that the chunk runs the same kernel where the choice depends on
      the batch.  Batch reductions instead: an fp64 reference over the whole batch, accumulated chunk by chunk on the GPU, with the
      full-size weight-gradient bounds (exact fp32 relative L2 <= 1e-5, max <= 1e-4; split-bf16 max <= 2e-4; bf16 storage L2 <= 1e-4).
No new tolerance is introduced.  Where a PixelNorm epilogue is involved the pre-activations carry the +-12 bias of test_gpu_full_size.py.
Every test ends with del / empty_cache and asserts torch.cuda.max_memory_allocated() <= 64 GiB.

The large-image shape is (33, 2048, 2048, 16) and its equivalents with 2^26 elements per image: that is what puts image 8 at T1, image
16 at T2 and image 32 at T3 in fp32 (large_offset_cases.LARGE says why it is not (33, 512, 512, 16), which crosses nothing).

Measured on an MI355X (worst over a case's images / modes; err = relative L2 / max of max|ref| unless said otherwise; nothing missed a bound):
  conv forward + LeakyReLU -> PixelNorm      f32 1.4e-7 / 6.0e-7 (bound 1e-6 / 2e-5); bf16x3 max 2.6e-6 (2e-4); bf16 storage: 0 elements beyond the
                                             bf16 neighbour, norms max 1.3e-6 (2e-5).  Kernels reached: tile, wino, persist (bilinear and ragged),
                                             up2f + border ring, mid (64 and 128 channels, plain and pooled input, K = 16 padded), generic (plain and
                                             pooled input), bf16 k16 / k32 / k64 / k128 / wide
  conv input gradient + PixelNorm backward   f32 6.1e-7 / 1.4e-6; bf16x3 max 6.5e-6; bf16 storage 0 beyond the neighbour
  conv weight gradient, stored / accumulated f32 7.7e-6 / 8.3e-6 (bound 1e-5 / 1e-4; the 128 -> 128 layer over 1.7e7 pixels is the closest), bf16x3
                                             max 2.9e-5 (2e-4), bf16 storage L2 5.1e-6 (1e-4)
  PixelNorm fwd / bwd2 / bwdbwd              f32 <= 9.6e-8 / 1.9e-7; bf16 storage 0 beyond the neighbour, norms max 1.6e-7
  ToImage fwd / bwd / bwd_pnbwd (+ _acc)     f32 <= 8.4e-8 / 5.7e-7; colour-weight gradient 1.0e-6 / 1.1e-6 (1e-5 / 1e-4), bf16 L2 1.1e-6
  FromImage fwd / dx / dw (+ _acc)           f32 <= 1.3e-7 / 3.1e-7; parameter sums 1.1e-6 / 1.4e-6; the _acc twins bit-equal to stored + existing
  channel_sum (+ _acc)                       9.2e-7 / 8.1e-7 (1e-5 / 1e-4); bf16 L2 6.5e-7
  up2 / pool2 and adjoints, up2_adjoint_pnbwd, lerp, fade_bwd    f32 <= 7.4e-8 / 1.8e-7 (pool2_adjoint exact), B = 33 and B = 129 alike
  s2_conv 1.1e-6, s2_wgrad 3.2e-6, bn_act_apply 7.9e-8, bn_act_bwd 1.1e-8, tanh_bwd 5.9e-8 (max; bound 5e-5); bn_stats max 1.9e-7 (1e-5)
  whole nets on 34 samples                   forwards bit-equal to their chunks; parameter gradients 1.5e-7 / 2.4e-7 of the fp64 chunk sum
Before the change to csrc/wide.hip that came with this module, the wide (C = 48) channel_sum and ToImage colour-weight gradient missed the
reduction bound at 4.5e7 pixels (1.3e-4 / 1.8e-4 and 1.4e-4 / 2.2e-4 against 1e-5 / 1e-4: one sequential fp32 accumulator per channel); they
sum in three levels now and are in the rows above.
Wall time of the module: 219 s for 105 cases, peak device memory 49.4 GiB.  Six cases take 13 - 39 s each, all of them the wide.hip
reductions (channel_sum, ToImage and FromImage parameter sums at C = 48): one thread per channel walks 4.5e7 pixels; every other case
takes 0.3 - 6 s.
"""
import gc

import numpy as np
import pytest
import torch

import fp64_conv as R
import large_offset_cases as L
from test_gpu_full_size import BF16_WGRAD_L2, BOUNDS, S2_TOL, _signed_bias, check, check_bf16

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOPE = 0.2
BF = torch.bfloat16
NAN = float("nan")


# ---- the harness ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _memory_cap():
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    print(f"STAT peak memory {peak / 2 ** 30:.1f} GiB")
    assert peak <= L.MEMORY_CAP, peak


def gen_of(*salt):
    return torch.Generator(device=DEV).manual_seed(1009 + sum((i + 1) * int(s) for i, s in enumerate(salt)))


def randn(gen, shape, dtype=torch.float32, scale=1.0, shift=0.0):
    """seeded normal draws, written image by image so that no temporary of the tensor's own size exists"""
    out = torch.empty(shape, device=DEV, dtype=dtype)
    step = max(1, (1 << 28) // max(1, out[0].numel()))
    for lo in range(0, shape[0], step):
        part = out[lo:lo + step]
        part.copy_(torch.randn(part.shape, device=DEV, generator=gen) * scale + shift)
    return out


def guarded(B, image_shape, dtype):
    """(buffer, view of the B images between two sentinel images): the view is NaN, the sentinels are L.SENTINEL"""
    buf = torch.full((B + 2, *image_shape), L.SENTINEL, device=DEV, dtype=dtype)
    mid = buf[1:B + 1]
    mid.fill_(NAN)
    return buf, mid


def check_written(tag, buf, mid):
    """check (a)"""
    assert bool((buf[0] == L.SENTINEL).all()) and bool((buf[-1] == L.SENTINEL).all()), (tag, "a sentinel image next to the output was written")
    step = max(1, (1 << 28) // max(1, mid[0].numel()))
    for lo in range(0, mid.shape[0], step):
        assert not bool(torch.isnan(mid[lo:lo + step]).any()), (tag, f"NaN in images {lo}..{lo + step - 1}: an element was never written")


def boundary(tensors):
    """union of the boundary images of every per-sample tensor of a call"""
    out = set()
    for t in tensors:
        out |= set(L.boundary_images(t.shape[0], t[0].numel(), t.element_size()))
    return sorted(out)


def per_sample(tag, B, chunk, ins, out_specs, launch, ref, judges):
    """ins: per-sample input tensors (leading dimension B; None allowed).  out_specs: [(image shape, dtype)].  launch(b, ins, outs)
    runs the entry point on b images.  ref(ins) -> the fp64 outputs for the given images.  judges: one check(tag, got, ref) per output."""
    bufs = [guarded(B, shape, dtype) for shape, dtype in out_specs]
    outs = [mid for _, mid in bufs]
    launch(B, ins, outs)
    for i, (buf, mid) in enumerate(bufs):
        check_written(f"{tag} out{i}", buf, mid)
    everything = [t for t in list(ins) + outs if t is not None]
    assert any(any(L.crosses(t.shape[0], t[0].numel(), t.element_size())) for t in everything), (tag, "no tensor of the case crosses a threshold")
    # (c) the whole tensor against the chunked twin
    for lo, n in chunks_of(B, chunk):
        part = [torch.full((n, *shape), NAN, device=DEV, dtype=dtype) for shape, dtype in out_specs]
        launch(n, [None if t is None else t[lo:lo + n] for t in ins], part)
        for i, (got, want) in enumerate(zip(outs, part)):
            assert torch.equal(got[lo:lo + n], want), (tag, f"output {i}, images {lo}..{lo + n - 1} differ from the chunked launch")
        del part
    # (b) the boundary images against fp64, one image at a time (the fp64 temporaries of one 2^26-element image are a few GB)
    for b in boundary(everything):
        refs = ref([None if t is None else t[b:b + 1] for t in ins])
        for i, (judge, want) in enumerate(zip(judges, refs)):
            judge(f"{tag} out{i} image {b}", outs[i][b:b + 1], want)
        del refs
    del bufs, outs


def chunks_of(B, chunk):
    """[(first image, count)]: whole chunks, the remainder joined to the last one (no launch on a handful of images, whose kernel
    choice may differ; the longest chunk is still below every threshold: large_offset_cases.LARGE_CHUNK)"""
    starts = list(range(0, max(B - B % chunk, chunk), chunk))
    return [(lo, (B - lo) if lo == starts[-1] else chunk) for lo in starts]


def reduction(tag, B, chunk, ins, launch, ref, judges):
    """launch(ins) -> the reduced outputs over the whole batch; ref(ins) -> the fp64 contributions of the given images (summed here)"""
    everything = [t for t in ins if t is not None]
    assert any(any(L.crosses(t.shape[0], t[0].numel(), t.element_size())) for t in everything), (tag, "no tensor of the case crosses a threshold")
    got = launch(ins)
    want = None
    for lo in range(0, B, chunk):
        part = ref([None if t is None else t[lo:lo + chunk] for t in ins])
        want = part if want is None else [a + b for a, b in zip(want, part)]
    for i, (judge, g, w) in enumerate(zip(judges, got, want)):
        judge(f"{tag} out{i}", g, w)


def act_judge(mode, extra=2e-5):
    if mode == "bf16":
        return lambda tag, got, ref: check_bf16(tag, got, ref, extra)
    return lambda tag, got, ref: check(tag, got, ref, BOUNDS[mode]["act"])


def norm_judge(mode):
    return lambda tag, got, ref: check(tag, got, ref, (None, 2e-5) if mode == "bf16" else BOUNDS[mode]["act"])


def wgrad_judge(mode):
    if mode == "bf16":
        def judge(tag, got, ref):
            l2 = float((got.double() - ref).norm() / ref.norm())
            print(f"STAT {tag}: rel_l2 {l2:.3e} (bound {BF16_WGRAD_L2})")
            assert got.dtype == torch.float32 and not bool(torch.isnan(got).any()) and l2 <= BF16_WGRAD_L2, (tag, l2)
        return judge
    return lambda tag, got, ref: check(tag, got, ref, BOUNDS[mode]["wgrad"])


class conv_mode:
    """the conv arithmetic mode of ops for the duration of a test; activations are bf16 in the "bf16" mode"""

    def __init__(self, ops, mode):
        self.ops, self.mode = ops, mode

    def __enter__(self):
        self.ops.set_conv_precision(self.mode)
        return BF if self.mode == "bf16" else torch.float32

    def __exit__(self, *exc):
        self.ops.set_conv_precision("f32")
        return False


def rbf(t):
    return t.to(BF).double()


# ---- 3x3 convolutions --------------------------------------------------------------------------------------------------------------
def conv_launcher(ngan, w, bias, res, scale, epilogue, dgrad=False, out_mode=0, names=None):
    """launch(b, [x, aux_in, aux_rn], [y, rnorm, pooled side]) through the C ABI with the caller's output tensors: what ops._run_conv /
    ops._run_dgrad do for one output-channel chunk (precision code from the library, packed weights, the border ring of precision 3 as a
    launch of its own).  names: a dict that records {b: (precision code, kernel name)} for the same-kernel check of the chunks."""
    ops, C = ngan.ops, ngan._C

    def launch(b, ins, outs):
        x, ay, arn = (list(ins) + [None, None])[:3]
        y, rn, yp = (list(outs) + [None, None])[:3]
        k = x.shape[3]
        n = y.shape[3]
        h, wd = (x.shape[1], x.shape[2]) if out_mode else (y.shape[1], y.shape[2])
        prec = ops._conv_prec(x, b, h, wd, k, n, res)
        if names is not None:
            names[b] = (prec, C.conv3x3_kernel_name(b, h, wd, k, n, res, epilogue, out_mode, prec))
        packed = ops._packed(w, 1 if dgrad else 0, scale, prec)
        flags = C.CONV_SKIP_BORDER if prec == 3 else 0
        ops._conv_launch(x, packed, bias, y, rn, ay, arn, yp, b, h, wd, k, n, res, epilogue, out_mode, SLOPE, ops.PIXELNORM_EPS, prec, flags)
        if prec == 3:
            C.call("ngan_conv3x3_up2_border", x, packed, bias, y, rn, b, h, wd, k, n, epilogue, SLOPE, ops.PIXELNORM_EPS)
    return launch


def in_shape(shape, res):
    B, H, W, K = shape
    return (B, 2 * H, 2 * W, K) if res == 1 else ((B, H // 2, W // 2, K) if res == 2 else (B, H, W, K))


LARGE_32_N = (33, 2048, 1024, 16)        # 16 -> 32 channels: the OUTPUT has LARGE_32's 2^26 elements per image
SMALL_128 = (8193, 64, 32, 128)          # the 128-channel layers: 2^18 elements per image
SMALL_LOW = (8193, 32, 32, 64)           # a conv resolution whose pooled INPUT is SMALL
CONV_FWD = [  # name, conv-resolution shape (B, H, W, K), N, resample, {mode: the kernel family the case is there for}, chunk
    ("large_16to16", L.LARGE, 16, 0, {"f32": "conv3x3_tile_kernel<", "bf16x3": "conv3x3_tile_kernel<", "bf16": "conv3x3_bf16_kernel<16, 16,"}, L.LARGE_CHUNK),
    ("large_16to16_up2", L.LARGE, 16, 2, {"f32": "conv3x3_wino_kernel<", "bf16x3": "conv3x3_up2f_kernel<", "bf16": "conv3x3_bf16_kernel<16, 16,"},
     L.LARGE_CHUNK),                                                                      # (up2f: with the border ring's launch)
    ("large_32to32", L.LARGE_32, 32, 0, {"f32": "conv3x3_wino_kernel<", "bf16x3": "conv3x3_tile_kernel<", "bf16": "conv3x3_bf16_kernel<32, 32,"},
     L.LARGE_CHUNK),
    ("large_32to32_up2", L.LARGE_32, 32, 2, {"bf16x3": "conv3x3_persist_kernel<"}, L.LARGE_CHUNK),          # bilinear input
    ("ragged_16to16", L.RAGGED, 16, 0, {"f32": "conv3x3_persist_kernel<", "bf16x3": "conv3x3_persist_kernel<"}, L.LARGE_CHUNK),   # W % 32 != 0
    # pooled input (the critic's pool-then-conv block): the INPUT (33, 4096, 4096, 16) is four times the output, 35 GB in fp32
    ("large_pooled_16to16", L.LARGE, 16, 1, {"f32": "conv3x3_kernel<", "bf16": "conv3x3_bf16_kernel<16, 16,"}, L.LARGE_CHUNK),
    ("large_pooled_16to32", LARGE_32_N, 32, 1, {"bf16x3": "conv3x3_mid_kernel<", "bf16": "conv3x3_bf16_kernel<16, 32,"}, L.LARGE_CHUNK),
    ("small_pooled_64to64", SMALL_LOW, 64, 1, {"f32": "conv3x3_kernel<", "bf16x3": "conv3x3_mid_kernel<", "bf16": "conv3x3_bf16_kernel<64, 64,"},
     L.SMALL_CHUNK),
    ("small_64to64", L.SMALL, 64, 0, {"f32": "conv3x3_mid_kernel<", "bf16x3": "conv3x3_mid_kernel<", "bf16": "conv3x3_bf16_kernel<64, 64,"}, L.SMALL_CHUNK),
    ("small_128to128", SMALL_128, 128, 0, {"f32": "conv3x3_mid_kernel<4,", "bf16x3": "conv3x3_mid_kernel<4,", "bf16": "conv3x3_bf16_kernel<128, 128,"},
     L.SMALL_CHUNK),
    ("small_64to16", L.SMALL, 16, 0, {"f32": "conv3x3_kernel<"}, L.SMALL_CHUNK),          # the generic exact-fp32 kernel
    ("small_48to64", L.SMALL_WIDE, 64, 0, {"bf16": "conv3x3_bf16_wide_kernel<"}, L.SMALL_CHUNK),
]


def _weights(w, scale, mode):
    return (rbf((w * scale).float()), 1.0) if mode == "bf16" else (w.double(), scale)


@pytest.mark.parametrize("case", [(c[0], m) for c in CONV_FWD for m in c[4]], ids=lambda c: f"{c[0]}-{c[1]}")
def test_conv_forward_with_pixelnorm_epilogue(ngan, case):
    name, mode = case
    _, shape, N, res, family, chunk = next(c for c in CONV_FWD if c[0] == name)
    B, H, W, K = shape
    ops, C = ngan.ops, ngan._C
    with conv_mode(ops, mode) as dt:
        gen = gen_of(B, H, K, N, res)
        x = randn(gen, in_shape(shape, res), dt)
        w = torch.randn(N, K, 3, 3, device=DEV, generator=gen)
        b12 = _signed_bias(gen, N, 12.0)
        scale = 1.3868 / np.sqrt(9 * K)
        names = {}
        launch = conv_launcher(ngan, w, b12, res, scale, ops.EPI_LRELU_PN, names=names)
        specs = [((H, W, N), dt), ((H, W), torch.float32)]
        judges = [act_judge(mode), norm_judge(mode)]
        prec = ops._conv_prec(x, B, H, W, K, N, res)
        side = mode != "bf16" and C.conv3x3_pooled_output(B, H, W, K, N, res, prec)
        if side:                                          # the pooled side output of the Winograd kernels: a third output tensor
            specs.append(((H // 2, W // 2, N), torch.float32))
            judges.append(act_judge(mode))
        wq, sq = _weights(w, scale, mode)

        def ref(ins):
            xin = ins[0].double()
            if mode == "bf16" and res:                    # the staging rounds the resampled input once (test_gpu_full_size._in_operand)
                staged = L.pooled_operand_bf16(ins[0]) if res == 1 else rbf(R.resample(xin, res).float())
                c = R.conv3x3(staged, wq, sq, 0, b12.double())
            else:
                c = R.conv3x3(xin, wq, sq, res, b12.double())
            assert float(c.abs().min()) > 1.0             # every pre-activation is far from LeakyReLU's kink
            y, r = R.lrelu_pixelnorm(c, SLOPE)
            return [y, r] + ([R.pool2(y)] if side else [])

        per_sample(f"conv_fwd {name} {mode}", B, chunk, [x], specs, launch, ref, judges)
        assert len(set(names.values())) == 1, ("the chunked twin ran another kernel", names)
        assert names[B][1].startswith(family[mode]), ("the case no longer reaches the kernel family it is there for", family[mode], names[B])
        print(f"STAT conv_fwd {name} {mode}: {names[B]}")
    del x


CONV_DGRAD = [  # name, gradient shape (B, H, W, N = the layer's outputs), K = the layer's inputs, pool-adjoint store, {mode: family}, chunk
    ("large_16to16_pnbwd", L.LARGE, 16, 0, {"f32": "conv3x3_tile_kernel<", "bf16x3": "conv3x3_tile_kernel<", "bf16": "conv3x3_bf16_kernel<16, 16,"},
     L.LARGE_CHUNK),
    ("large_pool_adjoint", L.LARGE_LOW, 16, 1, {"f32": "conv3x3_tile_kernel<", "bf16x3": "conv3x3_tile_kernel<", "bf16": "conv3x3_bf16_kernel<16, 16,"},
     L.LARGE_CHUNK),                                                                      # the OUTPUT (33, 2048, 2048, 16) crosses
    ("small_64to64_pnbwd", L.SMALL, 64, 0, {"f32": "conv3x3_mid_kernel<", "bf16x3": "conv3x3_mid_kernel<", "bf16": "conv3x3_bf16_kernel<64, 64,"},
     L.SMALL_CHUNK),
    ("small_128to128_pnbwd", SMALL_128, 128, 0, {"f32": "conv3x3_mid_kernel<4,", "bf16x3": "conv3x3_mid_kernel<4,", "bf16": "conv3x3_bf16_kernel<128, 128,"},
     L.SMALL_CHUNK),
]


@pytest.mark.parametrize("case", [(c[0], m) for c in CONV_DGRAD for m in c[4]], ids=lambda c: f"{c[0]}-{c[1]}")
def test_conv_input_gradient_with_pixelnorm_backward(ngan, case):
    name, mode = case
    _, shape, K, pool, family, chunk = next(c for c in CONV_DGRAD if c[0] == name)
    B, H, W, N = shape
    ops = ngan.ops
    with conv_mode(ops, mode) as dt:
        gen = gen_of(B, H, K, N, pool, 5)
        g = randn(gen, shape, dt)
        oh, ow = (2 * H, 2 * W) if pool else (H, W)
        ay = randn(gen, (B, oh, ow, K), dt)                # stands for the producer's output and norms
        arn = torch.rand(B, oh, ow, device=DEV, generator=gen) + 0.5
        w = torch.randn(N, K, 3, 3, device=DEV, generator=gen)
        scale = 1.3868 / np.sqrt(9 * K)
        names = {}
        launch = conv_launcher(ngan, w, None, 0, scale, ops.EPI_PN_BWD, dgrad=True, out_mode=pool, names=names)
        wq, sq = _weights(w, scale, mode)

        def ref(ins):
            gx = R.conv3x3_dgrad(ins[0].double(), wq, sq, pool)
            return [R.pixelnorm_bwd(gx, ins[1].double(), ins[2].double(), SLOPE)]

        per_sample(f"conv_dgrad {name} {mode}", B, chunk, [g, ay, arn], [((oh, ow, K), dt)], launch, ref, [act_judge(mode, 1e-4)])
        assert len(set(names.values())) == 1, ("the chunked twin ran another kernel", names)
        assert names[B][1].startswith(family[mode]), ("the case no longer reaches the kernel family it is there for", family[mode], names[B])
        print(f"STAT conv_dgrad {name} {mode}: {names[B]}")
    del g, ay, arn


CONV_WGRAD = [  # name, shape (B, H, W, Cin), Cout, resample, modes, images per fp64 chunk
    ("large_16x16", L.LARGE, 16, 0, ("f32", "bf16x3", "bf16"), L.LARGE_CHUNK),
    ("large_16x16_up2", L.LARGE, 16, 2, ("bf16x3", "bf16"), L.LARGE_CHUNK),
    ("large_16x16_pooled", L.LARGE, 16, 1, ("bf16x3", "bf16"), 2),          # the kernels' own pooled-input path (exact fp32 pools first: ops._pool_first)
    ("large_32x32", L.LARGE_32, 32, 0, ("f32", "bf16x3"), L.LARGE_CHUNK),
    ("small_64x64", L.SMALL, 64, 0, ("f32", "bf16x3", "bf16"), L.SMALL_CHUNK // 4),
    ("small_64x64_pooled", SMALL_LOW, 64, 1, ("bf16x3", "bf16"), L.SMALL_CHUNK // 4),
    ("small_128x128", SMALL_128, 128, 0, ("f32", "bf16x3", "bf16"), L.SMALL_CHUNK // 4),
]


@pytest.mark.parametrize("case", [(c[0], m) for c in CONV_WGRAD for m in c[4]], ids=lambda c: f"{c[0]}-{c[1]}")
def test_conv_weight_gradient_stored_and_accumulated(ngan, case):
    name, mode = case
    _, shape, N, res, _, chunk = next(c for c in CONV_WGRAD if c[0] == name)
    B, H, W, K = shape
    ops = ngan.ops
    with conv_mode(ops, mode) as dt:
        gen = gen_of(B, H, K, N, res, 9)
        x = randn(gen, in_shape(shape, res), dt)
        g = randn(gen, (B, H, W, N), dt)
        scale = 1.3868 / np.sqrt(9 * K)
        acc0 = torch.randn(N, K, 3, 3, device=DEV, generator=gen) * 1e3     # an existing gradient of the sums' scale (~ sqrt(2^31 / 16))

        def launch(ins):
            stored = ops._run_wgrad(ins[0], ins[1], res, scale)
            acc = acc0.clone()
            ops._run_wgrad(ins[0], ins[1], res, scale, accumulate_into=acc)
            return [stored, acc]

        def ref(ins):
            xin = ins[0].double()
            if mode == "bf16" and res:
                xin, r = (L.pooled_operand_bf16(ins[0]) if res == 1 else rbf(R.resample(xin, res).float())), 0
            else:
                r = res
            gw = L.conv3x3_wgrad_ref(xin, ins[1].double(), scale, r)
            return [gw, gw]

        def acc_judge(tag, got, want):
            wgrad_judge(mode)(tag, got, want + acc0.double())

        reduction(f"conv_wgrad {name} {mode}", B, chunk, [x, g], launch, ref, [wgrad_judge(mode), acc_judge])
    del x, g


# ---- LeakyReLU -> PixelNorm ---------------------------------------------------------------------------------------------------------
PN_SHAPES = [("large", L.LARGE, L.LARGE_CHUNK), ("small", L.SMALL, L.SMALL_CHUNK), ("wide", L.SMALL_WIDE, L.SMALL_CHUNK)]


def _k(name, dt):
    return name.replace("ngan_", "ngan_bf16_", 1) if dt == BF else name


@pytest.mark.parametrize("storage", ["float", "bf16"])
@pytest.mark.parametrize("shape_name", [s[0] for s in PN_SHAPES])
def test_pixelnorm_forward_and_backward(ngan, shape_name, storage):
    _, shape, chunk = next(s for s in PN_SHAPES if s[0] == shape_name)
    if shape_name == "wide" and storage == "bf16":
        shape = (2 * shape[0] - 1,) + shape[1:]            # bf16 storage: twice the images for the same bytes (T2 = T3 at the last image)
        chunk *= 2
    B, H, W, C = shape
    npi = H * W
    C_ = ngan._C
    dt = BF if storage == "bf16" else torch.float32
    mode = "bf16" if storage == "bf16" else "f32"
    gen = gen_of(B, H, C, 11)
    c = randn(gen, shape, dt)
    bias = _signed_bias(gen, C, 12.0)

    def fwd(b, ins, outs):
        C_.call(_k("ngan_lrelu_pixelnorm_fwd", dt), ins[0], bias, outs[0], outs[1], b * npi, C, SLOPE, 1e-8)

    def fwd_ref(ins):
        pre = ins[0].double() + bias.double()
        assert float(pre.abs().min()) > 1.0
        return list(R.lrelu_pixelnorm(pre, SLOPE))

    per_sample(f"pn_fwd {shape_name} {storage}", B, chunk, [c], [((H, W, C), dt), ((H, W), torch.float32)], fwd, fwd_ref,
               [act_judge(mode), norm_judge(mode)])
    # backward with both optional operands (bwd2: a second gradient; gr: the gradient w.r.t. the norms); y and r as a forward leaves them
    y = torch.empty(shape, device=DEV, dtype=dt)
    rn = torch.empty((B, H, W), device=DEV)
    fwd(B, [c], [y, rn])
    del c
    gy = randn(gen, shape, dt)
    gr = randn(gen, (B, H, W))

    def bwd(b, ins, outs):
        C_.call(_k("ngan_lrelu_pixelnorm_bwd2", dt), ins[0], ins[0], ins[1], ins[2], ins[3], outs[0], b * npi, C, SLOPE)

    def bwd_ref(ins):
        g = ins[0].double()
        return [L.pn_bwd_ref(g, g, ins[1].double(), ins[2].double(), ins[3].double(), SLOPE)]

    per_sample(f"pn_bwd2 {shape_name} {storage}", B, chunk, [gy, gr, y, rn], [((H, W, C), dt)], bwd, bwd_ref, [act_judge(mode, 1e-4)])
    del gr
    if shape_name == "large":                              # (the second-order kernel: the penalty pass runs it on the same tensors)
        h = randn(gen, shape, dt)

        def bwdbwd(b, ins, outs):
            C_.call(_k("ngan_lrelu_pixelnorm_bwdbwd", dt), ins[0], ins[1], ins[2], ins[3], outs[0], outs[1], outs[2], b * npi, C, SLOPE)

        def bwdbwd_ref(ins):
            return list(L.pn_bwdbwd_ref(ins[0].double(), ins[1].double(), ins[2].double(), ins[3].double(), SLOPE))

        per_sample(f"pn_bwdbwd {shape_name} {storage}", B, chunk, [h, gy, y, rn], [((H, W, C), dt), ((H, W, C), dt), ((H, W), torch.float32)],
                   bwdbwd, bwdbwd_ref, [act_judge(mode, 1e-4), act_judge(mode, 1e-4), norm_judge(mode)])
        del h
    del gy, y, rn


# ---- ToImage / FromImage / channel sums ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", ["float", "bf16"])
@pytest.mark.parametrize("shape_name", ["large", "wide"])
def test_to_image_forward_and_backward(ngan, shape_name, storage):
    """large: the lane-group kernels.  wide: C = 48, the wide.hip twins (one thread per pixel; the colour weights' gradient one thread
    per channel walking the pixels -- a second or two at this size, so the wide shape runs the PixelNorm-backward form only, which is
    the plain form's kernels with the norms given)."""
    shape, chunk = (L.LARGE, L.LARGE_CHUNK) if shape_name == "large" else (L.SMALL_WIDE, L.SMALL_CHUNK)
    B, H, W, C = shape
    npi = H * W
    C_ = ngan._C
    dt = BF if storage == "bf16" else torch.float32
    mode = "bf16" if storage == "bf16" else "f32"
    gen = gen_of(B, C, 13)
    x = randn(gen, shape, dt)
    wimg = torch.randn(1, C, device=DEV, generator=gen) * 0.3

    def fwd(b, ins, outs):
        C_.call(_k("ngan_to_image_fwd", dt), ins[0], wimg, outs[0], b * npi, C, 1)

    per_sample(f"to_image_fwd {shape_name} {storage}", B, chunk, [x], [((H, W, 1), torch.float32)], fwd,
               lambda ins: [L.to_image_ref(ins[0].double(), wimg.double())], [norm_judge(mode)])
    t = torch.empty((B, H, W, 1), device=DEV)
    fwd(B, [x], [t])
    g = randn(gen, (B, H, W, 1))
    rn = torch.rand(B, H, W, device=DEV, generator=gen) + 0.5
    ws = torch.empty(1024 * C, device=DEV)
    for pn in ((False, True) if shape_name == "large" else (True,)):
        gws = {}

        def bwd(b, ins, outs):
            gw = torch.full((1, C), NAN, device=DEV)
            if pn:
                C_.call(_k("ngan_to_image_bwd_pnbwd", dt), ins[0], ins[1], ins[2], ins[3], wimg, outs[0], gw, ws, b * npi, C, 1, SLOPE)
            else:
                C_.call(_k("ngan_to_image_bwd", dt), ins[0], ins[1], ins[2], wimg, outs[0], gw, ws, b * npi, C, 1)
            gws[b] = gw

        def bwd_ref(ins):
            gx, _ = L.to_image_bwd_ref(ins[0].double(), ins[1].double(), ins[2].double(), wimg.double())
            return [R.pixelnorm_bwd(gx, ins[2].double(), ins[3].double(), SLOPE) if pn else gx]

        tag = f"to_image_bwd{'_pnbwd' if pn else ''} {shape_name} {storage}"
        per_sample(tag, B, chunk, [g, t, x, rn], [((H, W, C), dt)], bwd, bwd_ref, [act_judge(mode, 1e-4 if pn else 3e-5)])
        # the colour weights' gradient: a reduction over the whole batch, against fp64 chunk by chunk
        want = torch.zeros(1, C, device=DEV, dtype=torch.float64)
        for lo in range(0, B, chunk):
            s = slice(lo, lo + chunk)
            _, q = L.to_image_bwd_ref(g[s].double(), t[s].double(), x[s].double(), wimg.double())
            want += (q * x[s].double()).sum(dim=(0, 1, 2)).reshape(1, C)
        wgrad_judge(mode)(f"{tag} gw", gws[B], want)
        if pn and shape_name == "large":                   # the accumulating twin (refused for the wide channel counts)
            acc, gx = torch.full((1, C), 100.0, device=DEV), torch.empty(shape, device=DEV, dtype=dt)
            C_.call(_k("ngan_to_image_bwd_pnbwd_acc", dt), g, t, x, rn, wimg, gx, acc, ws, B * npi, C, 1, SLOPE, 1)
            wgrad_judge(mode)(f"{tag} gw accumulated", acc, want + 100.0)
            del gx
    del x, t, g, rn


@pytest.mark.parametrize("storage", ["float", "bf16"])
@pytest.mark.parametrize("shape_name", ["large", "large_pooled", "wide", "grid_edge"])
def test_from_image_forward_and_backward(ngan, shape_name, storage):
    """wide: C = 48 -- the image gradient and the parameter sums are wide.hip's (one thread per pixel / per channel)"""
    B, H, W, C = {"grid_edge": L.GRID_EDGE, "wide": L.FROM_IMAGE_WIDE}.get(shape_name, L.FROM_IMAGE)
    pool = int(shape_name == "large_pooled")
    chunk = {"grid_edge": 64, "wide": 64}.get(shape_name, L.LARGE_CHUNK)
    C_ = ngan._C
    dt = BF if storage == "bf16" else torch.float32
    mode = "bf16" if storage == "bf16" else "f32"
    gen = gen_of(B, H, C, pool, 17)
    f = 2 if pool else 1
    x = randn(gen, (B, f * H, f * W, 1))
    wf = torch.randn(C, 1, device=DEV, generator=gen)
    bf = torch.randn(C, device=DEV, generator=gen)

    def fwd(b, ins, outs):
        C_.call(_k("ngan_from_image_fwd", dt), ins[0], wf, bf, outs[0], b, H, W, 1, C, pool)

    def run():
        per_sample(f"from_image_fwd {shape_name} {storage}", B, chunk, [x], [((H, W, C), dt)], fwd,
                   lambda ins: [L.from_image_ref(ins[0].double(), wf.double(), bf.double(), pool)], [act_judge(mode)])
    if shape_name == "grid_edge":
        # the grid edge is run, not only refused: B * H = 65535 rows on gridDim.y, one more row is NGAN_ERR_SHAPE (the CPU test).  The
        # shape crosses no threshold (it is the grid, not the offsets, that is at its edge): the harness's crossing assertion does not apply
        buf, y = guarded(B, (H, W, C), dt)
        fwd(B, [x], [y])
        check_written("from_image_fwd grid_edge", buf, y)
        for lo, n in chunks_of(B, chunk):
            part = torch.full((n, H, W, C), NAN, device=DEV, dtype=dt)
            fwd(n, [x[lo:lo + n]], [part])
            assert torch.equal(y[lo:lo + n], part), (lo, "differs from the chunked launch")
        act_judge(mode)(f"from_image_fwd grid_edge {storage}", y, L.from_image_ref(x.double(), wf.double(), bf.double(), pool))
        del x, buf, y
        return
    run()
    g = randn(gen, (B, H, W, C), dt)

    def dx(b, ins, outs):
        C_.call(_k("ngan_from_image_dx", dt), ins[0], wf, outs[0], b, H, W, 1, C, pool)

    per_sample(f"from_image_dx {shape_name} {storage}", B, chunk, [g], [((f * H, f * W, 1), torch.float32)], dx,
               lambda ins: [L.from_image_dx_ref(ins[0].double(), wf.double(), pool)], [norm_judge(mode)])

    ws = torch.empty(1024 * C * 2, device=DEV)

    def dw(ins):
        gw, gb = torch.full((C, 1), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
        C_.call(_k("ngan_from_image_dw", dt), ins[0], ins[1], gw, gb, ws, B, H, W, 1, C, pool)
        return [gw, gb]

    def dw_ref(ins):
        gg = ins[1].double()
        xp = R.pool2(ins[0].double()) if pool else ins[0].double()
        return [(gg * xp).sum(dim=(0, 1, 2)).reshape(C, 1), gg.sum(dim=(0, 1, 2))]

    reduction(f"from_image_dw {shape_name} {storage}", B, chunk, [x, g], dw, dw_ref, [wgrad_judge(mode), wgrad_judge(mode)])
    if shape_name != "wide":                               # the accumulating twin (refused for the wide channel counts)
        gw, gb = torch.full((C, 1), 100.0, device=DEV), torch.full((C,), -50.0, device=DEV)
        C_.call(_k("ngan_from_image_dw_acc", dt), x, g, gw, gb, ws, B, H, W, 1, C, pool, 3)
        plain = dw([x, g])
        wgrad_judge(mode)(f"from_image_dw_acc {shape_name} {storage} gw", gw, plain[0].double() + 100.0)
        wgrad_judge(mode)(f"from_image_dw_acc {shape_name} {storage} gb", gb, plain[1].double() - 50.0)
    del x, g


@pytest.mark.parametrize("storage", ["float", "bf16"])
@pytest.mark.parametrize("shape_name", ["large", "small", "wide"])
def test_channel_sum(ngan, shape_name, storage):
    """wide: C = 48, wide.hip's sum (one thread per channel walking the pixels; accumulate is refused there)"""
    _, shape, _ = next(s for s in PN_SHAPES if s[0] == shape_name)
    B, H, W, C = shape
    dt = BF if storage == "bf16" else torch.float32
    mode = "bf16" if storage == "bf16" else "f32"
    gen = gen_of(B, H, C, 19)
    g = randn(gen, shape, dt)
    ws = torch.empty(1024 * C, device=DEV)

    def launch(ins):
        out = torch.full((C,), NAN, device=DEV)
        ngan._C.call(_k("ngan_channel_sum", dt), ins[0], out, ws, B * H * W, C, 1.0)
        acc = torch.full((C,), 100.0, device=DEV)
        if shape_name == "wide":
            acc += out
        else:
            ngan._C.call(_k("ngan_channel_sum_acc", dt), ins[0], acc, ws, B * H * W, C, 1.0, 1)
        return [out, acc]

    def ref(ins):
        s = ins[0].double().sum(dim=(0, 1, 2))
        return [s, s]

    chunk = L.LARGE_CHUNK if shape_name == "large" else L.SMALL_CHUNK
    reduction(f"channel_sum {shape_name} {storage}", B, chunk, [g], launch, ref,
              [wgrad_judge(mode), lambda tag, got, want: wgrad_judge(mode)(tag, got, want + 100.0)])
    del g


# ---- resampling, fade-in arithmetic ---------------------------------------------------------------------------------------------------
RESAMPLERS = {  # name -> (entry point, larger side is the output, fp64 reference)
    "up2_fwd": ("ngan_up2_fwd", True, R.up2),
    "pool2_adjoint": ("ngan_pool2_adjoint", True, lambda g: R.resample_adjoint(g, 1)),
    "pool2_fwd": ("ngan_pool2_fwd", False, R.pool2),
    "up2_adjoint": ("ngan_up2_adjoint", False, lambda g: R.resample_adjoint(g, 2)),
}


@pytest.mark.parametrize("case", [(n, "float", 33) for n in RESAMPLERS] + [(n, "bf16", 33) for n in RESAMPLERS] +
                         [(n, "float", L.BOTH_SIDES_B) for n in RESAMPLERS], ids=lambda c: f"{c[0]}-{c[1]}-B{c[2]}")
def test_resampling_operators(ngan, case):
    """B = 33: only the larger side crosses.  B = 129 (fp32): the smaller side crosses T3 as well, the larger holds 34.6 GB."""
    name, storage, B = case
    entry, grows, ref64 = RESAMPLERS[name]
    _, h, w, C = L.LARGE_LOW
    dt = BF if storage == "bf16" else torch.float32
    mode = "bf16" if storage == "bf16" else "f32"
    gen = gen_of(B, len(name), 23)
    small, large = (h, w, C), (2 * h, 2 * w, C)
    x = randn(gen, (B, *(small if grows else large)), dt)

    def launch(b, ins, outs):
        ngan._C.call(_k(entry, dt), ins[0], outs[0], b, h, w, C)

    per_sample(f"{name} {storage} B={B}", B, L.LARGE_CHUNK, [x], [(large if grows else small, dt)], launch,
               lambda ins: [ref64(ins[0].double())], [act_judge(mode)])
    del x


@pytest.mark.parametrize("storage", ["float", "bf16"])
@pytest.mark.parametrize("shape_name", ["large", "wide"])
def test_up2_adjoint_with_pixelnorm_backward(ngan, shape_name, storage):
    """wide: C = 48 -- fp32 chains ngan_up2_adjoint's vector kernel and wide.hip's PixelNorm backward, bf16 storage runs wide.hip's fused one"""
    low, high, chunk = (L.LARGE_LOW, L.LARGE, L.LARGE_CHUNK) if shape_name == "large" else \
        ((L.SMALL_WIDE[0], 32, 32, 48), L.SMALL_WIDE, L.SMALL_CHUNK)
    B, h, w, C = low
    dt = BF if storage == "bf16" else torch.float32
    mode = "bf16" if storage == "bf16" else "f32"
    gen = gen_of(B, C, 29)
    g = randn(gen, high, dt)
    yprev = randn(gen, low, dt)
    rn = torch.rand(B, h, w, device=DEV, generator=gen) + 0.5

    def launch(b, ins, outs):
        ngan._C.call(_k("ngan_up2_adjoint_pnbwd", dt), ins[0], ins[1], ins[2], outs[0], b, h, w, C, SLOPE)

    def ref(ins):
        return [R.pixelnorm_bwd(R.resample_adjoint(ins[0].double(), 2), ins[1].double(), ins[2].double(), SLOPE)]

    per_sample(f"up2_adjoint_pnbwd {shape_name} {storage}", B, chunk, [g, yprev, rn], [((h, w, C), dt)], launch, ref, [act_judge(mode, 1e-4)])
    del g, yprev, rn


@pytest.mark.parametrize("storage", ["float", "bf16"])
def test_lerp_and_fade_backward(ngan, storage):
    B, H, W, C = L.LARGE
    n_img = H * W * C
    dt = BF if storage == "bf16" else torch.float32
    mode = "bf16" if storage == "bf16" else "f32"
    gen = gen_of(B, 31)
    a, b_ = randn(gen, L.LARGE, dt), randn(gen, L.LARGE, dt)
    alpha = torch.tensor([0.3], device=DEV)

    def lerp(b, ins, outs):
        ngan._C.call(_k("ngan_lerp", dt), ins[0], ins[1], alpha, outs[0], b * n_img)

    per_sample(f"lerp {storage}", B, L.LARGE_CHUNK, [a, b_], [((H, W, C), dt)], lerp,
               lambda ins: [ins[0].double() + alpha.double() * (ins[1].double() - ins[0].double())], [act_judge(mode)])
    del b_

    def fade(b, ins, outs):
        ngan._C.call(_k("ngan_fade_bwd", dt), ins[0], alpha, outs[0], outs[1], b * n_img)

    per_sample(f"fade_bwd {storage}", B, L.LARGE_CHUNK, [a], [((H, W, C), dt), ((H, W, C), dt)], fade,
               lambda ins: [(1 - alpha.double()) * ins[0].double(), alpha.double() * ins[0].double()], [act_judge(mode), act_judge(mode)])
    del a


# ---- stride 2 / BatchNorm (the WGAN nets) -------------------------------------------------------------------------------------------
def s2_judge(tag, got, ref):
    check(tag, got, ref, (None, S2_TOL))


@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
def test_stride2_convolution_and_its_weight_gradient(ngan, up):
    from neuron_gan_amd import wgan_ops as Wg
    B, H, W, C = L.SMALL
    M = 64
    hin, win = (H // 2, W // 2) if up else (H, W)          # the larger side is SMALL: the output when up, the input when down
    ho, wo = (2 * hin, 2 * win) if up else (hin // 2, win // 2)
    gen = gen_of(B, C, int(up), 37)
    x = randn(gen, (B, hin, win, C))
    w = 0.1 * torch.randn(*((C, M, 4, 4) if up else (M, C, 4, 4)), device=DEV, generator=gen)
    bias = torch.randn(M, device=DEV, generator=gen)
    sc = torch.rand(C, device=DEV, generator=gen) + 0.5
    sh = 0.3 * torch.randn(C, device=DEV, generator=gen)
    wp = Wg.pack(w, M, C, up)

    def launch(b, ins, outs):
        ngan._C.call("ngan_s2_conv", ins[0], wp, bias, sc, sh, 1, SLOPE, outs[0], b, hin, win, C, M, int(up), 0)

    def ref(ins):
        a = R.act_on_load(ins[0].double(), sc.double(), sh.double(), 1, SLOPE)
        return [R.s2_up(a, w.double(), bias.double()) if up else R.s2_down(a, w.double(), bias.double())]

    per_sample(f"s2_conv {'up' if up else 'down'}", B, L.SMALL_CHUNK, [x], [((ho, wo, M), torch.float32)], launch, ref, [s2_judge])
    g = randn(gen, (B, ho, wo, M))
    xform = (sc, sh, 1, SLOPE)

    def wgrad(ins):
        return [Wg.wgrad(ins[0], ins[1], tuple(w.shape), half_xf=xform) if up else Wg.wgrad(ins[1], ins[0], tuple(w.shape), full_xf=xform)]

    def wgrad_ref(ins):
        a = R.act_on_load(ins[0].double(), sc.double(), sh.double(), 1, SLOPE)
        return [L.s2_wgrad_ref(a, ins[1].double()) if up else L.s2_wgrad_ref(ins[1].double(), a)]

    reduction(f"s2_wgrad {'up' if up else 'down'}", B, L.SMALL_CHUNK // 4, [x, g], wgrad, wgrad_ref, [s2_judge])
    del x, g


def test_batchnorm_statistics_and_elementwise_passes(ngan):
    from neuron_gan_amd import wgan_ops as Wg
    B, H, W, C = L.SMALL
    npix = B * H * W
    C_ = ngan._C
    gen = gen_of(B, C, 41)
    y = randn(gen, L.SMALL, scale=2.0, shift=3.0)
    bn = torch.nn.BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(0.15 + 0.02 * torch.randn(C, device=DEV, generator=gen))
        bn.bias.copy_(_signed_bias(gen, C, 2.0, noise=0.1))
    scale, shift, mean, rstd = Wg.BNSpec(bn).fold(y, bn.weight, bn.bias)
    # the statistics: a reduction over the whole batch; fp64 moments chunk by chunk (sums of y and y^2 about 3, the draws' mean)
    s0 = torch.zeros(C, device=DEV, dtype=torch.float64)
    s1 = torch.zeros(C, device=DEV, dtype=torch.float64)
    for lo in range(0, B, L.SMALL_CHUNK // 4):
        d = y[lo:lo + L.SMALL_CHUNK // 4].double() - 3.0
        s0 += d.sum(dim=(0, 1, 2))
        s1 += (d * d).sum(dim=(0, 1, 2))
    m64 = 3.0 + s0 / npix
    var = s1 / npix - (s0 / npix) ** 2
    r64 = 1.0 / torch.sqrt(var + bn.eps)
    sc64 = bn.weight.detach().double() * r64
    sh64 = bn.bias.detach().double() - m64 * sc64
    for k, got, want in (("mean", mean, m64), ("rstd", rstd, r64), ("scale", scale, sc64), ("shift", shift, sh64)):
        check(f"bn_stats {k}", got, want, (None, 1e-5))
    check("chan_sum", Wg.chan_sum(y), 3.0 * npix + s0, (None, S2_TOL))

    def apply(b, ins, outs):
        C_.call("ngan_bn_act_apply", ins[0], scale, shift, 1, SLOPE, b * H * W, C, outs[0])

    per_sample("bn_act_apply", B, L.SMALL_CHUNK, [y], [((H, W, C), torch.float32)], apply,
               lambda ins: [R.act_on_load(ins[0].double(), sc64, sh64, 1, SLOPE)], [s2_judge])
    g = randn(gen, L.SMALL)

    def act_bwd(b, ins, outs):      # gamma null: the activation's backward alone (per sample; the BatchNorm part is the reductions above)
        C_.call("ngan_bn_act_bwd", ins[0], ins[1], scale, shift, None, None, None, 1, SLOPE, b * H * W, C, outs[0], None, None, None)

    def act_bwd_ref(ins):
        z = ins[0].double() * scale.double() + shift.double()
        return [ins[1].double() * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, SLOPE))]

    per_sample("bn_act_bwd (activation)", B, L.SMALL_CHUNK, [y, g], [((H, W, C), torch.float32)], act_bwd, act_bwd_ref, [s2_judge])
    t = torch.tanh(y * 0.2)

    def tanh_bwd(b, ins, outs):
        C_.call("ngan_tanh_bwd", ins[0], ins[1], outs[0], b * H * W * C)

    per_sample("tanh_bwd", B, L.SMALL_CHUNK, [t, g], [((H, W, C), torch.float32)], tanh_bwd,
               lambda ins: [ins[1].double() * (1 - ins[0].double() ** 2)], [s2_judge])
    del y, g, t


# ---- the Python plumbing: whole nets ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [True, False], ids=["first_block_fold", "unfused_pair"])
@pytest.mark.parametrize("pooled_side", [True, False], ids=["pooled_side", "pooling_pass"])
def test_headline_nets_on_34_samples_equal_their_chunks(ngan, fold, pooled_side):
    """The headline 512^2 nets: the generator on 34 latents, the critic on those 34 images in fp32.  Forward results bit-equal to the
    chunked forwards; the parameter gradients of the summed score equal the fp64 sum of the chunks' gradients within twice the full-size
    weight-gradient bound (both sides are within that bound of the truth).

    What this test does NOT do: cross a boundary.  Its largest tensor has 34 * 2^22 elements, four times below T1, and at 34 images the
    first-block fold is inside every limit of its row (the fold steps aside from 129 images on at this stage: its slab count), so the
    `fold` switch compares the fold with the unfused pair, not the fallback with the fold.  It covers the wrappers of ops.py and
    models.py on a batch that is no multiple of anything in the launch plans, chunk against whole; the index arithmetic beyond the
    thresholds is the kernel-level cases' above, which go through the same C ABI the wrappers call, and the fallback's boundary is
    checked on shapes alone by tests/test_index_limits_cpu.py.  Whole nets at a crossing size (2048^2) are not run: see DESIGN.md."""
    ops, models = ngan.ops, ngan.models
    g_widths, d_widths = [128, 64, 32, 32, 16, 16], [16, 16, 32, 32, 64, 128]          # bench.py's G_WIDTHS / D_WIDTHS
    B, chunk = 34, 17
    torch.manual_seed(34)
    G = models.Generator_PG(g_widths, image_size_init=16).to(DEV)
    D = models.Discriminator_PG(d_widths, image_size_init=16).to(DEV)
    G.set_resolution(512, 1.0)
    D.set_resolution(512, 1.0)
    saved = ops._first_block_allowed, ops._pool_out_allowed
    ops._first_block_allowed, ops._pool_out_allowed = fold, pooled_side
    try:
        z = torch.randn(B, 512, device=DEV, generator=gen_of(43))
        ops.latent_normalize_(z)
        with torch.no_grad():
            img = G(z)
            assert tuple(img.shape) == (B, 1, 512, 512) and not bool(torch.isnan(img).any())
            for lo in range(0, B, chunk):
                assert torch.equal(img[lo:lo + chunk], G(z[lo:lo + chunk])), ("generator", lo)

        def scores_and_grads(x):
            for p in D.parameters():
                p.grad = None
            with ops.first_order_only():
                s = D(x)
            s.sum().backward()
            return s.detach().clone(), {k: p.grad.detach().clone() for k, p in D.named_parameters() if p.grad is not None}

        s_all, g_all = scores_and_grads(img)
        assert s_all.numel() == B and not bool(torch.isnan(s_all).any())
        want = None
        for lo in range(0, B, chunk):
            s, g = scores_and_grads(img[lo:lo + chunk])
            assert torch.equal(s_all.reshape(-1)[lo:lo + chunk], s.reshape(-1)), ("critic", lo)
            want = {k: v.double() for k, v in g.items()} if want is None else {k: want[k] + v.double() for k, v in g.items()}
        assert set(want) == set(g_all) and len(g_all) >= 14          # (seven layers' weights and biases at least)
        l2b, mxb = BOUNDS["f32"]["wgrad"]
        worst = (0.0, 0.0)
        for k, gv in g_all.items():
            d = gv.double() - want[k]
            l2, mx = float(d.norm() / want[k].norm()), float(d.abs().max() / want[k].abs().max())
            worst = (max(worst[0], l2), max(worst[1], mx))
            assert l2 <= 2 * l2b and mx <= 2 * mxb, (k, l2, mx)
        print(f"STAT headline nets fold={fold} pooled_side={pooled_side}: parameter gradients rel_l2 {worst[0]:.3e} max {worst[1]:.3e}")
    finally:
        ops._first_block_allowed, ops._pool_out_allowed = saved
        ops.clear_packed()
    del G, D
