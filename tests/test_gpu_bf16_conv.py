"""The bf16-storage 3x3 convolution kernels (csrc/conv3x3_bf16.hip, conv3x3_bf16_impl.h, conv3x3_bf16_k{16,32,64,128}.hip,
conv3x3_bf16_wide.hip) through the C ABI (ngan_bf16_conv3x3_fwd), per element against fp64, at every one of the 80 template instances
pick_tile can choose and at the edges of their tilings, in both weight orientations: resample 0 with epilogues 0 and 1 at every
instance; the pooled and bilinear inputs, the PixelNorm backward, the pool-adjoint store and ToImage (with and without a stored y) in
every combination of split kind, narrow tile, tile height and weight path.  The case list, references, bounds, the exact-rounding
pin and the emulation are in tests/bf16_conv_cases.py; tests/test_bf16_conv_bounds_cpu.py settles the constants against the emulation
(never against a kernel) and pins which instances the list reaches.  tests/test_gpu_bf16.py and test_gpu_bf16_wide.py hold the older,
norm-relative checks of the same kernels.

Operands as stored (bf16 x / ay, the weight rne_bf16(w * scale), a resampled input rounded once); per element
      e_c = 2^-23 |c| + C_ACC 2^-24 absref   (C_ACC = 8; 16 at K = 144 and 256, 32 at K = 1024: bf16_conv_cases.RAISED)
propagated through the epilogue for the fp32 outputs (rnorm, the ToImage result); a bf16 output within 2^-8 |ref| + (1 + 2^-8) e and,
wherever ref lies farther than e from every bf16 midpoint, bit-equal to rne_bf16(ref) (at most 1e-2 of a case's elements undecided);
the stored sign equal to the fp64 sign wherever |c| > e_c.  The reference is evaluated in fp64 on the GPU (tests/fp64_conv.py).

Every output is prefilled with NaN and sits inside a larger allocation between two guard regions of one bit pattern, which must come
back untouched; no output element may stay NaN.

measured on MI355X (a record, not a bound: worst err / bound over all cases and both orientations; in brackets the emulation on the
CPU file's 2 x 6 x 44 image; 1 is the bound): the stored bf16 y 0.996 (0.996) -- one correct rounding reaches its bound, the margin is
in the pin: 0 of the 808 launches stored an element other than rne_bf16(ref) where the pin decides, at most 6.9e-3 of a case's elements
were undecided (the one-product case of the output split; typically 1e-3), and no stored sign contradicted fp64.  rnorm, the fp32 view
of the accumulators, per contraction width: K = 16 0.108 (0.089), 32 0.124 (0.077), 64 0.138 (0.080), 128 0.171 (0.087), 48 0.140
(0.091), 144 0.096 (0.089) and 256 0.097 (0.081) at C_ACC = 16, 1024 0.091 (0.068) at C_ACC = 32; the ToImage result 0.059 (0.037).  All
80 names appear in the STAT lines.  No kernel missed.  The module takes about 10 s (tests/test_gpu_conv_fwd.py: 10 s); a record, not a
limit."""
import pytest
import torch

import bf16_conv_cases as C
from test_gpu_conv_fwd import Guarded
from test_gpu_ops import DEV

pytestmark = pytest.mark.gpu
ARG, SHAPE = -1, -2                                                 # NGAN_ERR_ARG, NGAN_ERR_SHAPE (include/ngan.h)


class GuardedBf16(Guarded):
    """a bf16 output of `shape` (an even number of elements) prefilled with NaN between the guard regions"""

    def __init__(self, shape):
        super().__init__(tuple(shape[:-1]) + (shape[-1] // 2,))
        self.t = self.t.view(torch.bfloat16)
        self.t.fill_(float("nan"))
        assert tuple(self.t.shape) == tuple(shape)


def device_inputs(d):
    dv = {k: (v.to(DEV) if v is not None else None) for k, v in d.items()}
    for k in ("x", "ay"):
        if dv.get(k) is not None:
            dv[k] = dv[k].to(torch.bfloat16)                        # exact: the values are bf16's
    return dv


def run(ngan, c, mode):
    """launch the case: ({output: Guarded}, inputs)"""
    d = C.inputs(c, mode)
    dv = device_inputs(d)
    packed = ngan.ops._packed(dv["w"], mode, C.scale_of(c), C.PREC)
    out = {}
    if c.var != "noy":
        out["y"] = GuardedBf16(C.y_shape(c))
        if c.epi in (1, 3):
            out["rn"] = Guarded((c.B, c.H, c.W))
    if c.epi == 3:
        out["img"] = Guarded((c.B, c.H, c.W))
    t = lambda k: out[k].t if k in out else None
    aux_in = dv.get("ay") if c.epi == 2 else dv.get("wimg") if c.epi == 3 else None
    ngan._C.call("ngan_bf16_conv3x3_fwd", dv["x"], packed, dv["bias"], t("y"), t("rn"), aux_in, dv.get("arn"), t("img"),
                 c.B, c.H, c.W, c.K, c.N, c.res, c.epi, c.om, C.SLOPE, C.EPS)
    return out, d


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_bf16_conv_every_instance_against_fp64(ngan, case):
    c = case
    # (what the name function says of this call; it and the launcher both go through pick_tile)
    name = ngan._C.conv3x3_kernel_name(c.B, c.H, c.W, c.K, c.N, c.res, c.epi, c.om, C.PREC)
    assert name == C.kernel_name(c)
    bad = []
    for mode in (0, 1):
        out, d = run(ngan, c, mode)
        for k, g in out.items():
            assert g.intact(), ("wrote outside the output", k, c, mode)
            assert not bool(torch.isnan(g.t).any()), ("unwritten or NaN element", k, c, mode)
        st = C.check(c, mode, d, {k: g.t for k, g in out.items()}, dev=DEV)
        print(f"STAT bf16_conv {name} {C.case_id(c)} mode {mode}: err/bound " + " ".join(f"{k} {st[k]:.3f}" for k in ("y", "rn", "img") if k in st)
              + f" exact-miss {st['exact_miss']} undecided {st['undecided']:.2e} kink {st['kink']:.1e} sign {st['sign']}")
        bad += [(mode, f) for f in C.failures(st)]
    assert not bad, (c, name, bad)


def _pairs():
    tuned = [(K, N) for K in C.TUNED_K for N in C.CHANNELS]
    return tuned + [(K, N) for K in C.WIDE_K + (1024,) for N in C.CHANNELS]


@pytest.mark.parametrize("K,N", _pairs())
def test_packing_bit_for_bit(ngan, K, N):
    gen = torch.Generator().manual_seed(1000 * K + N)
    scale = 0.0713
    for mode in (0, 1):
        w = torch.randn(*((N, K) if mode == 0 else (K, N)), 3, 3, generator=gen)
        w[0, 0] = torch.tensor([[2.0 ** -8 + 2.0 ** -17, 1.0, -1.0], [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 0.0], [1e30, -1e-30, 1.0 + 2.0 ** -7]]) / scale
        n = ngan._C.lib().ngan_conv3x3_pack_elements(w.shape[0], w.shape[1], mode, C.PREC)
        assert n == C.pack_elements(K, N) > 0
        packed = ngan.ops._packed(w.to(DEV), mode, scale, C.PREC)
        assert packed.numel() * 2 >= n
        got = packed.view(torch.bfloat16)[:n].cpu()
        want = torch.from_numpy(C.pack_replica(w.numpy(), mode, scale)).to(torch.bfloat16)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (K, N, mode, int((got.view(torch.int16) != want.view(torch.int16)).sum()))
        # the zero tenth tap of K = 16, the zero-padded last slice of a wide width, and the one zero written into w above
        zeros = 16 * N if K == 16 else 9 * (128 * C._cdiv(K, 128) - K) * N if C.wide_ok(K) else 0
        assert int((want == 0).sum()) == zeros + 1


@pytest.mark.parametrize("case", C.REPEAT, ids=C.case_id)
def test_two_launches_are_bit_equal(ngan, case):
    runs = [run(ngan, case, 0)[0] for _ in range(2)]
    for k in runs[0]:
        a, b = runs[0][k].t, runs[1][k].t
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32), b.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32)), (k, case)
        assert not bool(torch.isnan(a).any()), (k, case)


def test_refusals_return_an_error_and_write_nothing(ngan):
    lib = ngan._C.lib()
    stream = torch.cuda.current_stream().cuda_stream
    B, H, W = 2, 5, 12
    x = torch.ones(B, 2 * H, 2 * W, 1040, device=DEV, dtype=torch.bfloat16)                  # large enough for every refused shape
    packed = torch.zeros(1 << 20, device=DEV)
    bias, wimg, arn = torch.zeros(128, device=DEV), torch.zeros(128, device=DEV), torch.ones(B, 2 * H, 2 * W, device=DEV)
    ay = torch.ones(B, 2 * H, 2 * W, 128, device=DEV, dtype=torch.bfloat16)
    outs = {"y": GuardedBf16((B, 2 * H, 2 * W, 128)), "rn": Guarded((B, H, W)), "img": Guarded((B, H, W))}
    p = lambda t: t.data_ptr() if t is not None else None

    def call(K=16, N=16, res=0, epi=0, om=0, b=None, aux_in=None, aux_rn=None, H_=H):
        return lib.ngan_bf16_conv3x3_fwd(p(x), p(packed), p(b), p(outs["y"].t), p(outs["rn"].t), p(aux_in), p(aux_rn), p(outs["img"].t),
                                         B, H_, W, K, N, res, epi, om, C.SLOPE, C.EPS, stream)
    cases = [(dict(N=48), SHAPE, "N=48"), (dict(K=24), SHAPE, "K=24"), (dict(K=1040), SHAPE, "K=1040"),
             (dict(epi=1, om=1), ARG, "out_mode"), (dict(epi=2, b=bias, aux_in=ay, aux_rn=arn), ARG, "no bias"),
             (dict(epi=3, N=64, aux_in=wimg), ARG, "N <= 32"), (dict(res=2), SHAPE, "even")]
    for kw, code, word in cases:
        assert call(**kw) == code, kw
        assert word in lib.ngan_last_error().decode(), (kw, lib.ngan_last_error())
    torch.cuda.synchronize()
    for k, g in outs.items():
        assert g.intact() and bool(torch.isnan(g.t).all()), f"a refused call wrote {k}"
    assert call(H_=4, res=2) == 0 and call(epi=2, aux_in=ay, aux_rn=arn) == 0                 # the same calls once legal
    torch.cuda.synchronize()
    assert outs["y"].intact() and not bool(torch.isnan(outs["y"].t.view(-1)[:B * H * W * 16]).any())
