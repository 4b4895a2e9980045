"""The forward / input-gradient 3x3 convolution kernels (csrc/conv3x3_generic.hip, _mid, _persist, _tile, _wino, _up2f) through the C ABI
(ngan_conv3x3_fwd_ex, ngan_conv3x3_up2_border), per element against fp64, at every one of the 323 template instances the launch switches
can produce and at the edges of their tilings -- ragged right columns and bottom rows, images of one tile and smaller than a tile,
clamped bilinear taps, whole and channel-split mid slices, every epilogue and the pool-adjoint store wherever a family offers them, the
pooled side output, walks of several tiles per workgroup, one product per output element in every split-bf16 family (where a truncating
hi / lo split shows, and only there) -- in both weight orientations.  The case list, references, bounds and
emulations are in tests/conv_fwd_cases.py; tests/test_conv_fwd_bounds_cpu.py settles the constants against emulations (never against a
kernel) and pins which instances the list reaches.

Per element, every output (y, rnorm, the ToImage result):   |got - ref| <= the epilogue's own rounding term + the first-order propagation of
      e_c = 2^-23 |c| + C_ACC 2^-24 absref (+ 2^-15 absref_direct for the split-bf16 codes 1, 2, 3)
through the epilogue; C_ACC = 8, 32 in the e_c of the direct fp32 form (conv_fwd_cases.RAISED; the epilogues' own terms keep 8); absref is the direct sum's twin, the Winograd
form's own twin for precision 4.  The LeakyReLU pattern is the stored output's, and wherever the fp64 pre-activation lies outside
|c| <= e_c the stored sign must be the fp64 sign.  The reference is evaluated in fp64 on the GPU (tests/fp64_conv.py).

Every output is prefilled with NaN and sits inside a larger allocation between two guard regions of one bit pattern, which must come
back untouched; no output element may stay NaN.  With NGAN_CONV_SKIP_BORDER the border ring must stay NaN until
ngan_conv3x3_up2_border writes it.  The pooled side output is bit-equal to ngan_pool2_fwd of the stored y.

measured on MI355X (a record, not a bound: worst err / bound per form over all cases and both orientations; in brackets the emulation of
that same case, then the CPU file's worst over its small images; 1 is the bound): direct fp32 0.318 (0.318 "seq", 0.161 "exact"; 0.285)
at C_ACC = 32, conv3x3_tile_kernel 32 -> 32 on (4, 64, 256) -- 1.27 of the bound C_ACC = 8 would give: the raise was needed, and the
fp32 MFMA behaves as the one-fma-after-the-other model does; per family generic 0.201, mid 0.215, persist 0.192, tile 0.318.
Split-bf16 0.144 (0.141; 0.142), the mid kernel with K = 16 padded, on the regular inputs; on the ten one-product cases 0.64 - 0.91
(mid 0.82, persist 0.88, tile 0.83, folded 0.91), each equal to its emulation to the three digits printed -- the split term is attainable and
these inputs come close -- where the emulation of a truncating split gives 1.5 - 2.8: the kernels and the packing round to nearest.  Winograd 0.090 (0.090 "seq", 0.057 "exact"; 0.083),
conv3x3_tile_kernel 16 -> 16 with the pool-adjoint store.  Folded bilinear 0.467 (0.467; 0.362), K = 32 without epilogue on
(16, 16, 256): the exact-fp32 border ring, at C_ACC = 8 and with 138 k elements there against 2.8 k on the small image; its folded
interior stays at 0.043.  rnorm stays below 0.10 and the ToImage result below 0.04 in every form.  No kernel missed a bound and no
stored sign contradicted fp64.  The module takes
about 10 s."""
import pytest
import torch

import conv_fwd_cases as C
from test_gpu_ops import DEV

pytestmark = pytest.mark.gpu
GUARD_BITS = 0x5A5A5A5A
GUARD = 8192            # floats before and after an output


class Guarded:
    """an output of `shape` prefilled with NaN between two guard regions"""

    def __init__(self, shape):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), GUARD_BITS, device=DEV, dtype=torch.int32)
        self.t = self.buf[GUARD:GUARD + n].view(torch.float32).view(*shape)
        self.t.fill_(float("nan"))
        self.n = n

    def intact(self):
        return bool((self.buf[:GUARD] == GUARD_BITS).all()) and bool((self.buf[GUARD + self.n:] == GUARD_BITS).all())


def run(ngan, c, mode, d=None):
    """launch the case: ({output: Guarded}, inputs on the device)"""
    ops, L = ngan.ops, ngan._C
    d = d or C.inputs(c, mode)
    dv = {k: (v.to(DEV) if v is not None else None) for k, v in d.items()}
    a = (c.B, c.H, c.W, c.K, c.N, c.res)
    packed = ops._packed(dv["w"], mode, C.scale_of(c), c.prec)
    out = {}
    if not (c.epi == 3 and c.var == "noy"):
        out["y"] = Guarded(C.y_shape(c))
        if c.epi in (1, 3):
            out["rn"] = Guarded((c.B, c.H, c.W))
    if c.epi == 3:
        out["img"] = Guarded((c.B, c.H, c.W))
    pooled = c.epi == 1 and c.om == 0 and C.pooled_output(c)
    assert pooled == (c.epi == 1 and c.om == 0 and L.conv3x3_pooled_output(*a, c.prec))
    if pooled:
        out["pooled"] = Guarded((c.B, c.H // 2, c.W // 2, c.N))
    t = lambda k: out[k].t if k in out else None
    aux_in = dv.get("ay") if c.epi == 2 else dv.get("wimg") if c.epi == 3 else None
    aux_out = t("img") if c.epi == 3 else t("pooled")
    flags = C.SKIP_BORDER if c.var == "split" else 0
    L.call("ngan_conv3x3_fwd_ex", dv["x"], packed, dv["bias"], t("y"), t("rn"), aux_in, dv.get("arn"), aux_out,
           *a, c.epi, c.om, C.SLOPE, C.EPS, c.prec, flags)
    if c.var == "split":
        ring = ~C.interior_mask(c, DEV)
        y = out["y"].t
        assert bool(torch.isnan(y[:, ring]).all()), ("NGAN_CONV_SKIP_BORDER: the border ring was written", c)
        assert not bool(torch.isnan(y[:, ~ring]).any()), ("NGAN_CONV_SKIP_BORDER: an interior element was not written", c)
        L.call("ngan_conv3x3_up2_border", dv["x"], packed, dv["bias"], y, t("rn"), c.B, c.H, c.W, c.K, c.N, c.epi, C.SLOPE, C.EPS)
    return out, d


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_conv_fwd_every_instance_against_fp64(ngan, case):
    c = case
    # what ngan_conv3x3_kernel_name says of this call against the replica of the routing.  This is not an observation of the kernel the
    # launcher ran: ngan_conv3x3_kernel_name and the switch in ngan_conv3x3_fwd_ex are separate code, tied together only by reading both
    # (they agree since the generic kernel's epilogue 2 was corrected in the former; tests/test_conv_fwd_bounds_cpu.py sweeps the pair)
    name = ngan._C.conv3x3_kernel_name(c.B, c.H, c.W, c.K, c.N, c.res, c.epi, c.om, c.prec)
    assert name == C.kernel_name(c)
    bad = []
    for mode in C.modes(c):
        out, d = run(ngan, c, mode)
        for k, g in out.items():
            assert g.intact(), ("wrote outside the output", k, c, mode)
            assert not bool(torch.isnan(g.t).any()), ("unwritten or NaN element", k, c, mode)
        stored = out["y"].t if "y" in out else None
        ref = C.reference(c, mode, d, stored_y=stored if c.epi in (1, 3) else None, dev=DEV)
        stats = {k: C.ratio(out[k].t, *ref[k]) for k in ("y", "rn", "img") if k in out}
        if c.epi in (1, 3):
            assert C.undecided_fraction(*ref["_c"]) <= 1e-4, (c, mode)
            if stored is not None:
                nv = C.sign_violations(*ref["_c"], stored)
                if nv:
                    bad.append((mode, "sign", nv))
        if "pooled" in out:
            assert torch.equal(out["pooled"].t, ngan.ops._pooled(out["y"].t)), ("the pooled side output is not ngan_pool2_fwd of the stored y", c, mode)
        print(f"STAT conv_fwd {C.FORM[c.prec]} {name} {C.case_id(c)} mode {mode}: err/bound " + " ".join(f"{k} {v:.3f}" for k, v in stats.items()))
        bad += [(mode, k, v) for k, v in stats.items() if not v <= 1.0]
    assert not bad, (c, name, C.second_launch(c), bad)


@pytest.mark.parametrize("case", C.WALK, ids=C.case_id)
def test_several_tiles_per_workgroup_are_bit_reproducible(ngan, case):
    runs = [run(ngan, case, 0)[0] for _ in range(2)]
    for k in runs[0]:
        a, b = runs[0][k].t, runs[1][k].t
        assert torch.equal(a, b) and not bool(torch.isnan(a).any()), (k, case)


@pytest.mark.parametrize("case", [c for c in C.UP2F if c.var == "split"], ids=C.case_id)
def test_folded_interior_plus_border_equals_the_one_call_form(ngan, case):
    pair = run(ngan, case, 0)[0]
    one = run(ngan, case._replace(var=""), 0, d=C.inputs(case, 0))[0]
    assert set(pair) == set(one)
    for k in pair:
        assert torch.equal(pair[k].t, one[k].t) and pair[k].intact() and one[k].intact(), (k, case)
