"""Settles the constants of tests/test_gpu_wide_f32.py on the CPU, against an emulation and never against the kernels.

1. Every per-pixel operator of tests/wide_f32_cases.py is evaluated in numpy fp32 in the summation order of csrc/wide.hip (one
   sequential sum per pixel in groups of four channels; parameter gradients sequential over the pixels), on the very inputs the
   GPU test uses, and compared with the fp64 reference: worst err / bound <= 0.5 with C_ACC = 8, so a correct fp32 implementation
   with another legitimate order (the lane-group kernels reduce as a tree) has a factor two in hand.  Where the emulation is above
   0.5 the constant of that operator and width is raised to the next power of two that brings it to 0.5 or below
   (wide_f32_cases.RAISED, with the emulated ratio); this test pins that every raise is needed, minimal and recorded correctly.
2. torch's own fp32 evaluation of every new convolution case of the GPU module stays inside run_both's tolerances (2e-4 forward and
   first order, 1e-3 second order, outlier cap 1e-4) against fp64 with the fp32 evaluation's LeakyReLU pattern: the tolerances are
   met by plain fp32 arithmetic at these contraction widths before any kernel is held to them."""
import collections

import pytest
import torch
import torch.nn.functional as F

import wide_f32_cases as W
from test_gpu_ops import SLOPE, lrelu_like, pn_ref, resample_ref, run_both
from wide_f32_cases import CONV_WIDE, PAD_CASES


def emulate_all(C, P):
    """(output name, emulated fp32 value, (ref, absref, n_round)) for every operator at (C, P)"""
    d = W.pn_inputs(C, P)
    for tag, b in (("pn_fwd", None), ("pn_fwd_bias", d["b"])):
        em = W.pn_fwd_emulate(d["c"], b)
        ref = W.pn_fwd_ref(d["c"], b, em["y"])
        yield from ((f"{tag}/{k}", em[k], ref[k]) for k in ref)
    for tag, gy2, gr in (("pn_bwd", None, None), ("pn_bwd_gr", None, d["gr"]), ("pn_bwd2", d["gy2"], None), ("pn_bwd2_gr", d["gy2"], d["gr"])):
        em = W.pn_bwd_emulate(d["gy"], gy2, gr, d["y"], d["rn_pos"])
        ref = W.pn_bwd_ref(d["gy"], gy2, gr, d["y"], d["rn_pos"])
        yield f"{tag}/gc", em["gc"], ref["gc"]
    em, ref = W.pn_bwdbwd_emulate(d["h"], d["gy"], d["y"], d["rn_pos"]), W.pn_bwdbwd_ref(d["h"], d["gy"], d["y"], d["rn_pos"])
    yield from ((f"pn_bwdbwd/{k}", em[k], ref[k]) for k in ref)
    shape = W.SHAPES[P]
    for ncol in (1, 3):
        e = W.edge_inputs(C, P, ncol)
        if ncol == 1:
            yield "channel_sum/out", W.channel_sum_emulate(e["g"])["out"], W.channel_sum_ref(e["g"])["out"]
        yield f"to_image_fwd{ncol}/t", W.to_image_fwd_emulate(e["x"], e["wimg"])["t"], W.to_image_fwd_ref(e["x"], e["wimg"])["t"]
        for tag, rn in (("to_image_bwd", None), ("to_image_bwd_pnbwd", e["rn_pos"])):
            em, ref = W.to_image_bwd_emulate(e["gt"], e["t"], e["x"], e["wimg"], rn), W.to_image_bwd_ref(e["gt"], e["t"], e["x"], e["wimg"], rn)
            yield from ((f"{tag}{ncol}/{k}", em[k], ref[k]) for k in ref)
        for pool in (0, 1):
            em, ref = W.from_image_dx_emulate(e["gimg"], e["wf"], shape, pool), W.from_image_dx_ref(e["gimg"], e["wf"], shape, pool)
            yield f"from_image_dx{ncol}_pool{pool}/gx", em["gx"], ref["gx"]
            img = e["img2"] if pool else e["img"]
            em, ref = W.from_image_dw_emulate(img, e["gimg"], pool), W.from_image_dw_ref(img, e["gimg"], pool)
            yield from ((f"from_image_dw{ncol}_pool{pool}/{k}", em[k], ref[k]) for k in ref)
    r = W.resample_inputs(C, P)
    yield "up2_adjoint/gx", W.up2_adjoint_emulate(r["g"])["gx"], W.up2_adjoint_ref(r["g"])["gx"]
    yield "up2_adjoint_pnbwd/out", W.up2_adjoint_pnbwd_emulate(r["g"], r["y"], r["rn_pos"])["out"], W.up2_adjoint_pnbwd_ref(r["g"], r["y"], r["rn_pos"])["out"]
    yield "pool2_fwd/y", W.pool2_emulate(r["g"])["y"], W.pool2_ref(r["g"])["y"]
    yield "pool2_adjoint/gx", W.pool2_adjoint_emulate(r["lo"])["gx"], W.pool2_adjoint_ref(r["lo"])["gx"]
    yield "lerp/out", W.lerp_emulate(r["a"], r["b"])["out"], W.lerp_ref(r["a"], r["b"])["out"]
    em, ref = W.fade_bwd_emulate(r["a"]), W.fade_bwd_ref(r["a"])
    yield from ((f"fade_bwd/{k}", em[k], ref[k]) for k in ref)


@pytest.fixture(scope="module")
def emulated():
    """(output name, C) -> {constant: worst err / bound over the pixel counts} for C_ACC = 8 and its doublings"""
    worst = collections.defaultdict(lambda: collections.defaultdict(float))
    for C in W.WIDTHS:
        for P in W.PIXELS:
            for name, got, (ref, absref, n) in emulate_all(C, P):
                for c in (8.0, 16.0, 32.0, 64.0):
                    worst[(name, C)][c] = max(worst[(name, C)][c], W.ratio(got, ref, absref, n, c))
    return worst


def test_emulated_ratios_leave_a_factor_two(emulated):
    over = {k: round(v[W.c_acc(*k)], 3) for k, v in emulated.items() if v[W.c_acc(*k)] > 0.5}
    for (name, C), v in sorted(emulated.items()):
        print(f"EMULATED {name} C={C}: {v[W.c_acc(name, C)]:.3f} (C_ACC {W.c_acc(name, C):g})")
    assert not over, over


def test_every_raised_constant_is_needed_minimal_and_recorded(emulated):
    for key, (c, recorded) in W.RAISED.items():
        assert key in emulated, key
        v = emulated[key]
        assert c in (16.0, 32.0, 64.0) and v[c / 2] > 0.5 >= v[c], (key, dict(v))
        assert abs(v[c] - recorded) < 0.02, (key, v[c], recorded)


@pytest.mark.parametrize("case", CONV_WIDE)
def test_torch_fp32_meets_the_conv_tolerances(case):
    t, res, scale = W.conv_tensors(case)

    def f32_op(d):
        return pn_ref(F.leaky_relu(F.conv2d(scale * resample_ref(d["x"], res), d["w"], d.get("b"), padding=1), SLOPE))

    with torch.no_grad():
        pattern = f32_op(t)
    run_both(f32_op, lambda d: pn_ref(lrelu_like(F.conv2d(scale * resample_ref(d["x"], res), d["w"], d.get("b"), padding=1), pattern)),
             t, [k for k in t if k != "x"], x_name="x", dev="cpu")


@pytest.mark.parametrize("case", PAD_CASES)
def test_torch_fp32_meets_the_padded_conv_tolerances(case):
    B, H, Wd, Cin, Cout, res, act = case
    t, res, scale = W.conv_tensors((B, H, Wd, Cin, Cout, res, True))

    def op(d, pattern=None):
        c = F.conv2d(scale * resample_ref(d["x"], res), d["w"], d["b"], padding=1)
        if not act:
            return torch.tanh(c)
        return pn_ref(F.leaky_relu(c, SLOPE) if pattern is None else lrelu_like(c, pattern))

    with torch.no_grad():
        pattern = op(t)
    run_both(op, lambda d: op(d, pattern), t, ["w", "b"], x_name="x", dev="cpu")
