"""The generator stem, the critic head (csrc/linear.hip) and the scalar heads of the losses (csrc/pointwise.hip) through the C ABI,
kernel by kernel and per element against fp64, at the smallest shapes that reach every branch of their dispatch: the stem forward's
unrolled k-groups and its tail, a fifth channel tile, C < 16 and the raised dynamic-LDS launch; both weight-gradient forms (MFMA with
nt < NT and accumulate, row-streaming with every waves-per-row count, both rows_per_block and a ragged last block); the head's three
forward paths (LDS, LDS + tail loop, no LDS), the grid-stride second trip of its input gradient, every accumulate code of its weight
gradient; the scalar heads past one wave, past one 256-stride trip and past the 64-chunk cap; ngan_axpby.  The fp32 and the
bf16-storage entry points run on the same shapes (bf16-representable activation operands, so the fp64 reference on them is exact).

Per element   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref   (+ 2^-8 |ref| for an output stored as bf16),   C_ACC = 8,
n_round and absref derived per output in tests/stem_head_cases.py.  The constants were settled on the CPU against fp32 emulations in
the kernels' summation order (tests/test_stem_head_bounds_cpu.py: every emulated ratio <= 0.5; one raise, the stored stem weight
gradient -> C_ACC 16), never against a kernel.  Every output buffer starts as NaN, so an element no thread wrote fails the comparison.

measured on MI355X (a record, not a bound: worst err / bound per entry point over all of its cases, fp32 / bf16 storage; 1 is the
bound): linear_lrelu_pn_fwd y 0.34 / 0.994 rn 0.20 / 0.20; linear_wgrad 0.32 / 0.38 (at
C_ACC 16), linear_wgrad_acc 0.47 / 0.52; linear_dgrad 0.44 / 0.44; final_dot_fwd 0.05 / 0.04; final_dot_dx 0.16 / 0.996; final_dot_dw gW
0.28 / 0.25 gb 0.09 / 0.09, _acc gW 0.17 / 0.23 gb 0.08 / 0.08; wloss_head loss 0.09 mean_real 0.05 mean_fake 0.02; wloss_head_bwd 0.22;
gp_head 0.13; gp_coef 0.16; sample_l2norm 0.13; scale_rows 0.10; xhat 0.25; latent_normalize 0.16; axpby 0.18, b null 0.09; lerp 0.17;
fade_bwd 0.08.  The two figures at the bound are the bf16 stores themselves: round-to-nearest of an 8-bit significand reaches 2^-8 |ref|
just above a power of two, and the bound's other terms are 2^-15 of that.  The fp32 figures of the stem are the emulation's to three
digits (0.340, 0.322, 0.466, 0.444): no kernel needed a fix and no constant moved.  The module takes 7 s."""
import numpy as np
import pytest
import torch

import stem_head_cases as S
import wide_f32_cases as W
from test_gpu_ops import DEV

pytestmark = pytest.mark.gpu
SLOPE, EPS = S.SLOPE, S.EPS
SENTINEL = 7.0


def dv(a, bf=False):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(torch.bfloat16) if bf else t


def nans(*shape, bf=False):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.bfloat16 if bf else torch.float32)


def host(t):
    return t.detach().float().cpu().numpy()


def name_of(op, bf):
    return ("ngan_bf16_" if bf else "ngan_") + op


class Checker:
    """collects err / bound of every output of one test and asserts at the end, so that one run shows every figure"""

    def __init__(self, case):
        self.case, self.bad = case, []

    def __call__(self, name, got, ref, bf=False, key=None):
        r, a, n = ref
        worst = S.ratio(host(got), r, a, n, S.c_acc(key or name))
        print(f"STAT stem_head {name}{' bf16' if bf else ''} {self.case}: {worst:.3f}")
        if not worst <= 1.0:
            self.bad.append((name, "bf16" if bf else "f32", worst))

    def done(self):
        assert not self.bad, (self.case, self.bad)


# ---- generator stem ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K,Sp,C", S.STEM_FWD + S.STEM_FWD_RAISED_LDS)
def test_linear_lrelu_pn_fwd_against_fp64(ngan, B, K, Sp, C):
    """ngan_linear_lrelu_pn_fwd / ngan_bf16_linear_lrelu_pn_fwd: y and rnorm; the rows b >= B of the last 16-sample chunk are not written"""
    call = ngan._C.call
    d = S.stem_inputs(K, Sp, C)
    z, w = d["z"][:B], d["w"]
    ck = Checker((B, K, Sp, C))
    for bf in (False, True):
        y, rn = nans(B + 1, Sp, C, bf=bf), nans(B + 1, Sp)
        y[B], rn[B] = SENTINEL, SENTINEL
        call(name_of("linear_lrelu_pn_fwd", bf), dv(z), dv(w), y, rn, B, K, Sp, C, S.STEM_SCALE, SLOPE, EPS)
        assert bool((y[B] == SENTINEL).all()) and bool((rn[B] == SENTINEL).all()), ("wrote past the batch", bf)
        ref = S.linear_fwd_ref(z, w, Sp, C, S.STEM_SCALE, host(y[:B]))
        ck("linear_lrelu_pn_fwd/y", y[:B], S.stored(ref["y"], S.BF16_STORE if bf else 0), bf)
        ck("linear_lrelu_pn_fwd/rn", rn[:B], ref["rn"], bf)
    ck.done()


def _wgrad_case(ngan, B, K, Sp, C, with_acc):
    call = ngan._C.call
    d = S.stem_inputs(K, Sp, C)
    rows = C * Sp
    ck = Checker((B, K, Sp, C))
    for bf in (False, True):
        z, gc = d["z"][:B], d["gc"][:B]
        if bf:
            gc = S.bf16(gc)
        ref = S.linear_wgrad_ref(z, gc, S.STEM_SCALE)["gW"]
        gw = nans(rows, K)
        call(name_of("linear_wgrad", bf), dv(z), dv(gc, bf), gw, B, K, Sp, C, S.STEM_SCALE)
        ck("linear_wgrad/gW", gw, ref, bf)
        gw = nans(rows, K)
        call(name_of("linear_wgrad_acc", bf), dv(z), dv(gc, bf), gw, B, K, Sp, C, S.STEM_SCALE, 0)
        ck("linear_wgrad_acc(0)/gW", gw, ref, bf, key="linear_wgrad/gW")
        if with_acc:
            gw = dv(d["buf"])
            call(name_of("linear_wgrad_acc", bf), dv(z), dv(gc, bf), gw, B, K, Sp, C, S.STEM_SCALE, 1)
            ck("linear_wgrad_acc/gW", gw, S.plus(ref, d["buf"]), bf)
    ck.done()


@pytest.mark.parametrize("B,K,Sp,C", S.WGRAD_MFMA)
def test_linear_wgrad_mfma_form_against_fp64(ngan, B, K, Sp, C):
    """ngan_linear_wgrad / ngan_linear_wgrad_acc (accumulate 0 and 1, the latter into a random buffer) and their bf16 twins where the
    MFMA form runs: K a multiple of 16, at most 512"""
    _wgrad_case(ngan, B, K, Sp, C, True)


@pytest.mark.parametrize("B,K,Sp,C", S.WGRAD_ROWS)
def test_linear_wgrad_row_streaming_form_against_fp64(ngan, B, K, Sp, C):
    """ngan_linear_wgrad / ngan_linear_wgrad_acc (accumulate 0) and their bf16 twins where the row-streaming form runs: K > 512 or K not
    a multiple of 16"""
    _wgrad_case(ngan, B, K, Sp, C, False)


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("K", S.WGRAD_ACC_REFUSED)
def test_linear_wgrad_acc_refuses_the_row_streaming_widths(ngan, K, bf):
    """accumulate = 1 exists in the MFMA form only: a negative status and a message elsewhere, and the buffer untouched"""
    d = S.stem_inputs(K, 9, 20)
    gw = dv(d["buf"])
    with pytest.raises(RuntimeError, match=r"status -\d+: .*accumulate needs K <= 512"):
        ngan._C.call(name_of("linear_wgrad_acc", bf), dv(d["z"][:3]), dv(d["gc"][:3], bf), gw, 3, K, 9, 20, S.STEM_SCALE, 1)
    assert np.array_equal(host(gw), d["buf"])


@pytest.mark.parametrize("B,K,Sp,C", S.DGRAD)
def test_linear_dgrad_against_fp64(ngan, B, K, Sp, C):
    """ngan_linear_dgrad / ngan_bf16_linear_dgrad"""
    d = S.stem_inputs(K, Sp, C)
    ck = Checker((B, K, Sp, C))
    for bf in (False, True):
        gc = S.bf16(d["gc"][:B]) if bf else d["gc"][:B]
        gz = nans(B, K)
        ngan._C.call(name_of("linear_dgrad", bf), dv(gc, bf), dv(d["w"]), gz, B, K, Sp, C, S.STEM_SCALE)
        ck("linear_dgrad/gz", gz, S.linear_dgrad_ref(gc, d["w"], S.STEM_SCALE)["gz"], bf)
    ck.done()


# ---- critic head ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,S2,C", S.HEAD_FWD)
def test_final_dot_fwd_against_fp64(ngan, B, S2, C):
    """ngan_final_dot_fwd / ngan_bf16_final_dot_fwd, bias null and non-null"""
    d = S.head_inputs(S2, C)
    ck = Checker((B, S2, C))
    for bf in (False, True):
        y = S.bf16(d["y"][:B]) if bf else d["y"][:B]
        for bias in (None, d["bias"]):
            out = nans(B)
            ngan._C.call(name_of("final_dot_fwd", bf), dv(y, bf), dv(d["w"]), dv(bias), out, B, S2, C, S.HEAD_SCALE)
            ck("final_dot_fwd/out", out, S.final_dot_fwd_ref(y, d["w"], bias, S.HEAD_SCALE)["out"], bf)
    ck.done()


@pytest.mark.parametrize("B,S2,C", S.HEAD_DX)
def test_final_dot_dx_against_fp64(ngan, B, S2, C):
    """ngan_final_dot_dx / ngan_bf16_final_dot_dx"""
    d = S.head_inputs(S2, C)
    ck = Checker((B, S2, C))
    ref = S.final_dot_dx_ref(d["go"][:B], d["w"], S.HEAD_SCALE)["gy"]
    for bf in (False, True):
        gy = nans(B, S2, C, bf=bf)
        ngan._C.call(name_of("final_dot_dx", bf), dv(d["go"][:B]), dv(d["w"]), gy, B, S2, C, S.HEAD_SCALE)
        ck("final_dot_dx/gy", gy, S.stored(ref, S.BF16_STORE if bf else 0), bf)
    ck.done()


@pytest.mark.parametrize("B,S2,C", S.HEAD_DW)
def test_final_dot_dw_against_fp64(ngan, B, S2, C):
    """ngan_final_dot_dw (with gb and with gb null), ngan_final_dot_dw_acc with accumulate 0, 1 (gW +=), 2 (gb +=), 3 and their bf16 twins"""
    call = ngan._C.call
    d = S.head_inputs(S2, C)
    ck = Checker((B, S2, C))
    go = d["go"][:B]
    for bf in (False, True):
        y = S.bf16(d["y"][:B]) if bf else d["y"][:B]
        ref = S.final_dot_dw_ref(y, go, S.HEAD_SCALE)
        gw, gb = nans(C, S2), nans(1)
        call(name_of("final_dot_dw", bf), dv(y, bf), dv(go), gw, gb, B, S2, C, S.HEAD_SCALE)
        ck("final_dot_dw/gW", gw, ref["gW"], bf)
        ck("final_dot_dw/gb", gb, ref["gb"], bf)
        gw = nans(C, S2)
        call(name_of("final_dot_dw", bf), dv(y, bf), dv(go), gw, None, B, S2, C, S.HEAD_SCALE)
        ck("final_dot_dw/gW", gw, ref["gW"], bf)
        for acc in (0, 1, 2, 3):
            gw = dv(d["bufw"]) if acc & 1 else nans(C, S2)
            gb = dv(d["bufb"]) if acc & 2 else nans(1)
            call(name_of("final_dot_dw_acc", bf), dv(y, bf), dv(go), gw, gb, B, S2, C, S.HEAD_SCALE, acc)
            if acc & 1:
                ck("final_dot_dw_acc/gW", gw, S.plus(ref["gW"], d["bufw"]), bf)
            else:
                ck("final_dot_dw_acc(0)/gW", gw, ref["gW"], bf, key="final_dot_dw/gW")
            if acc & 2:
                ck("final_dot_dw_acc/gb", gb, S.plus(ref["gb"], d["bufb"]), bf)
            else:
                ck("final_dot_dw_acc(0)/gb", gb, ref["gb"], bf, key="final_dot_dw/gb")
    ck.done()


# ---- scalar heads of the losses ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drift", S.DRIFTS)
@pytest.mark.parametrize("n_real,n_fake", S.WLOSS)
def test_wloss_head_and_bwd_against_fp64(ngan, n_real, n_fake, drift):
    """ngan_wloss_head; ngan_wloss_head_bwd with all three output gradients and with each of them null in turn"""
    call = ngan._C.call
    d = S.wloss_inputs(n_real, n_fake)
    ck = Checker((n_real, n_fake, drift))
    scores = dv(d["scores"])
    loss, mr, mf = nans(1), nans(1), nans(1)
    call("ngan_wloss_head", scores, n_real, n_fake, drift, loss, mr, mf)
    ref = S.wloss_head_ref(d["scores"], n_real, n_fake, drift)
    ck("wloss_head/loss", loss, ref["loss"])
    ck("wloss_head/mean_real", mr, ref["mean_real"])
    ck("wloss_head/mean_fake", mf, ref["mean_fake"])
    g = d["g"]
    for gl, gr, gf in ((g[0], g[1], g[2]), (None, g[1], g[2]), (g[0], None, g[2]), (g[0], g[1], None)):
        gs = nans(n_real + n_fake)
        ptr = [None if v is None else dv(np.array([v], np.float32)) for v in (gl, gr, gf)]
        call("ngan_wloss_head_bwd", scores, n_real, n_fake, drift, ptr[0], ptr[1], ptr[2], gs)
        ck("wloss_head_bwd/gs", gs, S.wloss_head_bwd_ref(d["scores"], n_real, n_fake, drift, gl, gr, gf)["gs"])
    ck.done()


@pytest.mark.parametrize("B", S.GP_B)
def test_gp_head_and_coef_against_fp64(ngan, B):
    """ngan_gp_head / ngan_gp_coef, norms in [0.5, 1.5)"""
    d = S.gp_inputs(B)
    ck = Checker((B,))
    norms = dv(d["norms_pos"])
    out, coef = nans(1), nans(B)
    ngan._C.call("ngan_gp_head", norms, B, S.LAMBDA, out)
    ck("gp_head/out", out, S.gp_head_ref(d["norms_pos"], S.LAMBDA)["out"])
    ngan._C.call("ngan_gp_coef", norms, B, S.LAMBDA, dv(d["g"]), coef)
    ck("gp_coef/coef", coef, S.gp_coef_ref(d["norms_pos"], S.LAMBDA, d["g"][0])["coef"])
    ck.done()


@pytest.mark.parametrize("B,n", S.L2NORM)
def test_sample_l2norm_against_fp64(ngan, B, n):
    """ngan_sample_l2norm: one chunk, n % 4 != 0 (allowed for B = 1: the tail on block 0), the 64-chunk cap and just past it"""
    d = S.l2norm_inputs(B, n)
    ck = Checker((B, n))
    norms, ws = nans(B), nans(64 * B)
    ngan._C.call("ngan_sample_l2norm", dv(d["g"]), norms, ws, B, n)
    ck("sample_l2norm/norms", norms, S.sample_l2norm_ref(d["g"])["norms"])
    ck.done()


@pytest.mark.parametrize("n", S.ROWS_N)
@pytest.mark.parametrize("B", S.ROWS_B)
def test_scale_rows_and_xhat_against_fp64(ngan, B, n):
    """ngan_scale_rows / ngan_xhat: 70000 is past the 256-block cap of their grids (the grid-stride second trip)"""
    d = S.rows_inputs(B, n)
    ck = Checker((B, n))
    out = nans(B, n)
    ngan._C.call("ngan_scale_rows", dv(d["g"]), dv(d["coef"]), out, B, n)
    ck("scale_rows/out", out, S.scale_rows_ref(d["g"], d["coef"])["out"])
    out = nans(B, n)
    ngan._C.call("ngan_xhat", dv(d["real"]), dv(d["fake"]), dv(d["eps"]), out, B, n)
    ck("xhat/out", out, S.xhat_ref(d["real"], d["fake"], d["eps"])["out"])
    ck.done()


@pytest.mark.parametrize("dim", S.LATENT_DIMS)
@pytest.mark.parametrize("rows", S.LATENT_ROWS)
def test_latent_normalize_against_fp64(ngan, rows, dim):
    """ngan_latent_normalize (in place): draws scaled by 3 so that the clamp at 5 acts"""
    d = S.latent_inputs(rows, dim)
    if dim >= 64:
        assert (np.abs(d["z"]) > S.LATENT_CLAMP).any()
    ck = Checker((rows, dim))
    z = dv(d["z"])
    ngan._C.call("ngan_latent_normalize", z, rows, dim, S.LATENT_CLAMP)
    ref = S.latent_normalize_ref(d["z"], S.LATENT_CLAMP)["z"]
    ck("latent_normalize/z", z, ref)
    got, hit = host(z), np.abs(d["z"]) > S.LATENT_CLAMP
    for r in range(rows):       # the clamp is visible in the result: the clamped elements of a row share one magnitude, bit for bit
        if hit[r].any():
            assert np.ptp(np.abs(got[r][hit[r]])) == 0.0, r
    ck.done()


@pytest.mark.parametrize("n", S.AXPBY_N)
def test_axpby_against_fp64(ngan, n):
    """ngan_axpby with b and with b null; 1100000 is past the 4096-block cap of the elementwise grids"""
    d = S.ew_inputs(n)
    ck = Checker((n,))
    out = nans(n)
    ngan._C.call("ngan_axpby", dv(d["a"]), dv(d["b"]), S.CA, S.CB, out, n)
    ck("axpby/out", out, S.axpby_ref(d["a"], d["b"], S.CA, S.CB)["out"])
    out = nans(n)
    ngan._C.call("ngan_axpby", dv(d["a"]), None, S.CA, S.CB, out, n)
    ck("axpby_null/out", out, S.axpby_ref(d["a"], None, S.CA, S.CB)["out"])
    ck.done()


@pytest.mark.parametrize("n", S.LERP_N)
def test_lerp_and_fade_bwd_past_the_grid_cap_against_fp64(ngan, n):
    """ngan_lerp / ngan_fade_bwd at one element and past the 4096-block cap (references: tests/wide_f32_cases.py)"""
    d = S.ew_inputs(n)
    ck = Checker((n,))
    alpha = torch.tensor([W.ALPHA], device=DEV)
    out = nans(n)
    ngan._C.call("ngan_lerp", dv(d["a"]), dv(d["b"]), alpha, out, n)
    ck("lerp/out", out, W.lerp_ref(d["a"], d["b"])["out"])
    ga, gb = nans(n), nans(n)
    ngan._C.call("ngan_fade_bwd", dv(d["a"]), alpha, ga, gb, n)
    ref = W.fade_bwd_ref(d["a"])
    ck("fade_bwd/ga", ga, ref["ga"])
    ck("fade_bwd/gb", gb, ref["gb"])
    ck.done()
