"""Settles the constants of tests/test_gpu_wgan_kernels.py on the CPU, against emulations and never against the kernels.

1. Every operator of tests/wgan_cases.py is evaluated in numpy fp32 in a legitimate order (the convolutions sequential over (tap,
   channel), the weight gradient sequential inside a k-split and then over the splits, the reductions sequential inside a chunk and then
   over the chunks, the stem sequential over k or the batch) on the very inputs the GPU module uses, and compared with the fp64
   reference: worst err / bound <= 0.5 with C_ACC = 8, so a correct kernel with another order (the MFMA's internal one, a butterfly)
   keeps a factor two.  Where the emulation is above 0.5 that (output, case) is raised to the next power of two (wgan_cases.RAISED);
   every raise is pinned as needed, minimal and recorded.
2. The BatchNorm statistics are emulated as the operation, centred two-pass.  The one-pass form about the pivot y[0, c]
   (var = s1 / n - (s0 / n)^2 of the shifted values) is emulated next to it as a record: its worst err / bound is rstd 13.44, scale
   11.76, shift 17.61 (C5-npix3278), running_var 8.86 and running_mean 1.44 (C257-npix64), mean 2.85 (C129-npix129): every one at a
   channel whose first pixel lies six sigma out, where s1 / n - (s0 / n)^2 cancels by a factor 73.  The kernel had that form; the GPU
   run confirmed the figures (tests/test_gpu_wgan_kernels.py) and ngan_bn_stats now checks its fp32 moments against fp64 ones.
3. Mutants: deliberately wrong emulations, each of which must exceed ratio 1 on the case the test names."""
import collections

import numpy as np
import pytest

import wgan_cases as W

CONSTANTS = (8.0, 16.0, 32.0, 64.0)


def conv_outputs(case, mutant=None):
    d = W.conv_inputs(case)
    refs, em = W.conv_refs(d), W.conv_emulate(d, mutant)
    return [(f"s2_{case[0]}/{k}", em[k], refs[k]) for k in refs]


def wgrad_outputs(case, mutant=None):
    d = W.wgrad_inputs(case)
    return [("s2_wgrad/dw", W.wgrad_emulate(d["half"], d["full"], d["half_xf"], d["full_xf"], mutant), W.wgrad_refs(d)["dw"])]


def red_outputs(case, mutant=None, onepass=False, npix=None, stats_only=False):
    return list(W.red_chain(W.red_inputs(case, npix), W.red_options(case), W.Emulated(mutant, onepass), stats_only))


def stem_outputs(case, mutant=None):
    d = W.stem_inputs(case)
    refs, em = W.stem_refs(d), W.stem_emulate(d, mutant)
    return [(f"stem/{k}", em[k], refs[k]) for k in refs]


def point_outputs(n):
    d = W.tanh_bwd_inputs(n)
    yield "tanh_bwd/o", W.tanh_bwd_emulate(d)["o"], W.tanh_bwd_refs(d)["o"]
    d = W.apply_inputs(n)
    xf = d["xf"]
    yield "bn_act_apply/a", W.bn_apply_emulate(d["y"], *xf)["a"], W.bn_apply_refs(d["y"], *xf)["a"]


def fold_outputs(C):
    d = W.fold_inputs(C)
    refs, em = W.fold_refs(d), W.fold_emulate(d)
    return [(f"bn_fold_eval/{k}", em[k], refs[k]) for k in refs]


def every_output():
    """(case id, output name, emulated value, (ref, absref, n_round)) for every operator and case of the GPU module"""
    for case in W.CONV_CASES:
        yield from ((W.conv_id(case),) + o for o in conv_outputs(case))
    for case in W.WGRAD_CASES:
        yield from ((W.wgrad_id(case),) + o for o in wgrad_outputs(case))
    for case in W.RED_CASES:
        yield from ((W.red_id(case),) + o for o in red_outputs(case))
    yield from (("C%d-npix%d" % W.BIG_CASE,) + o for o in red_outputs((W.BIG_CASE[0], None), npix=W.BIG_CASE[1]))
    for case in W.STEM_CASES:
        yield from ((W.stem_id(case),) + o for o in stem_outputs(case))
    for n in W.POINT_N:
        yield from ((f"n{n}",) + o for o in point_outputs(n))
    for C in W.FOLD_C:
        yield from ((f"C{C}",) + o for o in fold_outputs(C))


@pytest.fixture(scope="module")
def emulated():
    """(output name, case id) -> {constant: worst err / bound} for C_ACC = 8 and its doublings"""
    worst = collections.defaultdict(lambda: collections.defaultdict(float))
    for cid, name, got, (ref, absref, n) in every_output():
        for c in CONSTANTS:
            worst[(name, cid)][c] = max(worst[(name, cid)][c], W.ratio(got, ref, absref, n, c))
    return worst


def test_emulated_ratios_leave_a_factor_two(emulated):
    over = {k: round(v[W.c_acc(*k)], 3) for k, v in emulated.items() if v[W.c_acc(*k)] > 0.5}
    for (name, cid), v in sorted(emulated.items()):
        print(f"EMULATED {name} {cid}: {v[W.c_acc(name, cid)]:.3f} (C_ACC {W.c_acc(name, cid):g})")
    per_op = collections.defaultdict(float)
    for (name, cid), v in emulated.items():
        per_op[name] = max(per_op[name], v[W.c_acc(name, cid)])
    print("EMULATED worst per operator:", {k: round(v, 3) for k, v in sorted(per_op.items())})
    assert not over, over


def test_every_raised_constant_is_needed_minimal_and_recorded(emulated):
    for key, (c, recorded) in W.RAISED.items():
        assert key in emulated, key
        v = emulated[key]
        assert c in CONSTANTS[1:] and v[c / 2] > 0.5 >= v[c], (key, dict(v))
        assert abs(v[c] - recorded) < 0.02, (key, v[c], recorded)


def test_plans_match_the_issue():
    """K = 297 makes three splits with a ragged last one; C = 1024 at 16400 pixels takes red_chunk's re-chunking branch"""
    assert W.wgrad_plan(3, 9, 11, 20, 33)[:2] == (3, 100) and W.wgrad_plan(3, 3, 5, 20, 33)[0] == 1
    assert -(-W.BIG_CASE[1] // -(-16384 // W.BIG_CASE[0])) > 1024 and W.red_plan(W.BIG_CASE[1], W.BIG_CASE[0]) == (17, 965)
    assert W.red_plan(55, 300) == (55, 1) and W.red_plan(56, 300) == (55, 2)


def test_case_lists_cover_what_the_issue_names():
    cs = {c[2] for c in W.CONV_CASES}
    ms = {c[3] for c in W.CONV_CASES}
    assert cs == {1, 3, 4, 12, 20, 48} and ms == {1, 3, 17, 33, 65, 100}
    for d in ("down", "up"):
        mine = [c for c in W.CONV_CASES if c[0] == d]
        assert 16 <= len(mine) <= 20
        paths = {(c[2] % 4 == 0, 4 if c[3] > 32 else 2 if c[3] > 16 else 1) for c in mine}
        assert len(paths) == 6, paths
        assert {c[4] for c in mine} == set(W.XF_KINDS) and {c[5] for c in mine} == {True, False} and {c[1] for c in mine} == set(W.GRIDS)
    assert {(c[0], c[3]) for c in W.WGRAD_CASES} >= {(297, "half"), (297, "full"), (297, "neither"), (1, "half"), (45, "full")}
    opts = [W.red_options(c) for c in W.RED_CASES]
    for key in ("momentum", "eps", "track", "bwd", "want_affine"):
        assert len({o[key] for o in opts}) == (3 if key == "bwd" else 2), key
    assert {c[4] for c in W.STEM_CASES} == {"gw", "gb", "both"}


def worst_of(outputs, name):
    return max(W.ratio(got, ref, absref, n) for nm, got, (ref, absref, n) in outputs if nm == name)


def conv_case(cid):
    return next(c for c in W.CONV_CASES if W.conv_id(c) == cid)


# mutant -> [(the case that catches it, the output it shows in)]
CONV_MUTANTS = {
    "hw_swap": [("down-g45-C4-M3-affine_act-bias", "s2_down/y"), ("up-strip-C20-M17-none-bias", "s2_up/y"), ("down-narrow-C12-M1-none-nobias", "s2_down/dx")],
    "pad_first": [("down-g1-C3-M3-affine_act-bias", "s2_down/y"), ("up-g45-C48-M100-affine-bias", "s2_up/y"), ("down-g45-C1-M33-affine-nobias", "s2_down/dw")],
    "drop_chan": [("down-g45-C3-M17-act-bias", "s2_down/y"), ("down-g1-C20-M33-affine-nobias", "s2_down/y"), ("up-strip-C20-M17-none-bias", "s2_up/y")],
    "mask_m": [("down-g45-C12-M17-affine_act-nobias", "s2_down/y"), ("up-narrow-C3-M65-affine_act-bias", "s2_up/y")],
}


@pytest.mark.parametrize("mutant", sorted(CONV_MUTANTS))
def test_conv_mutants_are_caught(mutant):
    for cid, name in CONV_MUTANTS[mutant]:
        case = conv_case(cid)
        # padding before the transform reaches the weight gradient through its `full` operand
        r = _padded_wgrad_ratio(case) if name.endswith("/dw") else worst_of(conv_outputs(case, mutant), name)
        print(f"MUTANT {mutant} {cid} {name}: {r:.3g}")
        assert r > 1.0, (mutant, cid, name, r)
        assert worst_of(conv_outputs(case), name) <= 0.5


def _padded_wgrad_ratio(case):
    """the weight gradient of a down layer with the transform applied to the zero border of `full` as well: emulated by transforming a
    padded copy, which the correct emulation pads again (the second border meets no tap)"""
    d = W.conv_inputs(case)
    B, H, Wd, C = d["x"].shape
    full = W.xf_emulate(np.pad(d["x"], ((0, 0), (1, 1), (1, 1), (0, 0))), d["xf"])
    Hh, Wh = H // 2, Wd // 2
    K = B * Hh * Wh
    h2 = d["g"].reshape(K, -1)
    dw = np.zeros((h2.shape[1], C, 4, 4), np.float32)
    for ky in range(4):
        for kx in range(4):
            t = full[:, ky:ky + 2 * Hh:2, kx:kx + 2 * Wh:2, :].reshape(K, C)
            acc = np.zeros((h2.shape[1], C), np.float32)
            for k in range(K):
                acc = acc + h2[k][:, None] * t[k][None, :]
            dw[:, :, ky, kx] = acc
    ref, absref, n = W.conv_refs(d)["dw"]
    return W.ratio(dw, ref, absref, n)


def test_dropped_last_split_is_caught():
    case = next(c for c in W.WGRAD_CASES if W.wgrad_id(c) == "K297-CH20-CF33-full-affine_act")
    r = worst_of(wgrad_outputs(case, "drop_split"), "s2_wgrad/dw")
    print(f"MUTANT drop_split {W.wgrad_id(case)}: {r:.3g}")
    assert r > 1.0 and worst_of(wgrad_outputs(case), "s2_wgrad/dw") <= 0.5


def test_biased_running_variance_is_caught():
    """at the largest pixel count of the list n / (n - 1) is 1 + 6e-5, still far outside the bound"""
    for cid in ("C3-npix5463", "C129-npix2"):
        case = next(c for c in W.RED_CASES if W.red_id(c) == cid)
        assert W.red_options(case)["track"], cid
        r = worst_of(red_outputs(case, "biased_running", stats_only=True), "bn_stats/running_var")
        print(f"MUTANT biased_running {cid}: {r:.3g}")
        assert r > 1.0, (cid, r)


def test_skipped_last_pass_is_caught():
    case = next(c for c in W.RED_CASES if W.red_id(c) == "C300-npix7")
    outs = red_outputs(case, "skip_pass")
    for name in ("bn_stats/mean", "bn_stats/scale", "chan_sum/out"):
        r = worst_of(outs, name)
        print(f"MUTANT skip_pass C300-npix7 {name}: {r:.3g}")
        assert r > 1.0, (name, r)


def test_stem_bias_gradient_one_row_short_is_caught():
    for cid in ("K130-B65-S9-C5-both", "K65-B1-S1-C1-both"):
        case = next(c for c in W.STEM_CASES if W.stem_id(c) == cid)
        r = worst_of(stem_outputs(case, "gb_rows"), "stem/gb")
        print(f"MUTANT gb_rows {cid}: {r:.3g}")
        assert r > 1.0 and worst_of(stem_outputs(case), "stem/gb") <= 0.5


def test_one_pass_variance_about_the_first_pixel_against_the_bound():
    """a record and a discrimination check: the pivoted one-pass form on the statistics cases, per output, next to the two-pass form"""
    worst = collections.defaultdict(lambda: (0.0, None))
    for case in W.RED_CASES:
        for name, got, (ref, absref, n) in red_outputs(case, onepass=True, stats_only=True):
            r = W.ratio(got, ref, absref, n)
            if r > worst[name][0]:
                worst[name] = (r, W.red_id(case))
    for name, (r, cid) in sorted(worst.items()):
        print(f"ONEPASS {name}: {r:.3f} at {cid}")
    assert worst["bn_stats/rstd"][0] > 1.0, "the bound no longer tells the pivoted one-pass variance in fp32 from the operation"
