"""Settles the constants of tests/test_gpu_optim.py on the CPU, against an emulation and never against the kernels.

1. The fp32 emulation of tests/optim_cases.py (numpy, the kernels' own order) stays at err / bound <= 0.5 on every output of every
   launch (both rules, the plain, clip and EMA forms, every case), leaves everything outside the updated tensors bit-unchanged, advances
   the counts as `adam_advance_kernel` does and gives torch's classes at non-finite gradients.  The table of constants and emulated
   ratios in that module's docstring is asserted here, and every constant is minimal: K_M - 1, K_V / 2, K_P / 2 and K_U / 2 put the
   emulation above 0.5.
2. Wrong emulations -- the bias correction from t - 1, one count shared by all tensors, 1 - powf(beta, t) in fp32, 1 - beta2 formed in
   fp32 from the rounded beta2, eps added before the 1 / sqrt(bc2) scaling, 1 / sqrt(bc2) left out, grad_scale ignored, RMSprop's eps
   under the root, a clamp that flushes NaN, an average of the clamped value (the EMA launches pass clip = 0), an infinite gradient
   kept as inf by the lerp where torch has NaN -- miss a bound or a class on a named launch each, so the cases can fail.
3. The rows with p = 0 and |p| ~ 1e-3 lr are needed: a bias correction wrong by 1e-5 relative (`1 - powf(beta, t)`) stays inside the
   bound wherever |p| >= 0.3 in the same launch.
4. The references are torch.optim.Adam / RMSprop (foreach=False) in fp64 to 1e-12 relative: one step from the preset counts of the
   step-count cases, and five consecutive steps."""
import collections

import numpy as np
import pytest
import torch

import optim_cases as O


def run(rule, name, form, clip, wrong=None, k=O.K):
    case = O.cases(rule)[name]
    t32 = torch32(rule, name) if name.startswith("nonfinite") else None
    return O.check(case, form, clip, O.emulate(case, form, clip, wrong=wrong), k=k, torch32=t32)


_t32 = {}


def torch32(rule, name):
    if (rule, name) not in _t32:
        _t32[rule, name] = O.torch_step(O.cases(rule)[name], torch.float32)
    return _t32[rule, name]


def worst_over_launches(k=O.K):
    worst, where, faults = collections.defaultdict(float), {}, []
    for rule, name, form, clip in O.launches():
        ratios, wrong = run(rule, name, form, clip, k=k)
        faults += [(rule, name, form, clip, w) for w in wrong]
        for key, v in ratios.items():
            if not v <= worst[key]:
                worst[key], where[key] = v, (rule, name, form, clip)
    return worst, where, faults


@pytest.fixture(scope="module")
def emulated():
    return worst_over_launches()


def test_emulation_leaves_a_factor_two_and_the_table_is_right(emulated):
    worst, where, faults = emulated
    for key, v in sorted(worst.items()):
        print(f"EMULATED {key}: {v:.3f} (K {O.K[key]:g}) at {where[key]}")
    assert not faults, faults
    assert set(worst) == set(O.K) == set(O.RECORDED)
    assert len(O.launches()) >= 80
    for key, v in worst.items():
        assert v <= 0.5, (key, v, where[key])
        assert abs(v - O.RECORDED[key]) < 0.005, (key, v, O.RECORDED[key])
    # the docstring's table holds these very numbers
    for key, label in (("m", "K_M"), ("v", "K_V"), ("p", "K_P"), ("u", "K_U"), ("e", "EMA")):
        row = [ln.split() for ln in O.__doc__.splitlines() if ln.split()[:1] == [label]]
        assert len(row) == 1 and float(row[0][1]) == O.K[key] and float(row[0][2]) == O.RECORDED[key], (label, row)


@pytest.mark.parametrize("key,smaller", [("m", 3.0), ("v", 4.0), ("p", 1.0), ("u", 4.0)])
def test_every_constant_is_minimal(key, smaller):
    worst, where, _ = worst_over_launches(dict(O.K, **{key: smaller}))
    print(f"EMULATED {key} at K = {smaller:g}: {worst[key]:.3f} at {where[key]}")
    out = "p" if key == "u" else key                 # K_U stands in the p' bound: the whole of it is what leaves the half
    assert worst[out] > 0.5, (key, worst[out])


WRONG = [
    # fault, rule, case, form, clip, what must go wrong: an output above its bound, or a word of check()'s complaint
    ("bc_t_minus_1", "adam", "counts_b0.5_0.999", "plain", None, "u"),
    ("bc_t_minus_1", "adam", "geometry", "ema", None, "p"),
    ("shared_count", "adam", "counts_b0.5_0.999", "plain", None, "u"),
    ("shared_count", "adam", "counts_b0.8_0.999", "clip", 0.01, "u"),
    ("powf", "adam", "counts_b0.5_0.999", "plain", None, "u"),
    ("powf", "adam", "counts_b0.8_0.999", "ema", None, "u"),
    ("omb2_fp32", "adam", "counts_b0.5_0.999", "plain", None, "v"),
    ("omb2_fp32", "adam", "scales_lr1e-05_gs0.333", "plain", None, "v"),
    ("eps_before_scale", "adam", "counts_b0.5_0.999", "plain", None, "u"),
    ("no_bc2", "adam", "counts_b0.0_0.99", "plain", None, "u"),
    ("no_bc2", "adam", "skipped_stem", "plain", None, "p"),
    ("grad_scale_ignored", "adam", "scales_lr0.002_gs0.500", "plain", None, "m"),
    ("grad_scale_ignored", "rmsprop", "scales_lr1e-05_gs0.333", "ema", None, "v"),
    ("rms_eps_under_root", "rmsprop", "counts_b0.0_0.99", "plain", None, "u"),
    ("rms_eps_under_root", "rmsprop", "scales_lr0.002_gs1.000", "clip", 0.01, "p"),
    ("clamp_flushes_nan", "adam", "nonfinite", "clip", 0.01, "classes"),
    ("clamp_flushes_nan", "rmsprop", "nonfinite", "clip", 0.01, "classes"),
    ("lerp_keeps_inf", "adam", "nonfinite", "plain", None, "classes"),
    ("ema_reads_clipped", "adam", "geometry", "ema", None, "e"),
    ("ema_reads_clipped", "rmsprop", "clip", "ema", None, "e"),
]


@pytest.mark.parametrize("wrong,rule,name,form,clip,what", WRONG)
def test_a_wrong_emulation_is_caught(wrong, rule, name, form, clip, what):
    ratios, complaints = run(rule, name, form, clip, wrong=wrong)
    print(f"WRONG {wrong} {rule} {name} {form} {clip}: {ratios} {complaints}")
    if what in O.K:
        assert ratios[what] > 1.0, (wrong, what, ratios)
    else:
        assert any(what in c for c in complaints), (wrong, what, complaints)
    good, none = run(rule, name, form, clip)
    assert max(good.values()) <= 0.5 and not none


def test_the_small_parameter_rows_are_needed():
    """`1 - powf(beta, t)` is 1e-5 off at t = 1: 0.07 ulp of a parameter of 0.3, which the final rounding hides"""
    case = O.cases("adam")["counts_b0.5_0.999"]
    got = O.emulate(case, wrong="powf")
    ref = O.reference(case)
    normal = case.updated & (np.abs(case.buf["p"]) >= 0.3) & np.isin(case.seg_of, [i for i, s in enumerate(case.segs) if s.get("p") == "normal"])
    assert normal.sum() > 200
    on_normal = O.ratio(got["p"], *ref["p"], normal)
    small = O.check(case, "plain", None, got)[0]["u"]
    print(f"powf: p' ratio where |p| >= 0.3 {on_normal:.3f}, on the small-parameter rows {small:.3f}")
    assert on_normal <= 1.0 < small


# ---- 4: torch.optim in fp64 --------------------------------------------------------------------------------------------------------
def rel(a, b, scale=1e-300):
    """relative to the reference, or to `scale` where that is larger: m' = m + w (g' - m) cancels, and an fp64 evaluation is only good
    relative to its operands there"""
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), scale)))


@pytest.mark.parametrize("rule,name", [("adam", "counts_b0.5_0.999"), ("adam", "counts_b0.8_0.999"), ("adam", "counts_b0.0_0.99"),
                                       ("adam", "scales_lr0.002_gs0.333"), ("rmsprop", "counts_b0.0_0.99"),
                                       ("rmsprop", "scales_lr1e-05_gs0.500")])
def test_reference_is_torch_in_fp64_one_step(rule, name):
    """(the count 2^24 + 1 is left to torch's double: the reference reads the fp32 count, and both corrections are 1 there)"""
    case = O.cases(rule)[name]
    ref = O.reference(case, values=case.values(exact_doubles=True))
    want = O.torch_step(case, torch.float64)
    for key in ("m", "v", "p") if rule == "adam" else ("v", "p"):
        scale = (np.abs(case.buf["m"]) + np.abs(case.buf["g"])).astype(np.float64)[case.updated] if key == "m" else 1e-300
        d = rel(ref[key][0][case.updated], want[key][case.updated], scale)
        print(f"{rule} {name} {key}: {d:.2e}")
        assert d <= 1e-12, (key, d)


@pytest.mark.parametrize("rule", ["adam", "rmsprop"])
def test_reference_is_torch_in_fp64_five_steps(rule):
    case = O.cases(rule)["geometry"]
    rng = np.random.default_rng(5)
    mine = {k: v.astype(np.float64) for k, v in case.buf.items()}
    theirs = {k: v.copy() for k, v in mine.items()}
    steps = case.seg_step.copy()
    for it in range(5):
        g = rng.standard_normal(case.total)
        mine["g"], theirs["g"] = g, g
        sub = case.copy()
        sub.set_counts(steps)
        ref = O.reference(sub, values=case.values(exact_doubles=True), buf=mine)
        out = O.torch_step(sub, torch.float64, buf=theirs, steps=steps)
        for key in ("m", "v", "p") if rule == "adam" else ("v", "p"):
            scale = (np.abs(mine["m"]) + np.abs(g))[case.updated] if key == "m" else 1e-300
            mine[key] = np.where(case.updated, ref[key][0], mine[key])
            theirs[key] = out[key]
            assert rel(mine[key][case.updated], theirs[key][case.updated], scale) <= 1e-12, (it, key)
        steps = sub.counts_after()
    assert steps.tolist() == [s + 5 * a for s, a in zip(case.seg_step.tolist(), case.seg_active.tolist())]
