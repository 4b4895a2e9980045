"""Settles the constants of tests/test_gpu_mbstd.py's kernel tests on the CPU, against emulations and never against the kernels.

Every entry point of include/ngan_mbstd.h is evaluated in numpy fp32 in the kernels' own per-feature arithmetic (tests/mbstd_cases.py:
pair sums, fma chains, correctly rounded divisions and roots, fp64 sums over the features), on the very inputs and at the very shapes the
GPU test uses, and compared with the fp64 reference: worst err / bound <= 0.5 with C_ACC = 8, so a correct fp32 implementation in
another legitimate order has a factor two in hand.  Where an emulation is above 0.5 the constant of that output is raised to the next
power of two that brings it to 0.5 or below (mbstd_cases.RAISED, with the emulated ratio); this test pins that every raise is needed,
minimal and recorded correctly."""
import collections

import numpy as np
import pytest

import mbstd_cases as M

OUTPUTS = {"mbstd_fwd/s", "mbstd_bwd/gx", "mbstd_bwdbwd/dgs", "mbstd_bwdbwd/dx", "stdfield_add/out", "stdfield_ds/gs", "stdfield_dw/gw"}


def emulate_all():
    """(output name, emulated fp32 value, (ref, absref, n_round)) for every case of the GPU module"""
    for case in M.cases():
        _, seg, grp, _, _ = case
        for family in M.families_of(case):
            d = M.inputs(family, case)
            pairs = [("mbstd_fwd", M.mbstd_fwd_emulate(d["x"], seg, grp), M.mbstd_fwd_ref(d["x"], seg, grp)),
                     ("mbstd_bwd", M.mbstd_bwd_emulate(d["gs"], d["x"], seg, grp), M.mbstd_bwd_ref(d["gs"], d["x"], seg, grp)),
                     ("mbstd_bwdbwd", M.mbstd_bwdbwd_emulate(d["h"], d["gs"], d["x"], seg, grp),
                      M.mbstd_bwdbwd_ref(d["h"], d["gs"], d["x"], seg, grp))]
            if family == "random":      # the field family does not read x
                pairs += [("stdfield_add", M.stdfield_add_emulate(d["c"], d["s"], d["w_std"], d["scale"]),
                           M.stdfield_add_ref(d["c"], d["s"], d["w_std"], d["scale"])),
                          ("stdfield_ds", M.stdfield_ds_emulate(d["g"], d["w_std"], d["scale"]), M.stdfield_ds_ref(d["g"], d["w_std"], d["scale"])),
                          ("stdfield_dw", M.stdfield_dw_emulate(d["g"], d["s"], d["scale"]), M.stdfield_dw_ref(d["g"], d["s"], d["scale"]))]
            for op, em, ref in pairs:
                for k in ref:
                    yield f"{op}/{k}", em[k], ref[k]


@pytest.fixture(scope="module")
def emulated():
    """output name -> {constant: worst err / bound over the cases} for C_ACC = 8 and its doublings"""
    worst = collections.defaultdict(lambda: collections.defaultdict(float))
    for name, got, (ref, absref, n) in emulate_all():
        assert np.isfinite(np.asarray(got, np.float64)).all(), name
        for c in (8.0, 16.0, 32.0, 64.0):
            worst[name][c] = max(worst[name][c], M.ratio(got, ref, absref, n, c))
    return worst


def test_emulated_ratios_leave_a_factor_two(emulated):
    assert set(emulated) == OUTPUTS
    for name, v in sorted(emulated.items()):
        print(f"EMULATED {name}: {v[M.c_acc(name)]:.3f} (C_ACC {M.c_acc(name):g})")
    over = {k: round(v[M.c_acc(k)], 3) for k, v in emulated.items() if v[M.c_acc(k)] > 0.5}
    assert not over, over


def test_every_raised_constant_is_needed_minimal_and_recorded(emulated):
    for key, (c, recorded) in M.RAISED.items():
        assert key in emulated, key
        v = emulated[key]
        assert c in (16.0, 32.0, 64.0) and v[c / 2] > 0.5 >= v[c], (key, dict(v))
        assert abs(v[c] - recorded) < 0.02, (key, v[c], recorded)
    assert M.C_ACC == 8.0


def test_the_cases_reach_what_they_are_named_for():
    cases = M.cases()
    assert len(cases) == len(set(cases)) == len(M.GROUPING) + 2 * len(M.SIZES) * len(M.WIDTHS) - 2      # two cases are in both lists
    ge = {c[:3]: M.group_size(c[0] // c[1], c[2]) for c in cases}
    assert [ge[g] for g in M.GROUPING] == [4, 4, 3, 1, 4, 8]
    assert {c[0] // ge[c[:3]] for c in cases} >= {1, 2, 5}                                # one group, two, one per sample
    J = sorted({c[3] * c[3] * c[4] for c in cases})
    assert J[0] == 4 and all(j % 4 == 0 for j in J)
    assert any(j % M.BLOCK_FEATURES for j in J if j > M.BLOCK_FEATURES)               # a last block that is partly empty
    assert any(j < M.BLOCK_FEATURES for j in J) and max(J) // M.BLOCK_FEATURES == 32      # one block; several blocks per group
    # the nine position classes of the field: H = 1 the centre tap alone, H = 2 four corners, H = 3 the first interior pixel
    counts = {h: sorted(set(M.tap_masks(h, h).sum((0, 1)).reshape(-1).astype(int))) for h in M.SIZES}
    assert counts[1] == [1] and counts[2] == [4] and counts[3] == [4, 6, 9] and counts[16] == [4, 6, 9]
    for case in cases:
        fams = M.families_of(case)
        assert ("constant_group" in fams) == (ge[case[:3]] in (2, 4))
        x = M.inputs("pixelnormed", case)["x"].astype(np.float64)
        assert np.allclose((x * x).mean(-1), 1.0, atol=1e-6)
        if "constant_group" in fams:
            d = M.inputs("constant_group", case)
            xg = d["x"].reshape(-1, ge[case[:3]], d["x"][0].size)
            assert (xg == xg[:, :1]).all()
            s = M.mbstd_fwd_ref(d["x"], case[1], case[2])["s"][0]
            assert np.allclose(s, 1e-4, rtol=1e-12)                                    # sigma = sqrt(eps) at every feature
            em = M.mbstd_bwd_emulate(d["gs"], d["x"], case[1], case[2])["gx"]
            assert not em.any()                                                         # d = 0 exactly under the pair sum
        assert case[0] * case[3] * case[3] * case[4] < 64 or np.abs(M.inputs("large", case)["x"]).max() > 1e3
