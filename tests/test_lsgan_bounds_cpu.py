"""Settles the constants of tests/test_gpu_lsgan.py's kernel test on the CPU, against emulations and never against the kernels.

The two scalar heads of the least-squares losses are evaluated in numpy fp32 in their own summation order (tests/lsgan_cases.py:
stride-256 per-thread sums, the squares as fma chains, block_sum_256; the backward's fma and division), on the very inputs and at the
very shapes the GPU test uses, and compared with the fp64 reference: worst err / bound <= 0.5 with C_ACC = 8, so a correct fp32
implementation in another legitimate order has a factor two in hand.  Where an emulation is above 0.5 the constant of that output is
raised to the next power of two that brings it to 0.5 or below (lsgan_cases.RAISED, with the emulated ratio); this test pins that every
raise is needed, minimal and recorded correctly."""
import collections

import numpy as np
import pytest

import lsgan_cases as L


def emulate_all():
    """(output name, emulated fp32 value, (ref, absref, n_round)) for every case of the GPU module"""
    for family in L.FAMILIES:
        for n_real, n_fake in L.CASES:
            for t_real, t_fake in L.TARGETS:
                d = L.inputs(family, n_real, n_fake, t_real, t_fake)
                em, ref = L.lsloss_head_emulate(d["scores"], n_real, n_fake, t_real, t_fake), L.lsloss_head_ref(d["scores"], n_real, n_fake, t_real, t_fake)
                for k in ref:
                    yield f"lsloss_head/{k}", em[k], ref[k]
                for gl, gr, gf in L.null_patterns(d["g"]):
                    yield ("lsloss_head_bwd/gs", L.lsloss_head_bwd_emulate(d["scores"], n_real, n_fake, t_real, t_fake, gl, gr, gf)["gs"],
                           L.lsloss_head_bwd_ref(d["scores"], n_real, n_fake, t_real, t_fake, gl, gr, gf)["gs"])


@pytest.fixture(scope="module")
def emulated():
    """output name -> {constant: worst err / bound over the cases} for C_ACC = 8 and its doublings"""
    worst = collections.defaultdict(lambda: collections.defaultdict(float))
    for name, got, (ref, absref, n) in emulate_all():
        assert np.isfinite(np.asarray(got, np.float64)).all(), name
        for c in (8.0, 16.0, 32.0, 64.0):
            worst[name][c] = max(worst[name][c], L.ratio(got, ref, absref, n, c))
    return worst


def test_emulated_ratios_leave_a_factor_two(emulated):
    assert set(emulated) == {"lsloss_head/loss", "lsloss_head/mean_real", "lsloss_head/mean_fake", "lsloss_head_bwd/gs"}
    for name, v in sorted(emulated.items()):
        print(f"EMULATED {name}: {v[L.c_acc(name)]:.3f} (C_ACC {L.c_acc(name):g})")
    over = {k: round(v[L.c_acc(k)], 3) for k, v in emulated.items() if v[L.c_acc(k)] > 0.5}
    assert not over, over


def test_every_raised_constant_is_needed_minimal_and_recorded(emulated):
    for key, (c, recorded) in L.RAISED.items():
        assert key in emulated, key
        v = emulated[key]
        assert c in (16.0, 32.0, 64.0) and v[c / 2] > 0.5 >= v[c], (key, dict(v))
        assert abs(v[c] - recorded) < 0.02, (key, v[c], recorded)
    assert L.C_ACC == 8.0


def test_the_cases_reach_what_they_are_named_for():
    """the stride-256 loop, the four-wave reduction and the second block of the backward launch; the families' zero terms"""
    n = [a + b for a, b in L.CASES]
    assert L.CASES == [(1, 0), (1, 1), (4, 4), (3, 5), (16, 0), (255, 257), (256, 256), (300, 0), (1000, 24)]
    assert any(a > 256 for a, _ in L.CASES) and any(b > 256 for _, b in L.CASES)          # a second trip of either per-thread loop
    assert any(64 < a for a, _ in L.CASES) and any(v > 256 for v in n) and any(v <= 64 for v in n)
    assert [b for _, b in L.CASES].count(0) == 3                                            # the generator form
    for n_real, n_fake in L.CASES:
        for t_real, t_fake in L.TARGETS:
            s = L.inputs("on_target", n_real, n_fake, t_real, t_fake)["scores"]
            for lo, cnt, t in ((0, n_real, t_real), (n_real, n_fake, t_fake)):
                q = (cnt + 3) // 4
                assert (s[lo:lo + q] == np.float32(t)).all()
                near = s[lo + q:lo + min(2 * q, cnt)].astype(np.float64)
                assert (np.abs(near - t) <= 4 * 2.0 ** -23 * max(abs(t), 2.0 ** -126)).all()
            big = L.inputs("large", n_real, n_fake, t_real, t_fake)["scores"]
            assert big.dtype == np.float32 and (n_real + n_fake < 16 or np.abs(big).max() > 1e3)
    # the on-target quarter's loss terms and squared-part gradients are exact zeros in the reference
    d = L.inputs("on_target", 16, 0, 1.0, 0.0)
    g = L.lsloss_head_bwd_ref(d["scores"], 16, 0, 1.0, 0.0, 0.7, None, None)["gs"][0]
    assert not g[:4].any() and g[8:].all()
