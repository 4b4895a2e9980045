"""Settles the constants of tests/test_gpu_penalty.py on the CPU, against emulations and never against the kernels.

Both entry points of include/ngan_penalty.h are evaluated in numpy fp32 in the kernels' own order (tests/penalty_cases.py: the norms as
the two-stage sum of squares forms them, stride-256 per-thread sums of one fma per term, block_sum_256, the row scalar in gp_coef's
order), on the very inputs and at the very shapes the GPU test uses, and compared with the fp64 reference: worst err / bound <= 0.5
with C_ACC = 8, so a correct fp32 implementation in another legitimate order has a factor two in hand.  Where an emulation is above 0.5
the constant of that output is raised to the next power of two that brings it to 0.5 or below (penalty_cases.RAISED, with the emulated
ratio); this test pins that every raise is needed, minimal and recorded correctly."""
import collections

import numpy as np
import pytest

import penalty_cases as P


def emulate_all():
    """(output name, emulated fp32 value, (ref, absref, n_round, carried)) for every case of the GPU module"""
    for B, n, fam in P.CASES:
        g = P.inputs(B, n, fam)
        for form in P.FORMS:
            em = P.head_emulate(g, P.LAMBDA, form)
            ref = P.head_ref(g, P.LAMBDA, form)
            for k in ref:
                yield f"penalty_head{form}/{k}", em[k], ref[k]
            bw = P.bwd_emulate(g, em["norms"], P.LAMBDA, form, P.G_OUT)
            yield f"penalty_bwd{form}/grad", bw["grad"], P.bwd_ref(g, P.LAMBDA, form, P.G_OUT)["grad"]


@pytest.fixture(scope="module")
def emulated():
    """output name -> {constant: worst err / bound over the cases} for C_ACC = 8 and its doublings"""
    worst = collections.defaultdict(lambda: collections.defaultdict(float))
    for name, got, (ref, absref, n, carried) in emulate_all():
        assert np.isfinite(np.asarray(got, np.float64)).all(), name
        for c in (8.0, 16.0, 32.0, 64.0):
            worst[name][c] = max(worst[name][c], P.ratio_carried(got, ref, absref, n, carried, c))
    return worst


def test_emulated_ratios_leave_a_factor_two(emulated):
    assert len(emulated) == 6
    for name, v in sorted(emulated.items()):
        print(f"EMULATED {name}: {v[P.c_acc(name)]:.3f} (C_ACC {P.c_acc(name):g})")
    over = {k: round(v[P.c_acc(k)], 3) for k, v in emulated.items() if v[P.c_acc(k)] > 0.5}
    assert not over, over


def test_every_raised_constant_is_needed_minimal_and_recorded(emulated):
    for key, (c, recorded) in P.RAISED.items():
        assert key in emulated, key
        v = emulated[key]
        assert c in (16.0, 32.0, 64.0) and v[c / 2] > 0.5 >= v[c], (key, dict(v))
        assert abs(v[c] - recorded) < 0.02, (key, v[c], recorded)


def test_form_one_above_one_is_the_two_sided_chain():
    """where every norm is above 1 the one-sided form is the reference's two-sided one: the emulations agree bit for bit"""
    for B, n, fam in P.CASES:
        if fam != "above_one":
            continue
        g = P.inputs(B, n, fam)
        head, chain = P.head_emulate(g, P.LAMBDA, P.ONE_SIDED), P.chain_emulate(g, P.LAMBDA, P.G_OUT)
        grad = P.bwd_emulate(g, head["norms"], P.LAMBDA, P.ONE_SIDED, P.G_OUT)["grad"]
        for got, want in ((head["norms"], chain["norms"]), (head["penalty"], chain["penalty"]), (grad, chain["grad"])):
            assert got.dtype == want.dtype == np.float32 and got.tobytes() == want.tobytes(), (B, n)


def test_the_cases_reach_what_they_are_named_for():
    assert (1, 5) in P.SHAPES and max(B for B, _ in P.SHAPES) > 256 and sum(B > 256 for B, _ in P.SHAPES) == 2
    assert any(n % 4 and B == 1 for B, n in P.SHAPES)                                   # an unaligned tail (one row only)
    chunks = lambda n: min(max((n // 4 + 255) // 256, 1), 64)                           # noqa: E731  (ngan_penalty_head's grid)
    assert max(chunks(n) for _, n in P.SHAPES) == 64 and chunks(65540) == 64 and (65540 // 4) % 256 != 0
    assert chunks(1024) == 1 and 1024 // 4 == 256 and chunks(3072) == 3
    for fam in ("standard", "near_one"):
        nrm = np.concatenate([P.norms64(P.inputs(B, n, fam)) for B, n in P.SHAPES])
        assert (nrm < 1).any() and (nrm > 1).any(), fam
    near = np.concatenate([P.norms64(P.inputs(B, n, "near_one"))[::4] for B, n in P.SHAPES])
    assert (near < 1).any() and (near > 1).any()                                        # the few-ulps rows lie on either side too
    for B, n in P.SHAPES:
        assert (P.norms64(P.inputs(B, n, "above_one")) >= 1.2499).all() and (P.norms64(P.inputs(B, n, "above_one")) <= 4.0).all()
        std = P.norms64(P.inputs(B, n, "standard"))
        assert (std >= 0.2499).all() and (std <= 4.0).all()
        assert np.allclose(P.norms64(P.inputs(B, n, "large")), 1e3 * std, rtol=1e-6)
        g = P.inputs(B, n, "near_one")
        nrm = P.norms64(g)
        near = [b for b in range(B) if b % 4 == 0]
        assert near and (np.abs(nrm[near] - 1) < 8 * 2.0 ** -23).all()
        ones = P.exact_one_rows(B, "near_one")
        assert bool(ones) == (B >= 2)
        for form in P.FORMS:
            grad = P.bwd_ref(g, P.LAMBDA, form, P.G_OUT)["grad"][0]
            if ones:
                assert (nrm[ones] == 1.0).all() and (np.count_nonzero(g[ones], axis=1) == 1).all()
                assert (P.phi(nrm[ones], P.ONE_SIDED) == 0.0).all()
                if form == P.ONE_SIDED:
                    assert (grad[ones] == 0.0).all()                                    # the exact-one rows: exact zero in the reference
        z = P.zero_rows(B, "zero_row")
        gz = P.inputs(B, n, "zero_row")
        assert z == [B // 2] and not gz[z].any() and (P.norms64(gz)[z] == 0).all()
        assert gz.any() == (B > 1)
