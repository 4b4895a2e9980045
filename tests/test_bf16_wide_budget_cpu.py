"""Where the model-level tolerances of tests/test_gpu_bf16_wide.py come from: the CPU emulation of the bf16 mode (tests/lowprec_budget.py,
"bf16mode" row) on the oracle, for the same width sets, weights and draws.  Each bound must be at least 1.5 x the largest emulated
deviation over the sets.  No GPU needed."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lowprec_budget as LB  # noqa: E402
import test_gpu_bf16_wide as W  # noqa: E402


def test_wide_tolerances_cover_the_emulated_bf16_mode_deviation(ngan):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    worst = {"scalars / max scalar": 0.0, "|grad D|": 0.0, "D grads (rel L2)": 0.0, "G grads (rel L2)": 0.0}
    for n_colors, res, alpha, widths in W.WIDE_SETS:
        _, _, pg, pd, spec, x, z1, z2, eps, z3 = W.wide_case(ngan, n_colors, res, alpha, widths)
        row = LB.budget(str(widths), pg, pd, spec, x, z1, z2, eps, z3)["bf16mode"]
        for k in worst:
            worst[k] = max(worst[k], row[k])
    assert 1.5 * worst["scalars / max scalar"] <= W.TOL_SCALAR, worst
    assert 1.5 * worst["|grad D|"] <= W.TOL_NORM, worst
    assert 1.5 * max(worst["D grads (rel L2)"], worst["G grads (rel L2)"]) <= W.TOL_GRAD, worst
    # the bounds are not looser than the convention makes them: each is 1.5 x the emulation or an existing bound of test_gpu_bf16.py
    assert W.TOL_GRAD <= max(1.5 * max(worst["D grads (rel L2)"], worst["G grads (rel L2)"]) * 1.05, 3e-1), worst
    assert W.TOL_SCALAR <= max(1.5 * worst["scalars / max scalar"] * 1.05, 5e-2), worst
    assert W.TOL_NORM <= max(1.5 * worst["|grad D|"] * 1.05, 6e-2), worst
