"""Settles the constants of tests/test_gpu_first_block.py on the CPU, against emulations and never against the kernels, and sweeps the
launch plan of csrc/first_block.hip through the built library (host arithmetic: no GPU is needed).

Every kernel of the folded critic first block is evaluated in numpy fp32 in its own summation order (tests/first_block_cases.py), on the
very inputs and at the very shapes the GPU test uses, and compared with the fp64 reference: worst err / bound <= 0.5 with C_ACC = 8, so a
correct fp32 implementation in another legitimate order has a factor two in hand.  Where an emulation is above 0.5 the constant of that
output is raised to the next power of two that brings it to 0.5 or below (first_block_cases.RAISED: the folded tables, C_ACC 16); the
raise is pinned as needed, minimal and recorded correctly.  Each planted
defect of first_block_cases.DEFECTS is applied to the emulation and must exceed the bound on a case the test names."""
import collections
import os

import numpy as np
import pytest
import torch

import first_block_cases as F

f32 = np.float32
OUT_FWD, OUT_BWD = ("tables", "y", "rnorm"), ("S", "gW", "gwf", "gbf", "gbc")


@pytest.fixture(scope="module")
def built(ngan):
    if not os.path.exists(ngan._C.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ngan


def case_of(H, Wd, N):
    """the EDGE case with these H, W, N"""
    (c,) = [c for c in F.EDGE if (c[1], c[2], c[4]) == (H, Wd, N)]
    return c


def nan_like(a):
    return np.full(a.shape, np.nan, f32)


def fwd_ratios(case, defect=None, bf_null=False, bc_null=False):
    """{output: emulated err / bound} of the forward, and (sign violations, undecided share)"""
    d = F.inputs(*case)
    bf, bc = (None if bf_null else d["bf"]), (None if bc_null else d["bc"])
    tab = F.tables_emulate(d["w"], d["wf"], bf, d["scale"])["tables"]
    em = F.fwd_emulate(d["p"], tab, bc, defect)
    ref = F.fwd_ref(d["p"], d["w"], d["wf"], bf, bc, d["scale"], em["y"])
    out = {"tables": F.worst(tab, F.tables_ref(d["w"], d["wf"], bf, d["scale"])["tables"], "tables")}
    out.update({k: F.worst(em[k], ref[k], k) for k in ("y", "rnorm")})
    return out, (F.sign_violations(*ref["_pre"], em["y"]), F.undecided_fraction(*ref["_pre"]))


def bwd_ratios(case, defect=None, bf_null=False, mask=0, gbf_null=False, gbc_null=False, S=None):
    d = F.inputs(*case)
    bf = None if bf_null else d["bf"]
    if S is None:
        S = F.sums_emulate(d["p"], d["gc"], defect)["S"]
    bufs = {"gW": d["bufW"], "gwf": d["bufwf"], "gbf": d["bufbf"], "gbc": d["bufbc"]}
    bits = {"gW": 1, "gwf": 2, "gbf": 4, "gbc": 8}
    null = {"gbf": gbf_null, "gbc": gbc_null}
    start = {k: None if null.get(k) else (bufs[k] if mask & bits[k] else nan_like(bufs[k])) for k in bufs}
    em = F.finish_emulate(S, d["w"], d["wf"], bf, d["scale"], start, mask, defect)
    ref = F.bwd_ref(d["p"], d["gc"], d["w"], d["wf"], bf, d["scale"])
    out = {"S": F.worst(S, ref["S"], "S")}
    for k in bufs:
        if em[k] is not None:
            out[k] = F.worst(em[k], F.plus(ref[k], bufs[k]) if mask & bits[k] else ref[k], k)
    return out, S


def dx_ratios(case, pool, defect=None):
    d = F.inputs(*case)
    tab = F.tables_emulate(d["w"], d["wf"], d["bf"], d["scale"])["tables"]
    em = F.dx_emulate(d["gc"], tab, pool, defect)
    return {"gx": F.worst(em["gx"], F.dx_ref(d["gc"], d["w"], d["wf"], d["scale"], pool)["gx"], "gx")}


@pytest.fixture(scope="module")
def worst():
    """output -> (worst emulated err / bound over all cases, the case), and the worst undecided share"""
    out = collections.defaultdict(lambda: (0.0, None))
    signs = [0, 0.0]

    def take(ratios, tag):
        for k, v in ratios.items():
            if not v <= out[k][0]:
                out[k] = (v, tag)

    for case in F.FULL:
        r, (viol, und) = fwd_ratios(case)
        take(r, case)
        signs[0] += viol
        signs[1] = max(signs[1], und)
        take(bwd_ratios(case)[0], case)
        for pool in (0, 1):
            take({"gx pooled" if pool else "gx": dx_ratios(case, pool)["gx"]}, case)
    for case in F.NULL_SHAPES:
        take(fwd_ratios(case, bf_null=True)[0], (case, "bf null"))
        take(fwd_ratios(case, bc_null=True)[0], (case, "bc null"))
        take(bwd_ratios(case, bf_null=True)[0], (case, "bf null"))
        _, S = bwd_ratios(case)
        for mask, gbf_null, gbc_null in F.ACCUMULATE:
            r = bwd_ratios(case, mask=mask, gbf_null=gbf_null, gbc_null=gbc_null, S=S)[0]
            take({f"{k} acc" if mask & {"gW": 1, "gwf": 2, "gbf": 4, "gbc": 8}.get(k, 0) else k: v for k, v in r.items()}, (case, mask))
    for case in F.PLAN_CASES:
        take(bwd_ratios(case)[0], case)
    return dict(out), signs


def test_every_emulation_is_within_half_the_bound(worst):
    ratios, _ = worst
    for name, (v, case) in sorted(ratios.items()):
        print(f"EMULATED first_block {name}: {v:.3f} at {case}")
    base = lambda k: k.replace(" acc", "").replace(" pooled", "")
    assert set(map(base, ratios)) == set(OUT_FWD + OUT_BWD + ("gx",))
    bad = {k: v for k, v in ratios.items() if base(k) not in F.RAISED and not v[0] <= 0.5}
    assert not bad, bad
    for name, (c, pinned) in F.RAISED.items():           # every raise needed, minimal and recorded correctly
        got = max(v[0] for k, v in ratios.items() if base(k) == name)
        assert c > F.C_ACC and np.log2(c) % 1 == 0 and abs(got - pinned) < 5e-4 and got <= 0.5, (name, got)


def test_raised_entries_are_needed_and_minimal():
    """the tables alone are raised, to the next power of two; with C_ACC = 8 their emulation is above 0.5 (0.526)"""
    assert F.C_ACC == 8.0 and set(F.RAISED) == {"tables"} and F.RAISED["tables"][0] == 2 * F.C_ACC
    case = (3, 7, 33, 16, 32)
    d = F.inputs(*case)
    ref, absref, n, carried = F.tables_ref(d["w"], d["wf"], d["bf"], d["scale"])["tables"]
    got = F.tables_emulate(d["w"], d["wf"], d["bf"], d["scale"])["tables"]
    at8 = F.ratio(got, ref, absref, n, F.C_ACC)
    assert 0.5 < at8 < 0.55 and abs(F.worst(got, (ref, absref, n, carried), "tables") - F.RAISED["tables"][1]) < 5e-4, at8


def test_leaky_relu_signs_on_the_reference(worst):
    """the emulation never stores a sign the fp64 reference decides otherwise, and the share of undecided elements (|pre| <= e_c, on the
    reference alone) stays under the cap of 1e-2 of a case"""
    _, (violations, undecided) = worst
    assert violations == 0
    assert undecided <= 1e-2, undecided


def test_inputs_are_hard():
    """non-zero border pixels, bf of the size of wf * p, no symmetric taps, PixelNorm's mean square far above eps"""
    for case in F.FULL[::7]:
        d = F.inputs(*case)
        p, w = d["p"], d["w"]
        assert (p[:, 0] != 0).all() and (p[:, -1] != 0).all() and (p[:, :, 0] != 0).all() and (p[:, :, -1] != 0).all()
        assert 0.2 < np.abs(d["bf"]).mean() / max(np.abs(d["wf"]).mean() * np.abs(p).mean(), 1e-30) < 20 or case[3] == 1
        assert not np.array_equal(w, w[:, :, ::-1]) and not np.array_equal(w, w[:, :, :, ::-1])
        pre, _ = F.pre_ref(p, w, d["wf"], d["bf"], d["bc"], d["scale"])
        assert ((0.2 * pre) ** 2).mean(-1).min() > 1e4 * F.EPS


# ---- planted defects: (defect, case, which part, output) -------------------------------------------------------------------------------
ACC16 = F.NULL_SHAPES[0]
PLANTED = [
    ("bv_left", case_of(7, 3, 16), "fwd", "y"),                  # x = 0 takes the bias of a tap in the padding
    ("bv_right", case_of(7, 3, 16), "fwd", "y"),                 # x = W - 1
    ("bv_left", case_of(1, 1, 16), "fwd", "y"),                  # both masks on one pixel
    ("row_mask_chunk", case_of(9, 3, 16), "fwd", "y"),           # row 8 starts the second chunk and is not the image's first
    ("row_mask_chunk", case_of(9, 3, 16), "bwd", "gbf"),
    ("no_reprime", case_of(9, 3, 16), "fwd", "y"),               # row 7 belongs to the previous workgroup
    ("no_reprime", case_of(17, 33, 32), "bwd", "gW"),
    ("no_reprime", case_of(9, 3, 16), "dx", "gx"),
    ("pad_lanes", case_of(7, 65, 16), "bwd", "gW"),              # the second x-block: one live lane, fifteen padding lanes in its DPP row
    ("pad_lanes", case_of(7, 33, 32), "bwd", "gbc"),
    ("tail_pw8", case_of(7, 33, 32), "bwd", "gW"),               # two pixel groups share a DPP row
    ("dx_noflip", case_of(7, 3, 16), "dx", "gx"),
    ("dx_pool_no_quarter", case_of(7, 3, 16), "dx pooled", "gx"),
    ("gbc_tap", case_of(7, 3, 16), "bwd", "gbc"),
    ("acc_bits_swapped", ACC16, "acc 2", "gwf"),                 # gwf's bit steers gbf
    ("acc_bits_swapped", ACC16, "acc 4", "gbf"),
    ("scale_twice", case_of(7, 3, 16), "bwd", "gwf"),
    ("skip_c16", (3, 9, 65, 20, 16), "bwd", "gwf"),              # channels 16 .. 19 are left unwritten
    ("skip_c16", (1, 9, 33, 64, 32), "bwd", "gbf"),
]


@pytest.mark.parametrize("defect,case,part,output", PLANTED)
def test_planted_defect_exceeds_the_bound(defect, case, part, output):
    assert defect in F.DEFECTS and (case in F.FULL or case in F.NULL_SHAPES)

    def run(df):
        if part == "fwd":
            return fwd_ratios(case, df)[0][output]
        if part.startswith("dx"):
            return dx_ratios(case, int(part.endswith("pooled")), df)[output]
        mask = int(part.split()[1]) if part.startswith("acc") else 0
        return bwd_ratios(case, df, mask=mask)[0][output]

    clean, planted = run(None), run(defect)
    print(f"PLANTED first_block {defect} {output} {case}: {clean:.3f} -> {planted:.3g}")
    assert clean <= 0.5
    assert not planted <= 1.0, (defect, case, output, planted)


def test_every_listed_defect_is_planted():
    assert {p[0] for p in PLANTED} == set(F.DEFECTS)


# ---- the launch plan through the built library -----------------------------------------------------------------------------------------
GRID_B = (1, 2, 3, 5, 33, 64, 65, 1024, 1025, 8191, 8192, 65535, 65536)
GRID_H = (1, 2, 7, 8, 9, 16, 17, 1024, 3300, 4096, 8192, 8200, 524280, 524281)
GRID_W = (1, 2, 3, 31, 32, 33, 63, 64, 65, 1024, 4096, 32767, 32768)
GRID_C = (1, 16, 20, 64, 65)
GRID_N = (8, 16, 32, 64)


def grid():
    yield from F.HANGING
    yield from F.FULL + F.PLAN_CASES
    yield from ((1, 4096, 32768, 1, 16), (1, 4096, 32767, 1, 16), (2, 4096, 8192, 1, 32), (0, 8, 8, 16, 16), (1, 0, 8, 16, 16),
                (1, 8, 0, 16, 16), (1, 8, 8, 0, 16), (-1, 8, 8, 16, 16))
    for B in GRID_B:
        for H in GRID_H:
            for Wd in GRID_W:
                for C in GRID_C:
                    for N in GRID_N:
                        yield B, H, Wd, C, N


def test_plan_replica_matches_the_library(built):
    """ngan_first_block_plan == first_block_cases.plan over the grid, refusals included: the shapes whose R could not stop doubling,
    the 65536-row and 2^31-element limits, C = 65, N = 8 and 64, more than 1024 slabs"""
    n_ok = n_refused = 0
    for shape in grid():
        status, out = built._C.first_block_plan(*shape)
        want = F.plan(*shape)
        if want is None:
            assert status == F.NGAN_ERR_SHAPE and out[3] == 0, (shape, status, out)
            n_refused += 1
        else:
            assert status == 0 and out == want, (shape, status, out, want)
            gx, R, nchunk, slabs = out
            assert slabs <= F.MAX_SLABS and R >= F.FB_ROWS and nchunk == -(-shape[1] // R) and shape[0] * nchunk < 65536
            assert R == F.FB_ROWS or -(-shape[1] // (R // 2)) * gx * shape[0] > F.MAX_SLABS, ("R raised without need", shape, out)
            n_ok += 1
    assert n_ok > 1000 and n_refused > 1000
    for shape in F.HANGING:
        assert built._C.first_block_plan(*shape)[0] == F.NGAN_ERR_SHAPE
    assert built._C.first_block_plan(*F.SMALLEST_REFUSED, 16, 16)[0] == F.NGAN_ERR_SHAPE
    assert built._C.first_block_plan(1024, 1, 1, 16, 16) == (0, (1, 8, 1, 1024))
    assert F.plan(1, 524280, 1, 1, 16) is not None and F.plan(1, 524281, 1, 1, 16) is None           # B ceil(H / 8) < 65536
    assert F.plan(1, 4096, 32767, 1, 16) is not None and F.plan(1, 4096, 32768, 1, 16) is None       # B H W N < 2^31
    for case, want in F.PLAN_EXPECT.items():
        assert F.plan(*case) == want and built._C.first_block_plan(*case) == (0, want), case


def test_plan_query_is_declared_and_bound(built):
    """include/ngan_first_block.h, an extension section of ngan.h, declares the query; _C binds it"""
    import ctypes
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "ngan.h")).read()
    declared = set(re.findall(r"\b(ngan_[a-z0-9_]+)\s*\(", open(os.path.join(root, "include", "ngan_first_block.h")).read()))
    assert '#include "ngan_first_block.h"' in main and declared == {"ngan_first_block_plan"}
    assert declared <= set(built._C.exported_symbols())
    assert hasattr(ctypes.CDLL(built._C.LIB_PATH), "ngan_first_block_plan")


def test_refusal_message_names_the_slabs(built):
    assert built._C.first_block_plan(1025, 1, 1, 16, 16)[0] == F.NGAN_ERR_SHAPE
    assert "needs 1025 slabs (max 1024)" in built._C.lib().ngan_last_error().decode()
    assert built._C.first_block_plan(1, 8, 8, 65, 16)[0] == F.NGAN_ERR_SHAPE
    assert "unsupported" in built._C.lib().ngan_last_error().decode()
    assert built._C.lib().ngan_first_block_plan(1, 8, 8, 16, 16, None) == -1


def test_fusable_is_false_exactly_where_the_plan_refuses(built):
    """ops.first_block_fusable asks the library: meta tensors of the right shape, nothing is launched"""
    ops = built.ops
    assert ops._first_block_allowed and ops._conv_precision != 5

    def fusable(B, H, Wd, C, N, pool=False):
        x = torch.empty((B, 2 * H, 2 * Wd, 1) if pool else (B, H, Wd, 1), device="meta")
        return ops.first_block_fusable(x, torch.empty(C, 1, 1, 1, device="meta"), torch.empty(N, C, 3, 3, device="meta"), pool)

    n = 0
    for shape in grid():
        if min(shape) <= 0:
            continue
        assert fusable(*shape) == (F.plan(*shape) is not None), shape
        n += 1
    assert n > 10000
    for shape in F.HANGING:
        assert not fusable(*shape) and not fusable(*shape, pool=True)
    assert fusable(1024, 1, 1, 16, 16, pool=True) and not fusable(1025, 1, 1, 16, 16, pool=True)
    # two colours, or a FromImage over two colours: never the fold
    assert not ops.first_block_fusable(torch.empty(2, 8, 8, 2, device="meta"), torch.empty(16, 2, 1, 1, device="meta"),
                                       torch.empty(16, 16, 3, 3, device="meta"))
