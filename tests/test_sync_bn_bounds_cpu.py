"""Settles the constants of tests/test_gpu_sync_bn_kernels.py on the CPU, against emulations and never against the kernels.

1. The four launches of the synchronised BatchNorm are evaluated in numpy in kernel order (tests/sync_bn_cases.py: the lanes of a
   chunk and their in-order sum, sum_parts_f64's 16 x 16 order, the Chan merge in rank order, the finishes) on the very inputs the GPU
   module uses, and compared with the fp64 references: worst err / bound <= 0.5 with C_ACC = 8, or the (output, case) is listed in
   sync_bn_cases.RAISED with the next power of two that brings it there.
2. stage1 = "fp32" restates ngan_bn_moments as it was (chan_reduce_stage1<0>: fp32 sums per chunk about the part's first pixel, only
   the chunks added in fp64).  It must miss the bound of rstd on the outlier-pivot cases: the defect the per-element pin was written
   to find.  Every figure is printed.
3. Planted defects: deliberately wrong emulations, each of which must exceed ratio 1 on the case and output the test names.
4. The replica of red_chunk against the built library, and the conditions on the input family, on the references alone."""
import collections
import os

import numpy as np
import pytest

import sync_bn_cases as S
import wgan_cases as W

CONSTANTS = (8.0, 16.0, 32.0, 64.0)


def all_outputs(case, impl, merge_rank=0):
    yield from S.forward_chain(case, impl, merge_rank=merge_rank)
    for act in (0, 1):
        yield from S.backward_chain(case, impl, act)


@pytest.fixture(scope="module")
def emulated():
    """(output name, case id) -> {constant: worst err / bound} for C_ACC = 8 and its doublings"""
    worst = collections.defaultdict(lambda: collections.defaultdict(float))
    for case in S.CASES:
        cid = S.case_id(case)
        for name, got, (ref, absref, n) in all_outputs(case, S.Emulated()):
            for c in CONSTANTS:
                worst[(name, cid)][c] = max(worst[(name, cid)][c], W.ratio(got, ref, absref, n, c))
    return worst


def test_emulated_ratios_leave_a_factor_two(emulated):
    for (name, cid), v in sorted(emulated.items()):
        print(f"EMULATED {name} {cid}: {v[S.c_acc(name, cid)]:.3f} (C_ACC {S.c_acc(name, cid):g})")
    per_op = collections.defaultdict(float)
    for (name, cid), v in emulated.items():
        per_op[name] = max(per_op[name], v[S.c_acc(name, cid)])
    print("EMULATED worst per output:", {k: round(v, 3) for k, v in sorted(per_op.items())})
    over = {k: round(v[S.c_acc(*k)], 3) for k, v in emulated.items() if v[S.c_acc(*k)] > 0.5}
    assert not over, over


def test_every_raised_constant_is_needed_minimal_and_recorded(emulated):
    for key, (c, recorded) in S.RAISED.items():
        assert key in emulated, key
        v = emulated[key]
        assert c in CONSTANTS[1:] and v[c / 2] > 0.5 >= v[c], (key, dict(v))
        assert abs(v[c] - recorded) < 0.02, (key, v[c], recorded)
        # no output of the records or of the merge is raised: the outlier pivots meet the bound of the ordinary cases
        assert not key[0].startswith(("moments/", "merge/")), key


def worst_of(outputs, name):
    return max(W.ratio(got, ref, absref, n) for nm, got, (ref, absref, n) in outputs if nm == name)


def forward_only(case, impl, merge_rank=0):
    return list(S.forward_chain(case, impl, merge_rank=merge_rank))


def test_fp32_stage1_misses_the_bound_on_the_outlier_pivots():
    """ngan_bn_moments as it was: rstd (and what is formed from it) far outside the bound wherever a part's first pixel lies six sigma
    out, inside it on the correct emulation.  The lost roundings are printed per case, in units of 2^-23 relative."""
    named = ("C3-p614+1434", "C3-p10931+40+1", "C8-p1229+2867")
    for case in S.CASES[:-1]:
        cid = S.case_id(case)
        outs = forward_only(case, S.Emulated(stage1="fp32"))
        r = {k: worst_of(outs, f"merge/{k}") for k in ("mean", "rstd", "scale", "shift")}
        got, (ref, _, _) = next((g, rf) for nm, g, rf in outs if nm == "merge/rstd")
        units = float(np.max(np.abs(got.astype(np.float64) - ref) / np.abs(ref))) * 2.0 ** 23
        print(f"FP32STAGE1 {cid}: rstd {r['rstd']:.2f} scale {r['scale']:.2f} shift {r['shift']:.2f} mean {r['mean']:.2f} x the bound; "
              f"rstd off by {units:.1f} x 2^-23")
        if cid in named:
            assert r["rstd"] > 1.0 and r["scale"] > 1.0, (cid, r)
            assert worst_of(forward_only(case, S.Emulated()), "merge/rstd") <= 0.5


# defect -> [(the case that catches it, the output it shows in)]
DEFECTS = {
    "no_d2": [("C3-p614+1434", "merge/rstd"), ("C129-p1+385+1200", "merge/rstd")],
    "equal_means": [("C16-p4915+11469", "merge/mean"), ("C300-p113+1+1000", "merge/shift")],
    "local_xhat": [("C3-p614+1434", "bwd_partial/S1"), ("C17-p16391+10+1+964", "bwd_merged/dgamma")],
    "local_count": [("C8-p1229+2867", "bwd_merged/gy"), ("C256-p1281+1+63+500", "bwd_merged/gy_whole")],
    "dgamma_total": [("C16-p4096+4096", "bwd_merged/dgamma"), ("C3-p10931+40+1", "bwd_merged/dbeta_sum")],
    "local_unbiased": [("C8-p1229+2867", "merge/running_var"), ("C1-p5+278533+1+300", "merge/running_var")],
    "drop_ragged": [("C16-p4915+11469", "moments/M2"), ("C16-p4915+11469", "bwd_partial/S0"), ("C1-p5+278533+1+300", "merge/mean")],
    "drop_lanes16": [("C17-p16391+10+1+964", "moments/mean"), ("C256-p1281+1+63+500", "bwd_partial/S1"), ("C64-p4920+11480", "merge/rstd")],
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_defects_are_caught(defect):
    for cid, name in DEFECTS[defect]:
        case = S.case_of(cid)
        assert S.options(case)["track"] or "running" not in name, cid
        r = worst_of(all_outputs(case, S.Emulated(defect)), name)
        print(f"DEFECT {defect} {cid} {name}: {r:.3g}")
        assert r > 1.0, (defect, cid, name, r)
        assert worst_of(all_outputs(case, S.Emulated()), name) <= 0.5


def test_equal_weight_means_pass_on_the_equal_split():
    """why the ragged partitions are there: on two equal parts the wrong weights are the right ones"""
    case = S.case_of("C16-p4096+4096")
    outs = forward_only(case, S.Emulated("equal_means"))
    assert max(W.ratio(got, ref, absref, n) for _, got, (ref, absref, n) in outs) <= 0.5


def test_case_list_covers_what_the_issue_names():
    cs = {c for c, _ in S.CASES}
    assert cs >= {1, 3, 16, 17, 129, 256, 300, 1024}
    assert {len(p) for _, p in S.CASES} == {1, 2, 3, 4}
    assert any(len(set(p)) > 1 for _, p in S.CASES)
    nchunks = {S.red_chunk(n, C)[1] for C, p in S.CASES for n in p}
    ragged = {S.red_chunk(n, C)[1] for C, p in S.CASES for n in p if n % S.red_chunk(n, C)[0]}
    assert 1 in nchunks and any(1 < k < 16 for k in ragged) and any(16 < k < 1024 for k in ragged)
    for C in (1, 3, 17, 129, 256, 300):         # a single-pixel share at every thread layout
        assert any(1 in p and len(p) > 1 for c, p in S.CASES if c == C), C
    assert any(1 < n < S.lanes_of(C) for C, p in S.CASES for n in p)
    # the workgroup cap, and nothing larger than wgan_cases' big case
    assert (1024, (W.BIG_CASE[1],)) in S.CASES and S.red_chunk(W.BIG_CASE[1], 1024) == (17, 965)
    assert all(C * sum(p) <= W.BIG_CASE[0] * W.BIG_CASE[1] for C, p in S.CASES)
    assert len({(S.options(c)["momentum"], S.options(c)["eps"]) for c in S.CASES}) == 4 and {S.options(c)["track"] for c in S.CASES} == {True, False}


def test_red_chunk_replica_matches_the_library():
    import __graft_entry__ as graft
    pkg = graft.load_package()
    if not os.path.exists(pkg._C.LIB_PATH):
        graft.build()
    lib = pkg._C.lib()
    pairs = {(n, C) for C, p in S.CASES for n in p + (sum(p),)}
    pairs |= {(n, C) for C in (1, 3, 16, 17, 129, 256, 300, 1024, 20000) for n in (1, 16383, 16384, 16385, 1024 * 16, 1024 * 16 + 1, 2 ** 24 + 1)}
    for n, C in sorted(pairs):
        chunk, nparts = S.red_chunk(n, C)
        assert nparts <= 1024 and chunk * nparts >= n > chunk * (nparts - 1), (n, C)
        assert (chunk, nparts) == W.red_plan(n, C)
        assert lib.ngan_chan_reduce_workspace_floats(n, C) == 6 * nparts * C, (n, C)


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_input_family(case):
    """on the references alone: every part's first pixel is 6 +- 0.5 sigma from the channel mean in the designated channels; the
    constant channel's M2 is exactly 0, in every part and after an fp64 merge"""
    C, parts = case
    d = S.inputs(case)
    y64 = d["y"].astype(np.float64)
    assert d["six"] or sum(parts) == 1
    if d["six"]:
        mean, sigma = y64.mean(0), y64.std(0)
        for first in S.edges(parts)[:-1]:
            k = np.abs(y64[first, d["six"]] - mean[d["six"]]) / sigma[d["six"]]
            assert np.all(np.abs(k - 6.0) <= 0.5), (first, k)
    assert d["const"] == ([1] if C > 1 else [])
    recs = []
    for sl in S.slices(parts):
        ref = S.part_moments_ref(d["y"][sl])
        assert np.all(ref["M2"][0][d["const"]] == 0.0)
        if sl.stop - sl.start == 1:
            assert np.all(ref["M2"][0] == 0.0) and np.array_equal(ref["mean"][0], y64[sl.start])
        recs.append(np.concatenate([ref["count"][0], ref["mean"][0], ref["M2"][0]]))
    o = S.options(case)
    merged = S.merge_emulate(np.stack(recs), d["gamma"], d["beta"], o["eps"], o["momentum"], None, None)
    assert np.all(merged["rstd"][d["const"]] == np.float32(1.0 / np.sqrt(np.float64(np.float32(o["eps"])))))
    assert float(merged["n_total"][0]) == sum(parts)
