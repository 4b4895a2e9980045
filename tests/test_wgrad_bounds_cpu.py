"""Settles the constants of tests/test_gpu_wgrad.py on the CPU, against emulations and never against the kernels, and checks the host
side of the weight-gradient plan through the built library (no GPU).

Every case of tests/wgrad_cases.py is evaluated in numpy in the kernels' own order (tile walk, Winograd transforms with the sign trick,
MFMA groups both summed exactly and one fma after the other, per-wave back-transform, fixed-order wave sum; the k-step order of the
bf16 forms; the slab reductions) at the three precisions, written and accumulated, and compared with the fp64 reference: worst
err / bound <= 0.5 with C_ACC = 8, so a correct implementation in another legitimate order has a factor two in hand.  A raise would
be listed in wgrad_cases.RAISED (next power of two, emulated ratio) and pinned here; none was needed.  The 128-channel cases emulate
a prefix of 32 output channels (their elements are computed independently of one another); the 640-tile case runs whole.  The "seq"
form of the fp32 MFMA and the deferred reduction run on every case with at most 64 channels on either side and 64 tiles -- every
instance family is among them -- the "exact" form and the direct reduction on all.  Each planted defect must exceed the bound."""
import collections
import os

import numpy as np
import pytest

import wgrad_cases as C


@pytest.fixture(scope="module")
def built(ngan):
    if not os.path.exists(ngan._C.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ngan


def _co_limit(case):
    return C.CO_LIMIT.get(case[4])


def _small(case):
    B, H, W, Cin, Cout, res = case
    return max(Cin, Cout) <= 64 and C.plan(B, H, W, Cin, Cout, 1)["n_tiles"] <= 64


@pytest.fixture(scope="module")
def worst():
    """form -> worst emulated err / bound at C_ACC = 8 over all cases, and the entry that gave it"""
    out = collections.defaultdict(lambda: (0.0, None))
    for case in C.CASES:
        lim = _co_limit(case)
        for prec in C.PRECISIONS:
            modes = ("exact", "seq") if prec == 0 and _small(case) else ("exact",)
            for mode in modes:
                for path in (("direct", "deferred") if _small(case) else ("direct",)):
                    for acc in (0, 1):
                        got = C.emulate(case, prec, mode, acc, path, co_limit=lim)
                        r = C.check(case, prec, got, acc, lim, part_a=prec == 1)
                        assert C.check(case, prec, got, acc, lim) <= 1.0, (case, prec, mode, path, acc)
                        if r > out[C.FORM[prec]][0]:
                            out[C.FORM[prec]] = (r, (case, mode, path, acc))
    return dict(out)


def test_every_emulated_case_stays_within_half_the_bound(worst):
    print("emulated worst err / bound:", {k: (round(v[0], 3), v[1]) for k, v in worst.items()})
    assert set(worst) == set(C.FORM.values())
    for form, (r, where) in worst.items():
        assert r <= 0.5, (form, r, where)
    assert C.RAISED == {}, "a raise needs an emulated ratio above 0.5 at C_ACC = 8: none exists"


def test_split_term_covers_what_the_three_products_lack():
    """part B of the split-bf16 bound: the fp64 sum of lo.hi + hi.lo + hi.hi against the fp64 reference, per element, on every case"""
    worst = max((C.split_part_b(c), c) for c in C.CASES)
    print("split-bf16 term: worst |three products - ref| / ((2^-15 + 4 2^-24) absref):", worst)
    assert worst[0] <= 1.0, worst


def test_case_list_holds_the_required_edges():
    cases = set(C.CASES)
    assert {c[2] for c in C.NARROW} >= {1, 12, 16} and {c[1] for c in C.NARROW} >= {1, 18}
    assert {c[2] for c in C.WIDE + C.XF} >= {17, 40, 64, 96} and {c[1] for c in C.WIDE + C.XF} >= {1, 8, 12, 20}
    assert all(c[0] >= 2 for c in C.WIDE + C.XF)
    assert any(c[1:3] == (20, 96) and c[5] == 0 for c in C.XF)
    assert any(c[5] == 2 and c[1] == 2 for c in cases) and any(c[5] == 2 and c[2] == 2 for c in cases)
    assert all(c[1] % 2 == 0 and c[2] % 2 == 0 for c in cases if c[5] == 2)
    pairs = {(16, 16), (32, 32), (16, 32), (32, 16), (16, 64), (48, 32), (64, 64), (128, 128), (48, 80)}
    assert {c[3:5] for c in cases} >= pairs
    assert (2, 18, 16, 32, 32, 0) in cases and (2, 12, 17, 32, 32, 0) in cases
    assert {c[0] for c in C.TAILS} == {1, 15, 16, 17, 49, 64, 65, 113}
    for c in C.TAILS:
        assert all(C.plan(*c[:5], prec)["nwx"] == c[0] for prec in C.PRECISIONS)
    # tile walk: several tiles per workgroup with a step that is no multiple of tiles_x, carries in x, y and b
    steps = []
    for c in C.WALK[:2]:
        p = C.plan(*c[:5], 0)
        assert p["nwx"] == 16 and p["n_tiles"] > p["nwx"]
        steps.append((p["nwx"] % p["tiles_x"], (p["nwx"] // p["tiles_x"]) % p["tiles_y"], p["nwx"] // p["tiles_x"] // p["tiles_y"]))
    assert steps == [(0, 2, 2), (1, 2, 1)]        # (dx, dy, db) of TileWalk: dy and dx + the cursor carry into b and y
    assert C.plan(*C.WALK[2][:5], 0)["n_tiles"] == 640 and C.plan(*C.WALK[2][:5], 0)["nwx"] == 512
    big = max(cases, key=lambda c: c[0] * c[1] * c[2] * max(c[3], c[4]))
    assert big == (5, 128, 256, 16, 16, 0)
    # slicing: n_ci_slices > 1 together with Cout / co_s > 1
    assert any(C.plan(*c[:5], 1)["n_ci_slices"] > 1 and c[4] // C.plan(*c[:5], 1)["co_s"] > 1 for c in cases)


def test_replica_names_cover_every_instance():
    names = {C.kernel_name(c, prec) for c in C.CASES for prec in C.PRECISIONS}
    assert names == C.EXPECTED_NAMES, (sorted(C.EXPECTED_NAMES - names), sorted(names - C.EXPECTED_NAMES))
    # the cases that also run the "seq" MFMA form and the deferred reduction reach every instance by themselves
    assert {C.kernel_name(c, prec) for c in C.CASES if _small(c) for prec in C.PRECISIONS} == C.EXPECTED_NAMES


DEFECTS = [
    # (defect, case, precision): each on a case where the defect touches real data
    ("halo", (2, 8, 64, 64, 64, 0), 0), ("halo", (2, 8, 64, 64, 64, 0), 1), ("halo", (2, 8, 64, 64, 64, 0), 5),
    ("slab_twice", (17, 8, 32, 16, 16, 0), 0), ("slab_skipped", (17, 8, 32, 16, 16, 0), 0),
    ("slab_twice", (65, 8, 16, 16, 16, 0), 1), ("slab_skipped", (65, 8, 16, 16, 16, 0), 5),
    ("swap", (2, 8, 64, 64, 64, 0), 0), ("swap", (2, 12, 17, 32, 32, 0), 0), ("swap", (2, 8, 64, 64, 64, 0), 1),
    ("no_lohi", (2, 8, 17, 16, 64, 0), 1), ("no_lohi", (2, 12, 17, 16, 16, 1), 1),
    ("trunc", (1, 1, 1, 16, 16, 0), 1), ("trunc", (2, 2, 2, 16, 16, 2), 1),
]


@pytest.mark.parametrize("defect,case,prec", DEFECTS)
def test_planted_defect_misses_the_bound(defect, case, prec):
    for path in ("direct", "deferred"):
        good = C.check(case, prec, C.emulate(case, prec, "exact", 0, path), 0)
        bad = C.check(case, prec, C.emulate(case, prec, "exact", 0, path, defect=defect), 0)
        print(f"{defect} {case} precision {prec} {path}: {good:.3f} -> {bad:.3g}")
        assert good <= (1.0 if prec == 1 else 0.5) and bad > 1.0, (defect, path, good, bad)       # (precision 1: the split term is attainable)


def _reduce_cases():
    for nparts in C.REDUCE_NPARTS:
        for co_s, ci_s in C.REDUCE_SLICES:
            yield C.reduce_shape(co_s, ci_s), [(nparts, 0.37)]
    for i, src in enumerate(C.REDUCE_MULTI):
        yield C.reduce_shape(*C.REDUCE_SLICES[i % 4]), src
    for shape, src, _ in C.many_entries():
        yield shape, src


def test_reduce_many_emulation_stays_within_half_the_bound():
    worst = 0.0
    for shape, src in _reduce_cases():
        slabs = [C.synthetic_slabs(n, shape["M"], s) for s, (n, _) in enumerate(src)]
        scales = [sc for _, sc in src]
        ref = C.reduce_many_ref(slabs, scales)
        buf = C.synthetic_slabs(1, shape["M"], 99)[0]
        worst = max(worst, C.ratio(C.reduce_many_emulate(slabs, scales), *ref),
                    C.ratio(C.reduce_many_emulate(slabs, scales, buf), *C.plus(ref, buf)))
    print(f"reduce_many emulated worst err / bound: {worst:.3f}")
    assert worst <= 0.5
    # planted: one slab of one source skipped / added twice
    shape, src = C.reduce_shape(16, 16), [(33, 0.7), (129, 1.5)]
    slabs = [C.synthetic_slabs(n, shape["M"], s) for s, (n, _) in enumerate(src)]
    ref = C.reduce_many_ref(slabs, [0.7, 1.5])
    assert C.ratio(C.reduce_many_emulate([slabs[0], slabs[1][:-1]], [0.7, 1.5]), *ref) > 1
    assert C.ratio(C.reduce_many_emulate([np.concatenate([slabs[0], slabs[0][:1]]), slabs[1]], [0.7, 1.5]), *ref) > 1


def test_output_index_map_round_trips():
    """to_workspace / from_workspace are each other's inverse, and a swapped second slice is not"""
    gw = np.arange(64 * 32 * 9, dtype=np.float32).reshape(64, 32, 3, 3)
    slab = np.ascontiguousarray(gw.reshape(64, 32, 9).transpose(2, 0, 1))[None]
    for co_s, ci_s in C.REDUCE_SLICES:
        assert np.array_equal(C.from_workspace(C.to_workspace(slab, co_s, ci_s)[0], 64, 32, co_s, ci_s), gw)
    assert not np.array_equal(C.from_workspace(C.to_workspace(slab, 16, 16)[0], 64, 32, 16, 16, defect="swap"), gw)


# ---- host-only checks through the built library --------------------------------------------------------------------------------------
PAIRS = [(16, 16), (32, 32), (16, 32), (32, 16), (16, 64), (64, 16), (48, 32), (32, 48), (64, 64), (128, 128), (48, 80)]


def _check_plan(ngan, B, H, W, Cin, Cout):
    ws = ngan._C.wgrad_workspace_bytes(B, H, W, Cin, Cout)
    for prec in C.PRECISIONS:
        nwx, nslices, n_ci, co_s, ci_s = ngan._C.wgrad_plan(B, H, W, Cin, Cout, prec)
        assert nwx * nslices * 9 * co_s * ci_s * 4 <= ws, ("slabs past the workspace", (B, H, W, Cin, Cout), prec)
        assert n_ci * ci_s == Cin and (nslices // n_ci) * co_s == Cout and nslices % n_ci == 0, ((B, H, W, Cin, Cout), prec)
        p = C.plan(B, H, W, Cin, Cout, prec)
        assert (nwx, nslices, n_ci, co_s, ci_s) == (p["nwx"], p["nslices"], p["n_ci_slices"], p["co_s"], p["ci_s"]), ((B, H, W, Cin, Cout), prec)


def test_workspace_holds_the_plan_of_every_precision(built):
    for c in C.CASES:
        _check_plan(built, *c[:5])
    for Cin, Cout in PAIRS:
        for H in range(1, 71):
            for W in range(1, 71):
                _check_plan(built, 1 + (H + W) % 3, H, W, Cin, Cout)
    for B in (1, 16, 64, 600):                    # many tiles: the caps of 256 and 512 workgroups
        for Cin, Cout in PAIRS + [(512, 512), (16, 512)]:
            _check_plan(built, B, 64, 64, Cin, Cout)


def test_case_list_reaches_all_84_instances(built):
    names = collections.defaultdict(list)
    for c in C.CASES:
        for prec in C.PRECISIONS:
            name = built._C.conv3x3_wgrad_kernel_name(*c, prec)
            assert name == C.kernel_name(c, prec)
            names[name].append((c, prec))
    assert set(names) == C.EXPECTED_NAMES, (sorted(C.EXPECTED_NAMES - set(names)), sorted(set(names) - C.EXPECTED_NAMES))
