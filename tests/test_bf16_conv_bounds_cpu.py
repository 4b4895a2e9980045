"""Settles the constants of tests/test_gpu_bf16_conv.py on the CPU, against the emulation of tests/bf16_conv_cases.py and never against a
kernel, and checks the host side of the bf16-storage convolution's routing through the built library (no GPU).

  * the replica of pick_tile against ngan_conv3x3_kernel_name(..., precision 5) on a grid of (B, H, W, K, N) around every threshold
    (512 / 384 / 256 tiles, W <= 16, the tuned and the wide widths), the packed length against ngan_conv3x3_pack_elements, and the
    case list against all 80 names;
  * the covering: every instance with resample 0, epilogues 0 and 1; every other legal form in every (split kind, narrow, tile height,
    weight path);
  * the staged operand: for every resampled case the fp64 blend rounded once and the kernel's fp32 association rounded once are the
    same bf16 value at every element;
  * on the fp64 reference alone: at most 1e-2 of a case's bf16 elements lie within e of a bf16 midpoint (exact-rounding pin left
    undecided), at most 1e-4 of its pre-activations inside |c| <= e_c;
  * every distinct (K, N, resample, epilogue, store) of the case list, emulated on a 2 x 6 x 44 image (ragged against every tiling,
    even) in both orientations: worst err / bound <= 0.5 for every fp32 view (the convolution result c, the output before its store,
    rnorm, the ToImage result), so a correct kernel in another legitimate order has a factor two in hand; the stored bf16 output within
    its bound -- which one correct rounding reaches: 2^-8 |v| just above a power of two -- with no exact-rounding miss and no sign
    contradiction.  A width that exceeds 0.5 at C_ACC = 8 is listed in bf16_conv_cases.RAISED and pinned here;
  * each planted defect misses a bound or the pin."""
import collections
import os

import numpy as np
import pytest
import torch

import bf16_conv_cases as C

EMU_SHAPE = (2, 6, 44)
FP32_VIEWS = ("c", "y32", "rn", "img")


@pytest.fixture(scope="module")
def built(ngan):
    if not os.path.exists(ngan._C.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ngan


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _emu_list():
    return list(dict.fromkeys(C.Case(*EMU_SHAPE, *c[3:]) for c in C.CASES))


EMU = _emu_list()


def _judge(c, mode, got):
    """(check() of the stored outputs, {fp32 view: worst err / bound})"""
    d = C.inputs(c, mode)
    st = C.check(c, mode, d, {k: _t(got[k]) for k in ("y", "rn", "img") if k in got})
    ref = C.reference(c, mode, d, stored_y=_t(got["y"]) if ("y" in got and c.epi in (1, 3)) else None)
    views = {"c": C.F.ratio(_t(got["c"]), *ref["_c"])}
    views.update({k: C.F.ratio(_t(got[k]), *ref[k]) for k in FP32_VIEWS[1:] if k in got})
    return st, views


# ---- routing, through the built library ---------------------------------------------------------------------------------------------------
def test_replica_follows_the_name_function_on_a_sweep(built):
    L = built._C
    shapes = [(1, 1, 1), (2, 2, 2), (2, 5, 12), (2, 5, 16), (2, 5, 17), (2, 3, 40), (95, 6, 40), (96, 6, 40), (127, 12, 40), (128, 12, 40), (384, 4, 32),
              (383, 4, 32), (512, 8, 32), (511, 8, 32), (31, 7, 40), (32, 7, 40), (127, 5, 12), (128, 5, 12), (256, 2, 32), (255, 2, 32), (256, 4, 16),
              (255, 4, 16), (1, 64, 512), (16, 512, 512), (2, 60, 500), (43, 6, 40), (42, 6, 40)]
    names, n = set(), 0
    for B, H, W in shapes:
        for K in (16, 32, 48, 64, 96, 128, 144, 256, 512, 1024):
            for N in C.CHANNELS:
                name = L.conv3x3_kernel_name(B, H, W, K, N, 0, 0, 0, C.PREC)
                assert name == C.name_of(K, N, *C.pick_tile(B, H, W, N)), (B, H, W, K, N, name)
                names.add(name)
                n += 1
    assert n > 1000 and names == C.EXPECTED_NAMES
    lib = L.lib()
    for K in (16, 32, 48, 64, 128, 144, 256, 1024, 24, 1040):
        for N in C.CHANNELS + (48,):
            if K % 16 == 0 and N % 16 == 0:
                assert lib.ngan_conv3x3_pack_elements(N, K, 0, C.PREC) == C.pack_elements(K, N) == lib.ngan_conv3x3_pack_elements(K, N, 1, C.PREC), (K, N)
    assert C.pack_elements(24, 16) == C.pack_elements(1040, 16) == C.pack_elements(16, 48) == 0


def test_case_list_reaches_every_instance(built):
    names = {built._C.conv3x3_kernel_name(c.B, c.H, c.W, c.K, c.N, c.res, c.epi, c.om, C.PREC) for c in C.CASES}
    assert names == C.EXPECTED_NAMES == {C.kernel_name(c) for c in C.CASES}, sorted(C.EXPECTED_NAMES - names)
    assert len(names) == 80


# ---- the case list -------------------------------------------------------------------------------------------------------------------------
def test_facts_of_the_instances():
    """WREG, ring depth, slices and tile height as conv3x3_bf16_body derives them"""
    f = C.facts
    assert [f(K, 16, 4, False).path for K in (16, 32, 64, 128, 48)] == ["wreg", "wreg", "wreg", "ring", "wide"]        # S * NTW = 5, 9, 18, 36
    assert [f(K, 32, 4, False).path for K in (16, 32, 64, 128)] == ["wreg", "wreg", "ring", "ring"]                    # 10, 18, 36, 72
    assert [f(K, 64, 2, False).path for K in (16, 32, 64, 128)] == ["wreg", "wreg", "wreg", "ring"]                    # NTW = 1
    assert [f(K, 128, 2, False).path for K in (16, 32, 64, 128)] == ["wreg", "wreg", "ring", "ring"]                   # NTW = 2
    assert (f(16, 16, 4, True).RD, f(128, 16, 4, True).RD, f(144, 16, 4, True).RD) == (5, 8, 9)
    assert [f(K, 16, 4, True).NSL for K in (48, 128, 144, 256, 1024)] == [1, 1, 2, 2, 8]
    assert [(f(16, 16, p, n).TH, f(16, 16, p, n).TW) for p, n in C.SMALL_TILES] == [(8, 32), (4, 32), (2, 32), (4, 16)]
    assert [(f(16, 64, p, n).TH, f(16, 64, p, n).TW) for p, n in C.BIG_TILES] == [(2, 32), (1, 32), (4, 16), (2, 16)]


def test_case_list_covers_every_instance_and_form():
    plain = {(C.kernel_name(c), c.epi, m) for c in C.CASES if c.res == 0 and c.om == 0 and c.epi in (0, 1) and not c.var for m in (0, 1)}
    assert plain == {(n, e, m) for n in C.EXPECTED_NAMES for e in (0, 1) for m in (0, 1)}
    have, need = C.covering(C.CASES), C.required_covering()
    print("covering: %d (form, split, narrow, tile height, weight path) required, %d present" % (len(need), len(have)))
    for row in sorted(need):
        print("  ", row, sum(1 for c in C.CASES if C.covering([c]) == {row}), "case(s)")
    assert need <= have, sorted(need - have)
    assert len(need) == 12 * 9 + 12 * 7
    # every tile form: a ragged right column and bottom row, an image of exactly one tile; bilinear outputs with every tap clamped; a first,
    # an interior and a last tile in both directions per split kind; one product per element per split kind; the wide widths
    by_tile = collections.defaultdict(list)
    for c in C.CASES:
        f = C.facts_of(c)
        by_tile[(f.NS, f.TH, f.TW)].append(c)
    assert len(by_tile) == 8
    for (ns, th, tw), cs in by_tile.items():
        assert any(c.W % tw and (c.H % th or th == 1) for c in cs), (ns, th, tw)
        assert any(c.W == tw and c.H == th for c in cs), (ns, th, tw)
    assert all(c.H % 2 == 0 and c.W % 2 == 0 for c in C.CASES if c.res == 2)
    for ns in (False, True):
        cs = [c for c in C.CASES if C.facts_of(c).NS == ns]
        assert any(c.res == 2 and c.H == 2 and c.W == 2 for c in cs) and any(c.res == 2 and c.H == 2 and c.W > 32 for c in cs), ns
        assert any(C._cdiv(c.W, C.facts_of(c).TW) >= 3 and C._cdiv(c.H, C.facts_of(c).TH) >= 3 for c in cs), ns
        assert any(c.var == "onehot" for c in cs), ns
        assert any(c.H == 1 and c.W == 1 for c in cs), ns
    assert {c.K for c in C.CASES} == {16, 32, 64, 128, 48, 144, 256, 1024}
    assert {C.facts_of(c).path for c in C.REPEAT} == {"wreg", "ring", "wide"} and {C.facts_of(c).NS for c in C.REPEAT} == {False, True}
    for c in C.CASES:                                                    # size: what keeps a case at a fraction of a second
        assert c.B * c.H * c.W * c.K * c.N * 9 <= 2.5e9, c


def test_staged_operand_is_the_same_by_either_association():
    seen = set()
    for c in C.CASES:
        if c.res and c[:6] not in seen:
            seen.add(c[:6])
            d = C.inputs(c, 0)
            a, b = C.staged64(c, d), _t(C.staged32(c, d)).double()
            assert a.shape == b.shape == (c.B, c.H, c.W, c.K) and torch.equal(a, b), c
            x = d["x"]
            assert float(x.abs().min()) >= 2.0 ** -6 and float(x.abs().max()) < 8.0 and torch.equal(x, x.to(torch.bfloat16).float())
    assert len(seen) >= 40 and {k[5] for k in seen} == {1, 2}


def test_reference_alone_leaves_few_elements_undecided():
    """both caps on the fp64 reference, no kernel and no emulation: the share of the bf16 output within e of a midpoint (<= 1e-2) and of the
    pre-activations inside |c| <= e_c (<= 1e-4); every case of up to 2e9 multiply-adds here, every case in tests/test_gpu_bf16_conv.py"""
    n, worst = 0, (0.0, None)
    for c in C.CASES:
        if c.B * c.H * c.W * c.K * c.N * 9 > 2e9:
            continue
        for mode in (0, 1):
            ref = C.reference(c, mode, C.inputs(c, mode))
            r, e = ref["y32"]
            share = float((C.midpoint_distance(r) <= e).double().mean())
            worst = max(worst, (share, (c, mode)))
            assert share <= C.UNDECIDED_CAP, (c, mode, share)
            if c.epi in (1, 3):
                assert C.F.undecided_fraction(*ref["_c"]) <= 1e-4, (c, mode)
            n += 1
    print("largest undecided share of the exact-rounding pin: %.2e at %s" % worst)
    assert n >= 700


def test_midpoint_distance():
    r = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7, 1.0 - 2.0 ** -9, 1.0 + 2.0 ** -30, 3.0, -(1.5 + 2.0 ** -8), 0.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -9, 0.0, 2.0 ** -8, 0.0, 2.0 ** -9 + 2.0 ** -30, 2.0 ** -7, 0.0, 2.0 ** -9], dtype=torch.float64)
    assert torch.equal(C.midpoint_distance(r), want)


# ---- the emulation against the bounds -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worst():
    """(K, fp32 view) -> (worst emulated err / bound at the width's constant, where); ("y", K) the stored output's"""
    out = collections.defaultdict(lambda: (0.0, None))
    for c in EMU:
        for mode in (0, 1):
            st, views = _judge(c, mode, C.emulate(c, mode))
            assert not C.failures(st), (c, mode, st)
            views["y"] = st.get("y", 0.0)
            for k, r in views.items():
                if r > out[(c.K, k)][0]:
                    out[(c.K, k)] = (r, (c, mode))
    return dict(out)


def test_every_emulated_case_stays_within_half_the_bound(worst):
    print("emulated worst err / bound:", {k: round(v[0], 3) for k, v in sorted(worst.items())})
    assert {k[0] for k in worst} == {c.K for c in C.CASES}
    for (K, view), (r, where) in worst.items():
        assert r <= (1.0 if view == "y" else 0.5), (K, view, r, where)
    # the raises: pinned, and needed -- the same case exceeds 0.5 at C_ACC = 8 and at every power of two below the one listed
    assert set(C.RAISED) == {144, 256, 1024}
    for K, (raised, pinned) in C.RAISED.items():
        r, (c, mode) = worst[(K, "c")]
        assert abs(r - pinned) < 5e-3, (K, r, pinned)
        c64, _, absref = C.conv_reference(c, mode, C.inputs(c, mode))
        got = _t(C.emulate(c, mode)["c"])
        ca = 8.0
        while ca < raised:
            at = C.F.ratio(got, c64, 2.0 ** -23 * c64.abs() + ca * 2.0 ** -24 * absref)
            print("K = %d at C_ACC %d: %.3f" % (K, ca, at))
            assert at > 0.5, (K, ca, at)
            ca *= 2


# ---- planted defects ------------------------------------------------------------------------------------------------------------------------
S = EMU_SHAPE
DEFECTS = [
    ("trunc_store", C.Case(*S, 16, 16, 0, 0, 0)), ("trunc_store", C.Case(*S, 64, 64, 0, 1, 0)), ("trunc_store", C.Case(2, 5, 12, 32, 32, 0, 0, 0, "onehot")),
    ("trunc_weight", C.Case(*S, 32, 16, 0, 0, 0)), ("trunc_weight", C.Case(2, 3, 40, 32, 64, 0, 0, 0, "onehot")),
    ("halo", C.Case(*S, 16, 16, 0, 1, 0)), ("halo", C.Case(*S, 64, 64, 0, 0, 0)),
    ("chunk_swap", C.Case(*S, 32, 32, 0, 0, 0)), ("chunk_swap", C.Case(*S, 128, 64, 0, 1, 0)), ("chunk_swap", C.Case(*S, 144, 16, 0, 0, 0)),
    ("tap10", C.Case(*S, 16, 16, 0, 0, 0)), ("tap10", C.Case(*S, 16, 128, 0, 1, 0)),
    ("ring_stale", C.Case(*S, 128, 16, 0, 0, 0)), ("ring_stale", C.Case(*S, 64, 128, 0, 1, 0)), ("ring_stale", C.Case(*S, 144, 16, 0, 0, 0)),
    ("slice_pad", C.Case(*S, 48, 16, 0, 0, 0)), ("slice_pad", C.Case(*S, 144, 64, 0, 1, 0)),
    ("norm_wave", C.Case(*S, 16, 64, 0, 1, 0)), ("norm_wave", C.Case(*S, 64, 128, 0, 1, 0)),
    ("rn_group", C.Case(*S, 16, 16, 0, 1, 0)), ("rn_group", C.Case(*S, 16, 64, 0, 1, 0)), ("rn_group", C.Case(2, 6, 16, 16, 32, 0, 3, 0)),
    ("clamp", C.Case(*S, 16, 16, 2, 0, 0)), ("clamp", C.Case(*S, 64, 128, 2, 1, 0)),
    ("double_round", C.Case(*S, 16, 16, 2, 0, 0)), ("double_round", C.Case(*S, 144, 64, 2, 1, 0)),
    ("pool_twice", C.Case(*S, 16, 16, 0, 0, 1)), ("pool_twice", C.Case(*S, 64, 128, 0, 2, 1)),
    ("flip", C.Case(*S, 16, 16, 0, 0, 0)), ("flip", C.Case(*S, 144, 64, 0, 1, 0)),
]
ALL_DEFECTS = ("trunc_store", "trunc_weight", "halo", "chunk_swap", "tap10", "ring_stale", "slice_pad", "norm_wave", "rn_group", "clamp", "double_round",
               "pool_twice", "flip")


def test_every_planted_defect_is_listed():
    assert {d for d, _ in DEFECTS} == set(ALL_DEFECTS)


@pytest.mark.parametrize("defect,case", DEFECTS, ids=lambda v: v if isinstance(v, str) else C.case_id(v))
def test_planted_defect_misses_a_bound_or_the_pin(defect, case):
    for mode in ((1,) if defect == "flip" else (0, 1)):
        d = C.inputs(case, mode)
        good = C.check(case, mode, d, {k: _t(v) for k, v in C.emulate(case, mode).items() if k in ("y", "rn", "img")})
        bad = C.check(case, mode, d, {k: _t(v) for k, v in C.emulate(case, mode, defect=defect).items() if k in ("y", "rn", "img")})
        print(f"{defect} {C.case_id(case)} mode {mode}: {C.failures(good)} -> {C.failures(bad)}")
        assert not C.failures(good) and C.failures(bad), (defect, mode, good, bad)
