"""Settles the constants of tests/test_gpu_conv_fwd.py on the CPU, against emulations and never against the kernels, and checks the host
side of the forward / input-gradient routing through the built library (no GPU).

Every distinct (arithmetic form, contraction order, K, N, resample, epilogue, store) of tests/conv_fwd_cases.py is evaluated in numpy on
a small image (2 x 10 x 36: ragged against every tiling, even for the bilinear input) in the order the case's kernel family uses, in
both weight orientations, the fp32 MFMA both summed exactly and one fma after the other, and compared with the fp64 reference through
the epilogue: worst err / bound <= 0.5 with C_ACC = 8, so a correct implementation in another legitimate order has a factor two in hand.
The split-bf16 forms (precision codes 1, 2, 3) are settled in two parts as in tests/wgrad_cases.py: A, the emulation against the exact
sum of the three products it forms, through the epilogue, without the split term, at <= 0.5; B, that sum against the fp64 reference
within (2^-15 + C_ACC / 2 2^-24) absref at <= 1.  A raise is listed in conv_fwd_cases.RAISED and pinned here: one, the direct fp32 form
with the MFMA's products added one fma after the other (C_ACC 32).

Each planted defect must exceed the bound.  test_defects_that_todays_criteria_let_pass shows what the per-element bound sees and the
criteria of tests/test_gpu_ops.py do not (2e-4 of the max-norm; relative L2 1e-6 and max 2e-5 for the Winograd form), with the numbers."""
import collections
import os

import numpy as np
import pytest
import torch

import conv_fwd_cases as C
import fp64_conv

EMU_SHAPE = (2, 10, 36)


@pytest.fixture(scope="module")
def built(ngan):
    if not os.path.exists(ngan._C.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ngan


def _emu_list():
    """[(small case, orders, tile)], one per distinct numerics among the cases"""
    out = {}
    for c in C.CASES:
        small = C.Case(*EMU_SHAPE, *c[3:9])
        out.setdefault((small, C.family_orders(c)), C.tile_of(c))
    return [(k[0], k[1], v) for k, v in out.items()]


EMU = _emu_list()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _interior(c, t):
    """precision 3: the elements the folded form computes (the border ring is exact fp32)"""
    return t[:, 1:-1, 1:-1] if c.prec == 3 else t


def _ratios(c, mode, got, pre=None):
    """{output: worst err / bound} of an emulated result against the reference built on its own stored LeakyReLU pattern; "sign": inf
    if a stored sign contradicts an fp64 pre-activation outside |c| <= e_c"""
    d = C.inputs(c, mode)
    ref = C.reference(c, mode, d, stored_y=_t(got["y"]) if c.epi in (1, 3) else None, pre=pre)
    out = {k: C.ratio(_t(got[k]), *ref[k]) for k in got if k in ref}
    out["c"] = C.ratio(_t(got["c"]), *ref["_c"])
    if c.epi in (1, 3):
        out["sign"] = float("inf") if C.sign_violations(*ref["_c"], _t(got["y"])) else 0.0
    return out


def _part_a(c, mode, d):
    """(c64, e_c) of part A: the exact sum of the three products, the bound without the split term"""
    c64, e_c, absref = C.conv_reference(c, mode, d)
    sr = _t(C.split_reference(c, mode, d))
    direct = absref                                   # the split forms' absref is the direct sum's twin
    part_b = float((_interior(c, (sr - c64).abs()) / _interior(c, (C.SPLIT_TERM + C.C_ACC / 2 * 2.0 ** -24) * direct + 1e-30)).max())
    if c.prec == 3:                                   # the border ring has no split: the reference itself
        ring = ~C.interior_mask(c)[None, :, :, None]
        sr = torch.where(ring, c64, sr)
    return (sr, 2.0 ** -23 * sr.abs() + C.c_acc(C.FORM[c.prec]) * 2.0 ** -24 * absref), part_b


@pytest.fixture(scope="module")
def worst():
    """(form, output) -> (worst emulated err / bound at the form's constant -- C_ACC = 8, or what conv_fwd_cases.RAISED holds: 32 for the
    direct fp32 form -- and where); "split_b" -> part B of the split term"""
    out = collections.defaultdict(lambda: (0.0, None))
    for c, orders, tile in EMU:
        form = C.FORM[c.prec]
        for mode in C.modes(c):
            d = C.inputs(c, mode)
            split = c.prec in (1, 2, 3)
            pre = None
            if split:
                pre, b = _part_a(c, mode, d)
                if b > out["split_b"][0]:
                    out["split_b"] = (b, (c, mode))
            for mfma in (("exact", "seq") if c.prec in (0, 4) else ("exact",)):
                got = C.emulate(c, mode, mfma, orders=orders)
                whole = _ratios(c, mode, got)
                assert all(r <= 1.0 for r in whole.values()), (c, mode, mfma, whole)
                for k, r in (_ratios(c, mode, got, pre) if split else whole).items():
                    if r > out[(form, k)][0]:
                        out[(form, k)] = (r, (c, mode, mfma, orders))
    return dict(out)


def test_every_emulated_case_stays_within_half_the_bound(worst):
    print("emulated worst err / bound:", {k: (round(v[0], 3), v[1]) for k, v in worst.items()})
    assert {k[0] for k in worst if k != "split_b"} == set(C.FORM.values())
    for key, (r, where) in worst.items():
        assert r <= (1.0 if key == "split_b" else 0.5), (key, r, where)
    # the raise: pinned, and needed -- the same case exceeds 0.5 at C_ACC = 8 and at 16
    assert set(C.RAISED) == {("f32_direct", "c")}
    raised, pinned = C.RAISED[("f32_direct", "c")]
    r, (c, mode, mfma, orders) = worst[("f32_direct", "c")]
    assert raised == 32.0 and abs(r - pinned) < 5e-3, (r, pinned)
    c64, _, absref = C.conv_reference(c, mode, C.inputs(c, mode))
    got = _t(C.emulate(c, mode, mfma, orders=orders)["c"])
    at = {ca: C.ratio(got, c64, 2.0 ** -23 * c64.abs() + ca * 2.0 ** -24 * absref) for ca in (8.0, 16.0)}
    print("direct fp32, the worst case at C_ACC 8 and 16:", at)
    assert at[8.0] > at[16.0] > 0.5, at


def test_emulated_cases_cover_every_numerics_of_the_case_list():
    combos = {(C.FORM[c.prec], C.family_orders(c), c.epi, c.om, c.res) for c in C.CASES}
    assert combos == {(C.FORM[c.prec], o, c.epi, c.om, c.res) for c, o, _ in EMU}
    assert {o[0] for _, o, _ in EMU} == {"g_tap", "tap_g", "pair", "tap", "kg_tap", "wino"}


def test_inputs_keep_the_preactivations_off_the_kink():
    """the fp64 reference alone: at most 1e-4 of the pre-activations of an epilogue-1 / 3 case lie inside |c| <= e_c (every case of up to
    2e9 multiply-adds here; tests/test_gpu_conv_fwd.py asserts the same of every case on its fp64 reference)"""
    n = 0
    for c in C.CASES:
        if c.epi in (1, 3) and c.B * c.H * c.W * c.K * c.N * 9 <= 2e9:
            for mode in C.modes(c):
                c64, e_c, _ = C.conv_reference(c, mode, C.inputs(c, mode))
                assert C.undecided_fraction(c64, e_c) <= 1e-4, (c, mode)
                n += 1
    assert n >= 60


# ---- the case list --------------------------------------------------------------------------------------------------------------------
def test_case_list_holds_the_required_edges():
    cases = [c for c in C.CASES]
    assert all(C.available(c) for c in cases)
    fam = collections.defaultdict(list)
    for c in cases:
        fam[(C.route(c)[0], C.tile_of(c))].append(c)
    # every tiling: ragged right, ragged bottom, an image of one tile, an image smaller than a tile, B >= 2
    for tiling in {k for k in fam if k[0] in ("generic", "mid")} | {("persist", (8, 32)), ("tile", (8, 32)), ("wino", (8, 32)), ("up2f", (8, 32))}:
        th, tw = tiling[1]
        cs = fam[tiling]
        assert any(c.W % tw and c.W > tw for c in cs) or tiling[0] in ("tile", "wino"), tiling        # (tile / wino: W % 32 == 0 by routing)
        assert th == 1 or any(c.H % th and c.H > th for c in cs), tiling
        assert any(c.B >= 2 for c in cs), tiling
        if tiling[0] != "up2f":                                                                       # (precision 3 needs H >= 16)
            assert any(c.H <= th and c.W <= tw for c in cs), tiling
    for tiling in (k for k in fam if k[0] in ("generic", "mid") and k[1] != (8, 32)):
        cs = fam[tiling]
        assert any(c.H == 1 for c in cs) and any(c.W == 1 for c in cs), tiling
    small = [c for c in cases if C.route(c)[0] in ("generic", "mid")]
    assert any(c.H == 1 and c.W == 1 for c in small)
    assert any(c.res == 2 and c.H == 2 for c in small) and any(c.res == 2 and c.W == 2 for c in small)       # every tap clamped
    assert all(c.H % 2 == 0 and c.W % 2 == 0 for c in cases if c.res == 2)
    assert any(c.H < 8 and c.W < 32 for c in fam[("persist", (8, 32))])
    # several tiles per workgroup, one per persistent family: more tiles than workgroups -- every launcher sizes its grid as
    # persistent_grid(n_tiles, 256 * per_cu) with per_cu capped at 4, so a grid never exceeds 1024 whatever the occupancy query answers
    # (the 16-row Winograd instance gets 1050 tiles of its own from 70 images of 8 rows) -- a step of the walk (grid / 8 = 128, 64 or 32)
    # that is no multiple of tiles_x = 15 (carries in x, y and the batch), and a height that is no multiple of the tile's rows
    for f in ("persist", "tile", "wino", "up2f"):
        ws = [c for c in C.WALK if C.route(c)[0] == f]
        assert ws and all(C.n_tiles(c) > 1024 and c.H % C.tile_of(c)[0] and C._cdiv(c.W, 32) == 15 for c in ws), f
    assert {c.prec for c in C.WALK} == {0, 1, 3, 4}
    # the mid kernel: each K group with each slice, whole and split over workgroups
    for prec, ks in ((0, (32, 64, 128)), (1, (32, 64, 128)), (2, (16,))):
        for K in ks:
            for ns in (32, 64, 128):
                cs = [c for c in C.MID if c.prec == prec and c.K == K and C.mid_slice(C.mid_tiles(c.B, c.H, c.W), c.N) == ns]
                assert any(c.N == ns for c in cs), (prec, K, ns)
                assert ns == 128 or any(c.N > ns and c.epi in (1, 2) for c in cs), (prec, K, ns)
    # folded bilinear: K = 16 and 32, epilogues 0 and 1, the one-call form and interior + border
    assert {(c.K, c.epi, c.var) for c in C.UP2F} == {(K, e, v) for K in (16, 32) for e in (0, 1) for v in ("", "split")}
    # every epilogue and the pool-adjoint store in every family that offers them; the pooled side output; K outside the fast paths
    for f in ("persist", "tile", "wino"):
        assert {(c.epi, c.om) for c in cases if C.route(c)[0] == f} >= {(0, 0), (1, 0), (2, 0), (2, 1), (3, 0), (0, 1)}, f
    assert {(c.epi, c.om) for c in C.MID} == {(0, 0), (1, 0), (2, 0), (2, 1), (0, 1)}
    assert {(c.epi, c.om) for c in C.GENERIC} == {(0, 0), (1, 0), (2, 0), (2, 1), (0, 1)}
    assert sum(C.pooled_output(c) and c.epi == 1 for c in cases) >= 6
    assert {c.K for c in C.GENERIC} >= {48, 80}
    assert any(c.var == "noy" for c in cases)
    # size: no case above about 2.5e5 pixels x 32 channels or 7e4 pixels x 128 channels
    for c in cases:
        assert c.B * c.H * c.W * max(c.K, c.N) <= 2.7e5 * 32, c


def test_replica_names_cover_every_instance():
    names = {C.kernel_name(c) for c in C.CASES}
    assert names == C.EXPECTED_NAMES, (sorted(C.EXPECTED_NAMES - names), sorted(names - C.EXPECTED_NAMES))
    assert len(C.EXPECTED_NAMES) == 323 and C.UNREACHABLE == []
    seconds = {C.second_launch(c) for c in C.CASES}
    assert seconds == {None, "ngan_lrelu_pixelnorm_fwd", "ngan_lrelu_pixelnorm_bwd"} | {"conv3x3_up2_border_kernel<%d, %d>" % (e, K) for e in (0, 1) for K in (16, 32)}


# ---- planted defects ------------------------------------------------------------------------------------------------------------------
S2 = (2, 10, 70)            # two tile columns of 32 and a ragged third
PERSIST_F32, PERSIST_BF, MID_BF, WINO, UP2F = ("tap_g", False, "rsq"), ("pair", False, "rsq"), ("kg_tap", False, "sqrt"), ("wino", True, "rsq"), ("pair", False, "rsq")
DEFECTS = [
    # (defect, case, orders, tile)
    ("halo", C.Case(*S2, 16, 16, 0, 0, 0, 0), PERSIST_F32, (8, 32)), ("halo", C.Case(*S2, 16, 16, 0, 1, 0, 1), PERSIST_BF, (8, 32)),
    ("halo", C.Case(*S2, 16, 16, 0, 0, 0, 4), WINO, (8, 32)),
    ("strip", C.Case(*S2, 16, 16, 0, 0, 0, 0), PERSIST_F32, (8, 32)), ("strip", C.Case(*S2, 16, 16, 0, 1, 0, 4), WINO, (8, 32)),
    ("misstore", C.Case(*S2, 16, 16, 0, 0, 0, 0), PERSIST_F32, (8, 32)), ("misstore", C.Case(*S2, 16, 16, 0, 1, 0, 1), PERSIST_BF, (8, 32)),
    ("no_lohi", C.Case(*S2, 16, 16, 0, 0, 0, 1), PERSIST_BF, (8, 32)), ("no_lohi", C.Case(2, 5, 20, 64, 64, 0, 1, 0, 1), MID_BF, (4, 16)),
    ("no_lohi", C.Case(*S2, 16, 16, 2, 0, 0, 3), UP2F, (8, 32)),
    ("no_lohi_step", C.Case(2, 5, 20, 128, 64, 0, 0, 0, 1), MID_BF, (4, 16)),
    ("bias_slice", C.Case(2, 5, 20, 64, 64, 0, 0, 0, 1), MID_BF, (4, 16)), ("bias_slice", C.Case(2, 5, 20, 64, 128, 0, 1, 0, 0), ("g_tap", False, "sqrt"), (4, 16)),
    ("norm_slice", C.Case(2, 5, 20, 64, 64, 0, 1, 0, 1), MID_BF, (4, 16)), ("norm_slice", C.Case(2, 5, 20, 32, 128, 0, 1, 0, 0), ("g_tap", False, "sqrt"), (4, 16)),
    ("clamp", C.Case(2, 10, 36, 16, 16, 2, 0, 0, 0), PERSIST_F32, (8, 32)), ("clamp", C.Case(2, 10, 36, 16, 16, 2, 1, 0, 4), WINO, (8, 32)),
    ("clamp", C.Case(2, 10, 36, 32, 32, 2, 0, 0, 1), ("tap", False, "rsq"), (4, 32)),
    ("border_folded", C.Case(2, 10, 36, 16, 16, 2, 0, 0, 3), UP2F, (8, 32)), ("border_folded", C.Case(2, 10, 36, 32, 16, 2, 1, 0, 3), ("tap", False, "rsq"), (8, 32)),
    ("pool_twice", C.Case(*S2, 16, 16, 0, 0, 1, 0), PERSIST_F32, (8, 32)), ("pool_twice", C.Case(*S2, 16, 16, 0, 2, 1, 4), WINO, (8, 32)),
    ("pool_twice", C.Case(2, 5, 20, 64, 64, 0, 2, 1, 1), MID_BF, (4, 16)),
] + [("trunc", c, None, None) for c in C.ONE_PRODUCT]        # one product per element: the very cases tests/test_gpu_conv_fwd.py launches


def _worst(r):
    return max((v if v == v else float("inf")) for v in r.values())


@pytest.mark.parametrize("defect,case,orders,tile", DEFECTS, ids=lambda v: v if isinstance(v, str) else (C.case_id(v) if isinstance(v, C.Case) else ""))
def test_planted_defect_misses_the_bound(defect, case, orders, tile):
    for mode in C.modes(case):
        good = _worst(_ratios(case, mode, C.emulate(case, mode, orders=orders, tile=tile)))
        bad = _worst(_ratios(case, mode, C.emulate(case, mode, defect=defect, orders=orders, tile=tile)))
        print(f"{defect} {C.case_id(case)} mode {mode}: {good:.3f} -> {bad:.3g}")
        assert good <= (1.0 if case.prec in (1, 2, 3) else 0.5) and bad > 1.0, (defect, mode, good, bad)       # (the split term is attainable)


def _todays(c, got, ref):
    """the criteria of tests/test_gpu_ops.py on y: max |got - ref| / max |ref| < 2e-4 (Winograd: relative L2 < 1e-6 and max < 2e-5)"""
    g, r = _t(got).double(), ref
    mx, l2 = float((g - r).abs().max() / r.abs().max()), float((g - r).norm() / r.norm())
    return (l2 < 1e-6 and mx < 2e-5) if c.prec == 4 else mx < 2e-4, mx, l2


def test_defects_that_todays_criteria_let_pass():
    """What the per-element bound sees and today's criteria do not, on the emulations, mode 0 (err / bound of y; max |err| / max |ref|):
      trunc, one product per element   1.75 - 2.69 of the bound on the ten ONE_PRODUCT cases, which the GPU test launches (their correct
                                       emulation: 0.64 - 0.91); 1.6e-5 - 5.0e-5 of the max-norm: passes 2e-4 fourfold at least.  On the
                                       regular inputs a truncating split stays below 0.4 of the bound: only these cases see it
      no_lohi_step, K = 128            2.28 of the bound; 2.3e-4: at the edge of today's criterion
      no_lohi                          11 - 24 of the bound; 1.0e-3 - 1.2e-3: today's criterion sees it too, by 5x where the bound has 11x
    So of the two candidates only the truncating split stays inside today's criteria while it misses the bound, and a lost lo.hi product
    does once it is confined to one k-step of a long contraction.  The mis-stored tile component is an error of the size of the data
    (0.2 - 0.45 of the max-norm) and is caught by both wherever a shape has the faulty tile -- the historical bug escaped by being
    rare, not small: the cases with more tiles than resident workgroups are the defence there -- as are the dropped halo column, the
    unwritten strip, the slice-wise bias and norm, the clamp, the folded border and the pool-adjoint factor applied twice."""
    seen = {}
    for defect, case, orders, tile in DEFECTS:
        d = C.inputs(case, 0)
        got = C.emulate(case, 0, defect=defect, orders=orders, tile=tile)
        ref = C.reference(case, 0, d, stored_y=_t(got["y"]) if case.epi in (1, 3) else None)
        ok_today, mx, l2 = _todays(case, got["y"], ref["y"][0])
        new = C.ratio(_t(got["y"]), *ref["y"])
        print(f"{defect} {C.case_id(case)}: err / bound {new:.3g}, max-norm {mx:.3g}, rel L2 {l2:.3g}, passes today's criteria: {ok_today}")
        seen.setdefault(defect, []).append((ok_today, new))
    assert all(ok and new > 1.0 for ok, new in seen["trunc"]), seen["trunc"]
    for defect in set(seen) - {"trunc"}:
        assert all(not ok and new > 1.0 for ok, new in seen[defect]), (defect, seen[defect])


# ---- the added fp64 references against torch's own operators --------------------------------------------------------------------------------
def test_added_references_match_torch():
    gen = torch.Generator().manual_seed(5)
    c = torch.randn(2, 3, 5, 8, generator=gen, dtype=torch.float64)
    up = torch.nn.functional.interpolate(c.permute(0, 3, 1, 2), scale_factor=2, mode="nearest").permute(0, 2, 3, 1) * 0.25
    assert torch.equal(fp64_conv.pool_adjoint(c), up)
    g = torch.randn(2, 6, 10, 8, generator=gen, dtype=torch.float64)
    assert abs(float((fp64_conv.pool2(g) * c).sum() - (g * fp64_conv.pool_adjoint(c)).sum())) < 1e-12          # the adjoint of the 2x2 average
    w = torch.randn(8, generator=gen, dtype=torch.float64)
    t, ta = fp64_conv.to_image(c, w)
    assert torch.allclose(t, torch.tanh(torch.nn.functional.conv2d(c.permute(0, 3, 1, 2), w.view(1, 8, 1, 1))[:, 0]), rtol=0, atol=1e-14)
    assert bool((ta >= torch.atanh(t.abs().clamp(max=1 - 1e-12)) - 1e-9).all())
    # the Winograd twin bounds the form's own result and is no smaller than |c| - rounding
    x, wt = torch.randn(1, 5, 7, 16, generator=gen, dtype=torch.float64), torch.randn(16, 16, 3, 3, generator=gen, dtype=torch.float64)
    assert bool((C.winograd_absref(x.abs(), wt.abs()) >= fp64_conv.conv3x3(x, wt).abs() - 1e-9).all())


# ---- host-only checks through the built library ------------------------------------------------------------------------------------------
def _agree(L, c):
    a = (c.B, c.H, c.W, c.K, c.N, c.res)
    for req in (0, 1):
        assert L.conv3x3_algorithm(*a, req) == C.algorithm(*a, req), (c, req)
    if not C.available(c):
        return None
    assert bool(L.conv3x3_epilogue_fused(*a, c.epi, c.om, c.prec)) == C.epilogue_fused(c), c
    assert bool(L.conv3x3_pooled_output(*a, c.prec)) == C.pooled_output(c), c
    if c.epi == 3 and not C.epilogue_fused(c):
        return None
    name = L.conv3x3_kernel_name(*a, c.epi, c.om, c.prec)
    assert name == C.kernel_name(c), (c, name, C.kernel_name(c))
    return name


def test_case_list_reaches_every_instance(built):
    names = {_agree(built._C, c) for c in C.CASES}
    assert names == C.EXPECTED_NAMES, (sorted(C.EXPECTED_NAMES - names), sorted(names - C.EXPECTED_NAMES))


def test_kernel_name_follows_the_routing_on_a_sweep(built):
    """ngan_conv3x3_kernel_name, _algorithm, _epilogue_fused and _pooled_output against the replica of ngan_conv3x3_fwd_ex's routing on
    shapes around every threshold (256 tiles, 1.3 waste, W % 32, H >= 16, the channel groups), every epilogue, store and precision code.
    Found here: the generic kernel with epilogue 2 was named conv3x3_kernel<.., 2, 0>, an instance that does not exist (the launcher
    runs <.., 0, 0> and a PixelNorm pass), e.g. (2, 60, 500, 48, 16, 0, 2, 0, 0); fixed in ngan_conv3x3_kernel_name."""
    shapes = [(1, 1, 1), (2, 2, 2), (2, 6, 20), (4, 30, 140), (2, 30, 140), (2, 60, 500), (2, 60, 512), (1, 64, 512), (2, 64, 510), (16, 14, 500),
              (256, 8, 32), (256, 7, 30), (255, 8, 32), (256, 8, 24), (256, 8, 26), (64, 4, 16), (64, 5, 20), (4, 64, 256), (5, 110, 470)]
    n, names = 0, set()
    for B, H, W in shapes:
        for K in (16, 32, 48, 64, 128):
            for N in (16, 32, 64, 128):
                for res in ((0, 1, 2) if H % 2 == 0 and W % 2 == 0 else (0, 1)):
                    for epi, om in ((0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (2, 1)):
                        if om and res:
                            continue
                        if epi == 2 and res:
                            continue
                        for prec in (0, 1, 2, 3, 4):
                            if prec == 3 and (epi > 1 or om):
                                continue
                            name = _agree(built._C, C.Case(B, H, W, K, N, res, epi, om, prec))
                            n += name is not None
                            names.add(name)
    assert n > 5000 and names - {None} <= C.EXPECTED_NAMES
