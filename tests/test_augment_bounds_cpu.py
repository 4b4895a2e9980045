"""Settles the constants of tests/test_gpu_augment.py on the CPU, against an emulation and never against the kernels.

1. the fp32 emulation of both passes of csrc/augment.hip (tests/augment_cases.py, class Emulator) passes the bit comparison of pass 1
   on every case and stays at or below 0.5 of every bound at the recorded C_ACC; every recorded constant is minimal (half of it leaves
   some case above 0.5).  The EMULATED lines are the table DESIGN.md quotes.
2. the share of ambiguous pixels stays at or below 5 % for every sample of the table -- from the fp64 definition alone.
3. the definition is tied to torch: the dense resize matrices equal F.interpolate(bilinear, antialias) in fp64 to 1e-12, and on
   unambiguous pixels pass 1 equals the grid_sample(nearest, zeros, align_corners=False) restatement of tests/test_gpu_data.py.
4. fifteen wrong emulations each break their assertion on a named case (augment_cases.WRONG) on which, by 1, the correct one passes.
5. the host side of data.NeuronDataset: `pack_params` writes the record the kernel reinterprets, `draw_params` draws what torchvision's
   transforms draw."""
import collections
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_cases as A


@pytest.fixture(scope="module")
def tile(ngan):
    lib = ngan._C.lib()
    T = A.tile_pixels(lib)
    for R in A.GEOMETRY:                                            # the layout include/ngan.h states, at the sizes the tests use
        c = A.case(R)
        assert A.nblk_of(lib, c.B, c.P) == -(-c.P * c.P // T) == A.nblk_of(lib, 1, c.P)
    assert A.nblk_of(lib, 2, 384) > 64 and A.nblk_of(lib, 1, 49) == 2 and A.nblk_of(lib, 1, 6) == 1
    assert lib.ngan_augment_workspace_bytes(0, 8) == 0 and lib.ngan_augment_workspace_bytes(3, 0) == 0
    return T


@pytest.fixture(scope="module")
def emulated(tile):
    """R -> (canvas, partial) of the correct emulation"""
    return {R: A.Emulator().pass1(A.case(R).src, A.case(R).idx, A.case(R).rec, tile) for R in A.GEOMETRY}


def test_the_table_holds_what_it_names():
    for R in A.GEOMETRY:
        c = A.case(R)
        assert c.P == R + 2 * (R // 4) and c.src.shape == (A.N_IMAGES, c.P, c.P)
        assert all(S <= R and R % S == 0 for S in A.GEOMETRY[R])
        if R == 256:
            assert c.names == ["rot45_t", "odd_f1_c1"] and c.B == 2
            continue
        assert c.B > A.N_IMAGES and set(c.idx.tolist()) == set(range(A.N_IMAGES))                # B > N, every image, repeats
        assert not any(int(c.idx[b]) == b % A.N_IMAGES for b in range(c.B))
        fl = A.flags(c.rec)
        odd = [c.row(n) for n in ("odd_f0_c0", "odd_f1_c0", "odd_f0_c1", "odd_f1_c1")]
        assert sorted(map(tuple, fl[odd].tolist())) == [(0, 0), (0, 1), (1, 0), (1, 1)]
        assert ("rot45_t" in c.names) == ("rot30_ties" in c.names) == (c.P >= 40)
        d = round(0.1 * c.P)
        assert sorted(c.rec[[c.row(n) for n in ("t+x", "t-x")], 2].tolist()) == [-d, d]
        assert sorted(c.rec[[c.row(n) for n in ("t+y", "t-y")], 3].tolist()) == [-d, d]
        assert c.rec[c.row("all_outside"), 2] == c.P and c.rec[c.row("contrast_one"), 5] == 1.0
    c = A.case(33)
    assert c.rec[c.row("rot30_ties"), 1] == np.float32(0.5)                                       # the exact ties
    assert np.all(c.rec[c.row("bright_both_clamps"), 4:6] == 1.25) and np.all(c.rec[c.row("dim_0.75"), 4:6] == 0.75)


def test_both_clamps_act_on_the_saturated_patch(emulated):
    """brightness 1.25 saturates the patch above 0.85 in pass 1, contrast 1.25 pushes the saturated values past 1 again, and the dark
    patch below 0: without these the clamps of the colour operations would be dead code under the test"""
    for R in (33, 40, 64):
        c = A.case(R)
        b = c.row("bright_both_clamps")
        canvas = emulated[R][0][b].astype(np.float64)
        assert (canvas == 1.0).sum() >= 4
        blend = 1.25 * canvas - 0.25 * canvas.mean()
        assert (blend[canvas == 1.0] > 1.0).all() and (blend < 0.0).sum() >= 4


def test_emulation_passes_pass1_bit_for_bit_and_stays_inside_the_margin(emulated, tile):
    for R in A.GEOMETRY:
        c, d = A.case(R), A.definition_of(R)
        em = A.Emulator()
        canvas, _ = em.pass1(c.src, c.idx, c.rec, tile)
        assert all(v == (0, 0) for v in A.pass1_violations(canvas, d)), (R, A.pass1_violations(canvas, d))
        off = max(max(np.abs(xs - d.xs[b]).max(), np.abs(ys - d.ys[b]).max()) for b, (xs, ys) in enumerate(em.coords))
        used = off / (A.MARGIN_PER_PIXEL * c.P)
        print(f"EMULATED coordinates R={R} P={c.P}: fp32 - fp64 at most {used:.3f} of the margin")
        assert used <= 0.13
        if "all_outside" in c.names:
            assert not canvas[c.row("all_outside")].any()


def test_ambiguous_share_stays_under_the_cap():
    for R in A.GEOMETRY:
        c, d = A.case(R), A.definition_of(R)
        share = d.amb.reshape(c.B, -1).mean(axis=1)
        for name, s in zip(c.names, share):
            if s > 0:
                print(f"AMBIGUOUS R={R} P={c.P} {name}: {100 * s:.2f} %")
        assert share.max() <= A.AMBIGUOUS_CAP, (R, dict(zip(c.names, share.round(4))))
        for name in ("identity", "rot90_t", "rot180_t", "rot-90_t", "t+x", "t-y", "all_outside"):
            assert name not in c.names or share[c.row(name)] == 0.0
    # the exact ties are where the derivation puts them: both diagonals at 45 degrees on an even canvas, the centre row and column at
    # 30 degrees on an odd one
    assert abs(A.definition_of(40).amb[A.case(40).row("rot45_t")].mean() - 2 / 60) < 0.003
    assert abs(A.definition_of(33).amb[A.case(33).row("rot30_ties")].mean() - 1 / 49) < 0.001
    assert A.definition_of(40).amb[A.case(40).row("rot30_ties")].sum() == 0


def worst_ratios(emulated, tile, constants):
    """class -> {constant: worst emulated err / bound over all cases}"""
    worst = collections.defaultdict(lambda: collections.defaultdict(float))
    for R in A.GEOMETRY:
        c = A.case(R)
        canvas, partial = emulated[R]
        ref, absref = A.tile_sums(canvas, tile)
        for k in constants:
            worst["partials"][k] = max(worst["partials"][k], A.ratio(partial, ref, absref, k))
        for S in A.GEOMETRY[R]:
            out = A.Emulator().pass2(canvas, partial, c.rec, R, S)
            ref, absref, absform = A.pass2_definition(canvas, c.rec, R, S)
            for k in constants:
                worst[A.out_class(R, S)][k] = max(worst[A.out_class(R, S)][k], A.ratio(out, ref, absref, k))
                if S == R:
                    worst["out_full_abs"][k] = max(worst["out_full_abs"][k], A.ratio(out, ref, absform, k))
            print(f"EMULATED R={R} S={S}: out {max(A.out_ratios(out, (ref, absref, absform), R, S)):.3f}")
    return worst


def test_emulation_inside_the_bounds_and_every_constant_minimal(emulated, tile):
    constants = sorted({k * f for k in A.C_ACC.values() for f in (0.5, 1.0)})
    worst = worst_ratios(emulated, tile, constants)
    assert set(worst) == set(A.C_ACC)
    for name, k in A.C_ACC.items():
        print(f"EMULATED-WORST {name}: {worst[name][k]:.3f} at C_ACC = {k:g}, {worst[name][k / 2]:.3f} at {k / 2:g}")
        assert math.log2(k).is_integer() and worst[name][k] <= 0.5 < worst[name][k / 2], (name, dict(worst[name]))


def test_resize_matrices_equal_aten_antialias():
    g = torch.Generator().manual_seed(3)
    for R, S in A.CASES:
        if S == R:
            continue
        img = torch.rand(R, R, generator=g, dtype=torch.float64) * 2 - 1
        want = F.interpolate(img[None, None], size=(S, S), mode="bilinear", antialias=True, align_corners=False)[0, 0].numpy()
        Wm = A.aa_matrix(R, S)
        assert np.abs(Wm.sum(axis=1) - 1).max() < 1e-15
        assert np.abs(Wm @ img.numpy() @ Wm.T - want).max() <= 1e-12, (R, S)


def test_identity_colour_through_the_definition_is_crop_renormalise_resize():
    """with unit factors the whole of pass 2's definition is 2 crop - 1 through the matrices torch agrees with"""
    for R, S in A.CASES:
        c = A.case(R)
        b = c.row("identity") if "identity" in c.names else None
        if b is None:
            continue
        canvas = c.src[c.idx[b]][None]
        ref, _, _ = A.pass2_definition(canvas, c.rec[b:b + 1], R, S)
        crop = torch.from_numpy(canvas[0].astype(np.float64))[R // 4:R // 4 + R, R // 4:R // 4 + R] * 2 - 1
        want = crop if S == R else F.interpolate(crop[None, None], size=(S, S), mode="bilinear", antialias=True, align_corners=False)[0, 0]
        assert np.abs(ref[0] - want.numpy()).max() <= 1e-12


def test_pass1_equals_the_grid_sample_restatement_on_unambiguous_pixels():
    from test_gpu_data import ref_augment
    for R in (3, 4, 33, 40):
        c = A.case(R)
        rec = c.rec.copy()
        rec[:, 4:6] = 1.0                                            # geometry only: unit factors, so that ref_augment returns 2 canvas - 1
        d = A.pass1_definition(c.src, c.idx, rec)
        compared = 0
        for b, (_, angle, tx, ty, flip, *_rest) in enumerate(c.rows):
            want = ref_augment(torch.from_numpy(c.src[c.idx[b]].copy()), float(np.float32(angle)), tx, ty, flip, 1.0, 1.0, 0, c.P, c.P).numpy()
            keep = ~d.amb[b]
            assert np.array_equal((d.cand[b, 0] * np.float32(2) - np.float32(1))[keep], want[keep]), (R, c.names[b])
            compared += int(keep.sum())
        assert compared >= 0.95 * c.B * c.P * c.P


@pytest.mark.parametrize("wrong,R,S,row,what", A.WRONG)
def test_a_wrong_emulation_breaks_its_assertion(tile, wrong, R, S, row, what):
    c, d = A.case(R), A.definition_of(R)
    b = c.row(row)
    seen = {}
    for name, em in (("correct", A.Emulator()), (wrong, A.Emulator(wrong))):
        canvas, partial = em.pass1(c.src, c.idx, c.rec, tile)
        if what == "pass1":
            seen[name] = float(sum(A.pass1_violations(canvas, d)[b]))
            continue
        # pass 2 and the partial sums are judged as on the GPU: against the definition evaluated on the canvas they came with
        if what == "partials":
            ref, absref = A.tile_sums(canvas, tile)
            seen[name] = A.ratio(partial[b], ref[b], absref[b], A.C_ACC["partials"])
        else:
            out = em.pass2(canvas, partial, c.rec, R, S)
            seen[name] = A.out_ratios(out, A.pass2_definition(canvas, c.rec, R, S), R, S)[b]
    print(f"WRONG {wrong} R={R} S={S} {row} {what}: {seen[wrong]:.3g} (correct: {seen['correct']:.3g})")
    if what == "pass1":
        assert seen["correct"] == 0 and seen[wrong] > 0
    else:
        assert seen["correct"] <= 0.5 and seen[wrong] > 1.0


def test_every_wrong_emulation_has_a_case():
    assert {w[0] for w in A.WRONG} == set(A.WRONGS) and len(A.WRONGS) == 15


def test_first_64_partials_fault_cannot_show_below_65_tiles(tile):
    """why R = 256 is in the table: at every other size the partial-sum loop of pass 2 runs once per lane"""
    for R in A.GEOMETRY:
        c = A.case(R)
        nblk = -(-c.P * c.P // tile)
        assert (nblk > 64) == (R == 256)
    c = A.case(64)
    canvas, partial = A.Emulator().pass1(c.src, c.idx, c.rec, tile)
    assert np.array_equal(A.Emulator("first_64_partials_only").pass2(canvas, partial, c.rec, 64, 16),
                          A.Emulator().pass2(canvas, partial, c.rec, 64, 16))


def test_window_fault_shows_on_border_outputs_only(tile):
    c = A.case(40)
    canvas, partial = A.Emulator().pass1(c.src, c.idx, c.rec, tile)
    good, bad = (A.Emulator(w).pass2(canvas, partial, c.rec, 40, 5) for w in (None, "window_over_scale2"))
    ref, absref, _ = A.pass2_definition(canvas, c.rec, 40, 5)
    over = np.abs(bad - ref) > A.C_ACC["out_resized"] * 2.0 ** -24 * absref
    b = c.row("identity")
    assert over[b, 0].all() and over[b, -1].all() and over[b, :, 0].all() and over[b, :, -1].all() and not over[b, 1:-1, 1:-1].any()
    assert not (np.abs(good - ref) > A.C_ACC["out_resized"] * 2.0 ** -24 * absref).any()


# ---- host side ---------------------------------------------------------------------------------------------------------------------------
def dataset(ngan, R=8, **kw):
    return ngan.data.NeuronDataset(torch.zeros(2, 1, R, R), device="cpu", **kw)


def test_pack_params_writes_the_record_the_kernel_reads(ngan):
    for R in A.GEOMETRY:
        c = A.case(R)
        rec = ngan.data.NeuronDataset.pack_params(c.params())
        assert rec.shape == (c.B, 8) and rec.dtype == torch.float32 and rec.is_contiguous()
        assert np.array_equal(rec.numpy().view(np.int32), c.rec.view(np.int32)), R
    p = dict(angle=torch.tensor([30.0, -148.1]), tx=torch.tensor([3.0, -2.0]), ty=torch.tensor([0.0, 5.0]), flip=torch.tensor([1, 0]),
             brightness=torch.tensor([1.25, 0.75]), contrast=torch.tensor([0.8, 1.0]), contrast_first=torch.tensor([0, 1]))
    rec = ngan.data.NeuronDataset.pack_params(p).numpy()
    for b in range(2):
        rad = float(p["angle"][b]) * (math.pi / 180.0)                                           # the fp32 angle, taken in double
        want = [math.cos(rad), math.sin(rad), float(p["tx"][b]), float(p["ty"][b]), float(p["brightness"][b]), float(p["contrast"][b])]
        assert np.array_equal(rec[b, :6], np.array(want, dtype=np.float32))
        assert rec[b, 6:].view(np.int32).tolist() == [int(p["flip"][b]), int(p["contrast_first"][b])]
    assert rec[0, 1] == np.float32(0.5) and rec.tobytes() == rec.astype("<f4").tobytes() and rec.nbytes == 2 * 32


def test_draw_params_without_augmentations_is_the_identity(ngan):
    ds = dataset(ngan, augmentations=False, im_translation=0.1, seed=1)
    state = ds.gen.get_state()
    p = ds.draw_params(7)
    assert torch.equal(ds.gen.get_state(), state)                                                 # nothing is drawn
    assert all(p[k].shape == (7,) for k in p)
    assert not p["angle"].any() and not p["tx"].any() and not p["ty"].any() and not p["flip"].any() and not p["contrast_first"].any()
    assert bool((p["brightness"] == 1).all()) and bool((p["contrast"] == 1).all())
    rec = ds.pack_params(p).numpy()
    assert np.array_equal(rec, np.tile(np.array([1, 0, 0, 0, 1, 1, 0, 0], dtype=np.float32), (7, 1)))


def test_draw_params_draws_torchvisions_ranges_reproducibly(ngan):
    R, n = 40, 4000
    ds = dataset(ngan, R=R, augmentations=True, im_translation=0.1, seed=11)
    assert ds.canvas == A.canvas_of(R)
    p = ds.draw_params(n)
    d = round(0.1 * ds.canvas)
    assert float(p["angle"].min()) >= -180 and float(p["angle"].max()) <= 180 and float(p["angle"].min()) < -170 < 170 < float(p["angle"].max())
    for k in ("tx", "ty"):
        assert torch.equal(p[k], p[k].round()) and float(p[k].abs().max()) == d and set(p[k].tolist()) == set(range(-d, d + 1))
    for k in ("brightness", "contrast"):
        assert 0.75 <= float(p[k].min()) < 0.76 and 1.24 < float(p[k].max()) <= 1.25
    for k in ("flip", "contrast_first"):
        assert p[k].dtype == torch.int32 and set(p[k].tolist()) == {0, 1} and 0.45 < float(p[k].float().mean()) < 0.55
    again = dataset(ngan, R=R, augmentations=True, im_translation=0.1, seed=11).draw_params(n)
    other = dataset(ngan, R=R, augmentations=True, im_translation=0.1, seed=12).draw_params(n)
    assert all(torch.equal(p[k], again[k]) for k in p) and not torch.equal(p["angle"], other["angle"])


def test_zero_translation_consumes_no_uniforms(ngan):
    n = 9
    ds = dataset(ngan, augmentations=True, im_translation=0.0, seed=5)
    p = ds.draw_params(n)
    assert not p["tx"].any() and not p["ty"].any()
    g = torch.Generator().manual_seed(5)                              # the same stream, drawn by hand without the two translations
    u = lambda lo, hi: torch.empty(n).uniform_(lo, hi, generator=g)
    assert torch.equal(p["angle"], u(-180.0, 180.0))
    assert torch.equal(p["flip"], (torch.rand(n, generator=g) < 0.5).int())
    assert torch.equal(p["brightness"], u(0.75, 1.25)) and torch.equal(p["contrast"], u(0.75, 1.25))
    assert torch.equal(p["contrast_first"], (torch.rand(n, generator=g) < 0.5).int())
