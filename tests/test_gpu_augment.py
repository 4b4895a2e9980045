"""The input pipeline's augmentation kernels (csrc/augment.hip, `ngan_augment_batch`) pass by pass against fp64, through the C ABI on
buffers this test allocates: the cases, the definition and the bounds of tests/augment_cases.py, the constants settled on the CPU by
tests/test_augment_bounds_cpu.py against an emulation -- none was chosen after a GPU result.

Per (R, S) of augment_cases.CASES (canvases of 3, 6, 49, 60, 96 and 384 pixels: fewer pixels than a wave, one ragged tile, an odd
canvas, non-power-of-two scales, 4.5 tiles, 72 tiles):
  guards      workspace and output are slices of NaN-filled tensors with 64 floats either side: the guards keep their bits, and no NaN
              is left inside (an element no thread wrote fails)
  pass 1      the canvas, read back from the workspace: every unambiguous pixel bit-equal to its one admissible value, every ambiguous
              one (within 2^-20 P of a rounding boundary; at most 5 % of a sample) equal to one of its up to four
  partials    each within 4 2^-24 sum|v| of the fp64 tile sum of the kernel's own canvas
  pass 2      each output element within its bound of the fp64 definition evaluated on the kernel's own canvas
  exactness   identity geometry with unit factors gives 2 crop - 1 bit for bit at S = R; the all-outside sample has a zero canvas, zero
              partials and -1 everywhere -- exactly at S = R and wherever R / S is a power of two (every weight and every sum of weights
              is then a dyadic fraction below 2^24 ulps, so the sums of -w and the product of the weight sums are exact and their
              quotient is -1); at the scales 3, 5, 11 and 33 the fma chain and the product wys * wxs round differently (the emulation
              is 4 2^-24 off there) and the element bound is what holds
  repeat      a second call on fresh buffers returns the same bits, canvas, partials and output alike: the fixed-order sums
  data.py     NeuronDataset.batch(idx, params) returns the bits of the direct call
and the refusals: S not dividing R, S > R, R > P, B = 0 raise with the library's message and leave the output untouched."""
import numpy as np
import pytest
import torch

import augment_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64              # floats on either side of a buffer: 256 bytes, so the slice stays 16-byte aligned
NAN_BITS = torch.full((1,), float("nan")).view(torch.int32).item()


def guarded(n):
    flat = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    view = flat[GUARD:GUARD + n]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0
    return flat, view


def guards_kept(flat, n):
    bits = flat.view(torch.int32)
    return bool((bits[:GUARD] == NAN_BITS).all()) and bool((bits[GUARD + n:] == NAN_BITS).all())


def run(ngan, c, S):
    """one call on fresh guarded buffers -> canvas (B, P, P), partial (B, nblk), out (B, S, S) as numpy fp32"""
    lib = ngan._C.lib()
    nblk = A.nblk_of(lib, c.B, c.P)
    need = c.B * (c.P * c.P + nblk)
    assert need * 4 == lib.ngan_augment_workspace_bytes(c.B, c.P)
    src = torch.from_numpy(c.src.copy()).to(DEV)
    idx, rec = torch.from_numpy(c.idx.copy()).to(DEV), torch.from_numpy(c.rec.copy()).to(DEV)
    ws_flat, ws = guarded(need)
    out_flat, out = guarded(c.B * S * S)
    ngan._C.call("ngan_augment_batch", src, idx, rec, ws, out, A.N_IMAGES, c.B, c.P, c.R, S)
    torch.cuda.synchronize()
    assert guards_kept(ws_flat, need), "a guard of the workspace was written"
    assert guards_kept(out_flat, c.B * S * S), "a guard of the output was written"
    assert not bool(torch.isnan(ws).any()) and not bool(torch.isnan(out).any()), "an element was left unwritten"
    ws, out = ws.cpu().numpy(), out.cpu().numpy()
    return ws[:c.B * c.P * c.P].reshape(c.B, c.P, c.P), ws[c.B * c.P * c.P:].reshape(c.B, nblk), out.reshape(c.B, S, S)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("R,S", A.CASES)
def test_augment_batch_pass_by_pass_against_fp64(ngan, R, S):
    c, d = A.case(R), A.definition_of(R)
    T = A.tile_pixels(ngan._C.lib())
    canvas, partial, out = run(ngan, c, S)

    # every figure is printed before anything is asserted
    violations = A.pass1_violations(canvas, d)
    pref, pabs = A.tile_sums(canvas, T)
    pr = A.row_ratios(partial, pref, pabs, A.C_ACC["partials"])
    definition = A.pass2_definition(canvas, c.rec, R, S)
    orr = A.out_ratios(out, definition, R, S)
    forms = "" if S != R else " = max of |colour| form {:.3f}, absolute-value form {:.3f}".format(
        A.ratio(out, definition[0], definition[1], A.C_ACC["out_full"]), A.ratio(out, definition[0], definition[2], A.C_ACC["out_full_abs"]))
    share = d.amb.reshape(c.B, -1).mean(axis=1)
    print(f"STAT augment R={R} S={S}: pass1 wrong (unambiguous, ambiguous) {tuple(map(sum, zip(*violations)))}, ambiguous share at most "
          f"{100 * share.max():.2f} %, partials {max(pr):.3f} ({c.names[int(np.argmax(pr))]}), out {max(orr):.3f} ({c.names[int(np.argmax(orr))]}){forms}")

    assert share.max() <= A.AMBIGUOUS_CAP
    assert partial.shape == pref.shape
    bad = {c.names[b]: v for b, v in enumerate(violations) if v != (0, 0)}
    assert not bad, ("pass 1: (unambiguous pixels not bit-equal, ambiguous pixels outside their admissible values)", bad)
    bad = {c.names[b]: v for b, v in enumerate(pr) if not v <= 1.0}
    assert not bad, ("partial sums, err / bound", bad)
    bad = {c.names[b]: v for b, v in enumerate(orr) if not v <= 1.0}
    assert not bad, ("output, err / bound", bad)

    crop = R // 4
    if S == R and "identity" in c.names:
        b = c.row("identity")
        want = c.src[c.idx[b]][crop:crop + R, crop:crop + R] * np.float32(2) - np.float32(1)
        assert np.array_equal(bits(out[b]), bits(want))
    if "all_outside" in c.names:
        b = c.row("all_outside")
        assert not canvas[b].any() and not partial[b].any()
        scale = R // S
        if scale & (scale - 1) == 0:
            assert np.array_equal(bits(out[b]), bits(np.full((S, S), -1.0)))
        else:
            assert np.abs(out[b] + 1.0).max() <= A.C_ACC["out_resized"] * 2.0 ** -24

    again = run(ngan, c, S)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip((canvas, partial, out), again)), "a second call returned other bits"

    ds = ngan.data.NeuronDataset(torch.zeros(A.N_IMAGES, 1, R, R), augmentations=True, im_translation=0.1, device=DEV, seed=0)
    assert ds.canvas == c.P and tuple(ds.images.shape) == c.src.shape
    ds.images = torch.from_numpy(c.src.copy()).to(DEV)
    ds.set_image_size(S)
    params = c.params()
    assert np.array_equal(bits(ds.pack_params(params).numpy()), bits(c.rec))
    got = ds.batch(c.idx.tolist(), params=params)
    assert got.shape == (c.B, 1, S, S)
    assert np.array_equal(bits(got.cpu().numpy()[:, 0]), bits(out)), "NeuronDataset.batch and the direct call differ"


@pytest.mark.parametrize("N,B,P,R,S,why", [
    (5, 3, 60, 40, 16, "S does not divide R"),
    (5, 3, 60, 40, 80, "S > R"),
    (5, 3, 60, 64, 64, "R > P"),
    (5, 0, 60, 40, 40, "B = 0"),
])
def test_augment_batch_refuses(ngan, N, B, P, R, S, why):
    c = A.case(40)
    assert c.P == 60
    src = torch.from_numpy(c.src.copy()).to(DEV)
    idx, rec = torch.from_numpy(c.idx[:3].copy()).to(DEV), torch.from_numpy(c.rec[:3].copy()).to(DEV)
    ws_flat, ws = guarded(3 * (P * P + 8))
    out_flat, out = guarded(3 * 80 * 80)
    with pytest.raises(RuntimeError, match=rf"augment_batch: N={N} B={B} P={P} R={R} S={S} unsupported \(need S \| R <= P\)"):
        ngan._C.call("ngan_augment_batch", src, idx, rec, ws, out, N, B, P, R, S)
    torch.cuda.synchronize()
    for flat in (ws_flat, out_flat):
        assert bool((flat.view(torch.int32) == NAN_BITS).all()), (why, "a refused call wrote")
