"""The generator's spectral loss without a GPU: the fp64 restatement of tests/specloss_cases.py against torch autograd through
torch.fft.fft2, the fp32 emulation of the adjoint kernels against the restatement (every emulated err / bound is printed and at most
0.5: this is where C_INV is settled, before a kernel is looked at), the bound's power to tell six wrong kernels from the right one,
the descent check on the restatement, and the host side of the entry points of include/ngan_spectral.h.  The kernels themselves are
tested on the GPU (tests/test_gpu_specloss.py)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import specloss_cases as L
import spectrum_cases as S

f64 = np.float64


def autograd_ref(images, tgt, scale, floor, on):
    """(loss, per_image, c, grad) through torch autograd in fp64: fft2, |F|^2 / norm, ring means by index_add, the loss as defined"""
    x = torch.from_numpy(np.asarray(images, np.float32)[..., 0]).double().requires_grad_(True)
    B, R, _ = x.shape
    K = R // 2 + 1
    w = torch.from_numpy(S.window2d(R, on).astype(f64))
    F = torch.fft.fft2(w * x)
    P = (F.real ** 2 + F.imag ** 2) / S.norm(R, on)
    idx = torch.from_numpy(S.ring_index(R).ravel())
    sums = torch.zeros(B, int(idx.max()) + 1, dtype=torch.float64).index_add(1, idx, P.reshape(B, -1))
    radial = sums[:, :K] / torch.from_numpy(S.ring_counts(R).astype(f64))
    radial.retain_grad()
    t = torch.from_numpy(np.asarray(tgt, f64))
    q = torch.log((radial[:, 1:] / t[1:] + floor) / (1.0 + floor))
    per_image = (q * q).sum(1) / (R // 2)
    loss = scale * per_image.sum()
    loss.backward()
    return float(loss.detach()), per_image.detach().numpy(), radial.grad.numpy(), x.grad.numpy()


@pytest.mark.parametrize("on", (True, False))
@pytest.mark.parametrize("size", (16, 32, 64))
def test_restatement_against_autograd(size, on):
    x, tgt, scale, rounded = L.case(size, on)
    ref = L.specloss_ref(x.numpy(), tgt, scale, L.FLOOR, on, bounds=False, round_product=False)
    assert abs(ref["loss"] / rounded["loss"] - 1) < 1e-6            # the fp32 product of the definition moves the value this little
    loss, per_image, c, grad = autograd_ref(x.numpy(), tgt, scale, L.FLOOR, on)
    assert abs(loss - ref["loss"]) <= 1e-12 * abs(loss)
    assert np.allclose(per_image, ref["per_image"], rtol=1e-12, atol=0)
    assert np.allclose(c, ref["c"], rtol=1e-11, atol=1e-15 * np.abs(c).max())
    diff = np.abs(grad - ref["grad"]).max()
    print(f"R={size} window={int(on)} closed form against autograd: max |diff| {diff:.3e} of max |grad| {np.abs(grad).max():.3e}")
    assert diff <= 1e-12 * np.abs(grad).max()
    assert ref["c"][:, 0].max() == 0 == ref["c"][:, 0].min() and np.all(ref["per_image"] > 0)


def emulated_ratios(x, tgt, scale, ref, on):
    emu = L.specloss_emu(x, tgt, scale, L.FLOOR, on)
    return {"radial": L.ratio(emu["radial"], ref["radial"], ref["radial_bound"]),
            "per_image": L.ratio(emu["per_image"], ref["per_image"], ref["per_image_bound"]),
            "loss": L.ratio(emu["loss"], ref["loss"], ref["loss_bound"]),
            "c": L.ratio(emu["c"], ref["c"], ref["c_bound"]),
            "grad": max(L.ratio(emu["grad"][b], ref["grad"][b], ref["grad_bound"][b]) for b in range(x.shape[0]))}, emu


@pytest.mark.parametrize("on", (True, False))
@pytest.mark.parametrize("size", S.SMALL_SIZES)
def test_emulation_within_half_the_bound(size, on):
    x, tgt, scale, ref = L.case(size, on)
    ratios, emu = emulated_ratios(x.numpy(), tgt, scale, ref, on)
    per_family = [L.ratio(emu["grad"][b], ref["grad"][b], ref["grad_bound"][b]) for b in range(len(S.FAMILIES))]
    print(f"R={size} window={int(on)} emulated err/bound: " + " ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
    print("    gradient per family: " + " ".join(f"{f} {v:.4f}" for f, v in zip(S.FAMILIES, per_family)))
    assert max(ratios.values()) <= 0.5, (size, on, ratios)
    assert np.all(emu["grad"][:, 0, :] == 0) and np.all(emu["grad"][:, :, 0] == 0) if on else True     # w = 0 there: exact zeros


@pytest.mark.parametrize("size", (256, 512))
def test_emulation_within_half_the_bound_single_images(size):
    for b, fam in enumerate(S.LARGE_FAMILIES):
        x = S.images(size, 1, S.LARGE_FAMILIES)[b:b + 1].numpy()
        tgt = L.target(size)
        ref = L.specloss_ref(x, tgt, L.LAMBDA, L.FLOOR, True)
        ratios, _ = emulated_ratios(x, tgt, L.LAMBDA, ref, True)
        print(f"R={size} {fam:8s} emulated err/bound: " + " ".join(f"{k} {v:.4f}" for k, v in ratios.items()))
        assert max(ratios.values()) <= 0.5, (size, fam, ratios)


def test_emulation_upstream_and_addend():
    x, tgt, scale, _ = L.case(32)
    plain = L.specloss_emu(x.numpy(), tgt, scale)["grad"]
    assert np.array_equal(L.specloss_emu(x.numpy(), tgt, scale, upstream=0.25)["grad"], plain * np.float32(0.25))
    add = np.random.default_rng(5).standard_normal(plain.shape).astype(np.float32)
    assert np.array_equal(L.specloss_emu(x.numpy(), tgt, scale, addend=add)["grad"], add + plain)


@pytest.mark.parametrize("defect", L.DEFECTS)
def test_bound_tells_a_wrong_kernel_from_the_right_one(defect):
    """each defect, applied to the emulation, exceeds the bound at least tenfold somewhere on the two cases: the `rings` image with
    the window off, a white image with the window on.  At R = 16, the smallest size: the bound carries the forward's e, which grows
    as R^2 log R against spectra that grow as R^2 at most, so its power to discriminate is greatest there and falls with R.  The
    geometric defects stay above 10x up to R = 64 and more; the missing floor moves c by about floor / r relative and is seen through
    c's bound alone: 11.9x (rings) and 12.1x (white) at 16, 6.8x and 2.8x at 32."""
    worst = 0.0
    for fam, on in (("rings", False), ("white", True)):
        b = S.FAMILIES.index(fam)
        x = S.images(16, 1)[b:b + 1].numpy()
        tgt = L.target(16, on)
        ref = L.specloss_ref(x, tgt, L.LAMBDA, L.FLOOR, on)
        emu = L.specloss_emu(x, tgt, L.LAMBDA, L.FLOOR, on, defect=defect)
        r = max(L.ratio(emu["grad"], ref["grad"], ref["grad_bound"]), L.ratio(emu["c"], ref["c"], ref["c_bound"]))
        right = L.specloss_emu(x, tgt, L.LAMBDA, L.FLOOR, on)
        assert L.ratio(right["grad"], ref["grad"], ref["grad_bound"]) <= 0.5
        print(f"defect {defect:13s} on {fam:6s} window={int(on)}: err/bound {r:.1f}")
        worst = max(worst, r)
    assert worst >= 10.0, (defect, worst)


def test_descent_on_the_restatement():
    """32 bilinearly upsampled fields optimised directly against the spectrum of white ones: the reference itself takes the loss to a
    tenth and high_db from below -10 dB to above -3 dB, so the GPU test asks the kernels for nothing the definition does not give"""
    start, tgt, real = L.descent_inputs()
    scale = L.LAMBDA / start.shape[0]

    def loss_and_grad(x):
        ref = L.specloss_ref(x.permute(0, 2, 3, 1).numpy(), tgt, scale, L.FLOOR, True, bounds=False)
        return ref["loss"], torch.from_numpy(ref["grad"]).unsqueeze(1)

    before = L.high_db(real, start.numpy())
    first, last, final = L.descend(loss_and_grad, start)
    after = L.high_db(real, final)
    print(f"descent on the fp64 restatement: loss {first:.4f} -> {last:.4f}, high_db {before:.2f} -> {after:.2f} dB")
    assert last <= L.DESCENT["loss_factor"] * first
    assert before <= L.DESCENT["high_before"] and after > L.DESCENT["high_after"]


# ---- host side of the entry points ----------------------------------------------------------------------------------------------------
def test_header_table_and_refusals(ngan):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "ngan.h")).read()
    declared = set(re.findall(r"\b(ngan_[a-z0-9_]+)\s*\(", open(os.path.join(root, "include", "ngan_spectral.h")).read()))
    assert '#include "ngan_spectral.h"' in main
    assert declared == {"ngan_specloss_fwd", "ngan_specloss_head", "ngan_specloss_bwd", "ngan_specloss_fwd_workspace_bytes",
                        "ngan_specloss_bwd_workspace_bytes"} and declared <= set(ngan._C.exported_symbols())
    lib = ngan._C.lib()
    q = lib.ngan_specloss_fwd_workspace_bytes
    assert q(0, 32, 1) == q(1, 48, 1) == q(1, 8, 1) == q(1, 2048, 1) == q(1, 32, 3) == q(65536, 32, 1) == 0
    assert lib.ngan_specloss_bwd_workspace_bytes(2, 32, 3) == 0
    for size in S.SMALL_SIZES + S.LARGE_SIZES:
        half_plane = 3 * (size // 2 + 1) * size * 8
        assert lib.ngan_specloss_bwd_workspace_bytes(3, size, 1) == half_plane
        assert q(3, size, 1) == lib.ngan_spectrum_workspace_bytes(3, size, 1) > half_plane
    # refusals are decided before anything is launched, so they can be seen without a device: a dummy aligned address stands in
    p = ctypes.c_void_p(4096)
    err = lambda: lib.ngan_last_error().decode()                                  # noqa: E731
    assert lib.ngan_specloss_fwd(p, p, p, p, p, 1, 32, 3, 1, None) == -2 and "C=3" in err()
    assert lib.ngan_specloss_fwd(p, p, p, p, p, 1, 48, 1, 1, None) == -2 and "R=48" in err()
    assert lib.ngan_specloss_fwd(p, p, p, p, p, 0, 32, 1, 1, None) == -2 and "B=0" in err()
    assert lib.ngan_specloss_fwd(None, p, p, p, p, 1, 32, 1, 1, None) == -1 and "null" in err()
    assert lib.ngan_specloss_fwd(ctypes.c_void_p(4100), p, p, p, p, 1, 32, 1, 1, None) == -1 and "16-byte" in err()
    assert lib.ngan_specloss_head(p, p, p, 1, 32, 1.0, 0.0, p, p, p, p, p, None) == -1 and "floor" in err()
    assert lib.ngan_specloss_head(p, None, p, 1, 32, 1.0, 1e-3, p, p, p, p, p, None) == -1 and "null" in err()
    assert lib.ngan_specloss_bwd(p, p, p, None, p, p, 1, 32, 3, 1, None) == -2 and "C=3" in err()
    assert lib.ngan_specloss_bwd(p, p, None, None, p, p, 1, 32, 1, 1, None) == -1 and "null" in err()
    assert lib.ngan_specloss_bwd(p, p, p, ctypes.c_void_p(4104), p, p, 1, 32, 1, 1, None) == -1 and "16-byte" in err()
