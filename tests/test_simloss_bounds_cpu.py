"""The error bounds of the pairwise similarity loss, settled on the CPU (tests/simloss_cases.py has the oracle, the emulation and the
derivation): the emulation of the kernels stays inside every bound on every case, and each of six wrong kernels exceeds a bound at
least tenfold -- so the GPU tests, which hold the kernels to the same bounds, can fail.  No element of any output is left out: every
ratio is a maximum over the whole array."""
import functools

import numpy as np
import pytest

import simloss_cases as L

LAM, UP = 0.7, 0.37
SHAPES = [(b, 1024) for b in L.BATCHES] + [(3, 16), (5, 4100)]


@functools.lru_cache(maxsize=None)
def inputs(family, b, n):
    x = L.images(family, b, n)
    z = L.latents(b)
    addend = np.random.default_rng(5 + b).uniform(-1e-3, 1e-3, x.shape).astype(np.float32)
    return x, z, addend


def families(n):
    return [f for f in L.FAMILIES if f != "micrograph" or int(round(n ** 0.5)) ** 2 == n]


@pytest.mark.parametrize("center", [False, True], ids=["raw", "centred"])
@pytest.mark.parametrize("b, n", SHAPES)
def test_the_emulation_stays_within_every_bound(b, n, center):
    for family in families(n):
        x, z, addend = inputs(family, b, n)
        for up, add in ((1.0, None), (UP, addend)):
            out = L.emulate(x, z, LAM, center, up, add)
            got = L.ratios(out, x, z, LAM, center, up, add)
            print(f"STAT simloss_emu family={family} B={b} N={n} center={int(center)} up={up:g} addend={int(add is not None)} "
                  + " ".join(f"{k}={v:.3g}" for k, v in got.items()))
            assert max(got.values()) <= 1.0, (family, got)


@pytest.mark.parametrize("defect", L.DEFECTS)
def test_a_wrong_kernel_exceeds_its_bound_tenfold(defect):
    """diagonal_kept: no special case for j == i (the generic M formula stands on the diagonal, d_ii is not forced to 0);
    no_mix_diagonal: M_ii = 0; no_shift: r = 0; fp32_centring: the mean taken after the product sum, in fp32; b_squared: a
    1 / (B B) normaliser; not_symmetrised: dL/dS_ij counted once, not for (i, j) and (j, i)."""
    worst = {}
    for b, n in ((2, 1024), (5, 1024), (16, 1024), (64, 1024)):
        for family in L.FAMILIES:
            x, z, addend = inputs(family, b, n)
            got = L.ratios(L.emulate(x, z, LAM, True, UP, addend, defect=defect), x, z, LAM, True, UP, addend)
            worst[(b, family)] = max(got.values())
            print(f"STAT simloss_defect {defect} family={family} B={b} N={n} " + " ".join(f"{k}={v:.3g}" for k, v in got.items()))
    # at every batch size, on the noise and on the micrograph rows.  (The constructed families are printed only: with two identical or
    # opposite rows at B = 2 the cosine sits at an extremum, the gradient vanishes and so does r -- a kernel without r is right there.)
    held = {k: v for k, v in worst.items() if k[1] in ("noise", "micrograph")}
    assert all(v >= 10.0 for v in held.values()), {k: v for k, v in held.items() if v < 10.0}


def test_the_centring_figures_of_the_design_note():
    """DESIGN.md section 7 quotes three figures for 8 micrograph fields at 128 x 128: raw cosines 0.87 .. 0.91, centred 0.17 .. 0.32,
    latent cosines 0 +- 0.044 at 512 dimensions; the first two are properties of the synthetic fields and are held here"""
    x = L.images("micrograph", 8, 128 * 128)
    off = ~np.eye(8, dtype=bool)
    raw = L.oracle(x, L.latents(8), 1.0, False)["S"][off]
    cen = L.oracle(x, L.latents(8), 1.0, True)["S"][off]
    print(f"STAT simloss_centring raw {raw.min():.3f} .. {raw.max():.3f} centred {cen.min():.3f} .. {cen.max():.3f}")
    assert raw.min() > 0.8 and cen.max() < 0.5 and cen.max() < raw.min()
