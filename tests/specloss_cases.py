"""Spectral regularisation of the generator (include/ngan_spectral.h, csrc/specloss.hip, ops.SpectralLoss): an fp64 restatement of the
loss, its per-image values, the coefficients c = dL/dS and the image gradient in closed form; the per-element bounds; an fp32
emulation of the adjoint in the kernels' order.  Shared by tests/test_specloss_bounds_cpu.py (the restatement against torch autograd,
the emulation against the restatement: the constant is settled on the CPU) and tests/test_gpu_specloss.py (the kernels against the
restatement).  All notation is tests/spectrum_cases.py's, which this file imports.

Definition.  Per image x (one colour channel), S the radial spectrum (window w, F = fft2(w x), P = |F|^2 / norm), a target t[k] > 0, a
floor d and scale = lambda / B_global:
    r = S / t,  q = ln((r + d) / (1 + d)),  l[b] = sum_{k=1..R/2} q^2 / (R/2),  L = scale sum_b l[b]
    c[b][k] = dL/dS = scale / (R/2) 2 q / (t (r + d))  (k >= 1; 0 for bin 0, for t[k] <= 0 and for the corners k > R/2)
    a[f] = c[ring(f)] / (n_ring(f) norm),   dL/dx = 2 w Re(sum_f a[f] F[f] exp(+2 pi i f.p / R)) = 2 w R^2 ifft2(a o F)

Bounds, from fp64 reference quantities only, no element left out.  With Sb = spectrum_cases' radial_bound and g = t (r + d) - Sb > 0
(the slope 1 / (t (r + d)) of q at the worst point of the interval):
    |dq| <= Sb / g;   l: sum (2 |q| dq + dq^2) / (R/2);   L: scale sum of those + 2^-23 |L| (its one fp32 rounding, an ulp)
    c:   |A| (1 + |q| + dq) Sb / g^2 + 2^-23 |c|,  A = 2 scale / (R/2)            (dc/dS = A (1 - q) / (t (r + d))^2)
    gradient, per pixel:  2 w (T1 + T2 + T3) + 4 2^-24 |reference|  with
        T1 = e sum_f |a_f|                     the forward's e = C_ACC 2^-24 log2(R^2) sum |w x| on every F_f
        T2 = sum_f |da_f| |F_f|                da_f = (c's bound + 2 2^-24 |c|) / (n norm): the coefficient's error and roundings
        T3 = C_INV 2^-24 log2(R^2) sum_f |a_f F_f|     the inverse transform's own roundings
A pixel with w = 0 (row 0, column 0) has bound 0 and the kernel stores an exact zero there.
C_INV = 8, the project's constant.  tests/test_specloss_bounds_cpu.py prints the emulated err / bound of every case and holds it to
0.5; worst ratios there: gradient 0.0100 (R = 128, the impulse; 0.0055 for the single images at 256 and 512), c 0.046 at 16 .. 128 and
0.22 at 512 (its one fp32 rounding against an ulp), l 0.0087, L 0.15.  The bound is dominated by T1 and T2 (the forward's conservative
e), so the constant of T3 hardly shows; the six defects of the discrimination test still exceed the bound tenfold and more at R = 16
(12x for the missing floor, through c's bound; 27x to 2600x for the others).  On an MI355X the kernels give the emulation's gradient
bits on every case, and c 0.34 at 1024.

Shapes: the forward's (spectrum_cases): the family batch at R = 16, 32, 64, 128, single images of LARGE_FAMILIES at 256, 512, 1024."""
import functools

import numpy as np
import torch

import spectrum_cases as S

f32, f64 = np.float32, np.float64
C_INV = 8.0
FLOOR = 1e-3
LAMBDA = 1.0
DEFECTS = ("no_nyquist", "double_edges", "ring_shift", "no_window", "no_two", "no_floor")


@functools.lru_cache(maxsize=None)
def target(R, on=True):
    """the fp64 reference's mean radial spectrum of white_set(R, 8, 1): (R/2 + 1,) fp64, every bin about 1/3"""
    return S.radial_ref(S.white_set(R, 8, 1).numpy(), on).mean(0)


def head_ref(radial, tgt, scale, floor, use_floor=True):
    """(q, l, L, c) in fp64 from radial spectra (B, K)"""
    radial, tgt = np.asarray(radial, f64), np.asarray(tgt, f64)
    K = radial.shape[1]
    half = K - 1
    ok = (tgt > 0) & (np.arange(K) >= 1)
    t = np.where(ok, tgt, 1.0)
    r = radial / t
    if use_floor:
        q = np.where(ok, np.log((r + floor) / (1.0 + floor)), 0.0)
        c = np.where(ok, scale / half * 2.0 * q / (t * (r + floor)), 0.0)
    else:
        q = np.where(ok, np.log(np.where(ok, r, 1.0)), 0.0)
        c = np.where(ok, scale / half * 2.0 * q / (t * np.where(ok, r, 1.0)), 0.0)
    ell = (q * q).sum(1) / half
    return q, ell, scale * ell.sum(), c


def ring_table(R):
    """(R, R) int64 ring of every frequency in fft order and the mask of those kept (1 <= k <= R/2)"""
    idx = S.ring_index(R)
    return idx, (idx >= 1) & (idx <= R // 2)


def specloss_ref(images, tgt, scale, floor=FLOOR, on=True, bounds=True, round_product=True):
    """fp64 restatement of a batch of channels-last fp32 images (B, R, R, 1): {'radial', 'per_image', 'loss', 'c', 'grad' (B, R, R)} and,
    with bounds, {'radial_bound', 'per_image_bound', 'loss_bound', 'c_bound', 'grad_bound'}.  round_product=False (no bounds then):
    w x is taken in fp64 instead of as the fp32 product the definition names -- a function of x that autograd can be asked about."""
    x = np.asarray(images, f32)
    B, R = x.shape[0], x.shape[1]
    half, K = R // 2, R // 2 + 1
    tgt = np.asarray(tgt, f64)
    idx, keep = ring_table(R)
    n, nrm = S.ring_counts(R), S.norm(R, on)
    if round_product:
        ref = S.spectrum_ref(x, on)
        wx = S.windowed(x, on).astype(f64)[:, 0]
        F = np.fft.fft2(wx)
    else:
        assert not bounds
        wx = x[..., 0].astype(f64) * S.window2d(R, on).astype(f64)
        F = np.fft.fft2(wx)
        P = (F.real ** 2 + F.imag ** 2) / nrm
        ref = {"radial": np.stack([np.bincount(idx.ravel(), P[b].ravel())[:K] / n for b in range(B)])}
    q, ell, L, c = head_ref(ref["radial"], tgt, scale, floor)
    kk = np.where(keep, idx, 0)
    a = np.where(keep, c[:, kk] / (n[kk] * nrm), 0.0)                              # (B, R, R)
    w2 = 2.0 * S.window2d(R, on).astype(f64)
    grad = w2 * float(R) * R * np.fft.ifft2(a * F).real
    out = {"radial": ref["radial"], "per_image": ell, "loss": L, "c": c, "grad": grad, "q": q}
    if not bounds:
        return out
    Sb = ref["radial_bound"]
    ok = (tgt > 0) & (np.arange(K) >= 1)
    t = np.where(ok, tgt, 1.0)
    g = t * (ref["radial"] / t + floor) - Sb
    assert np.all(g[:, ok] > 0), "the radial bound reaches the floor: no slope to bound q with"
    dq = np.where(ok, Sb / np.where(ok, g, 1.0), 0.0)
    ell_b = (2.0 * np.abs(q) * dq + dq * dq).sum(1) / half + 1e-13 * ell
    A = abs(2.0 * scale / half)
    c_core = np.where(ok, A * (1.0 + np.abs(q) + dq) * Sb / np.where(ok, g, 1.0) ** 2, 0.0)
    c_b = c_core + 2.0 ** -23 * np.abs(c)
    e = S.C_ACC * 2.0 ** -24 * np.log2(float(R) * R) * np.abs(wx).sum((1, 2))      # (B,)
    da = np.where(keep, (c_b + 2.0 * 2.0 ** -24 * np.abs(c))[:, kk] / (n[kk] * nrm), 0.0)
    t1 = e * np.abs(a).sum((1, 2))
    t2 = (da * np.abs(F)).sum((1, 2))
    t3 = C_INV * 2.0 ** -24 * np.log2(float(R) * R) * np.abs(a * F).sum((1, 2))
    grad_b = w2 * (t1 + t2 + t3)[:, None, None] + 4.0 * 2.0 ** -24 * np.abs(grad)
    out.update({"radial_bound": Sb, "per_image_bound": ell_b, "loss_bound": abs(scale) * ell_b.sum() + 2.0 ** -23 * abs(L), "c_bound": c_b,
                "grad_bound": grad_b})
    return out


@functools.lru_cache(maxsize=None)
def case(R, on=True, families=S.FAMILIES):
    """(images (B, R, R, 1) fp32 tensor, target, scale, reference): computed once, shared by the tests, never written to"""
    x = S.images(R, 1, families)
    scale = LAMBDA / x.shape[0]
    return x, target(R, on), scale, specloss_ref(x.numpy(), target(R, on), scale, FLOOR, on)


def ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound; an element with bound 0 must be met exactly (inf otherwise)"""
    err = np.abs(np.asarray(got, f64) - np.asarray(ref, f64))
    bound = np.broadcast_to(np.asarray(bound, f64), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


# ---- fp32 emulation in the kernels' order ---------------------------------------------------------------------------------------------
def transform_emu(images, on=True):
    """(re, im) fp32 (B, K, R): the half-plane transform F[b][v][fy] as csrc/spectrum_fft.h's row and column passes leave it
    (spectrum_cases.spectrum_emu's own steps, kept before the squares are taken)"""
    wx = S.windowed(images, on)[:, 0]
    B, R, _ = wx.shape
    K = R // 2 + 1
    zr, zi = S.fft_emu(wx[:, 0::2, :], wx[:, 1::2, :])
    rev = (-np.arange(K)) % R
    yr, yi = zr[..., rev], zi[..., rev]
    zr, zi = zr[..., :K], zi[..., :K]
    gr, gi = np.empty((B, R, K), f32), np.empty((B, R, K), f32)
    gr[:, 0::2], gi[:, 0::2] = (zr + yr) * f32(0.5), (zi - yi) * f32(0.5)
    gr[:, 1::2], gi[:, 1::2] = (zi + yi) * f32(0.5), (yr - zr) * f32(0.5)
    return S.fft_emu(gr.transpose(0, 2, 1), gi.transpose(0, 2, 1))


def specloss_emu(images, tgt, scale, floor=FLOOR, on=True, upstream=1.0, addend=None, defect=None):
    """{'radial', 'per_image', 'loss', 'c' fp32, 'grad' fp32 (B, R, R)}: csrc/specloss.hip's arithmetic on numpy arrays.  The head in
    fp64 on the emulated radial values, c rounded once, the coefficient a = c / (n norm) divided in fp64 and rounded once; the column
    pass scales F, conjugates, transforms along fy and conjugates; the row pass completes the Hermitian half (real parts of columns 0
    and R/2), packs two rows, conjugates, transforms, conjugates; then (g (2 w)) upstream (+ addend).  defect: one of DEFECTS, a wrong
    kernel the bound must tell from the right one."""
    assert defect is None or defect in DEFECTS
    x = np.asarray(images, f32)
    B, R = x.shape[0], x.shape[1]
    half, K = R // 2, R // 2 + 1
    radial = S.spectrum_emu(x, on)["radial"]
    _, ell, L, c = head_ref(radial, tgt, scale, floor, use_floor=defect != "no_floor")
    n, nrm = S.ring_counts(R), S.norm_separable(R, on)
    a32 = (c / (n[:K] * nrm)).astype(f32)
    a32[:, 0] = 0
    idx = S.ring_index(R)[:, :K].T                                                 # (v, fy)
    if defect == "ring_shift":
        idx = idx + 1
    keep = (idx >= 1) & (idx <= half)
    coef = np.where(keep, a32[:, np.where(keep, idx, 0)], f32(0)).astype(f32)      # (B, K, R)
    fr, fi = transform_emu(x, on)
    pr, pi = fr * coef, -(fi * coef)
    hr, hi = S.fft_emu(pr, pi)
    hr, hi = hr.transpose(0, 2, 1), (-hi).transpose(0, 2, 1)                        # H[b][y][v]
    x0r, x0i, x1r, x1i = hr[:, 0::2], hi[:, 0::2], hr[:, 1::2], hi[:, 1::2]        # (B, R/2, K)
    zr, zi = np.zeros((B, half, R), f32), np.zeros((B, half, R), f32)
    edge = f32(2) if defect == "double_edges" else f32(1)
    for v in (0, half):
        zr[..., v], zi[..., v] = x0r[..., v] * edge, -(x1r[..., v] * edge)
    if defect == "no_nyquist":
        zr[..., half], zi[..., half] = 0, 0
    v = np.arange(1, half)
    zr[..., v], zi[..., v] = x0r[..., v] - x1i[..., v], -(x0i[..., v] + x1r[..., v])
    zr[..., R - v], zi[..., R - v] = x0r[..., v] + x1i[..., v], -(x1r[..., v] - x0i[..., v])
    gr, gi = S.fft_emu(zr, zi)
    g = np.empty((B, R, R), f32)
    g[:, 0::2], g[:, 1::2] = gr, -gi
    w = S.window2d(R, on and defect != "no_window")
    w2 = w if defect == "no_two" else f32(2) * w
    grad = (g * w2) * f32(upstream)
    if addend is not None:
        grad = np.asarray(addend, f32) + grad
    assert grad.dtype == f32
    return {"radial": radial, "per_image": ell, "loss": f32(L), "c": c.astype(f32), "grad": grad}


# ---- the descent check ----------------------------------------------------------------------------------------------------------------
DESCENT = {"R": 32, "n": 32, "lr": 0.05, "steps": 50, "loss_factor": 0.1, "high_before": -10.0, "high_after": -3.0}


def descent_inputs():
    """(start (32, 32, 32, 1) fp32, target (17,) fp64, real radial (32, 17) fp64): bilinearly upsampled fields against white ones"""
    real = S.radial_ref(S.white_set(DESCENT["R"], DESCENT["n"], 3).numpy(), True)
    return S.upsampled_set(DESCENT["R"], DESCENT["n"], 4), real.mean(0), real


def high_db(real_radial, images):
    return S.metric_ref(real_radial, S.radial_ref(np.asarray(images, f32), True))["high_db"]


def descend(loss_and_grad, start):
    """Adam (lr 0.05, 50 steps) on the images themselves; loss_and_grad(x (B, 1, R, R) tensor) -> (loss float, grad tensor like x).
    Returns (first loss, last loss, final images (B, R, R, 1) numpy)"""
    x = start.permute(0, 3, 1, 2).contiguous().clone()
    x.requires_grad_(True)
    opt = torch.optim.Adam([x], lr=DESCENT["lr"])
    first = None
    for _ in range(DESCENT["steps"]):
        loss, grad = loss_and_grad(x.detach())
        first = loss if first is None else first
        x.grad = grad.to(x.dtype)
        opt.step()
    last, _ = loss_and_grad(x.detach())
    return first, last, x.detach().permute(0, 2, 3, 1).cpu().numpy()
