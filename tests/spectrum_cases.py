"""Radial power spectrum of images (neuron-gan_amd/metrics.py, csrc/spectrum.hip): an fp64 restatement of the definition, seeded
input families, the per-element bound, and an fp32 emulation of the kernels in their own butterfly order with their own twiddles.
Shared by tests/test_spectrum_cpu.py (the restatement against brute force and Parseval, the emulation against the restatement: the
constant is settled on the CPU) and tests/test_gpu_spectrum.py (the kernels against the restatement).

Definition.  Images are channels-last fp32 (B, R, R, C), R a power of two in 16 .. 1024, C in (1, 3).
  window   h[i] = 0.5 - 0.5 cos(2 pi i / R) (periodic Hann) in fp64, rounded to fp32: the rounded values ARE the window.
           w[y][x] = h[y] h[x] is one fp32 product, x w one more.  Window off: w = 1, no product.
  F        F[fy][fx] = sum_{y,x} (w x)[y][x] exp(-2 pi i (fy y + fx x) / R) per image and channel (numpy fft2 in fp64 on the fp32 w x).
  P        |F|^2 / sum w^2; the divisor ("norm") is an fp64 constant of R.  The restatement sums the squares of the rounded products;
           the library uses the separable (sum h^2)^2 of the same taps, which differs by less than 2^-24 relative -- far inside the
           3 2^-23 P term of the bound.  White noise of variance s^2 has E[P] = s^2 everywhere.
  rings    signed frequencies u, v in [-R/2, R/2), d = u^2 + v^2; bin k is the integer with (2k-1)^2 <= 4d < (2k+1)^2 (k = 0 for
           d = 0), i.e. floor(sqrt(d) + 1/2) decided in integers.  Bins 0 .. R/2 are kept, the corners (k > R/2) dropped.
  S        S[k] = sum over channels and the ring's frequencies of P / (C n_k): (B, R/2 + 1) fp64.
  metric   mean over images per set and bin; ratio_db[k] = 10 log10(fake / real); distance_db = mean_{k=1..R/2} |ratio_db|;
           high_db = mean of ratio_db over R/4 < k <= R/2.

Bound, per spectral element (the project's form): a length-R^2 transform is log2(R^2) butterfly stages, each rounding relative to
sums that never exceed A = sum |w x|, so |F_got - F_ref| <= e = C_ACC 2^-24 log2(R^2) A, and
    |P_got - P_ref| <= (2 |F_ref| e + e^2) / norm + 3 2^-23 P_ref
(the three roundings: the two products and the addition of |F|^2; the kernel's division by norm in fp64 and the rounding of the
stored fp32 power fit in the slack of that term).  A ring's bound is the mean of its elements' bounds; no element is left out.
C_ACC = 8, the project's constant: tests/test_spectrum_cpu.py prints the emulated err / bound of every case and holds it to 0.5.

Shapes.  The kernels are compiled per R (seven instantiations); what changes between them:
    R = 16    16 rows / 8 columns per workgroup: one row group per image, 32 of 256 threads hold a butterfly, radix-4 stages only
    R = 32    32 rows / 16 columns per workgroup: one row group, radix-2 tail
    R = 64    32 rows / 16 columns: two row groups, every thread one butterfly
    R = 128   16 rows / 8 columns from here on: eight row groups, radix-2 tail, two radix-2 butterflies per thread
    R = 256, 512, 1024   2, 4, 8 radix-4 butterflies per thread; 512 has the radix-2 tail; bins beyond the 256th share a thread
The column pass's last workgroup of every size holds one valid column (fx = R/2) and zero fill.  So: the whole family batch at
R = 16, 32, 64, 128 with C = 1 and 3, and single images (B = 1, C = 1) at 256, 512 and 1024."""
import functools

import numpy as np
import torch

f32, f64 = np.float32, np.float64
C_ACC = 8.0
SMALL_SIZES = (16, 32, 64, 128)
LARGE_SIZES = (256, 512, 1024)          # B = 1, C = 1, the families of LARGE_FAMILIES
COLORS = (1, 3)
FAMILIES = ("impulse", "rings", "corner", "constant", "white", "arbor", "upsampled")
LARGE_FAMILIES = ("impulse", "rings", "white")


def seed_of(tag, *shape):
    s = tag
    for v in shape:
        s = (s * 131 + int(v)) % (2 ** 31 - 1)
    return s


# ---- definition -----------------------------------------------------------------------------------------------------------------------
def window(R):
    """the R Hann taps as fp64 numbers that are exactly representable in fp32"""
    i = np.arange(R, dtype=f64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * i / R)).astype(f32).astype(f64)


def window2d(R, on=True):
    """w[y][x] as the kernel forms it: one fp32 product of two taps (ones with the window off)"""
    if not on:
        return np.ones((R, R), f32)
    h = window(R).astype(f32)
    return h[:, None] * h[None, :]


def norm(R, on=True):
    return float((window2d(R, on).astype(f64) ** 2).sum())


def norm_separable(R, on=True):
    """the library's divisor: (sum h^2)^2 of the fp32 taps in fp64; R^2 with the window off"""
    return float((window(R) ** 2).sum() ** 2) if on else float(R) * float(R)


def ring_of(d):
    """the integer rule on an int64 array of d = u^2 + v^2"""
    d = np.asarray(d, np.int64)
    k = np.floor(np.sqrt(d.astype(f64)) + 0.5).astype(np.int64)
    for _ in range(2):                                    # settle the estimate in integers
        k = np.where((2 * k - 1) ** 2 > 4 * d, k - 1, k)
        k = np.where((2 * k + 1) ** 2 <= 4 * d, k + 1, k)
    k = np.where(d == 0, 0, k)
    assert np.all(((2 * k - 1) ** 2 <= 4 * d) | (d == 0)) and np.all(4 * d < (2 * k + 1) ** 2)
    return k


@functools.lru_cache(maxsize=None)
def ring_index(R):
    """(R, R) int64 in fft order (index f is the signed frequency f for f < R/2, f - R otherwise): the bin of every frequency"""
    f = np.arange(R, dtype=np.int64)
    f = np.where(f < R // 2, f, f - R)
    return ring_of(f[:, None] ** 2 + f[None, :] ** 2)


@functools.lru_cache(maxsize=None)
def ring_counts(R):
    """n_0 .. n_{R/2}"""
    return np.bincount(ring_index(R).ravel())[:R // 2 + 1].astype(np.int64)


def windowed(images, on=True):
    """(B, C, R, R) fp32: x w as the kernel loads it"""
    x = np.asarray(images, f32).transpose(0, 3, 1, 2)
    return x * window2d(x.shape[-1], on) if on else x.copy()


def spectrum_ref(images, on=True):
    """fp64 reference of a batch: {'power' (B, C, R, R/2+1), 'power_bound', 'radial' (B, R/2+1), 'radial_bound', 'full' (B, C, R, R)}"""
    wx = windowed(images, on).astype(f64)
    B, C, R, _ = wx.shape
    nrm = norm(R, on)
    F = np.fft.fft2(wx)
    P = (F.real ** 2 + F.imag ** 2) / nrm
    A = np.abs(wx).sum((2, 3), keepdims=True)
    e = C_ACC * 2.0 ** -24 * np.log2(float(R) * R) * A
    bound = (2.0 * np.abs(F) * e + e * e) / nrm + 3.0 * 2.0 ** -23 * P
    idx, n = ring_index(R).ravel(), ring_counts(R)
    K = R // 2 + 1
    radial, rbound = np.zeros((B, K)), np.zeros((B, K))
    for b in range(B):
        radial[b] = np.bincount(idx, P[b].sum(0).ravel())[:K] / (C * n)
        rbound[b] = np.bincount(idx, bound[b].sum(0).ravel())[:K] / (C * n)
    return {"power": P[..., :K], "power_bound": bound[..., :K], "radial": radial, "radial_bound": rbound, "full": P}


def radial_ref(images, on=True):
    return spectrum_ref(images, on)["radial"]


def metric_ref(real, fake):
    """the two-set metric on radial spectra (n, R/2 + 1) fp64"""
    real, fake = np.asarray(real, f64), np.asarray(fake, f64)
    K = real.shape[1]
    R = 2 * (K - 1)
    mr, mf = real.mean(0), fake.mean(0)
    ok = (mr > 0) & (mf > 0)
    ratio = np.full(K, np.nan)
    ratio[ok] = 10.0 * np.log10(mf[ok] / mr[ok])
    k = np.arange(K)
    score, high = ok & (k >= 1), ok & (k > R // 4)
    return {"real": mr, "fake": mf, "ratio_db": ratio, "distance_db": float(np.abs(ratio[score]).mean()),
            "high_db": float(ratio[high].mean()), "skipped_bins": int((~ok[1:]).sum())}


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------------
def ring_frequencies(R):
    """[(k, u, v, a_k)]: for every k = 1 .. R/2 a signed frequency (u along y, v along x) of ring k and the amplitude 1 + k / R.  k = 1
    lies on the axis u = 0, k = 2 on v = 0, k = R/2 is (-R/2, 0), its own conjugate, and ring R/2 carries a second cosine at
    (1, -R/2) (the column v = -R/2 off the axis, which the half-plane layout stores once with weight 1); the rest sweep the angles."""
    out = [(1, 0, 1, 1 + 1 / R), (2, 2, 0, 1 + 2 / R)]
    for k in range(3, R // 2):
        th = (k * 0.6180339887498949 * np.pi) % np.pi
        u, v = int(round(k * np.cos(th))), int(round(k * np.sin(th)))
        if int(ring_of(u * u + v * v)) != k:
            u, v = 0, -k
        out.append((k, u, v, 1 + k / R))
    out.append((R // 2, -R // 2, 0, 1.5))
    out.append((R // 2, 1, -R // 2, 1.5))
    assert all(int(ring_of(u * u + v * v)) == k for k, u, v, _ in out)
    return out


def cosine(R, u, v, a):
    y, x = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    return a * np.cos(2.0 * np.pi * ((u * y + v * x) % R) / R)


def white(gen, R, c, n=1):
    return torch.rand(n, R, R, c, generator=gen) * 2 - 1


def upsampled(gen, R, c, n=1):
    """bilinear x2 (align_corners=False, the generator's own upsampling) of a half-size white field"""
    x = (torch.rand(n, c, R // 2, R // 2, generator=gen) * 2 - 1)
    x = torch.nn.functional.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    return x.permute(0, 2, 3, 1).contiguous()


def arbor(gen, R, c):
    """a neuron-like image: an exact -1 background with a few thin bright random walks (the idea of msssim_cases.arbor)"""
    img = torch.full((R, R, c), -1.0)
    for _ in range(2):
        y, x = (torch.rand(2, generator=gen) * R).tolist()
        ang = float(torch.rand(1, generator=gen)) * 6.283
        for _ in range(R):
            img[int(y) % R, int(x) % R] = torch.rand(c, generator=gen) * 0.8 + 0.2
            ang += float(torch.randn(1, generator=gen)) * 0.3
            y, x = y + np.sin(ang), x + np.cos(ang)
    return img


def family(name, R, c, gen):
    """one fp32 (R, R, c) image"""
    if name == "impulse":
        img = torch.zeros(R, R, c)
        img[R // 3, R // 5] = 1.0
        return img
    if name == "rings":
        tot = sum(cosine(R, u, v, a) for _, u, v, a in ring_frequencies(R))
        return torch.from_numpy(tot).float().unsqueeze(-1).repeat(1, 1, c)
    if name == "corner":
        return torch.from_numpy(cosine(R, R // 2 - 1, R // 2 - 1, 1.0)).float().unsqueeze(-1).repeat(1, 1, c)
    if name == "constant":
        return torch.full((R, R, c), -1.0)
    if name == "white":
        return white(gen, R, c)[0]
    if name == "arbor":
        return arbor(gen, R, c)
    if name == "upsampled":
        return upsampled(gen, R, c)[0]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def images(R, c, families=FAMILIES):
    """fp32 (len(families), R, R, c), one image per family, in order"""
    gen = torch.Generator().manual_seed(seed_of(17, R, c))
    return torch.stack([family(f, R, c, gen) for f in families]).float().contiguous()


@functools.lru_cache(maxsize=None)
def case(R, c, on, families=FAMILIES):
    """(images, reference) of one shape and window setting: computed once, shared by the tests, never written to"""
    x = images(R, c, families)
    return x, spectrum_ref(x.numpy(), on)


def white_set(R, n, seed, c=1):
    return white(torch.Generator().manual_seed(seed_of(23, R, n, seed)), R, c, n).contiguous()


def upsampled_set(R, n, seed, c=1):
    return upsampled(torch.Generator().manual_seed(seed_of(29, R, n, seed)), R, c, n).contiguous()


# ---- fp32 emulation in the kernels' order ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twiddles(R):
    """(re, im) fp32 of exp(-2 pi i k / R), k < R: cospi / sinpi of 2 k / R in fp64 (exact argument, exact zeros and ones on the axes,
    reduced to the first octant as a correctly working sincospi does), rounded once -- the table the kernels build in LDS"""
    k = np.arange(R)
    q, r = (4 * k) // R, k % (R // 4)                    # quadrant, position inside it
    fold = r > R // 8
    rr = np.where(fold, R // 4 - r, r).astype(f64)
    c0, s0 = np.cos(2.0 * np.pi * rr / R), np.sin(2.0 * np.pi * rr / R)
    c, s = np.where(fold, s0, c0), np.where(fold, c0, s0)
    c, s = np.where(r == 0, 1.0, c), np.where(r == 0, 0.0, s)
    cq = np.choose(q, [c, -s, -c, s])
    sq = np.choose(q, [s, c, -s, -c])
    return cq.astype(f32), (-sq).astype(f32)


def _cmul(wr, wi, tr, ti):
    return wr * tr - wi * ti, wr * ti + wi * tr


def fft_emu(re, im):
    """the kernels' Stockham transform along the last axis: radix-4 stages, a radix-2 tail for odd log2 R; every operation is one
    fp32 rounding (contraction is off in csrc/spectrum.hip)"""
    re, im = np.asarray(re, f32), np.asarray(im, f32)
    R = re.shape[-1]
    lead = re.shape[:-1]
    twr, twi = twiddles(R)
    n, s = R, 1
    while n >= 4:
        n1 = n // 4
        xr, xi = re.reshape(lead + (4, n1, s)), im.reshape(lead + (4, n1, s))
        ar, br, cr, dr = (xr[..., j, :, :] for j in range(4))
        ai, bi, ci, di = (xi[..., j, :, :] for j in range(4))
        p = np.arange(n1) * s
        w = [(twr[m * p][:, None], twi[m * p][:, None]) for m in (1, 2, 3)]
        apcr, apci, amcr, amci = ar + cr, ai + ci, ar - cr, ai - ci
        bpdr, bpdi = br + dr, bi + di
        jr, ji = -(bi - di), br - dr                     # j (b - d)
        y0 = (apcr + bpdr, apci + bpdi)
        y1 = _cmul(*w[0], amcr - jr, amci - ji)
        y2 = _cmul(*w[1], apcr - bpdr, apci - bpdi)
        y3 = _cmul(*w[2], amcr + jr, amci + ji)
        re = np.stack([y0[0], y1[0], y2[0], y3[0]], axis=-2).reshape(lead + (R,))
        im = np.stack([y0[1], y1[1], y2[1], y3[1]], axis=-2).reshape(lead + (R,))
        n, s = n1, 4 * s
    if n == 2:
        xr, xi = re.reshape(lead + (2, s)), im.reshape(lead + (2, s))
        re = np.stack([xr[..., 0, :] + xr[..., 1, :], xr[..., 0, :] - xr[..., 1, :]], axis=-2).reshape(lead + (R,))
        im = np.stack([xi[..., 0, :] + xi[..., 1, :], xi[..., 0, :] - xi[..., 1, :]], axis=-2).reshape(lead + (R,))
    assert re.dtype == f32 and im.dtype == f32
    return re, im


def spectrum_emu(images, on=True):
    """{'power' (B, C, R, R/2+1) fp32, 'radial' (B, R/2+1) fp64}: csrc/spectrum.hip's arithmetic on numpy fp32 arrays.  Row pass: rows
    2t and 2t+1 packed as re + i im, transformed along x, split by the conjugate symmetry (one addition and one exact halving per
    part); column pass: the transform along y of columns fx = 0 .. R/2; |F|^2 = re re + im im with three roundings; fp64 from there
    (the order of the fp64 sums is the kernel's business and invisible at this precision)."""
    wx = windowed(images, on)
    B, C, R, _ = wx.shape
    K = R // 2 + 1
    zr, zi = fft_emu(wx[:, :, 0::2, :], wx[:, :, 1::2, :])
    rev = (-np.arange(K)) % R
    yr, yi = zr[..., rev], zi[..., rev]
    zr, zi = zr[..., :K], zi[..., :K]
    gr, gi = np.empty((B, C, R, K), f32), np.empty((B, C, R, K), f32)
    gr[:, :, 0::2], gi[:, :, 0::2] = (zr + yr) * f32(0.5), (zi - yi) * f32(0.5)
    gr[:, :, 1::2], gi[:, :, 1::2] = (zi + yi) * f32(0.5), (yr - zr) * f32(0.5)
    fr, fi = fft_emu(gr.transpose(0, 1, 3, 2), gi.transpose(0, 1, 3, 2))          # (B, C, fx, fy)
    mag = (fr * fr + fi * fi).transpose(0, 1, 3, 2)                              # (B, C, fy, fx)
    assert mag.dtype == f32
    nrm = norm_separable(R, on)
    weight = np.full(K, 2.0)
    weight[0] = weight[-1] = 1.0
    idx, n = ring_index(R)[:, :K].ravel(), ring_counts(R)
    radial = np.zeros((B, K))
    for b in range(B):
        radial[b] = np.bincount(idx, (mag[b].astype(f64).sum(0) * weight).ravel())[:K] / (C * n * nrm)
    return {"power": (mag.astype(f64) / nrm).astype(f32), "radial": radial}
