"""MS-SSIM between pairs of images (neuron-gan_amd/metrics.py, csrc/msssim.hip): an fp64 restatement of the definition with the
absolute-value twins of the bound, seeded inputs, and an fp32 emulation of the kernel in its own summation order.  Shared by
tests/test_msssim_cpu.py (the restatement against scipy, the emulation against the restatement: the constant is settled on the CPU)
and tests/test_gpu_msssim.py (the kernels against the restatement).

Definition (Wang, Simoncelli and Bovik 2003).  Images are channels-last (P, R, R, C) in an interval of width L (2: [-1, 1]).  Window:
g[i] = exp(-(i - 5)^2 / (2 1.5^2)), i = 0 .. 10, normalised in fp64, then rounded to fp32 (the rounded values ARE the window).
"Valid" filtering: a scale of width H yields (H - 10)^2 entries per channel.  With the weighted moments ma, mb, E[aa], E[bb], E[ab]:
    va = E[aa] - ma^2, vb likewise, cov = E[ab] - ma mb, C1 = (0.01 L)^2, C2 = (0.03 L)^2
    cs = (2 cov + C2) / (va + vb + C2),   l = (2 ma mb + C1) / (ma^2 + mb^2 + C1),   ssim = l cs
per scale the mean over all entries and channels; next scale = 2 x 2 average; S = min(5, 1 + floor(log2(R / 11))) scales; weights the
first S of (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) renormalised; MS-SSIM = prod_{s<S} max(cs_s, 0)^w_s max(ssim_S, 0)^w_S.

Bound, the project's form, per map entry:   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref
The kernel's error sits in the five moments: each is two nested 11-term fmaf chains (and one product rounding for the second
moments), an error relative to the moment of the absolute values (all window weights are positive).  To first order a ratio
q = num / den moves by (d num + |q| d den) / den, and d num, d den are relative to the terms of num and den with absolute values
carried through:  with A1 = E|a|, B1 = E|b|, A2 = E[aa], B2 = E[bb], AB = E|ab|
    cs:    num' = 2 (AB + A1 B1) + C2,  den' = (A2 + A1^2) + (B2 + B1^2) + C2,   absref_cs = (num' + |cs| den') / (va + vb + C2)
    l:     num' = 2 A1 B1 + C1,         den' = A1^2 + B1^2 + C1,                 absref_l  = (num' + |l| den') / (ma^2 + mb^2 + C1)
    ssim:  absref = |l| absref_cs + |cs| absref_l
On a flat background va + vb + C2 is C2 = 3.6e-3 against moments near 1: absref_cs is then several hundred, which is the
cancellation of E[x^2] - mu^2 said in numbers.  n_round (fp32 roundings at or after the last addition, each relative to the value):
cs and l: the last fmaf of num, the last addition of den, the division = 3 each; ssim: 3 + 3 + the product = 7.  The per-pair bound of
a scale is the mean of the per-entry bounds, in fp64 (the kernel's fp64 sums add nothing visible).  No entry is left out anywhere.
C_ACC = 8, the project's constant (tests/wide_f32_cases.py): tests/test_msssim_cpu.py prints the emulated err / bound of every case
and holds it to 0.5; had one exceeded it, C_ACC would be raised to the next power of two there, before a kernel is looked at.
Whole metric: every factor max(v, 0)^w is monotone in v, so the bound is the wider side of
[prod max(v_s - bound_s, 0)^w_s, prod max(v_s + bound_s, 0)^w_s] around the reference."""
import functools

import numpy as np
import torch

f32, f64 = np.float32, np.float64
C_ACC = 8.0
N_ROUND = {"cs": 3, "ssim": 7}
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
WIN = 11
DATA_RANGE = 2.0

# ---- shapes: the smallest that reach every branch (the kernel's output tile is 32 x 32, one workgroup per tile and pair) ----------
SCALE_SIZES = (16, 32, 64, 256)      # valid maps 6 (one ragged tile), 22 (one ragged tile), 54 (2 x 2 tiles, ragged), 246 (8 x 8, ragged)
COLORS = (1, 3)
METRIC_SIZES = (16, 64, 256)         # 1, 3 and 5 scales


def n_scales(size):
    s = 0
    while size >= 16 and s < 5:
        s, size = s + 1, size // 2
    return s


def weights(scales):
    w = np.array(WEIGHTS[:scales], dtype=f64)
    return w / w.sum()


def window():
    """the 11 taps as fp64 numbers that are exactly representable in fp32"""
    i = np.arange(WIN, dtype=f64)
    g = np.exp(-(i - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    return (g / g.sum()).astype(f32).astype(f64)


def constants(data_range=DATA_RANGE):
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


def seed_of(tag, *shape):
    s = tag
    for v in shape:
        s = (s * 131 + int(v)) % (2 ** 31 - 1)
    return s


# ---- seeded inputs --------------------------------------------------------------------------------------------------------------------
def smooth_field(gen, size, c):
    """a random field in [-1, 1] with structure at a few pixels: uniform noise under two 3 x 3 box filters, stretched"""
    x = torch.rand(1, c, size + 4, size + 4, generator=gen) * 2 - 1
    x = torch.nn.functional.avg_pool2d(torch.nn.functional.avg_pool2d(x, 3, stride=1), 3, stride=1)
    return (x[0] * 3.0).clamp(-1, 1).permute(1, 2, 0).contiguous()


def arbor(gen, size, c):
    """a neuron-like image: an exact -1 background with a few thin bright random walks; most windows are flat"""
    img = torch.full((size, size, c), -1.0)
    for _ in range(2):
        y, x = (torch.rand(2, generator=gen) * size).tolist()
        ang = float(torch.rand(1, generator=gen)) * 6.283
        for _ in range(size):
            yi, xi = int(y) % size, int(x) % size
            img[yi, xi] = torch.rand(c, generator=gen) * 0.8 + 0.2
            ang += float(torch.randn(1, generator=gen)) * 0.3
            y, x = y + np.sin(ang), x + np.cos(ang)
    return img


FAMILIES = ("same", "corr 0.9", "corr 0.3", "corr -0.5", "negated", "independent", "neuron", "neuron same", "neuron vs flat",
            "constant equal", "constant different", "corner")


@functools.lru_cache(maxsize=None)
def pairs(size, c):
    """(a, b): fp32 (len(FAMILIES), size, size, c), one pair per family, in FAMILIES' order"""
    gen = torch.Generator().manual_seed(seed_of(11, size, c))
    a_all, b_all = [], []
    for fam in FAMILIES:
        a = smooth_field(gen, size, c)
        if fam == "same":
            b = a.clone()
        elif fam.startswith("corr"):
            rho = float(fam.split()[1])
            b = (rho * a + (1 - rho * rho) ** 0.5 * smooth_field(gen, size, c)).clamp(-1, 1)
        elif fam == "negated":
            b = -a                                             # cs < 0 everywhere: the clamp of the combination
        elif fam == "independent":
            b = smooth_field(gen, size, c)
        elif fam == "neuron":
            a, b = arbor(gen, size, c), arbor(gen, size, c)
        elif fam == "neuron same":
            a = arbor(gen, size, c)
            b = a.clone()
        elif fam == "neuron vs flat":
            a, b = arbor(gen, size, c), torch.full((size, size, c), -1.0)
        elif fam == "constant equal":
            a, b = torch.full((size, size, c), -1.0), torch.full((size, size, c), -1.0)
        elif fam == "constant different":
            a, b = torch.full((size, size, c), 0.3), torch.full((size, size, c), -0.7)
        elif fam == "corner":
            k = max(5, size // 8)                              # equal but for the bottom-right k x k block, which only the last
            b = a.clone()                                      # outputs of the last (ragged) tiles see, the outermost 10 rows and
            b[-k:, -k:] = -a[-k:, -k:].sign() * 1.0            # columns of it through the far end of their halo alone
        a_all.append(a)
        b_all.append(b)
    return torch.stack(a_all).float().contiguous(), torch.stack(b_all).float().contiguous()


# ---- fp64 restatement -----------------------------------------------------------------------------------------------------------------
def filt(x):
    """valid separable filtering of fp64 (P, H, H, C) -> (P, H - 10, H - 10, C)"""
    g = [float(t) for t in window()]
    v = x.shape[1] - WIN + 1
    rows = sum(g[k] * x[:, :, k:k + v] for k in range(WIN))
    return sum(g[k] * rows[:, k:k + v] for k in range(WIN))


def pool2_ref(x):
    """2 x 2 average in fp64"""
    return 0.25 * (x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2])


def scale_maps(a, b, data_range=DATA_RANGE):
    """per entry, fp64: {'cs', 'ssim'} -> (ref map, absref map)"""
    a, b = a.double(), b.double()
    c1, c2 = constants(data_range)
    ma, mb, eaa, ebb, eab = filt(a), filt(b), filt(a * a), filt(b * b), filt(a * b)
    a1, b1, ab = filt(a.abs()), filt(b.abs()), filt((a * b).abs())
    den_cs = (eaa - ma * ma) + (ebb - mb * mb) + c2
    cs = (2 * (eab - ma * mb) + c2) / den_cs
    abs_cs = ((2 * (ab + a1 * b1) + c2) + cs.abs() * ((eaa + a1 * a1) + (ebb + b1 * b1) + c2)) / den_cs
    den_l = ma * ma + mb * mb + c1
    lum = (2 * ma * mb + c1) / den_l
    abs_l = ((2 * a1 * b1 + c1) + lum.abs() * (a1 * a1 + b1 * b1 + c1)) / den_l
    return {"cs": (cs, abs_cs), "ssim": (lum * cs, lum.abs() * abs_cs + cs.abs() * abs_l)}


def scale_ref(a, b, data_range=DATA_RANGE):
    """{'cs', 'ssim'} -> (ref, bound), fp64 arrays of one value per pair: the mean of the map and the mean of the per-entry bound"""
    out = {}
    for name, (ref, absref) in scale_maps(a, b, data_range).items():
        bound = N_ROUND[name] * 2.0 ** -23 * ref.abs() + C_ACC * 2.0 ** -24 * absref
        out[name] = (ref.mean((1, 2, 3)).numpy(), bound.mean((1, 2, 3)).numpy())
    return out


def combine(values, bounds=None):
    """values: list over the scales of (P,) arrays (cs ... cs, ssim) -> MS-SSIM (P,); with bounds also its propagated bound"""
    w = weights(len(values))
    ms = np.prod([np.maximum(v, 0.0) ** w[s] for s, v in enumerate(values)], axis=0)
    if bounds is None:
        return ms
    hi = np.prod([np.maximum(v + e, 0.0) ** w[s] for s, (v, e) in enumerate(zip(values, bounds))], axis=0)
    lo = np.prod([np.maximum(v - e, 0.0) ** w[s] for s, (v, e) in enumerate(zip(values, bounds))], axis=0)
    return ms, np.maximum(hi - ms, ms - lo)


def msssim_ref(a, b, data_range=DATA_RANGE):
    """(MS-SSIM, bound) per pair, fp64.  Each scale's reference starts from the fp32 images the kernels start from (the pooled
    images are rounded to fp32 once, as ngan_msssim_pool2 does, so the bound carries the scale kernels' error alone)"""
    scales = n_scales(a.shape[1])
    vals, bnds = [], []
    for s in range(scales):
        r = scale_ref(a, b, data_range)["ssim" if s == scales - 1 else "cs"]
        vals.append(r[0])
        bnds.append(r[1])
        if s < scales - 1:
            a, b = pool2_ref(a.double()).float(), pool2_ref(b.double()).float()
    return combine(vals, bnds)


# ---- fp32 emulation in the kernel's order ---------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _chain(x, axis):
    """acc = 0; acc = fmaf(g[k], x[k], acc), k = 0 .. 10, along `axis` (1: rows of the image, i.e. the column pass; 2: the row pass)"""
    g = window().astype(f32)
    v = x.shape[axis] - WIN + 1
    acc = np.zeros([v if d == axis else n for d, n in enumerate(x.shape)], f32)
    for k in range(WIN):
        sl = [slice(None)] * x.ndim
        sl[axis] = slice(k, k + v)
        acc = _fma(g[k], x[tuple(sl)], acc)
    return acc


def scale_emu(a, b, data_range=DATA_RANGE):
    """{'cs', 'ssim'} -> (P,) fp64: csrc/msssim.hip's arithmetic on fp32 numpy arrays (P, H, H, C)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    c1, c2 = (f32(v) for v in constants(data_range))
    mom = [_chain(_chain(x, 2), 1) for x in (a, b, a * a, b * b, a * b)]      # products rounded to fp32, rows first, then columns
    ma, mb, eaa, ebb, eab = mom
    va, vb, cov = _fma(-ma, ma, eaa), _fma(-mb, mb, ebb), _fma(-ma, mb, eab)
    cs = _fma(f32(2), cov, c2) / ((va + vb) + c2)
    lum = _fma(f32(2), ma * mb, c1) / ((ma * ma + mb * mb) + c1)
    ssim = lum * cs
    assert cs.dtype == f32 and ssim.dtype == f32
    return {"cs": cs.astype(f64).mean((1, 2, 3)), "ssim": ssim.astype(f64).mean((1, 2, 3))}


def pool2_emu(x):
    x = np.asarray(x, f32).astype(f64)
    return (0.25 * ((x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2]))).astype(f32)


def msssim_emu(a, b, data_range=DATA_RANGE):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    scales = n_scales(a.shape[1])
    vals = []
    for s in range(scales):
        vals.append(scale_emu(a, b, data_range)["ssim" if s == scales - 1 else "cs"])
        if s < scales - 1:
            a, b = pool2_emu(a), pool2_emu(b)
    return combine(vals)


@functools.lru_cache(maxsize=None)
def scale_case(size, c):
    """(a, b, reference) of the family batch at one size: computed once, shared by the tests, never written to"""
    a, b = pairs(size, c)
    return a, b, scale_ref(a, b)


@functools.lru_cache(maxsize=None)
def metric_case(size, c):
    """four pairs (same, corr 0.3, negated, neuron vs flat) through the whole metric: (a, b, MS-SSIM, bound)"""
    a, b = pairs(size, c)
    pick = [FAMILIES.index(f) for f in ("same", "corr 0.3", "negated", "neuron vs flat")]
    a, b = a[pick].contiguous(), b[pick].contiguous()
    ref, bound = msssim_ref(a, b)
    return a, b, ref, bound
