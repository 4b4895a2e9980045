"""Cases, oracle and emulation of the adaptive augmentation controller (include/ngada.h; csrc/ada.hip, csrc/ada_bits.h).

Every check built on this module is exact: the counters are integers, and p / last_r are fp32 values compared bit for bit with an
emulation that follows csrc/ada_bits.h line by line.  Nothing here has a tolerance.

Score cases are built so that the comparison of a score with the threshold does not depend on the order the kernel sums in:
  * "dyadic" cases: every score is a multiple of 1/8 of magnitude at most 8, so any sum of up to 65536 of them is exact in fp64 in any
    order and the midpoint -- two correctly rounded divisions, one addition, one halving of exact sums -- has the same bits in any order.
    They are laid out around two dyadic means, with scores placed exactly ON the midpoint (deliberate ties);
  * "far" cases: normal draws; the builder asserts that no real score lies within 1e-6 of the exactly rounded fp64 midpoint.  Any
    summation order of n values of magnitude at most 16 errs by at most n * 2^-53 * (16 n) in the sum, i.e. n * 2^-53 * 16 in the mean:
    1.2e-10 at n = 65536, so a comparison that clears 1e-6 cannot flip.
  * cases with NaN and +-inf: the class of the sum (NaN, +inf, -inf, finite) does not depend on the order either.
The oracle counts with Python integers and forms the midpoint from math.fsum; the emulation sums in the kernel's own order."""
import math
from fractions import Fraction

import numpy as np

F32, F64 = np.float32, np.float64
SIZES = (1, 2, 5, 8, 63, 64, 65, 257, 65536)          # batch sizes of the accumulate checks (the issue's list)
THREADS = 256                                          # ada::THREADS


# ---- scores -------------------------------------------------------------------------------------------------------------------------
def _around(rng, n, mean, tie_delta):
    """n multiples of 1/8 whose sum is exactly n * mean: pairs mean +- d (the first pair at +- tie_delta, so that one of the two lies on
    the midpoint), and `mean` itself when n is odd"""
    out = [mean] if n % 2 else []
    deltas = [tie_delta] + [float(rng.integers(0, 17)) / 8.0 for _ in range(n // 2 - 1)] if n >= 2 else []
    for d in deltas:
        out += [mean + d, mean - d]
    out = np.array(out, dtype=F64)
    rng.shuffle(out)
    return out.astype(F32)


def dyadic_case(n_real, n_fake, seed):
    rng = np.random.default_rng(seed)
    mr, mf = float(rng.integers(-8, 9)) / 4.0, float(rng.integers(-8, 9)) / 4.0
    if n_real == 1:
        mf = mr                                                                # the only real score is the midpoint: a tie
    mid = 0.5 * (mr + mf)
    real, fake = _around(rng, n_real, mr, mid - mr), _around(rng, n_fake, mf, 0.5)
    assert float(np.sum(real.astype(F64))) == n_real * mr and float(np.sum(fake.astype(F64))) == n_fake * mf
    assert np.abs(real).max() <= 8 and np.abs(fake).max() <= 8 and np.any(real.astype(F64) == mid), "no tie with the midpoint"
    return real, fake


def far_case(n_real, n_fake, seed, margin=1e-6):
    for attempt in range(64):
        rng = np.random.default_rng(1000 * seed + attempt)
        real = np.clip(rng.normal(0.3, 1.0, n_real), -15, 15).astype(F32)
        fake = np.clip(rng.normal(-0.4, 1.0, n_fake), -15, 15).astype(F32)
        mid = 0.5 * (math.fsum(real.astype(F64)) / n_real + math.fsum(fake.astype(F64)) / n_fake)
        if np.abs(real.astype(F64) - mid).min() > margin and np.abs(real.astype(F64) - 0.5).min() > margin:
            return real, fake
    raise AssertionError("no draw clears the margin")


def special_cases():
    """(name, real, fake, mode, threshold): NaN and +-inf among the scores, and a NaN threshold"""
    nan, inf = float("nan"), float("inf")
    base = np.array([-1.0, 0.25, nan, 0.5, inf, -inf, 0.5, 2.0, nan, 0.0], dtype=F32)
    fake = np.array([0.5, -0.5, 1.0], dtype=F32)
    return [
        ("nan_inf_threshold", base, fake, 0, 0.5),
        ("nan_threshold", base, fake, 0, nan),
        ("inf_threshold", base, fake, 0, inf),
        ("nan_inf_midpoint", base, fake, 1, 0.0),                                      # a NaN among the reals: t is NaN, n alone counts
        ("nan_in_fakes", np.array([1.0, -1.0, 3.0], dtype=F32), np.array([nan, 0.0], dtype=F32), 1, 0.0),
        ("posinf_in_reals", np.array([1.0, inf, -2.0, inf], dtype=F32), fake, 1, 0.0),   # t = +inf: finite scores below, inf itself a tie
        ("neginf_in_fakes", np.array([1.0, -inf, -2.0], dtype=F32), np.array([-inf, 0.0], dtype=F32), 1, 0.0),
        ("both_inf", np.array([inf, 1.0, -inf], dtype=F32), fake, 1, 0.0),
    ]


def score_cases(sizes=SIZES):
    """(name, real, fake, mode, threshold) over the sizes: dyadic and far scores in both modes, unequal counts, the special values"""
    out = []
    for k, b in enumerate(sizes):
        nf = b if k % 2 == 0 else max(1, (b * 3) // 4 + 1)                     # n_fake = n_real, or another count
        dr, df = dyadic_case(b, nf, 11 + k)
        out.append((f"dyadic_mid_{b}", dr, df, 1, 0.0))
        out.append((f"dyadic_thr_{b}", dr, None if k % 3 else df, 0, 0.5 if k % 2 else float(dr[0])))    # 0.5 or a score itself: ties
        fr, ff = far_case(b, nf, 31 + k)
        out.append((f"far_mid_{b}", fr, ff, 1, 0.0))
        out.append((f"far_thr_{b}", fr, None, 0, 0.5))
    return out + special_cases()


# ---- accumulate: oracle and emulation ------------------------------------------------------------------------------------------------
def _exact_sum(x):
    x = np.asarray(x, dtype=F64)
    if np.isnan(x).any() or (np.isposinf(x).any() and np.isneginf(x).any()):
        return float("nan")
    if np.isinf(x).any():
        return float("inf") if np.isposinf(x).any() else float("-inf")
    return math.fsum(x)


def oracle_counts(real, fake, mode, threshold):
    """(pos, neg, n) as Python integers: the threshold of mode 1 from exactly rounded sums"""
    t = float(threshold) if mode == 0 else 0.5 * (_exact_sum(real) / len(real) + _exact_sum(fake) / len(fake))
    pos = sum(1 for s in real.tolist() if s > t)
    neg = sum(1 for s in real.tolist() if s < t)
    return pos, neg, len(real)


def device_sum(x):
    """the kernel's order: thread k adds elements k, k + 256, ... ascending in fp64; a butterfly over each wave of 64; the four waves
    in order"""
    lanes = np.zeros(THREADS, dtype=F64)
    x = np.asarray(x, dtype=F32)
    for start in range(0, len(x), THREADS):
        chunk = x[start:start + THREADS].astype(F64)
        lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
    v = lanes.reshape(4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, np.arange(64) ^ o]
    r = v[:, 0]
    return ((r[0] + r[1]) + r[2]) + r[3]


def emulate_accumulate(counters, real, fake, mode, threshold):
    """ngada_accumulate on a list of four Python integers, following accumulate_kernel and ada::midpoint / ada::side"""
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == 1:
            mr = device_sum(real) / F64(len(real))
            mf = device_sum(fake) / F64(len(fake))
            t = F64(0.5) * (mr + mf)
        else:
            t = F64(F32(threshold))
        v = np.asarray(real, dtype=F32).astype(F64)
        pos, neg = int(np.count_nonzero(v > t)), int(np.count_nonzero(v < t))
    return [counters[0] + pos, counters[1] + neg, counters[2] + len(real), counters[3]]


# ---- update: cases, oracle and emulation ---------------------------------------------------------------------------------------------
def update_cases():
    """(pos, neg, n, p, last_r, target, span, p_max): both clamps, n = 0, d = 0, a NaN p, counts above 2^31 and near 2^40.  Every case
    has a product target * n that fp64 holds exactly, so the sign of the fp64 difference is the sign of the exact one."""
    t06 = float(F32(0.6))
    big, huge = (1 << 33) + 5, (1 << 40) - 3
    grid = [
        (6, 2, 8, 0.25, 0.1, 0.25, 1000.0, 1.0),              # r = 0.5 above the target: up by 8 / 1000
        (2, 6, 8, 0.25, 0.1, 0.25, 1000.0, 1.0),              # below: down
        (6, 2, 8, 0.25, 0.1, 0.5, 1000.0, 1.0),               # d = 0 exactly: p stays
        (0, 0, 0, 0.25, -0.75, 0.6, 1000.0, 1.0),             # n = 0: p and last_r stay
        (1, 7, 8, 0.001, 0.0, 0.6, 1000.0, 1.0),              # lower clamp
        (0, 8, 8, 0.0, 0.0, 0.6, 8.0, 1.0),                   # at the lower clamp already
        (8, 0, 8, 0.999, 0.0, 0.6, 1000.0, 1.0),              # upper clamp at 1
        (8, 0, 8, 0.29, 0.0, 0.6, 100.0, 0.3),                # upper clamp at p_max = fp32(0.3)
        (8, 0, 8, 0.5, 0.0, 0.6, 100.0, 0.3),                 # above p_max (a resumed run under a lower clamp): comes down to it
        (8, 0, 8, 0.0, 0.0, 0.6, 100.0, 0.0),                 # p_max = 0
        (5, 3, 8, float("nan"), 0.0, 0.0, 1000.0, 1.0),       # a NaN p becomes 0
        (3, 5, 8, float("nan"), 0.0, 0.6, 1000.0, 1.0),
        (13, 3, 16, 0.5, 0.0, t06, 500000.0, 1.0),            # Karras's settings, one interval of four batches of four
        (9, 7, 16, 0.5, 0.0, t06, 500000.0, 1.0),
        (big, 0, big, 0.125, 0.0, 0.5, float(1 << 36), 1.0),  # counts above 2^31
        ((big + 1) // 2, big // 2, big, 0.125, 0.0, 0.5, float(1 << 36), 1.0),
        (huge, 1, huge + 1, 0.0, 0.0, 0.75, float(1 << 42), 1.0),     # near 2^40
        (1, huge, huge + 1, 0.9, 0.0, 0.75, float(1 << 42), 1.0),
        (huge // 2, huge // 2, huge - 1, 0.3, 0.2, 0.0, 1e12, 1.0),   # pos = neg with target 0: d = 0
        (4, 0, 4, 0.0, 0.0, 0.6, 4.0, 1.0),                   # one update spans the whole range
        (7, 1, 8, 0.3, 0.0, 0.6, 3.0, 1.0),                   # a span that does not divide evenly
    ]
    for pos, neg, n, _, _, target, _, _ in grid:
        prod = Fraction(float(F32(target))) * n
        assert Fraction(float(prod)) == prod, "the product target * n must be exact in fp64"
    return grid


def oracle_update(pos, neg, n, p, last_r, target, span, p_max):
    """The rule as the header states it: the sign from exact rational arithmetic on Python integers, the step in fp64 (Python floats
    are IEEE doubles, one rounding per operation), the result rounded to fp32 once.  -> (p, last_r) as np.float32"""
    d = Fraction(pos - neg) - Fraction(float(F32(target))) * n
    s = 0 if n == 0 else (d > 0) - (d < 0)
    q = float(F32(p)) + float(s * n) / float(span)
    q = q if q > 0.0 else 0.0
    q = q if q < float(F32(p_max)) else float(F32(p_max))
    r = F32(float(pos - neg) / float(n)) if n else F32(last_r)
    return F32(q), r


def emulate_update(pos, neg, n, p, last_r, target, span, p_max):
    """ada::update line by line in numpy scalars -> (p, last_r) as np.float32"""
    with np.errstate(invalid="ignore"):
        diff = F64(pos - neg)
        nd = F64(n)
        tn = F64(F32(target)) * nd
        d = diff - tn
        s = F64(0.0) if n == 0 else F64(int(d > 0.0) - int(d < 0.0))
        sn = s * nd
        move = sn / F64(span)
        q = F64(F32(p)) + move
        q = q if q > 0.0 else F64(0.0)
        pm = F64(F32(p_max))
        q = q if q < pm else pm
        return F32(q), (F32(diff / nd) if n else F32(last_r))


def bits(x):
    """the bit pattern of an fp32 value or array, for exact comparison (a NaN equals itself, -0 differs from +0)"""
    return np.asarray(x, dtype=F32).view(np.int32)
