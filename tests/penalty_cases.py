"""The one-sided and zero-centred forms of the gradient penalty (include/ngan_penalty.h, csrc/penalty.hip): cases, fp64 references with
their absolute-value twins, the per-element bound and fp32 emulations in the kernels' own order.  Shared by tests/test_gpu_penalty.py
(the kernels against the references) and tests/test_penalty_bounds_cpu.py (the emulations against the references: the constants are
settled on the CPU, before any kernel is looked at).  `ratio`'s form, `draws`, `seed_of` and C_ACC are those of tests/stem_head_cases.py.

Bound, per element:   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref + carried,   C_ACC = 8
  The reference is fp64 on the fp32 input g; the kernels see the norm only after it was rounded to fp32, so `carried` is what the
  norm's own error leaves in the output.  The norm's bound is ngan_sample_l2norm's (tests/stem_head_cases.py: n_round 1, absref = ref):
      e_n = (1 + C_ACC / 2) 2^-23 n
  and it is carried through phi (the head) or c_b (the backward) as max |f(n +- e_n) - f(n)|, evaluated in fp64 at both ends (both
  functions are monotone in n, the kink at n = 1 of form 1 included).  Near n = 1 that term is the bound: (n - 1)^2 has no relative
  accuracy there.
n_round per output, from csrc/penalty.hip:
  norms     sqrtf of a sum of squares (positive terms: absref = ref)                                                              1
  penalty   lambda * s / B: two roundings.  n - 1 is exact for n >= 1 (and clamped away below), the terms are positive and each
            enters the sum through one fma: absref = ref                                                                          2
  gradient  form 1: g_out * 2 and n - 1 exact; * lambda, * (n - 1), B * n, the division (gp_coef's four), the product with g       5
            form 2: g_out * lambda, / B, the product with g                                                                       3
            no sum: absref = |ref|
RAISED lists the outputs whose emulated worst err / bound exceeds 0.5 with C_ACC = 8, as tests/stem_head_cases.py does."""
import functools

import numpy as np

import stem_head_cases as S
from stem_head_cases import C_ACC, _block_sum_256, _fma, _lanes, draws, r32, ratio, sample_l2norm_emulate, seed_of  # noqa: F401

f32, f64 = np.float32, np.float64
ONE_SIDED, ZERO_CENTRED = 1, 2
FORMS = (ONE_SIDED, ZERO_CENTRED)
# (B, n): the smallest shapes at which each path exists
SHAPES = [
    (1, 5),          # one row, unaligned tail
    (1, 4),          # one row, aligned
    (3, 1024),       # exactly one 16-byte load per thread of one block
    (5, 3072),       # a typical multi-block row
    (2, 65540),      # all 64 chunks, and a tail (of 16-byte loads) that is not a multiple of 256
    (16, 4096),      # a common batch size
    (257, 4),        # the head's per-thread loop at its second trip
    (300, 8),        # the same, and more rows than one workgroup has threads
]
FAMILIES = ["standard", "above_one", "near_one", "zero_row", "large"]
CASES = [(B, n, fam) for B, n in SHAPES for fam in FAMILIES]
LAMBDA = 10.0
G_OUT = 0.7
# output name -> (raised C_ACC, emulated worst err / bound at that constant)
RAISED = {}
NEAR_ULPS = (-3, -2, -1, 1, 2, 3)


def c_acc(name):
    return float(RAISED.get(name, (C_ACC, None))[0])


def _spread(B, n):
    """u_b in [0, 1), both halves present from B = 2 on; the two one-row shapes take one half each"""
    phase = 0.2 if n % 2 else 0.7
    return (phase + 0.6180339887498949 * np.arange(B)) % 1.0


def target_norms(B, n, family):
    u = _spread(B, n)
    t = 0.25 * 16.0 ** u                                        # [0.25, 4)
    if family == "above_one":
        t = 1.25 * 3.2 ** u                                     # [1.25, 4)
    elif family == "large":
        t = t * 1e3
    elif family == "near_one":
        rows = np.arange(B)
        t = np.where(rows % 4 == 0, 1.0 + np.array(NEAR_ULPS)[(rows // 4) % 6] * 2.0 ** -23, t)
    return t


def exact_one_rows(B, family):
    return [b for b in range(B) if family == "near_one" and b % 4 == 1]


def zero_rows(B, family):
    return [B // 2] if family == "zero_row" else []


@functools.lru_cache(maxsize=None)
def inputs(B, n, family):
    """g (B, n) fp32: standard normal rows scaled in fp64 to the family's norms"""
    g = draws(seed_of(41, B, n, FAMILIES.index(family)), g=(B, n))["g"].astype(f64)
    g = g * (target_norms(B, n, family) / np.sqrt((g ** 2).sum(1)))[:, None]
    for b in exact_one_rows(B, family):
        g[b] = 0.0
        g[b, b % n] = -1.0 if b % 8 == 1 else 1.0
    for b in zero_rows(B, family):
        g[b] = 0.0
    g = g.astype(f32)
    g.setflags(write=False)
    return g


def phi(nrm, form):
    return np.maximum(nrm - 1.0, 0.0) ** 2 if form == ONE_SIDED else 0.5 * nrm ** 2


def coef(nrm, form, lam, g_out, B):
    """c_b in fp64"""
    if form == ZERO_CENTRED:
        return np.full(nrm.shape, float(g_out) * r32(lam) / B)
    safe = np.where(nrm > 1.0, nrm, 1.0)
    return np.where(nrm > 1.0, float(g_out) * 2 * r32(lam) * (safe - 1.0) / (B * safe), 0.0)


def _carried(f, nrm):
    e = (1 + C_ACC / 2) * 2.0 ** -23 * nrm
    return np.maximum(np.abs(f(nrm + e) - f(nrm)), np.abs(f(nrm - e) - f(nrm)))


def norms64(g):
    return np.sqrt((g.astype(f64) ** 2).sum(1))


def head_ref(g, lam, form):
    """name -> (ref, absref, n_round, carried)"""
    nrm = norms64(g)
    r = np.array([r32(lam) * phi(nrm, form).mean()])
    carried = np.array([r32(lam) * _carried(lambda v: phi(v, form), nrm).mean()])
    return {"norms": (nrm, nrm, 1, np.zeros_like(nrm)), "penalty": (r, r, 2, carried)}


def bwd_ref(g, lam, form, g_out):
    nrm, B = norms64(g), g.shape[0]
    c = coef(nrm, form, lam, g_out, B)
    r = c[:, None] * g.astype(f64)
    carried = _carried(lambda v: coef(v, form, lam, g_out, B), nrm)[:, None] * np.abs(g.astype(f64))
    return {"grad": (r, np.abs(r), 5 if form == ONE_SIDED else 3, carried)}


def ratio_carried(got, ref, absref, n_round, carried, c=C_ACC):
    """worst err / bound over the elements: stem_head_cases.ratio with the carried term in the bound"""
    got = np.asarray(got, dtype=f64)
    bound = n_round * 2.0 ** -23 * np.abs(ref) + c * 2.0 ** -24 * absref + carried + 1e-30
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    return float((np.abs(got - ref) / bound).max())


# ---- fp32 emulations: the order of csrc/penalty.hip ---------------------------------------------------------------------------------
def head_emulate(g, lam, form):
    """penalty_sumsq_kernel + penalty_finish_kernel: the norms as sample_l2norm_emulate forms them; then per-thread sums with stride
    256 (one fma per term), block_sum_256, lambda * s / B"""
    norms = sample_l2norm_emulate(np.asarray(g))["norms"]
    if form == ONE_SIDED:
        a = np.maximum(norms - f32(1), f32(0))
        b = a
    else:
        a, b = f32(0.5) * norms, norms
    a, b = _lanes(a, 256), _lanes(b, 256)
    s = np.zeros(256, f32)
    for t in range(a.shape[0]):
        s = _fma(a[t], b[t], s)
    return {"norms": norms, "penalty": np.array([f32(lam) * _block_sum_256(s) / f32(len(norms))], f32)}


def bwd_emulate(g, norms, lam, form, g_out):
    """penalty_bwd_kernel: the row's scalar in gp_coef_kernel's order (form 1; +0.0 rows where the norm is not above 1) or
    g_out * lambda / B (form 2), one product per element"""
    B = g.shape[0]
    if form == ZERO_CENTRED:
        return {"grad": (f32(g_out) * f32(lam) / f32(B)) * np.asarray(g)}
    live = norms > f32(1)
    safe = np.where(live, norms, f32(2))
    c = f32(g_out) * f32(2) * f32(lam) * (safe - f32(1)) / (f32(B) * safe)
    with np.errstate(invalid="ignore"):
        out = np.where(live[:, None], c[:, None] * np.asarray(g), f32(0))
    return {"grad": out.astype(f32)}


# the existing two-sided chain in its own order (stem_head_cases), for the CPU test's anchor: form 1 with every norm above 1 is the chain
def chain_emulate(g, lam, g_out):
    norms = sample_l2norm_emulate(np.asarray(g))["norms"]
    return {"norms": norms, "penalty": S.gp_head_emulate(norms, lam)["out"],
            "grad": S.scale_rows_emulate(np.asarray(g), S.gp_coef_emulate(norms, lam, g_out)["coef"])["out"]}
