"""The scalar heads of the least-squares losses (ngan_lsloss_head / ngan_lsloss_head_bwd, the last section of csrc/pointwise.hip): inputs,
fp64 references with their absolute-value twins, the per-element bound and fp32 emulations in the kernels' own summation order.  Shared
by tests/test_gpu_lsgan.py (the kernels against the references) and tests/test_lsgan_bounds_cpu.py (the emulations against the
references: the constants are settled on the CPU, before any kernel is looked at).  Conventions, `ratio`, `draws`, `seed_of` and the
emulation helpers are those of tests/stem_head_cases.py.

Bound, per element:   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref,   C_ACC = 8
n_round per output, from the kernel source (the roundings applied AFTER the element's last addition; the rounding of a last addition
itself counts as one), counted as that file's header counts wloss_head:
  lsloss_head      mean_real / mean_fake: sum / n                                                                                  1
                   loss: qr / n_real + qf / n_fake, the last addition (the two divisions come before it: terms' roundings, which
                   the absref term carries); n_fake = 0: qr / n_real, the division                                                 1
                   d = s - t is one correctly rounded subtraction of two fp32 inputs (relative to |d|, whatever cancels), d * d
                   enters an fma: every term (s - t)^2 is positive and carries a relative error, so absref = ref
  lsloss_head_bwd  fma(2 gl, s - t, gm) / n: the fma's addition, the division (2 gl is exact; s - t rounds before the addition: a
                   term's rounding).  absref = (2 |gl| (|s| + |t|) + |gm|) / n                                                     2

RAISED, as in tests/stem_head_cases.py: the outputs whose emulated worst err / bound exceeds 0.5 with C_ACC = 8, with the next power of
two that brings it to 0.5 or below and the emulated ratio at that constant; tests/test_lsgan_bounds_cpu.py pins both.  No entry: the
emulated worst ratios are loss 0.17, mean_real 0.10, mean_fake 0.10, gs 0.20."""
import numpy as np

from stem_head_cases import C_ACC, _block_sum_256, _fma, _lanes, draws, r32, ratio, seed_of  # noqa: F401  (re-exported)

f32, f64 = np.float32, np.float64
# output name -> (raised C_ACC, emulated worst err / bound at that constant)
RAISED = {}

# (n_real, n_fake): one score; one each; below a wave; uneven halves; the generator form; either side of the stride-256 loop with the second
# block of the backward launch; exactly one trip each; a second trip alone; four trips against part of a wave
CASES = [(1, 0), (1, 1), (4, 4), (3, 5), (16, 0), (255, 257), (256, 256), (300, 0), (1000, 24)]
# (t_real, t_fake): the reference's coding (critic: real 1, fake 0; generator, n_fake = 0: 1) and one other pair, so that both arguments act
TARGETS = [(1.0, 0.0), (0.75, -0.5)]
FAMILIES = ["standard", "large", "on_target"]


def c_acc(name):
    return float(RAISED.get(name, (C_ACC, None))[0])


def inputs(family, n_real, n_fake, t_real, t_fake):
    """{"scores": (n_real + n_fake,), "g": (3,)}.  standard: normal draws; large: scaled by 1e3; on_target: in each half the first quarter
    of the scores equal their target exactly (zero terms, zero gradients of the squared part) and the second quarter lie within four
    ulps of it, on either side"""
    n = n_real + n_fake
    d = draws(seed_of(41 + FAMILIES.index(family), n_real, n_fake), scores=(n,), g=(3,), u=(n,))
    s = d["scores"]
    if family == "large":
        s = (s * f32(1e3)).astype(f32)
    elif family == "on_target":
        s = s.copy()
        for lo, cnt, t in ((0, n_real, f32(t_real)), (n_real, n_fake, f32(t_fake))):
            q = (cnt + 3) // 4
            s[lo:lo + q] = t
            k = np.clip(np.rint(d["u"][lo + q:lo + min(2 * q, cnt)] * 2), -4, 4)           # whole ulps in [-4, 4]
            step = np.spacing(np.abs(t)) if t != 0 else f32(2.0 ** -149)
            s[lo + q:lo + min(2 * q, cnt)] = (f64(t) + k * f64(step)).astype(f32)
    return {"scores": s, "g": d["g"]}


def lsloss_head_emulate(scores, n_real, n_fake, t_real, t_fake):
    """lsloss_head_kernel: per-thread sums with stride 256 (the squares as fma chains), block_sum_256 each"""
    tr, tf = f32(t_real), f32(t_fake)
    real, fake = _lanes(scores[:n_real], 256), _lanes(scores[n_real:], 256)
    # (the zero padding of _lanes must add nothing to the squares either: mask it)
    mr, mf = _lanes(np.ones(n_real, f32), 256), _lanes(np.ones(n_fake, f32), 256)
    sr, qr, sf, qf = (np.zeros(256, f32) for _ in range(4))
    for t in range(real.shape[0]):
        d = ((real[t] - tr) * mr[t]).astype(f32)
        sr = sr + real[t]
        qr = _fma(d, d, qr)
    for t in range(fake.shape[0] if n_fake else 0):
        d = ((fake[t] - tf) * mf[t]).astype(f32)
        sf = sf + fake[t]
        qf = _fma(d, d, qf)
    sr, qr, sf, qf = (_block_sum_256(v) for v in (sr, qr, sf, qf))
    lr = qr / f32(n_real)
    loss = lr + qf / f32(n_fake) if n_fake else lr
    one = lambda v: np.array([v], f32)  # noqa: E731
    return {"loss": one(loss), "mean_real": one(sr / f32(n_real)), "mean_fake": one(sf / f32(n_fake) if n_fake else f32(0))}


def lsloss_head_ref(scores, n_real, n_fake, t_real, t_fake):
    s = scores.astype(f64)
    tr, tf = r32(t_real), r32(t_fake)
    real, fake = s[:n_real], s[n_real:]
    loss = ((real - tr) ** 2).mean() + (((fake - tf) ** 2).mean() if n_fake else 0.0)
    mr, mra = real.mean(), np.abs(real).mean()
    mf, mfa = (fake.mean(), np.abs(fake).mean()) if n_fake else (0.0, 0.0)
    one = lambda v: np.array([v])  # noqa: E731
    return {"loss": (one(loss), one(loss), 1), "mean_real": (one(mr), one(mra), 1), "mean_fake": (one(mf), one(mfa), 1)}


def lsloss_head_bwd_emulate(scores, n_real, n_fake, t_real, t_fake, gl, gr, gf):
    gl, gr, gf = (f32(0) if v is None else f32(v) for v in (gl, gr, gf))
    gl2 = f32(2) * gl
    real = _fma(gl2, scores[:n_real] - f32(t_real), gr) / f32(n_real)
    fake = _fma(gl2, scores[n_real:] - f32(t_fake), gf) / f32(max(n_fake, 1))
    return {"gs": np.concatenate([real, fake]).astype(f32)}


def lsloss_head_bwd_ref(scores, n_real, n_fake, t_real, t_fake, gl, gr, gf):
    gl, gr, gf = (0.0 if v is None else float(v) for v in (gl, gr, gf))
    s = scores.astype(f64)
    tr, tf = r32(t_real), r32(t_fake)
    real, fake = s[:n_real], s[n_real:]
    g = np.concatenate([(gl * 2 * (real - tr) + gr) / n_real, (gl * 2 * (fake - tf) + gf) / max(n_fake, 1)])
    a = np.concatenate([(abs(gl) * 2 * (np.abs(real) + abs(tr)) + abs(gr)) / n_real,
                        (abs(gl) * 2 * (np.abs(fake) + abs(tf)) + abs(gf)) / max(n_fake, 1)])
    return {"gs": (g, a, 2)}


def null_patterns(g):
    """(g_loss, g_real, g_fake): all three present, then each null in turn"""
    return ((g[0], g[1], g[2]), (None, g[1], g[2]), (g[0], None, g[2]), (g[0], g[1], None))
