"""Cases, fp64 references, per-element bounds and an fp32 emulation for the fused optimiser steps of csrc/adam.hip (`adam_kernel`,
`rmsprop_kernel`, each plain, CLIP and EMA, and `adam_advance_kernel`; per-element formulas `adam_coef`, `adam_update`,
`rmsprop_update`, `ema_update` of csrc/ngan_common.h, shared with the stem epilogues of csrc/linear.hip).  No tests here, and nothing
of the package is imported: tests/test_optim_bounds_cpu.py settles the constants on the emulation, tests/test_gpu_optim.py runs the
kernels on the same cases.

References (fp64, torch's semantics: no weight decay, no amsgrad, no momentum, not centred), with u = 2^-24
    g' = g * grad_scale
    Adam      m' = m + (1 - b1)(g' - m);  v' = b2 v + (1 - b2) g'^2;  update = (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps);  p' = p - update
    RMSprop   v' = alpha v + (1 - alpha) g'^2;  update = lr g' / (sqrt(v') + eps);  p' = p - update
    clip      p' clamped to [-c, c];     EMA   e' = e + w (p'_stored - e), p'_stored the fp32 value the step stored
lr, b1, b2, alpha, eps, grad_scale, 1 - b1, 1 - b2, 1 - alpha and w are the fp32 values the kernel reads, as doubles; the bias
corrections bc = 1 - beta^t are formed from the DOUBLE betas, as torch forms them, and t is the count the kernel reads (the fp32 count
after `adam_advance_kernel`).  So the device's -expm1f(t * ln beta), and the fp32 rounding of ln beta, are under test.

Bounds, per element, derived from the kernel text (nothing is fitted to a kernel's result):
    m'   K_M u (|m| + (1 - b1) |g' - m|)      g' rounded once (|g'| <= |m| + |g' - m|), the difference once, the fma once: 3 roundings
    v'   K_V u v'                              g' enters squared (2), two products, the fma: 5 roundings of positive terms
    p'   K_P u |p'| + K_U u |update| + (lr / bc1) e_m / denom     (Adam; e_m the m' bound: the cancellation in g' - m carried through)
    p'   K_P u |p'| + K_U u |update|                               (RMSprop)
         the final subtraction rounds once (K_P).  The update collects, each rounding at most u:
           lr / bc1             5 u    bc1 within 4 u (x = t ln beta: ln beta rounded on the host and the product rounded on the device
                                       move bc by |x| e^x / (1 - e^x) <= 1 times u each; expm1f within one ulp, 2 u), the division
           1 / sqrt(bc2)        4 u    half of bc2's 4 u, the root, the reciprocal
           sqrtf(v')            3.5 u  half of v's 5 u, the root
           * 1 / sqrt(bc2), + eps, the quotient, * step size    4 u
         16.5 u in all if every rounding aligned
    e'   3 u (|e| + w |p' - e|)               tests/test_gpu_ema.py
The constants are the smallest (powers of two; small integers for K_M and the average's 3) at which the emulation below
stays at err / bound <= 0.5 over every case of this file; tests/test_optim_bounds_cpu.py pins the table:

    constant   value   emulated worst err / bound
    K_M        4       0.428     (0.571 at 3, the count of roundings: the next integer)
    K_V        8       0.421     (0.842 at 4)
    K_P        2       0.494     (0.987 at 1: the final rounding alone, on the rows with |p| ~ 0.3)
    K_U        8       0.357     (read on the rows with p = 0 and |p| ~ 1e-3 lr, where K_P u |p'| hides nothing; at 4 the p' row is 0.680)
    EMA        3       0.332     (the constant of tests/test_gpu_ema.py, kept)
The constant of the update follows the same rule as the others.  It is below the worst-case count above (16.5 u, every rounding aligned, which the emulation's
roundings are not): the p' bound is asserted as a whole, and K_P u |p'| and the carried e_m term stand in it next to K_U u |update|.

Emulation: numpy fp32 in the kernels' own order -- gv = g * gscale; fmaf(omb1, gv - m, m); fmaf(b2, v, omb2 * gv * gv);
sqrtf(vv) * inv_sqrt_bc2 + eps; p - step_size * (mv / den); bc = -expm1f(t * ln_beta) with t and ln_beta in fp32; clamp_sym;
ema_update as one fma (a product of two fp32 values is exact in fp64, so fp64 multiply-add rounded to fp32 is the fused operation up
to a double rounding); an infinite g' makes m' NaN once 1 - b1 >= 0.5, as torch's lerp_ does (its g - (g - m)(1 - w) branch is
inf - inf) and as `adam_update` does.  `wrong=` names a fault; each misses a bound, a count or a class on a case
named in the CPU test.

Offsets beyond 2^31 elements are not tested here: the optimiser steps walk the flat parameter buffers (a few hundred MB at the widest
preset: 2^26 elements), which do not come near a 32-bit boundary in any step, so they are outside the scope of the index-width audit.
The activation-sized entry points are inside it: tests/large_offset_cases.py holds the table of their index widths and limits, and
tests/test_gpu_large_offsets.py runs them on tensors beyond 2^31 bytes, 2^32 bytes and 2^31 elements."""
import zlib

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
SEG_ALIGN = 64          # FlatParams' alignment of a tensor inside the flat buffers (train.py)
CHUNK = 4096            # elements per work item (train.py ADAM_CHUNK, csrc/adam.hip CHUNK)
K = dict(m=4.0, v=8.0, p=2.0, u=8.0, e=3.0)
RECORDED = dict(m=0.428, v=0.421, p=0.494, u=0.357, e=0.332)       # the docstring's table
FORMS = ("plain", "clip", "ema")
STEP_COUNTS = (1, 2, 3, 10, 1000, 6931, 100000, 2 ** 24)              # 6931: t ln 0.999 ~ -ln 1000; 2^24: the fp32 count stops advancing
# (0.5, 0.999): the reference's betas and the package configuration's default; (0.8, 0.999): the command line's default beta1 (make_trainer
# passes config.beta1 with beta2 = 0.999 to both trainers, the WGAN one included); (0.0, 0.99): beta1 = 0, ln 0 = -inf, bc1 = 1 at every t
BETAS = ((0.5, 0.999), (0.8, 0.999), (0.0, 0.99))


def f32d(x):
    """the fp32 value of a host double, as a double (what `w32` of test_gpu_ema.py does)"""
    return float(F32(x))


def hyper_adam(lr, betas, eps=1e-8, grad_scale=1.0):
    """the nine floats of include/ngan.h, formed from doubles as FusedAdam forms them"""
    b1, b2 = float(betas[0]), float(betas[1])
    ln = [np.log(b) if b > 0 else -np.inf for b in (b1, b2)]
    return np.array([lr, b1, b2, eps, grad_scale, 1.0 - b1, 1.0 - b2, ln[0], ln[1]], dtype=F32)


def hyper_rmsprop(lr, alpha=0.99, eps=1e-8, grad_scale=1.0):
    return np.array([lr, alpha, eps, grad_scale, 1.0 - alpha], dtype=F32)


def layout(lengths):
    offs, total = [], 0
    for n in lengths:
        offs.append(total)
        total += (n + SEG_ALIGN - 1) // SEG_ALIGN * SEG_ALIGN
    return offs, total


def work_list(lengths):
    cseg, coff = [], []
    for i, n in enumerate(lengths):
        for o in range(0, n, CHUNK):
            cseg.append(i)
            coff.append(o)
    return np.array(cseg, dtype=np.int32), np.array(coff, dtype=np.int64)


def sentinels(total):
    """what every alignment gap and inactive tensor holds before a launch, in p, g, m, v, e"""
    j = np.arange(total)
    return dict(p=(7.25 + j % 13).astype(F32), g=np.full(total, 1000.0, dtype=F32), m=(-3.5 - j % 7).astype(F32),
                v=(11.0 + j % 5).astype(F32), e=(-9.75 + j % 11).astype(F32))


class Case:
    """one launch: hyper-parameters, segment tables, and buffers p, g, m, v, e with sentinels outside the active tensors"""

    def __init__(self, name, rule, segs, lr=2e-3, betas=(0.5, 0.999), alpha=0.99, eps=1e-8, grad_scale=1.0, ema_beta=0.999,
                 clips=(0.01,), n0=0):
        self.name, self.rule, self.segs = name, rule, segs
        self.lr, self.betas, self.alpha, self.eps, self.grad_scale = float(lr), tuple(map(float, betas)), float(alpha), eps, grad_scale
        self.hyper = hyper_adam(lr, betas, eps, grad_scale) if rule == "adam" else hyper_rmsprop(lr, alpha, eps, grad_scale)
        self.ema_w = np.array([1.0 - ema_beta], dtype=F32)
        self.clips, self.n0 = clips, n0
        self.lengths = [s["len"] for s in segs]
        self.offsets, self.total = layout(self.lengths)
        self.seg_off = np.array(self.offsets, dtype=np.int64)
        self.seg_len = np.array(self.lengths, dtype=np.int64)
        self.seg_active = np.array([s["active"] for s in segs], dtype=np.int32)
        self.seg_step = np.array([s["step"] for s in segs], dtype=F32)
        self.chunk_seg, self.chunk_off = work_list(self.lengths)
        self.skipped = sorted(set(self.chunk_seg[:n0].tolist()))       # tensors whose chunks the launch leaves out (the fused stem)
        assert not set(self.skipped) & set(self.chunk_seg[n0:].tolist())
        self.buf = sentinels(self.total)
        self.seg_of = np.full(self.total, -1)
        self.exact = np.zeros(self.total, dtype=bool)                   # elements whose p must come out bit-unchanged (g = m = v = 0)
        rng = np.random.default_rng(zlib.crc32(f"{name}/{rule}".encode()))
        for i, (s, o, n) in enumerate(zip(segs, self.offsets, self.lengths)):
            if s["active"]:
                self.seg_of[o:o + n] = i
                self._fill(rng, s, slice(o, o + n), n)
        self.updated = (self.seg_of >= 0) & ~np.isin(self.seg_of, self.skipped)
        self.finite = np.isfinite(self.buf["g"])

    def _fill(self, rng, s, sl, n):
        gs = s.get("gscale", 1.0)
        g = rng.standard_normal(n)
        g = np.where(np.abs(g) < 1e-3, 1e-3, g) * gs
        first = s["step"] == 0
        m = np.zeros(n) if first else 0.5 * gs * rng.standard_normal(n)
        v = np.zeros(n) if first else gs * gs * rng.uniform(0.2, 2.0, n)
        kind = s.get("p", "normal")
        if kind == "normal":
            p = 0.3 * rng.standard_normal(n)
        elif kind == "zero":
            p = np.zeros(n)
        elif kind == "tiny":
            p = 1e-3 * self.lr * rng.standard_normal(n)
        else:                                           # "clip": on, next to and far from +-c, c the first clip of the case
            c = self.clips[0]
            near = rng.choice([0.0, 0.3, 1.0, 3.0, 30.0], n) * self.lr * rng.choice([-1.0, 1.0], n)
            p = np.where(rng.uniform(size=n) < 0.8, rng.choice([-c, c], n) + near, 0.3 * rng.standard_normal(n))
        g, m, v, p = (a.astype(F32) for a in (g, m, v, p))
        zero = s.get("zero")
        if zero == "all":                               # g = m = v = 0: update exactly 0, p bit-unchanged
            g[:], m[:], v[:] = 0, 0, 0
            g[1::2] = -0.0
            self.exact[sl] = True
        elif zero == "grad":                            # g = +-0 with state
            g[:] = 0
            g[1::2] = -0.0
        else:                                           # every intermediate stays a normal fp32 number
            omb2 = float(self.hyper[6] if self.rule == "adam" else self.hyper[4])
            gg = omb2 * (g.astype(F64) * f32d(self.grad_scale)) ** 2
            assert gg.min() >= TINY and (first or v.min() >= TINY), (self.name, gg.min())
        for idx, val in s.get("nonfinite", ()):
            g[idx] = val
        for key, a in (("p", p), ("g", g), ("m", m), ("v", v)):
            self.buf[key][sl] = a
        self.buf["e"][sl] = (p.astype(F64) + 0.01 * rng.standard_normal(n)).astype(F32)

    # ---- altered copies: the cached cases are never modified; `updated` follows from seg_of and skipped in one place ----------------
    def copy(self):
        """a case of its own arrays for the segment state (the buffers are shared: pass others as `buf=`)"""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.seg_active, c.seg_step, c.seg_of = self.seg_active.copy(), self.seg_step.copy(), self.seg_of.copy()
        return c

    def set_active(self, i, flag):
        self.seg_active[i] = 1 if flag else 0
        self.seg_of[self.offsets[i]:self.offsets[i] + self.lengths[i]] = i if flag else -1
        self.updated = (self.seg_of >= 0) & ~np.isin(self.seg_of, self.skipped)

    def set_counts(self, seg_step):
        self.seg_step = np.array(seg_step, dtype=F32)

    def set_hyper(self, lr=None, grad_scale=None, ema_beta=None):
        self.lr = self.lr if lr is None else float(lr)
        self.grad_scale = self.grad_scale if grad_scale is None else grad_scale
        self.hyper = (hyper_adam(self.lr, self.betas, self.eps, self.grad_scale) if self.rule == "adam"
                      else hyper_rmsprop(self.lr, self.alpha, self.eps, self.grad_scale))
        if ema_beta is not None:
            self.ema_w = np.array([1.0 - ema_beta], dtype=F32)

    def counts_after(self):
        """the fp32 counts `adam_advance_kernel` leaves: + 1.0f for active tensors (2^24 + 1 rounds back to 2^24)"""
        return np.where(self.seg_active != 0, self.seg_step + F32(1.0), self.seg_step).astype(F32)

    def values(self, exact_doubles=False):
        """hyper-parameters of the reference: the fp32 values the kernel reads as doubles, the double betas for the bias corrections;
        exact_doubles: everything from the host's doubles (torch in fp64, for the comparison with torch.optim)"""
        if self.rule == "adam":
            b1, b2 = self.betas
            if exact_doubles:
                return dict(lr=self.lr, b1=b1, b2=b2, eps=self.eps, gs=self.grad_scale, omb1=1.0 - b1, omb2=1.0 - b2, B1=b1, B2=b2)
            h = self.hyper.astype(F64)
            return dict(lr=h[0], b1=h[1], b2=h[2], eps=h[3], gs=h[4], omb1=h[5], omb2=h[6], B1=b1, B2=b2)
        if exact_doubles:
            return dict(lr=self.lr, alpha=self.alpha, eps=self.eps, gs=self.grad_scale, oma=1.0 - self.alpha)
        h = self.hyper.astype(F64)
        return dict(lr=h[0], alpha=h[1], eps=h[2], gs=h[3], oma=h[4])

    def t_elem(self):
        t = np.ones(self.total)
        t[self.seg_of >= 0] = self.counts_after().astype(F64)[self.seg_of[self.seg_of >= 0]]
        return t


def clamp64(p, c):
    return np.minimum(np.maximum(p, -c), c)          # (NaN passes through both)


def reference(case, clip=None, k=K, values=None, buf=None):
    """{output: (fp64 reference, bound)} over the whole buffer (meaningful on case.updated); "upd" is the update with a zero bound"""
    h = values or case.values()
    b = {key: a.astype(F64) for key, a in (buf or case.buf).items()}
    with np.errstate(all="ignore"):
        g1 = b["g"] * h["gs"]
        if case.rule == "adam":
            t = case.t_elem()
            bc1, bc2 = 1.0 - h["B1"] ** t, 1.0 - h["B2"] ** t
            m1 = b["m"] + h["omb1"] * (g1 - b["m"])
            v1 = h["b2"] * b["v"] + h["omb2"] * g1 * g1
            den = np.sqrt(v1) / np.sqrt(bc2) + h["eps"]
            upd = (h["lr"] / bc1) * m1 / den
            e_m = k["m"] * U * (np.abs(b["m"]) + h["omb1"] * np.abs(g1 - b["m"]))
            carried = (h["lr"] / bc1) * e_m / den
        else:
            v1 = h["alpha"] * b["v"] + h["oma"] * g1 * g1
            upd = h["lr"] * g1 / (np.sqrt(v1) + h["eps"])
            carried = 0.0
        p1 = b["p"] - upd
        out = {"v": (v1, k["v"] * U * v1), "upd": (upd, np.zeros_like(upd)),
               "p": (p1 if clip is None else clamp64(p1, clip), k["p"] * U * np.abs(p1) + k["u"] * U * np.abs(upd) + carried)}
        if case.rule == "adam":
            out["m"] = (m1, e_m)
    return out


def ema_reference(e, p_stored, w, k=K):
    e64, p64, w = e.astype(F64), p_stored.astype(F64), float(w)
    with np.errstate(all="ignore"):
        return e64 + w * (p64 - e64), k["e"] * U * (np.abs(e64) + w * np.abs(p64 - e64))


# ---- the fp32 emulation ---------------------------------------------------------------------------------------------------------------
def fmaf(a, b, c):
    with np.errstate(all="ignore"):
        return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def clamp_sym(p, c):
    c = F32(c)
    return np.where(p < -c, -c, np.where(p > c, c, p)).astype(F32)


def emulate(case, form="plain", clip=None, wrong=None, buf=None):
    """the launch pair in numpy fp32: {"p", "m", "v", "e", "step"} (m untouched by RMSprop, e unless form == "ema")"""
    b = {key: a.copy() for key, a in (buf or case.buf).items()}
    h = case.hyper
    one = F32(1.0)
    step = case.counts_after()
    upd = case.updated
    seg = np.where(case.seg_of >= 0, case.seg_of, 0)
    with np.errstate(all="ignore"):
        gs = one if wrong == "grad_scale_ignored" else h[4 if case.rule == "adam" else 3]
        gv = (b["g"] * gs).astype(F32)
        if case.rule == "adam":
            lr, b1, b2, eps, omb1, omb2, ln1, ln2 = h[0], h[1], h[2], h[3], h[5], h[6], h[7], h[8]
            t = step.copy()
            if wrong == "bc_t_minus_1":
                t = (t - one).astype(F32)
            if wrong == "shared_count":
                t[:] = t[np.flatnonzero(case.seg_active)[0]]
            if wrong == "powf":
                bc1, bc2 = (one - np.power(b1, t, dtype=F32)).astype(F32), (one - np.power(b2, t, dtype=F32)).astype(F32)
            else:
                bc1, bc2 = (-np.expm1((t * ln1).astype(F32))).astype(F32), (-np.expm1((t * ln2).astype(F32))).astype(F32)
            if wrong == "omb2_fp32":
                omb2 = one - b2
            step_size = (lr / bc1).astype(F32)[seg]
            isb2 = np.ones_like(bc2) if wrong == "no_bc2" else (one / np.sqrt(bc2)).astype(F32)
            isb2 = isb2[seg]
            mv = fmaf(omb1, (gv - b["m"]).astype(F32), b["m"])
            if wrong != "lerp_keeps_inf" and omb1 >= 0.5:          # torch's lerp_ at weight >= 0.5: g - (g - m)(1 - w), inf - inf
                mv = np.where(np.isinf(gv), F32(np.nan), mv)
            vv = fmaf(b2, b["v"], ((omb2 * gv).astype(F32) * gv).astype(F32))
            if wrong == "eps_before_scale":
                den = ((np.sqrt(vv) + eps).astype(F32) * isb2).astype(F32)
            else:
                den = ((np.sqrt(vv) * isb2).astype(F32) + eps).astype(F32)
            pv = (b["p"] - (step_size * (mv / den).astype(F32)).astype(F32)).astype(F32)
            b["m"] = np.where(upd, mv, b["m"])
        else:
            lr, alpha, eps, oma = h[0], h[1], h[2], h[4]
            vv = fmaf(alpha, b["v"], ((oma * gv).astype(F32) * gv).astype(F32))
            den = np.sqrt((vv + eps).astype(F32)) if wrong == "rms_eps_under_root" else (np.sqrt(vv) + eps).astype(F32)
            pv = (b["p"] - (lr * (gv / den).astype(F32)).astype(F32)).astype(F32)
        b["v"] = np.where(upd, vv, b["v"])
        if form == "clip":
            stored = np.fmin(np.fmax(pv, F32(-clip)), F32(clip)) if wrong == "clamp_flushes_nan" else clamp_sym(pv, clip)
        else:
            stored = pv
        b["p"] = np.where(upd, stored, b["p"])
        if form == "ema":
            # the launch passes clip = 0 to the EMA instantiation: a kernel that averaged the clamped value would average zeros
            read = clamp_sym(stored, 0.0) if wrong == "ema_reads_clipped" else stored
            b["e"] = np.where(upd, fmaf(case.ema_w[0], (read - b["e"]).astype(F32), b["e"]), b["e"])
    b["step"] = step
    del b["g"]
    return b


# ---- torch.optim on the CPU: the classes of non-finite elements (fp32) and the references' agreement (fp64) ---------------------------
def torch_step(case, dtype, buf=None, steps=None):
    """torch.optim.Adam / RMSprop (foreach=False) on the active, not skipped tensors with the case's state preset; g * grad_scale is the
    .grad.  Returns {"p", "m", "v"} over the whole buffer in `dtype` (untouched elsewhere)."""
    import torch
    buf = buf or case.buf
    out = {key: torch.from_numpy(buf[key].astype(F64)).to(dtype).clone() for key in ("p", "m", "v")}
    steps = case.seg_step if steps is None else steps
    for i, (o, n) in enumerate(zip(case.offsets, case.lengths)):
        if not case.seg_active[i] or i in case.skipped:
            continue
        sl = slice(o, o + n)
        p = torch.nn.Parameter(out["p"][sl].clone())
        p.grad = (torch.from_numpy(buf["g"][sl].astype(F64)) * (f32d(case.grad_scale) if dtype == torch.float32 else case.grad_scale)).to(dtype)
        if case.rule == "adam":
            opt = torch.optim.Adam([p], lr=case.lr, betas=case.betas, eps=case.eps, foreach=False)
            opt.state[p] = {"step": torch.tensor(float(steps[i])), "exp_avg": out["m"][sl].clone(), "exp_avg_sq": out["v"][sl].clone()}
        else:
            opt = torch.optim.RMSprop([p], lr=case.lr, alpha=case.alpha, eps=case.eps, foreach=False)
            opt.state[p] = {"step": torch.tensor(float(steps[i])), "square_avg": out["v"][sl].clone()}
        opt.step()
        out["p"][sl] = p.detach()
        if case.rule == "adam":
            out["m"][sl], out["v"][sl] = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
        else:
            out["v"][sl] = opt.state[p]["square_avg"]
    return {key: a.numpy() for key, a in out.items()}


def classes(a):
    """0 finite, 1 infinite, 2 NaN"""
    return np.where(np.isnan(a), 2, np.where(np.isinf(a), 1, 0))


# ---- the check both test modules apply ------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def ratio(got, ref, bound, mask):
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(F64) - ref)[mask]
        bd = bound[mask]
        r = np.where(bd > 0, err / np.where(bd > 0, bd, 1.0), np.where(err == 0, 0.0, np.inf))
        r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def check(case, form, clip, got, k=K, torch32=None, buf=None):
    """got: {"p", "m", "v", "e", "step"} after the launch (numpy fp32, whole buffers).  Returns ({output: worst err / bound}, [what is
    wrong besides the bounds]): the caller prints the ratios, then asserts ratios <= its limit and an empty list.  `u` is the p' ratio
    on the rows with p = 0 or |p| ~ 1e-3 lr alone.  torch32: `torch_step(case, torch.float32)`, for the classes at non-finite g."""
    before = buf or case.buf
    ref = reference(case, clip if form == "clip" else None, k, buf=buf)
    mask = case.updated & np.isfinite(before["g"])
    worst, wrong = {}, []
    outs = ("m", "v", "p") if case.rule == "adam" else ("v", "p")
    for key in outs:
        worst[key] = ratio(got[key], *ref[key], mask)
    small = mask & np.isin(case.seg_of, [i for i, s in enumerate(case.segs) if s.get("p") in ("zero", "tiny")])
    if small.any():
        worst["u"] = ratio(got["p"], *ref["p"], small)
    if form == "ema":
        worst["e"] = ratio(got["e"], *ema_reference(before["e"], got["p"], case.ema_w[0], k), mask)
    # everything outside the updated tensors keeps its bits: alignment gaps, inactive tensors, tensors whose chunks were left out
    for key in ("p", "m", "v", "e"):
        same = bits(got[key]) == bits(before[key])
        if not same[~case.updated].all():
            wrong.append(f"{key}: {int((~same[~case.updated]).sum())} elements outside the updated tensors changed")
        if key == "e" and form != "ema" and not same.all():
            wrong.append("e changed without an EMA form")
        if key == "m" and case.rule != "adam" and not same.all():
            wrong.append("m changed under RMSprop")
    if not (bits(got["step"]) == bits(case.counts_after())).all():
        wrong.append(f"counts {got['step'].tolist()} != {case.counts_after().tolist()}")
    unmoved = before["p"] if form != "clip" else clamp_sym(before["p"], clip)
    if not (bits(got["p"]) == bits(unmoved))[case.exact & case.updated].all():
        wrong.append("g = m = v = 0 moved p")
    if form == "clip":
        inside = np.abs(got["p"][mask]) <= F32(clip)
        if not inside.all():
            wrong.append(f"|p'| > c at {int((~inside).sum())} elements")
    odd = case.updated & ~np.isfinite(before["g"])
    if odd.any():
        assert torch32 is not None
        for key in outs:
            want = classes(torch32[key])[odd]
            if key == "p" and form == "clip":
                want = classes(clamp64(torch32["p"].astype(F64), clip))[odd]
            if not (classes(got[key])[odd] == want).all():
                wrong.append(f"{key}: classes {classes(got[key])[odd].tolist()} at non-finite g, torch gives {want.tolist()}")
    return worst, wrong


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def seg(n, step=0, active=1, **kw):
    return dict(len=n, step=float(step), active=active, **kw)


def step_count_case(rule, betas):
    """one launch, tensors at different counts: per count a tensor with |p| ~ 0.3, one with p = 0 and one with |p| ~ 1e-3 lr; every
    fourth tensor inactive.  The count preset to 2^24 stays there (the true step 2^24 + 1 has the same corrections, 1 to fp64)."""
    segs = []
    for t in STEP_COUNTS + (2 ** 24 + 1,):
        for kind, n in (("normal", 97), ("zero", 65), ("tiny", 33)):
            segs.append(seg(n, t - 1, p=kind))
            if len(segs) % 4 == 3:
                segs.append(seg(70, 5, active=0))
    return Case(f"counts_b{betas[0]}_{betas[1]}", rule, segs, betas=betas, alpha=betas[1])


def scale_cases(rule):
    out = []
    for lr in (2e-3, 1e-5):
        for gscale in (1.0, 0.5, 1.0 / 3.0):
            segs = []
            for s in (1e-6, 1e-2, 1.0, 100.0):
                segs += [seg(129, 0, gscale=s), seg(61, 9, gscale=s), seg(40, 9, gscale=s, p="tiny")]
            out.append(Case(f"scales_lr{lr:g}_gs{gscale:.3f}", rule, segs, lr=lr, grad_scale=gscale))
    return out


GEOMETRY = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 12289)      # the 256-thread stride and the 4096-element chunk from both sides


def geometry_case(rule):
    segs = []
    for i, n in enumerate(GEOMETRY):
        segs.append(seg(n, i % 4))
        if i % 2 == 0:
            segs.append(seg((65, 4097, 1, 256, 300, 64)[i // 2], 7, active=0))       # 6 of 17 inactive
    return Case("geometry", rule, segs)


def many_segments_case(rule):
    """300 tensors: a second block of adam_advance_kernel"""
    return Case("many_segments", rule, [seg(1 + i % 3, i % 7, active=1 - i % 2) for i in range(300)])


def skipped_stem_case(rule):
    """the work list from chunk n0 on: tensor 0 (two chunks) is the fused stem's, its count advances and nothing else of it moves"""
    return Case("skipped_stem", rule, [seg(4097, 3), seg(300, 3), seg(64, 0, active=0), seg(4096, 0), seg(5, 11)], n0=2)


def zero_case(rule):
    return Case("zeros", rule, [seg(66, 0, zero="all"), seg(66, 4, zero="all"), seg(67, 4, zero="grad"),
                                seg(67, 4, zero="grad", p="zero"), seg(20, 4)])


def clip_case(rule):
    return Case("clip", rule, [seg(700, 0, p="clip"), seg(700, 50, p="clip"), seg(64, 2, active=0), seg(257, 6931, p="clip")],
                clips=(0.01, 0.0))


def nonfinite_case(rule, betas=(0.5, 0.999)):
    """a NaN, a +inf and a -inf gradient; Adam on either side of torch's lerp_ branch at weight 1 - beta1 = 0.5"""
    bad = ((3, np.nan), (64, np.inf), (129, -np.inf))
    name = "nonfinite" if betas[0] == 0.5 else f"nonfinite_b{betas[0]}"
    return Case(name, rule, [seg(130, 0, nonfinite=bad), seg(130, 12, nonfinite=bad), seg(50, 12)], betas=betas)


_cache = {}


def cases(rule):
    """every case of one rule, built once and never modified"""
    if rule not in _cache:
        out = [step_count_case(rule, b) for b in (BETAS if rule == "adam" else ((0.0, 0.99),))]
        out += scale_cases(rule)
        out += [geometry_case(rule), many_segments_case(rule), skipped_stem_case(rule), zero_case(rule), clip_case(rule),
                nonfinite_case(rule)]
        if rule == "adam":
            out.append(nonfinite_case(rule, (0.8, 0.999)))
        _cache[rule] = {c.name: c for c in out}
    return _cache[rule]


def launches():
    """(rule, case name, form, clip) of every launch both test modules check"""
    out = []
    for rule in ("adam", "rmsprop"):
        for name, c in cases(rule).items():
            for form in FORMS:
                for clip in (c.clips if form == "clip" else (None,)):
                    out.append((rule, name, form, clip))
    return out
