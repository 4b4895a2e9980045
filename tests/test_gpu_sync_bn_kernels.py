"""The four launches of the synchronised BatchNorm (csrc/stride2.hip: ngan_bn_moments -> ngan_bn_merge_fold forward,
ngan_bn_act_bwd_partial -> ngan_bn_act_bwd_merged backward) per element against fp64, through the C ABI, on the cases of
tests/sync_bn_cases.py: a tensor's pixel range cut into the 1 - 4 unequal contiguous parts the ranks hold, one record per part, the
records stacked as all_gather stacks them, every rank's merge.  Per element
    |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref,   C_ACC = 8
with absref and n_round of tests/sync_bn_cases.py, settled on the CPU by tests/test_sync_bn_bounds_cpu.py (every emulated ratio
<= 0.5, no constant raised) and never against a kernel.  The fp64 records are held to the same form against their own part's fp64
moments and sums.  Counts (a record's count, n_total, num_batches_tracked) are exact.  Every output and workspace lies between two
guards of 64 sentinel elements that must come back intact; outputs start as NaN and none may be left.  The backward starts from
statistics fixed by the test (the whole tensor's fp64 ones rounded to fp32), so it does not inherit the forward's error; it runs with
act 0 and act 1.

What it covers that tests/test_gpu_wgan_sync_bn.py's max-norm half does not: every part's first pixel six sigma from its channel's
mean (each rank pivots on its own first pixel), mean / sigma of 1000, a constant channel, one-pixel shares (M2 exactly 0), shares
below the lane count, C = 1 / 3 / 17 / 129 / 256 / 300 / 1024 (every thread layout of the two reductions, a second block of
sum_parts_f64, the two-pass loop above 256 channels), 1 / < 16 / > 16 chunks with ragged last ones, red_chunk's 1024-workgroup cap.

The forward cases forced one kernel change.  ngan_bn_moments summed d = y - y[0, c] and d^2 in fp32 per chunk (chan_reduce_stage1<0>)
and only added the chunks in fp64; M2 = s1 - s0 s0 / n cancels by 1 + 2 (s0 / n)^2 / var.  Measured on MI355X on the parent commit's
library: 11 of the 13 forward cases over the bound, the record's M2 23.6 and mean 3.63 times the bound, merged rstd 10.79 and scale
8.95 (C3-p614+1434: rstd off by 54 x 2^-23), shift 5.36 (C8-p1229+2867), running_var 15.5 and mean 1.54 (C3-p10931+40+1) -- rstd per
case where the stage1 = "fp32" emulation puts it, to three digits.  ngan_bn_moments now takes the single-GPU path's fp64 stage 1
(bn_stats_stage1<false>), and sum_parts_f64 reads double partials.

measured on MI355X after the fix (a record, not a bound: worst err / bound per output over the cases): moments count / mean / M2
0.000; merge mean 0.098 rstd 0.097 scale 0.140 shift 0.250 running_mean 0.097 running_var 0.096, n_total and num_batches_tracked exact;
bn_act_apply 0.166; bwd_partial S0 0.175 S1 0.439; bwd_merged gy 0.227 dgamma 0.439 dbeta 0.175, the shares added up dgamma 0.067
dbeta 0.048.  Every figure is the emulation's to three digits but shift's (emulated 0.323: the kernel's beta - mean * scale is
compiled as one fma).  The module takes about 6 s."""
import numpy as np
import pytest
import torch

import sync_bn_cases as S
import wgan_cases as W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SLOPE = S.SLOPE
GUARD = 64
SENTINEL = 12345.0
NBT0 = 0


def dv(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


class Guarded:
    """device buffers between two guards of GUARD sentinel elements, NaN inside"""

    def __init__(self):
        self.bufs = []

    def alloc(self, n, dtype=torch.float32):
        raw = torch.full((int(n) + 2 * GUARD,), SENTINEL, device=DEV, dtype=dtype)
        body = raw[GUARD:GUARD + int(n)]
        body.fill_(float("nan"))
        self.bufs.append((raw, int(n)))
        return body

    def verify(self):
        for raw, n in self.bufs:
            assert bool((raw[:GUARD] == SENTINEL).all()) and bool((raw[GUARD + n:] == SENTINEL).all()), ("guard overwritten", n)
        self.bufs = []


@pytest.fixture
def guarded():
    g = Guarded()
    yield g
    g.verify()


class Checker:
    """collects err / bound of every output of one case and asserts at the end, so that one run shows every figure"""

    def __init__(self, cid):
        self.cid, self.bad, self.worst = cid, [], {}

    def __call__(self, name, got, ref):
        r, a, n = ref
        g = np.asarray(got)
        assert not np.isnan(g).any(), (name, self.cid, "an element was never written")
        worst, idx = W.ratio_at(g, r, a, n, S.c_acc(name, self.cid))
        self.worst[name] = max(self.worst.get(name, 0.0), worst)
        if not worst <= 1.0:
            self.bad.append((name, round(worst, 3), tuple(int(i) for i in np.unravel_index(idx, r.shape))))

    def done(self, tag=""):
        for name, w in sorted(self.worst.items()):
            print(f"STAT sync_bn {name} {self.cid}{tag}: {w:.3f}")
        assert not self.bad, (self.cid, self.bad)


class Kernels:
    """sync_bn_cases' `impl` over the C entry points"""

    def __init__(self, ngan, guarded, case):
        self.call, self.lib, self.g = ngan._C.call, ngan._C.lib(), guarded
        self.C, self.parts = case
        self.per_rank = []          # every rank's merge outputs, as device tensors

    def work(self, npix):
        return self.g.alloc(self.lib.ngan_chan_reduce_workspace_floats(npix, self.C))

    def moments(self, yp):
        rec = self.g.alloc(1 + 2 * self.C, torch.float64)
        self.call("ngan_bn_moments", dv(yp), yp.shape[0], self.C, rec, self.work(yp.shape[0]))
        return host(rec)

    def merge(self, recs, d, o, rank=0):
        """every rank merges the same gathered records into buffers of its own; returns rank 0's"""
        C, world = self.C, recs.shape[0]
        recs_d, gamma, beta = dv(recs.reshape(-1)), dv(d["gamma"]), dv(d["beta"])
        for _ in range(world):
            out = {k: self.g.alloc(C) for k in ("mean", "rstd", "scale", "shift")}
            out["n_total"] = self.g.alloc(1, torch.float64)
            rm, rv, nbt = (dv(d["run_mean"]), dv(d["run_var"]), torch.full((1,), NBT0, device=DEV, dtype=torch.int64)) if o["track"] else (None, None, None)
            self.call("ngan_bn_merge_fold", recs_d, world, C, gamma, beta, out["mean"], out["rstd"], out["scale"], out["shift"], rm, rv, nbt,
                      float(o["momentum"]), float(o["eps"]), out["n_total"])
            if o["track"]:
                out.update(running_mean=rm, running_var=rv, num_batches_tracked=nbt)
            self.per_rank.append(out)
        got = {k: host(v) for k, v in self.per_rank[0].items()}
        got.setdefault("num_batches_tracked", np.array([float(NBT0)]))
        return got

    def apply(self, y, scale, shift, act):
        a = self.g.alloc(y.size)
        self.call("ngan_bn_act_apply", dv(y), self.per_rank[0]["scale"], self.per_rank[0]["shift"], act, SLOPE, y.shape[0], self.C, a)
        return host(a).reshape(y.shape)

    def bwd_partial(self, yp, gp, st, act, eps):
        rec = self.g.alloc(2 * self.C, torch.float64)
        self.call("ngan_bn_act_bwd_partial", dv(yp), dv(gp), dv(st["scale"]), dv(st["shift"]), dv(st["mean"]), dv(st["rstd"]), act, SLOPE,
                  yp.shape[0], self.C, rec, self.work(yp.shape[0]))
        return host(rec)

    def bwd_merged(self, yp, gp, st, gamma, act, recs, rank, n_total):
        C = self.C
        gy, dg, db = self.g.alloc(yp.size), self.g.alloc(C), self.g.alloc(C)
        self.call("ngan_bn_act_bwd_merged", dv(yp), dv(gp), dv(st["scale"]), dv(st["shift"]), dv(st["mean"]), dv(st["rstd"]), dv(gamma), act,
                  SLOPE, yp.shape[0], C, dv(recs.reshape(-1)), recs.shape[0], rank, torch.tensor([n_total], device=DEV, dtype=torch.float64),
                  gy, dg, db, self.g.alloc(3 * C))
        return {"gy": host(gy).reshape(yp.shape), "dgamma": host(dg), "dbeta": host(db)}


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_moments_merge_and_stored_activation(ngan, guarded, case):
    """every part's moments record against that part's own fp64 moments; the merge of the stacked records against the whole tensor's
    fp64 statistics, with ngan_bn_act_apply on its scale and shift; every rank's merge of the same records bit for bit the same"""
    C, parts = case
    for n in parts:
        assert ngan._C.lib().ngan_chan_reduce_workspace_floats(n, C) == 6 * S.red_chunk(n, C)[1] * C
    impl = Kernels(ngan, guarded, case)
    ck = Checker(S.case_id(case))
    for name, got, ref in S.forward_chain(case, impl, act=S.CASES.index(case) % 2):
        ck(name, got, ref)
    assert len(impl.per_rank) == len(parts)
    for other in impl.per_rank[1:]:
        assert other.keys() == impl.per_rank[0].keys()
        for k, v in impl.per_rank[0].items():
            assert torch.equal(v, other[k]), (k, "the ranks' merges differ")
    assert float(impl.per_rank[0]["n_total"]) == sum(parts)
    if S.options(case)["track"]:
        assert int(impl.per_rank[0]["num_batches_tracked"]) == NBT0 + 1
    guarded.verify()
    ck.done()


@pytest.mark.parametrize("case,act", [(c, a) for c in S.CASES for a in (0, 1)], ids=lambda v: S.case_id(v) if isinstance(v, tuple) else f"act{v}")
def test_backward_records_input_gradient_and_shares(ngan, guarded, case, act):
    """every part's backward record against that part's fp64 sums; every rank's merged launch: its slice of gy against the whole
    tensor's fp64 gradient (and gy reassembled), its dgamma / dbeta share against its part's sums, the shares added up against the
    whole tensor's dgamma / dbeta"""
    impl = Kernels(ngan, guarded, case)
    ck = Checker(S.case_id(case))
    for name, got, ref in S.backward_chain(case, impl, act):
        ck(name, got, ref)
    guarded.verify()
    ck.done(f" act{act}")
