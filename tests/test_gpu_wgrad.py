"""The 3x3 weight-gradient kernels (csrc/conv3x3_wgrad.hip) through the C ABI, per element against fp64, at every one of the 84 template
instances of launch_wgrad and at the edges of their tiling -- ragged right columns and bottom rows, every XF tile position, clamped
bilinear taps, the 2x2 average on load at all three precisions (the fp32 instances of which no other caller reaches), every slice
shape with several slices on both sides, tile walks that carry in x, y and b, every tail of wgrad_reduce_kernel's part loop -- and the
slab reduction ngan_conv3x3_wgrad_reduce_many on synthetic slabs (every NG, its 8-way unroll and tail, 1 - 4 sources of unequal
nparts and scales, a call of 26 entries across the batch of 24, the output index map), the deferred path of ops.deferred_wgrad()
bit for bit against a direct reduction, and bit-reproducibility.  The case list, references, bound and emulations are in
tests/wgrad_cases.py; tests/test_wgrad_bounds_cpu.py pins which instances the list reaches.

Per element   |got - ref| <= n_round 2^-23 |ref| + C_ACC 2^-24 absref (+ 2^-15 absref for the split-bf16 form),   C_ACC = 8, n_round 1
written / 2 accumulated; absref is the direct sum's twin for the bf16 forms and the Winograd form's own twin for fp32.  The constants
were settled on the CPU against emulations (every emulated ratio <= 0.5), never against a kernel.

Workspace: it is allocated with a guard region of its own size behind ngan_conv3x3_wgrad_workspace_bytes, the guard holds one bit
pattern and the workspace a NaN with a payload.  After a slab-only call (accumulate 2) the guard is intact bit for bit and no
sentinel is left in the first nparts * nslices * 9 * co_s * ci_s floats: every slab element was written, none past the end.
Every gradient buffer of a writing call starts as NaN.

measured on MI355X (a record, not a bound: worst err / bound per form over all cases, emulated figure in brackets; 1 is the bound):
fp32 Winograd 0.169 (0.169), (1, 1, 16, 64, 64, 1) written; split-bf16 0.535 (0.535; its accumulation part alone 0.279), the 1 x 1 image,
where one product per element meets the split term; plain bf16 0.166 (0.160); reduce_many on synthetic slabs 0.372 (0.372).  The
deferred-path test found that two records for one gradient shared a launch and raced on it (fixed in ngan_conv3x3_wgrad_reduce_many:
such a record starts the next launch); no constant moved.  The module takes 5 s."""
import struct

import numpy as np
import pytest
import torch

import wgrad_cases as C
from test_gpu_ops import DEV

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN_BITS = 0x7FC0BEEF           # a quiet NaN with a payload: "never written"
GUARD_BITS = 0x5A5A5A5A


def dv(a, bf=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.to(BF) if bf else t


def host(t):
    return t.detach().float().cpu().numpy()


def guarded_workspace(ngan, case):
    """(buffer, n): n workspace floats holding the NaN sentinel, then a guard of max(n, 4096) floats"""
    n = ngan._C.wgrad_workspace_bytes(*case[:5]) // 4
    buf = torch.full((n + max(n, 4096),), GUARD_BITS, device=DEV, dtype=torch.int32)
    buf[:n] = NAN_BITS
    return buf.view(torch.float32), n


def guard_intact(ws, n):
    return bool((ws.view(torch.int32)[n:] == GUARD_BITS).all())


def launch(ngan, case, prec, x, g, gw, ws, accumulate):
    B, H, W, Cin, Cout, res = case
    if prec == 5:
        ngan._C.call("ngan_bf16_conv3x3_wgrad", x, g, gw, ws, B, H, W, Cin, Cout, res, C.SCALE, accumulate)
    else:
        ngan._C.call("ngan_conv3x3_wgrad", x, g, gw, ws, B, H, W, Cin, Cout, res, C.SCALE, accumulate, prec)


def reduce_many(ngan, records):
    """records: [(slab tensors, gw tensor, [(nparts, scale)], shape dict, accumulate)]"""
    raw = b"".join(C.pack_entry([s.data_ptr() for s in slabs], gw.data_ptr(), src, shape, acc) for slabs, gw, src, shape, acc in records)
    assert len(raw) == 104 * len(records) == struct.calcsize(C.ENTRY_FMT) * len(records)
    ngan._C.wgrad_reduce_many(raw, len(records))


def plan_shape(ngan, case, prec):
    nwx, nslices, n_ci, co_s, ci_s = ngan._C.wgrad_plan(*case[:5], prec)
    return nwx, dict(nslices=nslices, n_ci_slices=n_ci, co_s=co_s, ci_s=ci_s, K=case[3], Cout=case[4], M=nslices * 9 * co_s * ci_s)


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: "x".join(map(str, c)))
def test_wgrad_every_instance_against_fp64(ngan, case):
    """written, accumulated into a random gradient, and slab-only + deferred reduction, at precisions 0, 1 and 5"""
    B, H, W, Cin, Cout, res = case
    bad = []
    for prec in C.PRECISIONS:
        bf = prec == 5
        d = C.inputs(case, C.storage_of(prec))
        x, g = dv(d["x"], bf), dv(d["g"], bf)
        name = ngan._C.conv3x3_wgrad_kernel_name(*case, prec)
        assert name == C.kernel_name(case, prec)
        nwx, shape = plan_shape(ngan, case, prec)
        stats = []
        for accumulate in (0, 1):
            gw = dv(d["buf"]) if accumulate else torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV)
            ws, n = guarded_workspace(ngan, case)
            launch(ngan, case, prec, x, g, gw, ws, accumulate)
            assert guard_intact(ws, n), ("wrote past the workspace", case, prec, accumulate)
            got = host(gw)
            assert not np.isnan(got).any(), ("unwritten or NaN gradient element", case, prec, accumulate)
            stats.append(C.check(case, prec, got, accumulate))
        # slabs only: every element written, none past the end; then the deferred reduction of that one slab set
        ws, n = guarded_workspace(ngan, case)
        gw = torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV)
        launch(ngan, case, prec, x, g, gw, ws, 2)
        used = nwx * shape["M"]
        assert used <= n and guard_intact(ws, n), ("wrote past the workspace", case, prec, 2)
        assert not bool((ws.view(torch.int32)[:used] == NAN_BITS).any()), ("slab element never written", case, prec)
        assert bool(torch.isnan(gw).all()), ("a slab-only call touched the gradient", case, prec)
        reduce_many(ngan, [([ws], gw, [(nwx, C.SCALE)], shape, 0)])
        stats.append(C.check(case, prec, host(gw), 0))
        print(f"STAT wgrad {C.FORM[prec]} {name} {case}: written {stats[0]:.3f} accumulated {stats[1]:.3f} deferred {stats[2]:.3f}")
        bad += [(prec, k, s) for k, s in zip(("written", "accumulated", "deferred"), stats) if not s <= 1.0]
    assert not bad, (case, bad)


def _slab_sets(src, M):
    return [C.synthetic_slabs(n, M, s) for s, (n, _) in enumerate(src)]


def _check_reduced(tag, got, slabs, src, shape, buf):
    ref = C.reduce_many_ref(slabs, [sc for _, sc in src])
    if buf is not None:
        ref = C.plus(ref, buf)
    r, a, n = ref
    gw = lambda v: C.from_workspace(v, shape["Cout"], shape["K"], shape["co_s"], shape["ci_s"])
    worst = C.ratio(got, gw(r), gw(a), n)
    print(f"STAT wgrad_reduce_many {tag}: {worst:.3f}")
    return worst


@pytest.mark.parametrize("nparts", C.REDUCE_NPARTS)
def test_reduce_many_every_group_count_and_tail(ngan, nparts):
    """one source of `nparts` slabs per slice shape, 2 x 2 slices, written and accumulated: four entries in one call, twice"""
    for accumulate in (0, 1):
        records, expect = [], []
        for co_s, ci_s in C.REDUCE_SLICES:
            shape, src = C.reduce_shape(co_s, ci_s), [(nparts, 0.37)]
            slabs = _slab_sets(src, shape["M"])
            buf = C.synthetic_slabs(1, shape["M"], 99)[0] if accumulate else None
            start = C.from_workspace(buf, shape["Cout"], shape["K"], co_s, ci_s) if accumulate else np.full((shape["Cout"], shape["K"], 3, 3), np.nan, np.float32)
            gw = dv(start)
            records.append(([dv(s) for s in slabs], gw, src, shape, accumulate))
            expect.append((gw, slabs, src, shape, buf))
        reduce_many(ngan, records)
        for gw, slabs, src, shape, buf in expect:
            assert _check_reduced(f"nparts {nparts} {shape['co_s']}x{shape['ci_s']} acc {accumulate}", host(gw), slabs, src, shape, buf) <= 1.0


def test_reduce_many_sources_of_unequal_size_and_scale(ngan):
    for accumulate in (0, 1):
        for i, src in enumerate(C.REDUCE_MULTI):
            shape = C.reduce_shape(*C.REDUCE_SLICES[i % 4])
            slabs = _slab_sets(src, shape["M"])
            buf = C.synthetic_slabs(1, shape["M"], 99)[0] if accumulate else None
            gw = dv(C.from_workspace(buf, shape["Cout"], shape["K"], shape["co_s"], shape["ci_s"])) if accumulate else \
                torch.full((shape["Cout"], shape["K"], 3, 3), float("nan"), device=DEV)
            reduce_many(ngan, [([dv(s) for s in slabs], gw, src, shape, accumulate)])
            assert _check_reduced(f"sources {src} acc {accumulate}", host(gw), slabs, src, shape, buf) <= 1.0


def test_reduce_many_across_the_batch_of_24(ngan):
    """26 entries of mixed sizes in one call: two launches, first_block of every entry"""
    records, expect = [], []
    for shape, src, accumulate in C.many_entries():
        slabs = _slab_sets(src, shape["M"])
        buf = C.synthetic_slabs(1, shape["M"], 99)[0] if accumulate else None
        gw = dv(C.from_workspace(buf, shape["Cout"], shape["K"], shape["co_s"], shape["ci_s"])) if accumulate else \
            torch.full((shape["Cout"], shape["K"], 3, 3), float("nan"), device=DEV)
        records.append(([dv(s) for s in slabs], gw, src, shape, accumulate))
        expect.append((gw, slabs, src, shape, buf))
    reduce_many(ngan, records)
    worst = [_check_reduced(f"entry {i}", host(gw), slabs, src, shape, buf) for i, (gw, slabs, src, shape, buf) in enumerate(expect)]
    assert max(worst) <= 1.0, worst


def test_reduce_many_two_records_for_one_gradient(ngan):
    """six sources as two records (four, then two) that accumulate into ONE gradient in one call, between records for other
    gradients: the second record must see the first one's result (they may not share a launch), per element against fp64"""
    shape = C.reduce_shape(16, 16)
    src = C.REDUCE_MULTI[2] + C.REDUCE_MULTI[0]
    slabs = _slab_sets(src, shape["M"])
    buf = C.synthetic_slabs(1, shape["M"], 99)[0]
    gw = dv(C.from_workspace(buf, 32, 32, 16, 16))
    other = [torch.full((32, 32, 3, 3), float("nan"), device=DEV) for _ in range(2)]
    dslabs = [dv(s) for s in slabs]
    reduce_many(ngan, [(dslabs[:1], other[0], src[:1], shape, 0), (dslabs[:4], gw, src[:4], shape, 1),
                       (dslabs[1:2], other[1], src[1:2], shape, 0), (dslabs[4:], gw, src[4:], shape, 1)])
    assert _check_reduced("two records, one gradient", host(gw), slabs, src, shape, buf) <= 1.0
    for o, k in zip(other, (0, 1)):
        assert _check_reduced(f"neighbour record {k}", host(o), slabs[k:k + 1], src[k:k + 1], shape, None) <= 1.0


DEFERRED_CASE = (2, 12, 40, 32, 32, 0)
ROLES = (1, 0, 0, 1, 0, 0)


def test_deferred_path_equals_a_direct_reduction_bit_for_bit(ngan, conv_precision):
    """six contributions to one gradient inside ops.deferred_wgrad(): two records (four sources, then two, accumulating) in the canonical
    order -- by role, then by arrival -- equal to the same six slab sets reduced by a direct ngan_conv3x3_wgrad_reduce_many call"""
    ops = ngan.ops
    prec = ops.PRECISIONS[conv_precision]
    B, H, W, Cin, Cout, res = DEFERRED_CASE
    gen = torch.Generator().manual_seed(41)
    xs = [torch.randn(B, H, W, Cin, generator=gen).to(DEV) for _ in ROLES]
    gs = [torch.randn(B, H, W, Cout, generator=gen).to(DEV) for _ in ROLES]
    scales = [0.05 * (i + 1) * (-1) ** i for i in range(6)]
    start = torch.randn(Cout, Cin, 3, 3, generator=gen).to(DEV)
    gw = start.clone()
    with ops.deferred_wgrad():
        for x, g, sc, role in zip(xs, gs, scales, ROLES):
            ops._run_wgrad(x, g, res, sc, accumulate_into=gw, role=role)
        assert torch.equal(gw, start), "the deferred calls write slabs only"
    nwx, shape = plan_shape(ngan, DEFERRED_CASE, prec)
    slabs = []
    for x, g in zip(xs, gs):
        ws, n = guarded_workspace(ngan, DEFERRED_CASE)
        ngan._C.call("ngan_conv3x3_wgrad", x, g, gw, ws, B, H, W, Cin, Cout, res, 1.0, 2, prec)
        slabs.append(ws)
    order = sorted(range(6), key=lambda i: ROLES[i])
    assert order == [1, 2, 4, 5, 0, 3]
    want = start.clone()
    reduce_many(ngan, [([slabs[i] for i in part], want, [(nwx, scales[i]) for i in part], shape, 1) for part in (order[:4], order[4:])])
    assert torch.equal(gw, want)
    assert not torch.equal(gw, start)


@pytest.mark.parametrize("prec", C.PRECISIONS)
def test_multi_tile_result_is_bit_reproducible(ngan, prec):
    case = C.WALK[0]
    B, H, W, Cin, Cout, res = case
    d = C.inputs(case, C.storage_of(prec))
    x, g = dv(d["x"], prec == 5), dv(d["g"], prec == 5)
    runs = []
    for _ in range(2):
        gw = torch.full((Cout, Cin, 3, 3), float("nan"), device=DEV)
        ws, n = guarded_workspace(ngan, case)
        launch(ngan, case, prec, x, g, gw, ws, 0)
        runs.append(gw)
    assert torch.equal(runs[0], runs[1]) and not bool(torch.isnan(runs[0]).any())
