"""The fused optimiser steps (csrc/adam.hip; per-element formulas of csrc/ngan_common.h, shared with the stem epilogues of
csrc/linear.hip) per element against fp64: m', v' (square_avg), p' and the average e' of `ngan_adam_step`, `ngan_rmsprop_step`, both
`_clip` and both `_ema` forms, through the C ABI (`_C.call`) on the buffers of tests/optim_cases.py -- step counts preset from 1 to
2^24, three pairs of betas, gradient scales 1e-6 to 100, grad_scale and lr from the device vector, parameters of 0 and 1e-3 lr (so
that the final rounding of p' hides nothing of the update), zero and non-finite gradients, tensor lengths around the 256-thread
stride and the 4096-element chunk, 300 tensors, a work list that starts after the stem's chunks, clipping at 0.01 and 0.

Every bound is  err <= bound  with the references, bounds and constants of tests/optim_cases.py, settled on the CPU
(tests/test_optim_bounds_cpu.py: the emulation stays at half of each) and never against a kernel.  Besides the bounds, per launch:
everything outside the updated tensors (alignment gaps, inactive tensors, tensors whose chunks were left out) keeps its bits in p, m,
v and the average; the counts are `count + 1.0f` for active tensors and bit-unchanged for the others; g = m = v = 0 leaves p
bit-unchanged; |p'| <= c exactly after a clip form, whose result has the bits of the plain entry point followed by clamp_; a NaN or
infinite gradient leaves the classes torch.optim leaves (fp32, CPU).

Then: 64 consecutive launches on carried state with a tensor that joins at launch 20; the FusedAdam / FusedRMSprop wrappers from a
loaded count of 999 (the hyper vector they build); the stem epilogues `ngan_linear_wgrad_adam` / `_rmsprop` at count 1000, bit-equal to
`ngan_linear_wgrad` + the flat step, which is held to the bounds; and a captured `ngan_adam_step_ema` launch pair replayed with other
lr, grad_scale, ema weight, active flags and gradients each time.

measured on MI355X (a record, not a bound: worst err / bound per output over all launches; 1 is the bound): see DESIGN.md, "The
optimiser steps per element"."""
import collections

import numpy as np
import pytest
import torch

import optim_cases as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAUNCHES = O.launches()


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def upload(case, buf=None):
    d = {k: dv(v) for k, v in (buf or case.buf).items()}
    d.update(seg_off=dv(case.seg_off), seg_len=dv(case.seg_len), seg_active=dv(case.seg_active), step=dv(case.seg_step),
             chunk_seg=dv(case.chunk_seg), chunk_off=dv(case.chunk_off), hyper=dv(case.hyper), ema_w=dv(case.ema_w))
    return d


def launch(call, rule, form, clip, d, n_seg, n0=0):
    """one entry point of include/ngan.h on the device buffers d; the work list starts at chunk n0"""
    state = (d["m"], d["v"]) if rule == "adam" else (d["v"],)
    args = (d["p"], d["g"], *state, d["seg_off"], d["seg_len"], d["seg_active"], d["step"], n_seg, d["chunk_seg"][n0:],
            d["chunk_off"][n0:], int(d["chunk_seg"].numel()) - n0, d["hyper"], int(d["hyper"].numel()))
    if form == "clip":
        call(f"ngan_{rule}_step_clip", *args, float(clip))
    elif form == "ema":
        call(f"ngan_{rule}_step_ema", *args, d["e"], d["ema_w"])
    else:
        call(f"ngan_{rule}_step", *args)


def download(d):
    torch.cuda.synchronize()
    return {k: d[k].cpu().numpy() for k in ("p", "m", "v", "e", "step")}


_t32 = {}


def torch32(case):
    """torch.optim in fp32 on the CPU, for the classes at non-finite gradients (computed once per case)"""
    if not np.isfinite(case.buf["g"]).all():
        key = (case.rule, case.name)
        if key not in _t32:
            _t32[key] = O.torch_step(case, torch.float32)
        return _t32[key]
    return None


def judge(tag, case, form, clip, got, buf=None, limit=1.0):
    """print every figure, then assert"""
    ratios, complaints = O.check(case, form, clip, got, torch32=None if buf else torch32(case), buf=buf)
    print(f"STAT optim {tag}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= limit}
    assert not bad and not complaints, (tag, bad, complaints)
    return ratios


@pytest.mark.parametrize("rule,name,form,clip", LAUNCHES)
def test_step_against_fp64(ngan, rule, name, form, clip):
    case = O.cases(rule)[name]
    d = upload(case)
    launch(ngan._C.call, rule, form, clip, d, len(case.segs), case.n0)
    got = download(d)
    judge(f"{rule} {form} {name} clip={clip}", case, form, clip, got)
    if name == "skipped_stem":                                   # the stem's count advances with the others, its data stays
        assert got["step"][0] == case.seg_step[0] + 1 and case.skipped == [0]
    if form == "clip":                                           # include/ngan.h: the bits of the unclipped step followed by clamp_
        d2 = upload(case)
        launch(ngan._C.call, rule, "plain", None, d2, len(case.segs), case.n0)
        torch.cuda.synchronize()
        upd = dv(case.updated)
        want = torch.where(upd, d2["p"].clamp(-clip, clip), d2["p"])
        assert torch.equal(torch.isnan(want), torch.isnan(d["p"]))
        if clip > 0:
            assert torch.equal(want.view(torch.int32), d["p"].view(torch.int32))
        else:                                                    # c = 0: clamp_ leaves the sign of the zero to the library; the value is 0
            assert torch.equal(want.nan_to_num(7.0), d["p"].nan_to_num(7.0))
        assert torch.equal(d2["v"].view(torch.int32), d["v"].view(torch.int32))
        assert torch.equal(d2["m"].view(torch.int32), d["m"].view(torch.int32))


def test_count_at_2_pow_24_stays_and_the_step_is_in_bound(ngan):
    """the fp32 count stops at 2^24 (2^24 + 1 rounds back); both corrections are 1 there.  Two launches: the second, from the state the
    first left (counts read back, three tensors already at 2^24), is held to the bounds like any other"""
    base = O.cases("adam")["counts_b0.5_0.999"]
    at = [i for i, s in enumerate(base.segs) if s["step"] == 2.0 ** 24]
    assert len(at) == 3 and all(base.seg_active[i] for i in at)
    d = upload(base)
    launch(ngan._C.call, "adam", "plain", None, d, len(base.segs))
    torch.cuda.synchronize()
    before = {key: d[key].cpu().numpy() for key in ("p", "g", "m", "v", "e")}
    case = base.copy()
    case.set_counts(d["step"].cpu().numpy())
    reached = [i for i, s in enumerate(base.segs) if s["step"] == 2.0 ** 24 - 1]
    assert len(reached) == 3 and all(case.seg_step[i] == 2.0 ** 24 for i in at + reached)
    launch(ngan._C.call, "adam", "plain", None, d, len(base.segs))
    got = download(d)
    judge("adam plain second launch, counts at 2^24", case, "plain", None, got, buf=before)
    assert all(got["step"][i] == 2.0 ** 24 for i in at + reached)
    assert all(got["step"][i] == base.seg_step[i] + 2 for i in range(len(base.segs)) if base.seg_active[i] and base.seg_step[i] < 1e6)


# ---- carried state -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,form", [("adam", "ema"), ("rmsprop", "plain"), ("adam", "clip")])
def test_64_launches_on_carried_state(ngan, rule, form):
    """each launch against the one-step fp64 reference from the state read back before it; tensor 2 joins at launch 20"""
    segs = [O.seg(70), O.seg(5), O.seg(300, active=0), O.seg(130), O.seg(64, active=0)]
    case = O.Case("carried", rule, segs)
    d = upload(case)
    rng = np.random.default_rng(11)
    worst = collections.defaultdict(float)
    for k in range(64):
        if k == 20:
            case.set_active(2, True)
            d["seg_active"].copy_(dv(case.seg_active))
        g = (rng.standard_normal(case.total) * 10.0 ** rng.integers(-3, 2)).astype(np.float32)
        d["g"].copy_(dv(g))
        torch.cuda.synchronize()
        before = {key: d[key].cpu().numpy() for key in ("p", "g", "m", "v", "e")}
        case.set_counts(d["step"].cpu().numpy())
        launch(ngan._C.call, rule, form, 0.01, d, len(segs))
        got = download(d)
        ratios, complaints = O.check(case, form, 0.01, got, buf=before)
        assert not complaints, (k, complaints)
        for key, v in ratios.items():
            worst[key] = v if not v <= worst[key] else worst[key]
        want = [k + 1.0, k + 1.0, max(0.0, k - 19.0), k + 1.0, 0.0]
        assert got["step"].tolist() == want, (k, got["step"].tolist())
    print(f"STAT optim {rule} {form} 64 launches: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), dict(worst)


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["adam", "rmsprop"])
def test_wrapper_from_a_loaded_count(ngan, rule):
    """FusedAdam / FusedRMSprop.step() with flat.seg_step preset to 999, as load_optimizer_state leaves it, after set_lr and
    set_grad_scale: the t = 1000 reference with the hyper vector of optim_cases (formed independently from the same doubles)"""
    lengths, active = (5000, 37, 4096, 1), (1, 0, 1, 1)
    segs = [O.seg(n, 999, a) for n, a in zip(lengths, active)]
    case = O.Case("wrapper", rule, segs, lr=3e-4, betas=(0.5, 0.999), alpha=0.99, grad_scale=0.5)
    net = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(n, device=DEV)) for n in lengths])
    train = ngan.train
    cls = train.FusedAdam if rule == "adam" else train.FusedRMSprop
    flat = train.FlatParams(net, cls.STATE)
    assert flat.offsets == case.offsets and flat.total == case.total
    opt = cls(flat, 2e-3, (0.5, 0.999)) if rule == "adam" else cls(flat, 2e-3, 0.99)
    opt.set_lr(3e-4)
    opt.set_grad_scale(0.5)
    flat.set_active([p for p, a in zip(flat.params, active) if a])
    names = dict(p="flat", g="grad", m="exp_avg", v="exp_avg_sq") if rule == "adam" else dict(p="flat", g="grad", v="square_avg")
    for key, attr in names.items():
        getattr(flat, attr).copy_(dv(case.buf[key]))
    flat.seg_step.fill_(999.0)
    opt.step()
    torch.cuda.synchronize()
    assert np.array_equal(opt.hyper.cpu().numpy().view(np.uint32), case.hyper.view(np.uint32)), (opt.hyper.tolist(), case.hyper.tolist())
    got = {key: getattr(flat, attr).cpu().numpy() for key, attr in names.items() if key != "g"}
    got.update(step=flat.seg_step.cpu().numpy(), e=case.buf["e"])
    if rule != "adam":
        got["m"] = case.buf["m"]
    judge(f"{rule} wrapper t=1000", case, "plain", None, got)


# ---- the stem epilogues ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["adam", "rmsprop"])
def test_stem_epilogue_at_a_late_count(ngan, rule):
    """ngan_linear_wgrad_adam / _rmsprop at count 1000 give the bits of ngan_linear_wgrad into a gradient buffer followed by the flat
    step on it (include/ngan.h); the flat step is then held to the fp64 bounds on that very gradient, which pins the epilogue"""
    call = ngan._C.call
    B, Kd, S2, C = 5, 144, 9, 20
    n = C * S2 * Kd
    case = O.Case("stem", rule, [O.seg(n, 999)], lr=1e-3)
    gen = torch.Generator().manual_seed(31)
    z, gc = torch.randn(B, Kd, generator=gen).to(DEV), torch.randn(B, S2, C, generator=gen).to(DEV)
    scale = 0.0613
    gw = torch.zeros(n, device=DEV)
    call("ngan_linear_wgrad", z, gc, gw, B, Kd, S2, C, scale)
    torch.cuda.synchronize()
    buf = dict(case.buf, g=gw.cpu().numpy())
    assert buf["g"].shape == (case.total,)
    a, b = upload(case, buf), upload(case, buf)
    launch(call, rule, "plain", None, a, 1)
    after = torch.full((1,), 1000.0, device=DEV)                  # the stem launch reads the already advanced count
    if rule == "adam":
        call("ngan_linear_wgrad_adam", z, gc, b["p"], b["m"], b["v"], after, b["hyper"], 9, B, Kd, S2, C, scale)
    else:
        call("ngan_linear_wgrad_rmsprop", z, gc, b["p"], b["v"], b["hyper"], 5, B, Kd, S2, C, scale)
    got = download(a)
    assert float(a["step"][0]) == 1000.0
    for key in ("p", "m", "v"):
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), key
    assert not torch.equal(a["p"], dv(buf["p"]))
    judge(f"{rule} stem epilogue == flat step, t=1000", case, "plain", None, got, buf=buf)


# ---- live values under a captured graph ------------------------------------------------------------------------------------------------
def test_replays_read_the_values_of_the_moment(ngan):
    """one captured ngan_adam_step_ema launch pair (a single chain), replayed four times; lr, grad_scale, the average's weight, one
    tensor's active flag and the gradients change between replays without a re-capture"""
    segs = [O.seg(300, 4), O.seg(4097, 0), O.seg(65, 9, active=0), O.seg(1, 2)]
    case = O.Case("replay", "adam", segs)
    d = upload(case)
    call = ngan._C.call
    warm = upload(case)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch(call, "adam", "ema", None, warm, len(segs))       # the module is loaded before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(call, "adam", "ema", None, d, len(segs))
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    moments = [dict(lr=2e-3, gs=1.0, beta=0.999, flip=None), dict(lr=1.7e-3, gs=0.5, beta=0.9, flip=2),
               dict(lr=1e-5, gs=1.0 / 3.0, beta=0.5, flip=1), dict(lr=4e-4, gs=0.25, beta=0.99, flip=1)]
    for k, mo in enumerate(moments):
        if mo["flip"] is not None:
            case.set_active(mo["flip"], not case.seg_active[mo["flip"]])
        case.set_hyper(lr=mo["lr"], grad_scale=mo["gs"], ema_beta=mo["beta"])
        g = rng.standard_normal(case.total).astype(np.float32)
        for key, a in (("g", g), ("hyper", case.hyper), ("ema_w", case.ema_w), ("seg_active", case.seg_active)):
            d[key].copy_(dv(a))
        torch.cuda.synchronize()
        before = {key: d[key].cpu().numpy() for key in ("p", "g", "m", "v", "e")}
        case.set_counts(d["step"].cpu().numpy())
        graph.replay()
        got = download(d)
        judge(f"adam ema replay {k} lr={mo['lr']:g} gs={mo['gs']:.3f} w={case.ema_w[0]:g}", case, "ema", None, got, buf=before)
        assert not np.array_equal(got["p"], before["p"])
    assert got["step"].tolist() == [8.0, 3.0, 12.0, 6.0]          # tensor 1 sat out replay 2, tensor 2 replay 0: the counts advance only where active
