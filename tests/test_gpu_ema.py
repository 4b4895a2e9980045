"""The averaged generator (ema_beta) on the GPU: the kernels against fp64, the folded forms against the plain steps and against the
standalone ngan_ema_step, the trainers (both optimisers, fused and stored stem, bf16 mode), graph replay, growth, the weight swap of
averaged_generator(), two ranks on one GPU, checkpoints and the eval tool.

Update rule (include/ngan.h):  e' = fmaf(w, p' - e, e),  w = fp32(1 - beta).
Kernel bound, per element, against the fp64 evaluation e + w (p' - e) on the same fp32 inputs (p' the fp32 value the kernel stored):
    |e' - ref| <= 3 * 2^-24 * (|e| + w |p' - e|)
derived, not fitted: the difference d = p' - e is rounded once (<= 2^-24 |d|, scaled by w), the fused multiply-add once
(<= 2^-24 |e'| <= 2^-24 (|e| + w |d|) (1 + 2^-24)); together below 2.1 * 2^-24 (|e| + w |d|).
Trajectory bound over T steps: every step contracts earlier errors by beta and adds at most one kernel bound, so the sum is below
(1 / (1 - beta)) * 3 * 2^-24 * max_t(|e_t| + w |p_t - e_t|)."""
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import load_golden

import test_gpu_models as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def w32(beta):
    """the weight the kernels read: fp32(1 - beta) rounded from the double, as a double"""
    return float(np.float32(1.0 - beta))


def ema_ref(e, p, w):
    """fp64 update and its bound on fp32 tensors e (before), p (the stored new parameter)"""
    e64, p64 = e.double(), p.double()
    return e64 + w * (p64 - e64), 3 * U * (e64.abs() + w * (p64 - e64).abs())


def assert_step(e_old, p_new, e_new, w, what=""):
    ref, bound = ema_ref(e_old, p_new, w)
    err = (e_new.double() - ref).abs()
    worst = float((err - bound).max())
    print(f"{what}: max |e' - ref| {float(err.max()):.3e}, max bound {float(bound.max()):.3e}")
    assert worst <= 0.0, (what, worst)


# ---- 1-3: the flat kernels ------------------------------------------------------------------------------------------------------
LENGTHS = (5000, 37, 4096, 12289, 1)          # odd lengths, one exact chunk, one above a 4096-element chunk, one single element
ACTIVE = (1, 0, 1, 1, 1)


def flat_case(ngan, kind):
    torch.manual_seed(23)
    net = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, device=DEV) * 0.3) for n in LENGTHS])
    cls = ngan.train.FusedRMSprop if kind == "rmsprop" else ngan.train.FusedAdam
    flat = ngan.train.FlatParams(net, cls.STATE)
    opt = cls(flat, 2e-3)
    flat.set_active([p for p, a in zip(flat.params, ACTIVE) if a])
    return flat, opt


def segments(flat):
    return [(o, p.numel(), a) for o, p, a in zip(flat.offsets, flat.params, ACTIVE)]


@pytest.mark.parametrize("beta", [0.999, 0.9])
def test_ema_step_kernel(ngan, beta):
    flat, _ = flat_case(ngan, "adam")
    w = torch.tensor([1.0 - beta], dtype=torch.float32, device=DEV)
    e0 = torch.randn_like(flat.flat) * 0.3
    e = e0.clone()
    ngan._C.call("ngan_ema_step", flat.flat, e, flat.seg_off, flat.seg_len, flat.seg_active, flat.chunk_seg, flat.chunk_off,
                 int(flat.chunk_seg.numel()), w)
    torch.cuda.synchronize()
    touched = torch.zeros_like(e, dtype=torch.bool)
    for o, n, a in segments(flat):
        if a:
            assert_step(e0[o:o + n], flat.flat[o:o + n], e[o:o + n], w32(beta), f"ngan_ema_step seg@{o}")
            touched[o:o + n] = True
    assert torch.equal(e[~touched], e0[~touched])              # inactive tensors and the alignment gaps are untouched
    assert not torch.equal(e[touched], e0[touched])


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_flat_steps_with_average(ngan, kind):
    """two steps: (2) p, m, v, step counts bit-equal to the plain entry point, inactive averages untouched; (1) the average within the
    kernel bound of fp64; (3) plain step + ngan_ema_step gives the same bits"""
    C = ngan._C
    beta = 0.99
    fa, oa = flat_case(ngan, kind)            # plain
    fb, ob = flat_case(ngan, kind)            # folded
    assert torch.equal(fa.flat, fb.flat)
    w = torch.tensor([1.0 - beta], dtype=torch.float32, device=DEV)
    e_fold = torch.randn_like(fa.flat) * 0.3
    e_sep = e_fold.clone()
    state = (lambda f: (f.exp_avg, f.exp_avg_sq)) if kind == "adam" else (lambda f: (f.square_avg,))
    name = f"ngan_{kind}_step"
    for it in range(2):
        g = torch.randn_like(fa.flat)
        fa.grad.copy_(g)
        fb.grad.copy_(g)
        e_before = e_fold.clone()
        tail = lambda f, o: (f.seg_off, f.seg_len, f.seg_active, f.seg_step, len(f.params), f.chunk_seg, f.chunk_off,
                             int(f.chunk_seg.numel()), o.hyper, o.hyper.numel())
        C.call(name, fa.flat, fa.grad, *state(fa), *tail(fa, oa))
        C.call(name + "_ema", fb.flat, fb.grad, *state(fb), *tail(fb, ob), e_fold, w)
        C.call("ngan_ema_step", fa.flat, e_sep, fa.seg_off, fa.seg_len, fa.seg_active, fa.chunk_seg, fa.chunk_off,
               int(fa.chunk_seg.numel()), w)
        torch.cuda.synchronize()
        assert torch.equal(fa.flat, fb.flat) and torch.equal(fa.seg_step, fb.seg_step), it
        for a, b in zip(state(fa), state(fb)):
            assert torch.equal(a, b), it
        assert torch.equal(e_fold, e_sep), it                                       # (3)
        for o, n, a in segments(fb):
            if a:
                assert_step(e_before[o:o + n], fb.flat[o:o + n], e_fold[o:o + n], w32(beta), f"{name}_ema it{it} seg@{o}")
            else:
                assert torch.equal(e_fold[o:o + n], e_before[o:o + n])
    assert fb.seg_step.cpu().tolist() == [2.0 * a for a in ACTIVE]


# ---- 1-3: the four stem forms, both MFMA instantiations ---------------------------------------------------------------------------
@pytest.mark.parametrize("act", ["f32", "bf16"])
@pytest.mark.parametrize("rule", ["adam", "rmsprop"])
@pytest.mark.parametrize("B,K,S2,C", [(6, 32, 9, 20), (5, 512, 4, 24), (5, 144, 9, 20)])      # K <= 128 and K > 128: NT = 8 and NT = 32; rows % 64 != 0; 144: nt = 9 < NT = 32
def test_stem_epilogues_with_average(ngan, rule, act, B, K, S2, C):
    Cc = ngan._C
    torch.manual_seed(31)
    beta = 0.999
    rows = C * S2
    n = rows * K
    p0 = (torch.randn(rows, K) * 0.1).to(DEV)
    pa, pb = p0.clone(), p0.clone()
    ma, mb, va, vb = (torch.zeros_like(p0) for _ in range(4))
    e_fold = (p0 + torch.randn_like(p0) * 0.01).contiguous()
    e_sep = e_fold.clone()
    w = torch.tensor([1.0 - beta], dtype=torch.float32, device=DEV)
    if rule == "adam":
        hyper = torch.tensor([1e-3, 0.5, 0.999, 1e-8, 1.0, 0.5, 1.0 - 0.999, np.log(0.5), np.log(0.999)], dtype=torch.float32, device=DEV)
    else:
        hyper = torch.tensor([1e-3, 0.99, 1e-8, 1.0, 1.0 - 0.99], dtype=torch.float32, device=DEV)
    step = torch.zeros(1, dtype=torch.float32, device=DEV)
    chunks = list(range(0, n, 4096))
    seg = dict(off=torch.zeros(1, dtype=torch.int64, device=DEV), len=torch.tensor([n], dtype=torch.int64, device=DEV),
               act=torch.ones(1, dtype=torch.int32, device=DEV), cseg=torch.zeros(len(chunks), dtype=torch.int32, device=DEV),
               coff=torch.tensor(chunks, dtype=torch.int64, device=DEV))
    for it in range(2):
        z = torch.randn(B, K).to(DEV)
        gc = torch.randn(B, S2, C).to(DEV)
        if act == "bf16":
            gc = gc.bfloat16()
        step += 1.0                                # the stem launches read the already advanced count
        e_before = e_fold.clone()
        if rule == "adam":
            Cc.call(ngan.ops._k("ngan_linear_wgrad_adam", gc), z, gc, pa, ma, va, step, hyper, hyper.numel(), B, K, S2, C, 0.0613)
            Cc.call(ngan.ops._k("ngan_linear_wgrad_adam_ema", gc), z, gc, pb, mb, vb, step, hyper, hyper.numel(), B, K, S2, C, 0.0613,
                    e_fold, w)
        else:
            Cc.call(ngan.ops._k("ngan_linear_wgrad_rmsprop", gc), z, gc, pa, va, hyper, hyper.numel(), B, K, S2, C, 0.0613)
            Cc.call(ngan.ops._k("ngan_linear_wgrad_rmsprop_ema", gc), z, gc, pb, vb, hyper, hyper.numel(), B, K, S2, C, 0.0613,
                    e_fold, w)
        Cc.call("ngan_ema_step", pa, e_sep, seg["off"], seg["len"], seg["act"], seg["cseg"], seg["coff"], len(chunks), w)
        torch.cuda.synchronize()
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb), it      # (2)
        assert not torch.equal(pb, p0)
        assert torch.equal(e_fold, e_sep), it                                               # (3)
        assert_step(e_before, pb, e_fold, w32(beta), f"stem {rule} {act} K={K} it{it}")      # (1)


# ---- 4: the trainer -----------------------------------------------------------------------------------------------------------
def draws_for(fix, n, seed=5):
    res, _, _, latent, batch, _ = fix["meta"]
    res, latent, batch = int(res), int(latent), int(batch)
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        z = [torch.randn(batch, latent, generator=gen) for _ in range(3)]
        z = [(v / v.norm(dim=1, keepdim=True)).to(DEV) for v in z]
        out.append(dict(real=(torch.rand(batch, 1, res, res, generator=gen) * 2 - 1).to(DEV), z_d=z[0], z_gp=z[1],
                        eps=torch.rand(batch, 1, 1, 1, generator=gen).to(DEV), z_g=z[2]))
    return out


def run(tr, s):
    return tr.train_iteration(s["real"], s["z_d"], s["z_gp"], s["eps"], s["z_g"])


def assert_trajectory(e0, weights, e_final, beta, what=""):
    """the fp64 recurrence over the recorded fp32 weights, and the trajectory bound of the module docstring"""
    w = w32(beta)
    e = e0.double()
    worst = torch.zeros_like(e)
    for p in weights:
        d = p.double() - e
        worst = torch.maximum(worst, e.abs() + w * d.abs())
        e = e + w * d
    bound = (1.0 / (1.0 - beta)) * 3 * U * worst
    err = (e_final.double() - e).abs()
    print(f"{what}: max |ema - fp64 recurrence| {float(err.max()):.3e}, max bound {float(bound.max()):.3e}")
    assert float((err - bound).max()) <= 0.0, (what, float(err.max()))


def trainer_case(ngan, fixture, optimizer, fused_stem, beta=0.9, steps=12):
    fix = load_golden(fixture)
    seq = draws_for(fix, steps)
    G0, D0 = T.build_small(ngan, fix)
    off = ngan.train.PGGANTrainer(G0, D0, learning_rate=1e-3, optimizer=optimizer, fused_stem=fused_stem)
    G1, D1 = T.build_small(ngan, fix)
    on = ngan.train.PGGANTrainer(G1, D1, learning_rate=1e-3, optimizer=optimizer, fused_stem=fused_stem, ema_beta=beta)
    assert on.fused_stem == fused_stem and off.fused_stem == fused_stem and off.flat_g.ema is None
    e0 = on.flat_g.ema.clone()
    assert torch.equal(e0, on.flat_g.flat)
    weights = []
    for s in seq:
        run(off, s)
        run(on, s)
        assert torch.equal(on.flat_g.flat, off.flat_g.flat)                       # averaging moves nothing else
        weights.append(on.flat_g.flat.clone())
    torch.cuda.synchronize()
    assert torch.equal(on.flat_d.flat, off.flat_d.flat) and torch.equal(on.flat_g.seg_step, off.flat_g.seg_step)
    assert not torch.equal(weights[-1], e0)
    assert_trajectory(e0, weights, on.flat_g.ema, beta, f"{fixture} {optimizer} fused_stem={fused_stem}")
    # inactive tensors: average == parameter, bit for bit
    for p, o, a in zip(on.flat_g.params, on.flat_g.offsets, on.flat_g.active_host):
        if not a:
            assert torch.equal(on.flat_g.ema[o:o + p.numel()], on.flat_g.flat[o:o + p.numel()])


@pytest.mark.parametrize("fused_stem", [True, False])
@pytest.mark.parametrize("optimizer", ["adam", "rmsprop"])
@pytest.mark.parametrize("fixture", ["small_res16_fade_warm", "small_res8_warm"])
def test_trainer_average_follows_the_recurrence(ngan, fixture, optimizer, fused_stem):
    trainer_case(ngan, fixture, optimizer, fused_stem)


def test_trainer_average_in_the_bf16_mode(ngan):
    """the master weights are fp32 in the bf16 mode, so is the average: the same bound"""
    try:
        ngan.ops.set_conv_precision("bf16")
        trainer_case(ngan, "small_res16_fade_warm", "adam", True)
    finally:
        ngan.ops.set_conv_precision("f32")


def test_separate_form_gives_the_same_bits(ngan):
    """ema_fold = False (plain launches + ngan_ema_step, the form the fold is measured against) through the trainer"""
    fix = load_golden("small_res16_fade_warm")
    seq = draws_for(fix, 3)
    out = []
    for fold in (True, False):
        G, D = T.build_small(ngan, fix)
        tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3, ema_beta=0.9)
        tr.opt_g.ema_fold = fold
        for s in seq:
            run(tr, s)
        torch.cuda.synchronize()
        out.append((tr.flat_g.flat.clone(), tr.flat_g.ema.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert not torch.equal(out[0][0], out[0][1])


# ---- 5: graphs ------------------------------------------------------------------------------------------------------------------
def captured_pair(ngan, fixture="small_res16_fade_warm", n=4, beta=0.9, **kw):
    fix = load_golden(fixture)
    seq = draws_for(fix, n)
    mk = lambda: ngan.train.PGGANTrainer(*T.build_small(ngan, fix), learning_rate=1e-3, ema_beta=beta, **kw)
    return fix, seq, mk


def replay(tr, static, s):
    for k, v in static.items():
        v.copy_(s[k])
    tr.replay(s["real"])


def test_graph_replay_equals_eager_and_decay_is_live(ngan):
    fix, seq, mk = captured_pair(ngan)
    eager, tr = mk(), mk()
    static = {k: seq[0][k].clone() for k in ("z_d", "z_gp", "eps", "z_g")}
    tr.capture(seq[0]["real"], draws=static)
    assert torch.equal(tr.flat_g.ema, tr.flat_g.flat) and float(tr.flat_g.seg_step.sum()) == 0.0      # capturing is not training
    for s in seq[:3]:
        run(eager, s)
        replay(tr, static, s)
    torch.cuda.synchronize()
    assert torch.equal(tr.flat_g.flat, eager.flat_g.flat) and torch.equal(tr.flat_g.ema, eager.flat_g.ema)
    assert not torch.equal(tr.flat_g.ema, tr.flat_g.flat)
    # another decay between replays: no re-capture, the next replay averages with it
    e_before = tr.flat_g.ema.clone()
    graphs = tr._graph
    tr.set_ema_beta(0.5)
    eager.set_ema_beta(0.5)
    run(eager, seq[3])
    replay(tr, static, seq[3])
    torch.cuda.synchronize()
    assert tr._graph is graphs
    assert torch.equal(tr.flat_g.ema, eager.flat_g.ema)
    assert_step(e_before, tr.flat_g.flat, tr.flat_g.ema, 0.5, "replay after set_ema_beta(0.5)")
    ref_old, bound_old = ema_ref(e_before, tr.flat_g.flat, w32(0.9))
    assert float(((tr.flat_g.ema.double() - ref_old).abs() - bound_old).max()) > 0.0                  # not the captured decay


# ---- 6: growth ------------------------------------------------------------------------------------------------------------------
def test_average_across_growth(ngan):
    torch.manual_seed(5)
    G = ngan.models.Generator_PG([32, 16, 16], image_size_init=4, latent_dim=32).to(DEV)
    D = ngan.models.Discriminator_PG([16, 16, 32], image_size_init=4).to(DEV)
    beta = 0.9
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3, alpha_step=0.5, ema_beta=beta)
    f = tr.flat_g
    gen = torch.Generator().manual_seed(9)

    def iterate():
        real = (torch.rand(4, 1, G.image_size, G.image_size, generator=gen) * 2 - 1).to(DEV)
        e_old = f.ema.clone()
        tr.train_iteration(real)
        torch.cuda.synchronize()
        for n, p, o, a in zip(f.names, f.params, f.offsets, f.active_host):
            sl = slice(o, o + p.numel())
            if a:          # the recurrence for every tensor the step trains ...
                assert_step(e_old[sl], f.flat[sl], f.ema[sl], w32(beta), f"res {G.image_size} alpha {G.alpha_value():.1f} {n}")
            else:          # ... and an untouched average for the others (not yet grown, or a ToIm retired by a completed fade)
                assert torch.equal(f.ema[sl], e_old[sl]), n
        return e_old

    def keys_ok():
        assert list(tr.ema_state().keys()) == [n for n, _ in G.named_parameters()] == list(G.state_dict().keys())

    def slices(active):
        return [(n, slice(o, o + p.numel())) for n, p, o, a in zip(f.names, f.params, f.offsets, f.active_host) if bool(a) == active]

    keys_ok()
    for _ in range(2):
        iterate()
    late = [n for n, _ in slices(False)]
    assert any(n.startswith("conv_block_list.0") for n in late) and any(n.startswith("conv_block_list.1") for n in late)
    for n, sl in slices(False):
        assert torch.equal(f.ema[sl], f.flat[sl]), n                           # never updated: average == parameter
    assert all(not torch.equal(f.ema[sl], f.flat[sl]) for n, sl in slices(True) if n.endswith("weight"))
    before = f.ema.clone()
    assert tr.start_epoch(3, transit_sch=[3, 20])                               # growth: res 8, alpha 0
    assert G.image_size == 8 and torch.equal(f.ema, before)                     # refresh_stage leaves the average alone
    keys_ok()
    joined = [(n, sl) for n, sl in slices(True) if n in late]
    assert joined
    for n, sl in joined:
        assert torch.equal(f.ema[sl], f.flat[sl]), n                           # until its first update
    e_old = iterate()                                                           # alpha = 0: the new block's gradient is exactly zero
    for n, sl in joined:
        assert torch.equal(e_old[sl], before[sl]), n
    for n, sl in slices(False):
        assert torch.equal(f.ema[sl], f.flat[sl]), n
    assert not tr.start_epoch(4, transit_sch=[3, 20])                           # alpha 0.5
    keys_ok()
    iterate()                                                                   # the block moves, its average follows the recurrence
    assert all(not torch.equal(f.ema[sl], f.flat[sl]) for n, sl in joined if n.endswith("weight"))
    assert tr.start_epoch(5, transit_sch=[3, 20])                               # alpha 1.0: the fade completes, the block is merged
    assert G.alpha_value() >= 1
    keys_ok()
    iterate()
    for n, sl in slices(False):
        if n.startswith("conv_block_list"):                                     # the block that has not joined yet
            assert torch.equal(f.ema[sl], f.flat[sl]), n


# ---- 7: the swap ------------------------------------------------------------------------------------------------------------------
def test_averaged_generator_swaps_and_restores(ngan):
    fix, seq, mk = captured_pair(ngan)
    tr, twin = mk(), mk()
    statics = []
    for t in (tr, twin):
        st = {k: seq[0][k].clone() for k in ("z_d", "z_gp", "eps", "z_g")}
        t.capture(seq[0]["real"], draws=st)
        statics.append(st)
        for s in seq[:2]:
            replay(t, st, s)
    torch.cuda.synchronize()
    assert torch.equal(tr.flat_g.flat, twin.flat_g.flat) and not torch.equal(tr.flat_g.ema, tr.flat_g.flat)
    z = seq[3]["z_g"]
    before, e_before = tr.flat_g.flat.clone(), tr.flat_g.ema.clone()
    state = tr.ema_state()
    fresh, _ = T.build_small(ngan, fix)
    fresh.load_state_dict(state)
    with torch.no_grad():
        want = fresh(z)
        live = tr.G(z).clone()
        allocated = torch.cuda.memory_allocated()
        with tr.averaged_generator() as g:
            assert g is tr.G
            assert torch.cuda.memory_allocated() - allocated <= (4 << 20) + (1 << 20)      # a 4 MB scratch, no copy of the net
            got = tr.G(z).clone()
            assert torch.equal(tr.flat_g.flat, e_before)
        back = tr.G(z).clone()
    torch.cuda.synchronize()
    assert torch.equal(got, want) and not torch.equal(got, live)
    assert torch.equal(back, live)                                               # packed weights refreshed on the way out too
    assert torch.equal(tr.flat_g.flat, before) and torch.equal(tr.flat_g.ema, e_before)
    for s in seq[2:]:                                                            # the graphs captured before are still valid
        replay(tr, statics[0], s)
        replay(twin, statics[1], s)
        torch.cuda.synchronize()
        assert torch.equal(tr.flat_g.flat, twin.flat_g.flat) and torch.equal(tr.flat_d.flat, twin.flat_d.flat)
        assert torch.equal(tr.flat_g.ema, twin.flat_g.ema)


# ---- 8: two ranks on one GPU ----------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _same_on_all_ranks(t, world):
    t = t.detach().reshape(-1).cpu().contiguous()
    out = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(out, t)
    return all(torch.equal(out[0], x) for x in out[1:])


def _rank_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(4)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from __graft_entry__ import load_package
        import test_gpu_wgan as TW
        ngan = load_package()
        fix = load_golden("small_res16_fade_warm")
        batch = int(fix["meta"][4])
        half = batch // world
        sl = slice(rank * half, (rank + 1) * half)
        seq = draws_for(fix, 3)
        beta = 0.9
        for fused in (True, False):             # gathered factors into the fused stem; the stored-gradient stem; the flat tail in both
            G, D = T.build_small(ngan, fix)
            tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3, fused_stem=fused, ema_beta=beta)
            assert tr.world == world and tr.fused_stem == fused
            e0, weights = tr.flat_g.ema.clone(), []
            for s in seq:
                tr.train_iteration(s["real"][sl], s["z_d"][sl], s["z_gp"][sl], s["eps"][sl], s["z_g"][sl])
                weights.append(tr.flat_g.flat.clone())
            torch.cuda.synchronize()
            assert not torch.equal(tr.flat_g.ema, e0)
            assert _same_on_all_ranks(tr.flat_g.flat, world), f"weights differ across ranks (fused_stem={fused})"
            assert _same_on_all_ranks(tr.flat_g.ema, world), f"averages differ across ranks (fused_stem={fused})"
            assert_trajectory(e0, weights, tr.flat_g.ema, beta, f"rank {rank} fused_stem={fused}")
        # the WGAN trainer, synchronised BatchNorm: an iteration pair
        Gw, Dw = TW.make_nets([32, 16, 8], [8, 16, 32], 16, 64)
        trw = ngan.train.WGANTrainer(Gw.to(DEV), Dw.to(DEV), learning_rate=1e-3, sync_batchnorm=True, ema_beta=beta)
        assert trw.flat_d.ema is None
        gen = torch.Generator().manual_seed(7)
        e0, weights = trw.flat_g.ema.clone(), []
        for _ in range(2):
            real = (torch.rand(8, 1, 64, 64, generator=gen) * 2 - 1).to(DEV)
            zd, zg = torch.randn(8, 16, generator=gen).to(DEV), torch.randn(8, 16, generator=gen).to(DEV)
            trw.train_iteration(real[rank * 4:rank * 4 + 4], zd[rank * 4:rank * 4 + 4], zg[rank * 4:rank * 4 + 4])
            weights.append(trw.flat_g.flat.clone())
        torch.cuda.synchronize()
        assert not torch.equal(trw.flat_g.ema, e0)
        assert _same_on_all_ranks(trw.flat_g.ema, world), "WGAN averages differ across ranks"
        assert_trajectory(e0, weights, trw.flat_g.ema, beta, f"rank {rank} WGAN")
        assert list(trw.ema_state().keys()) == [n for n, _ in trw.G.named_parameters()]
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_hold_the_same_average():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
    for p in procs:
        if p.is_alive():            # a rank that died leaves its peer waiting in a collective
            p.kill()
            p.join()
    results = sorted(q.get(timeout=5) for _ in range(2))
    assert results == [(0, "ok"), (1, "ok")], results
    assert all(p.exitcode == 0 for p in procs)


def test_wgan_trainer_average_one_gpu(ngan):
    """one rank, captured: the averaged WGAN generator follows the recurrence; its BatchNorm buffers stay the live ones"""
    import test_gpu_wgan as TW
    beta = 0.9
    G, D = TW.make_nets([32, 16, 8], [8, 16, 32], 16, 64)
    tr = ngan.train.WGANTrainer(G.to(DEV), D.to(DEV), learning_rate=1e-3, optimizer="rmsprop", ema_beta=beta)
    gen = torch.Generator().manual_seed(3)
    real = (torch.rand(4, 1, 64, 64, generator=gen) * 2 - 1).to(DEV)
    static = {"z_d": torch.randn(4, 16, generator=gen).to(DEV), "z_g": torch.randn(4, 16, generator=gen).to(DEV)}
    tr.capture(real, draws=static)
    e0, weights = tr.flat_g.ema.clone(), []
    assert torch.equal(e0, tr.flat_g.flat)
    for _ in range(3):
        static["z_d"].copy_(torch.randn(4, 16, generator=gen))
        static["z_g"].copy_(torch.randn(4, 16, generator=gen))
        tr.replay(real)
        weights.append(tr.flat_g.flat.clone())
    torch.cuda.synchronize()
    assert_trajectory(e0, weights, tr.flat_g.ema, beta, "WGAN one GPU, replayed")
    buffers = [b.clone() for b in tr.G.buffers()]
    before, average = tr.flat_g.flat.clone(), tr.flat_g.ema.clone()
    assert buffers and not torch.equal(before, average)
    with tr.averaged_generator():
        assert torch.equal(tr.flat_g.flat, average)
        assert all(torch.equal(a, b) for a, b in zip(buffers, tr.G.buffers()))
    assert torch.equal(tr.flat_g.flat, before) and torch.equal(tr.flat_g.ema, average)


# ---- 9: checkpoints, the epoch driver's second grid, the eval tool ------------------------------------------------------------------
def short_run(ngan, tmp_path, tag, ema_beta):
    models, train, utils = ngan.models, ngan.train, ngan.utils
    cfg = types.SimpleNamespace(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[3], N_epochs=4,
                                alpha_step=0.5, learning_rate=2e-3, checkpointing_period=2, ID=tag)
    torch.manual_seed(5)
    G = models.Generator_PG([32, 16], image_size_init=4, latent_dim=32).to(DEV)
    D = models.Discriminator_PG([16, 32], image_size_init=4).to(DEV)
    data = train.TensorImageDataset.synthetic(8, 8, device=DEV)
    tr = train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, alpha_step=cfg.alpha_step, device_latents=True, ema_beta=ema_beta)
    f = str(tmp_path / f"GenDisc_{tag}.pth")
    ck = utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=torch.device(DEV), trainer=tr,
                            extra_checkpoint_period=1e3)
    samples = tmp_path / f"samples_{tag}"
    samples.mkdir()
    train.pggan_train(tr, data, cfg, checkpoint=ck, epoch_final=cfg.N_epochs + 1, log=lambda *_: None, samples_dir=str(samples))
    return tr, f, samples, cfg


def png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_checkpoint_driver_grid_and_eval_tool(ngan, tmp_path, capsys):
    utils = ngan.utils
    tr, f, samples, cfg = short_run(ngan, tmp_path, "e001", 0.9)
    # the driver wrote both grids at every checkpoint (epochs 2 and 4, the second after a growth event), same latents
    for epoch in (2, 4):
        a, b = png(samples / f"Samples_e001_{epoch}.png"), png(samples / f"Samples_ema_e001_{epoch}.png")
        assert a.shape == b.shape and not np.array_equal(a, b), epoch
    saved = utils.load_checkpoint_dict(f)
    assert list(saved["Generator_ema_state"].keys()) == list(saved["Generator_state"].keys())
    want = tr.ema_state()
    assert all(torch.equal(v, want[k].cpu()) for k, v in saved["Generator_ema_state"].items())
    # resume restores the average (and the driver's second grid left the training weights alone: they are what was saved)
    G2 = ngan.models.Generator_PG([32, 16], image_size_init=4, latent_dim=32).to(DEV)
    D2 = ngan.models.Discriminator_PG([16, 32], image_size_init=4).to(DEV)
    tr2 = ngan.train.PGGANTrainer(G2, D2, learning_rate=cfg.learning_rate, device_latents=True, ema_beta=0.9)
    utils.Checkpointer(G2, D2, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=torch.device(DEV), trainer=tr2).load_state()
    assert G2.image_size == tr.G.image_size
    assert torch.equal(tr2.flat_g.flat, tr.flat_g.flat) and torch.equal(tr2.flat_g.ema, tr.flat_g.ema)
    # the eval tool
    out_w, out_e = str(tmp_path / "w.png"), str(tmp_path / "e.png")
    torch.manual_seed(123)                                     # (the tool draws its latents from the global generator, as the reference's)
    assert ngan.eval.main(["-n", "4", "-weights", f, "-output", out_w]) == 0
    torch.manual_seed(123)
    assert ngan.eval.main(["-n", "4", "-weights", f, "-output", out_e, "--ema"]) == 0
    a, b = png(out_w), png(out_e)
    side = 2 * (tr.G.image_size_max + 2) + 2                   # 2 x 2 images, padding 2
    assert a.shape == b.shape == (side, side) and not np.array_equal(a, b)
    # ... and what --ema loads is the averaged generator: the same images as the trainer's G inside averaged_generator()
    loaded = ngan.models.Generator_PG.from_state_dict(f, device=torch.device(DEV), verbose=False, use_ema=True).to(DEV)
    z = ngan.utils.sample_latent_vec((4, 32), device=DEV)
    with torch.no_grad(), tr.averaged_generator():
        assert torch.equal(loaded(z), tr.G(z))
    # a checkpoint of a run without averaging: --ema names the missing key; an averaging trainer resumes from its weights and says so
    _, f0, samples0, _ = short_run(ngan, tmp_path, "p001", 0.0)
    assert not list(samples0.glob("Samples_ema_*")) and len(list(samples0.glob("Samples_p001_*"))) == 2
    assert "Generator_ema_state" not in utils.load_checkpoint_dict(f0)
    with pytest.raises(KeyError, match="Generator_ema_state"):
        ngan.eval.main(["-n", "4", "-weights", f0, "-output", out_e, "--ema"])
    assert ngan.eval.main(["-n", "4", "-weights", f0, "-output", str(tmp_path / "p.png")]) == 0
    capsys.readouterr()
    utils.Checkpointer(G2, D2, cfg.learning_rate, f0, N_epochs=cfg.N_epochs, verbose=False, device=torch.device(DEV), trainer=tr2).load_state()
    out = capsys.readouterr().out
    assert "starts from the loaded weights" in out and len(out.strip().splitlines()) == 1
    assert all(torch.equal(v, G2.state_dict()[k]) for k, v in tr2.ema_state().items())
