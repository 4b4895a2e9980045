"""Adaptive discriminator augmentation on the GPU: the kernels of csrc/ada.hip and the live parameter mappings through the entry points
of include/ngada.h against the oracle and the emulation of tests/ada_cases.py, then the trainer (eager, captured and replayed), the
epoch driver with its checkpoint, and two ranks.  Every comparison is exact: integer counters, and fp32 values bit for bit.
On an MI355X the module takes 10 s, 4 of them the two spawned ranks."""
import ctypes
import types

import numpy as np
import pytest
import torch

import ada_cases as A
from test_gpu_specloss import (_free_port, batch_draws, driver_draws, same, small_nets, state_of, target16, DRIVER_CFG)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 64
SENTINEL = -7
POLICY = "color,translation,cutout"


class Guarded:
    """a device buffer of n elements with PAD sentinel elements on either side (16-byte alignment of the payload is kept)"""

    def __init__(self, n, dtype, fill=None):
        self.whole = torch.full((n + 2 * PAD,), SENTINEL, device=DEV, dtype=dtype)
        self.view = self.whole[PAD:PAD + n]
        if fill is not None:
            self.view.copy_(torch.as_tensor(fill, dtype=dtype))

    def intact(self):
        return bool((self.whole[:PAD] == SENTINEL).all()) and bool((self.whole[PAD + self.view.numel():] == SENTINEL).all())

    def untouched(self):
        return bool((self.whole == SENTINEL).all())


# ---- ngada_accumulate ---------------------------------------------------------------------------------------------------------------
CASES = A.score_cases()
START = [7, 1 << 40, (1 << 40) + 9, 3]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_accumulate_counts_exactly_and_adds(ngan, case):
    """the counters against the integer oracle, exactly; a second call adds to the first; `updates` and the guard bands stay"""
    _, real, fake, mode, thr = case
    pos, neg, n = A.oracle_counts(real, fake, mode, thr)
    r = Guarded(len(real), torch.float32, real)
    f = None if fake is None else Guarded(len(fake), torch.float32, fake)
    c = Guarded(4, torch.int64, START)
    for k in (1, 2):
        ngan.ops.ada_accumulate(r.view, None if f is None else f.view, c.view, mode, thr)
        torch.cuda.synchronize()
        assert c.view.tolist() == [START[0] + k * pos, START[1] + k * neg, START[2] + k * n, START[3]], (k, pos, neg, n)
    assert c.intact() and r.intact() and (f is None or f.intact())
    assert np.array_equal(A.bits(r.view.cpu().numpy()), A.bits(real))


def test_accumulate_and_update_refusals_launch_nothing(ngan):
    lib = ngan._C.lib()
    c, p, s = Guarded(4, torch.int64), Guarded(2, torch.float32), Guarded(8, torch.float32, np.ones(8, dtype=np.float32))
    cp, pp, sp = (ctypes.c_void_p(g.view.data_ptr()) for g in (c, p, s))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ngada_accumulate(sp, None, 8, 8, 1, 0.0, cp, stream) == -1
    assert lib.ngada_accumulate(sp, sp, 8, 8, 2, 0.0, cp, stream) == -1
    assert lib.ngada_accumulate(sp, sp, 0, 8, 1, 0.0, cp, stream) == -2
    assert lib.ngada_accumulate(sp, sp, 8, 65537, 1, 0.0, cp, stream) == -2
    assert lib.ngada_accumulate(None, sp, 8, 8, 0, 0.0, cp, stream) == -1
    assert lib.ngada_update(cp, None, 0.6, 64.0, 1.0, stream) == -1
    assert lib.ngada_update(cp, pp, 0.6, 0.0, 1.0, stream) == -1
    assert lib.ngada_update(cp, pp, 0.6, 64.0, 1.5, stream) == -1
    assert lib.ngada_update(cp, pp, 2.0, 64.0, 1.0, stream) == -1
    with pytest.raises(RuntimeError, match="mode 1 needs fake_scores"):        # the wrapper carries the library's message
        ngan.ops.ada_accumulate(s.view, None, torch.zeros(4, dtype=torch.int64, device=DEV), mode=1)
    torch.cuda.synchronize()
    assert c.untouched() and p.untouched() and s.intact()


# ---- ngada_update -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(A.update_cases())))
def test_update_matches_the_emulation_bit_for_bit(ngan, k):
    pos, neg, n, p0, last_r, target, span, p_max = case = A.update_cases()[k]
    c = Guarded(4, torch.int64, [pos, neg, n, 5])
    p = Guarded(2, torch.float32, np.array([p0, last_r], dtype=np.float32))
    ngan.ops.ada_update(c.view, p.view, target, span, p_max)
    torch.cuda.synchronize()
    want = A.emulate_update(*case)
    got = p.view.cpu().numpy()
    assert (int(A.bits(got[0])), int(A.bits(got[1]))) == (int(A.bits(want[0])), int(A.bits(want[1]))), (case, got, want)
    assert c.view.tolist() == [0, 0, 0, 6] and c.intact() and p.intact()
    assert 0.0 <= float(got[0]) <= float(np.float32(p_max))


# ---- the live parameter mappings ------------------------------------------------------------------------------------------------------
P_VALUES = (0.0, 2.0 ** -24, 0.3, 0.5, 1.0 - 2.0 ** -24, 1.0)


def _uniforms(b, seed, p_values):
    """(b, 8) uniforms in [0, 1) with the gate columns salted with the probabilities themselves, 0 and the largest value below 1"""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(b, 8, generator=g)
    salt = torch.tensor(list(p_values)[:-1] + [0.0, 1.0 - 2.0 ** -24], dtype=torch.float32)
    for col in (0, 2, 3, 4, 5, 6):
        rows = torch.randint(0, b, (len(salt),), generator=g)
        u[rows, col] = salt
    return u.to(DEV)


@pytest.mark.parametrize("r", [16, 512])
@pytest.mark.parametrize("b", [1, 255, 256, 257])
def test_live_tables_equal_the_by_value_tables(ngan, b, r):
    """ngada_diffaug_params / ngada_diffgeo_params with p in device memory write what ngan_diffaug_params / ngan_diffgeo_params write
    with the same p by value, bit for bit, for every p, every policy mask, and with guard bands intact"""
    ops = ngan.ops
    u = _uniforms(b, 100 * b + r, P_VALUES)
    for p in P_VALUES:
        p_dev = torch.tensor([p, 123.0], dtype=torch.float32, device=DEV)
        for mask in range(32):
            if mask & 7 and not mask >> 3:
                want, live = Guarded(b * 8, torch.int32), Guarded(b * 8, torch.int32)
                ops.diffaug_params(u, want.view.view(b, 8), r, mask, p)
                ops.diffaug_params_live(u, live.view.view(b, 8), r, mask, p_dev)
            elif mask >> 3 and not mask & 7:
                want, live = Guarded(b * 8, torch.float32), Guarded(b * 8, torch.float32)
                ops.diffgeo_params(u, want.view.view(b, 8), r, mask, p)
                ops.diffgeo_params_live(u, live.view.view(b, 8), r, mask, p_dev)
            else:
                continue
            assert torch.equal(want.view.view(torch.int32), live.view.view(torch.int32)), (p, mask)
            assert live.intact() and want.intact()
    assert float(p_dev[1]) == 123.0


def test_tables_follow_an_update_on_the_stream_and_a_nan_closes_every_gate(ngan):
    """update, then the two mappings, on one stream with no host read in between: the tables are those of the new p; a NaN p gives
    identity rows"""
    ops, b, r = ngan.ops, 257, 16
    u = _uniforms(b, 9, (0.25, 0.75, 1.0))
    counters = torch.tensor([8, 0, 8, 0], dtype=torch.int64, device=DEV)
    p = torch.tensor([0.25, 0.0], dtype=torch.float32, device=DEV)
    t, g = torch.empty(b, 8, dtype=torch.int32, device=DEV), torch.empty(b, 8, dtype=torch.float32, device=DEV)
    ops.ada_update(counters, p, 0.6, 16.0, 1.0)                                 # r = 1 above 0.6: p = 0.25 + 8 / 16
    ops.diffaug_params_live(u, t, r, 7, p)
    ops.diffgeo_params_live(u, g, r, 24, p)
    torch.cuda.synchronize()
    assert p.tolist() == [0.75, 1.0] and counters.tolist() == [0, 0, 0, 1]
    t_want, g_want = torch.empty_like(t), torch.empty_like(g)
    ops.diffaug_params(u, t_want, r, 7, 0.75)
    ops.diffgeo_params(u, g_want, r, 24, 0.75)
    t_old = ops.diffaug_params(u, torch.empty_like(t), r, 7, 0.25)
    assert torch.equal(t, t_want) and torch.equal(g.view(torch.int32), g_want.view(torch.int32)) and not torch.equal(t, t_old)
    p[0] = float("nan")
    ops.diffaug_params_live(u, t, r, 7, p)
    ops.diffgeo_params_live(u, g, r, 24, p)
    assert torch.equal(t, ops.diffaug_table([ops.DIFFAUG_IDENTITY], DEV).repeat(b, 1))
    assert torch.equal(t, ops.diffaug_params(u, torch.empty_like(t), r, 7, 0.0))
    assert torch.equal(g.view(torch.int32), ops.diffgeo_params(u, torch.empty_like(g), r, 24, 0.0).view(torch.int32))
    assert ops.diffgeo_table_rows(g) == [ops.DIFFGEO_IDENTITY] * b
    p[0] = 7.0                                                                  # above 1: every gate open, as p = 1
    ops.diffaug_params_live(u, t, r, 7, p)
    assert torch.equal(t, ops.diffaug_params(u, torch.empty_like(t), r, 7, 1.0))


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------
ADA = dict(diffaug=POLICY, ada_target=0.6, ada_interval=2, ada_kimg=0.064, ada_p_init=0.5)       # span 64: 8 reals move p by 1/8


def trainer(ngan, nets=None, **kw):
    return ngan.train.PGGANTrainer(*(nets or small_nets(ngan)), learning_rate=1e-3, device_latents=True, **kw)


def ada_of(tr):
    torch.cuda.synchronize()
    return tr._ada.counters.tolist(), [int(v) for v in A.bits(tr._ada.p.cpu().numpy())], tr.ada_iteration


def spy_on_updates(ngan, monkeypatch):
    """record (counters before, p before, p after) of every ops.ada_update: the TEST reads the device, the product does not"""
    seen, plain = [], ngan.ops.ada_update

    def spy(counters, p, target, span, p_max=1.0):
        torch.cuda.synchronize()
        before = (counters.tolist(), p.cpu().numpy().copy())
        plain(counters, p, target, span, p_max)
        torch.cuda.synchronize()
        seen.append(before + (p.cpu().numpy().copy(), (target, span, p_max)))
    monkeypatch.setattr(ngan.ops, "ada_update", spy)
    return seen


def run_pair(ngan, iterations, nets=None, setup=None, **kw):
    """`iterations` eager iterations and capture + as many replays from the same draws -> (eager trainer, replayed trainer).
    nets: a factory of (G, D); setup(trainer): what a switch needs before its first step"""
    batches = [batch_draws(ngan, 70 + i, 4) for i in range(iterations)]

    def make():
        tr = trainer(ngan, nets=nets() if nets else None, **kw)
        if setup:
            setup(tr)
        return tr
    eager = make()
    for d in batches:
        eager.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"])
    tr, static = make(), None
    for d in batches:
        own = {k: d[k] for k in ("z_d", "z_gp", "eps", "z_g")}
        if static is None:
            static = {k: v.clone() for k, v in own.items()}
        if not tr.has_graph(d["real"].shape):                                   # (lazy regularisation keeps graphs per phase)
            before = ada_of(tr)
            tr.capture(d["real"], draws=static)
            assert ada_of(tr) == before, "capture() moved the controller"
        for k, v in own.items():
            static[k].copy_(v)
        tr.replay(d["real"])
    return eager, tr


def test_eager_and_replayed_runs_agree_and_follow_the_emulation(ngan, monkeypatch):
    """8 iterations at 16 x 16, batch 4, interval 2: the same weights, counters and p eager and replayed; at each of the 2 x 4 due
    iterations p_next is the emulation applied to the counters read just before, which hold the 8 reals seen since"""
    seen = spy_on_updates(ngan, monkeypatch)
    eager, tr = run_pair(ngan, 8, **ADA)
    assert same(state_of(eager), state_of(tr)) and ada_of(eager) == ada_of(tr)
    assert len(seen) == 8 and ada_of(tr)[2] == 8 and ada_of(tr)[0] == [0, 0, 0, 4]
    moved = 0
    for (pos, neg, n, updates), p_before, p_after, (target, span, p_max) in seen:
        assert n == 8 and 0 <= pos and 0 <= neg and pos + neg <= 8 and (target, span, p_max) == (0.6, 64.0, 1.0)
        want = A.emulate_update(pos, neg, n, p_before[0], p_before[1], target, span, p_max)
        assert (int(A.bits(p_after[0])), int(A.bits(p_after[1]))) == (int(A.bits(want[0])), int(A.bits(want[1])))
        moved += p_after[0] != p_before[0]
    assert moved >= 6, "p hardly moved: the case does not exercise the controller"
    for a, b in zip(seen[:4], seen[4:]):                                        # the eager and the replayed run, update by update
        assert a[0] == b[0] and np.array_equal(A.bits(a[2]), A.bits(b[2]))


def test_capture_leaves_the_controller_as_it_found_it(ngan):
    tr = trainer(ngan, **ADA)
    for i in range(3):                                                          # an odd count: counters are not empty, p has moved once
        d = batch_draws(ngan, 90 + i, 4)
        tr.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"])
    before, weights = ada_of(tr), state_of(tr)
    assert before[0][2] == 4 and before[0][3] == 1 and before[2] == 3
    tr.capture(d["real"], warmup=2, draws={k: d[k].clone() for k in ("z_d", "z_gp", "eps", "z_g")})
    assert ada_of(tr) == before and same(state_of(tr), weights)


def test_every_critic_pass_of_an_iteration_counts(ngan):
    """n_critic = 2: both critic steps count; n_critic = 0: the monitoring-only pass counts"""
    d = batch_draws(ngan, 95, 4)
    for n_critic, want in ((2, 8), (0, 4), (1, 4)):
        tr = trainer(ngan, n_critic=n_critic, **dict(ADA, ada_interval=3))
        tr.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"])
        counters = ada_of(tr)[0]
        assert counters[2] == want and counters[0] + counters[1] <= want and counters[3] == 0, (n_critic, counters)


def test_the_switch_off_is_the_trainer_without_the_arguments(ngan):
    """ada_target = 0: the same bits after 3 iterations, eager and replayed, the same RNG states, no new attribute or buffer"""
    def run(replayed, kw):
        tr = trainer(ngan, diffaug=POLICY, diffaug_p=0.5, **kw)
        torch.manual_seed(21)
        x = batch_draws(ngan, 3, 4)["real"]
        for _ in range(3):
            tr.step(x) if replayed else tr.train_iteration(x)
        torch.cuda.synchronize()
        return state_of(tr), torch.cuda.get_rng_state(DEV), tr._aug.generator.get_state(), tr
    off_kw = dict(ada_target=0.0, ada_interval=4, ada_kimg=500.0, ada_p_init=0.0)
    for replayed in (False, True):
        want, off = run(replayed, {}), run(replayed, off_kw)
        assert same(off[0], want[0]) and torch.equal(off[1], want[1]) and torch.equal(off[2], want[2]), replayed
        assert set(vars(off[3])) == set(vars(want[3])) and not any("ada" in k for k in vars(off[3]))
        assert len(off[3]._training_state()) == len(want[3]._training_state()) and off[3]._aug.live_p is None
        on = run(replayed, dict(ada_target=0.6, ada_interval=2, ada_kimg=0.064, ada_p_init=0.5))
        assert torch.equal(on[2], want[2]) and torch.equal(on[1], want[1])      # it draws as much, from both streams


@pytest.mark.parametrize("variant", ["lsgan", "bf16", "r1_lazy_ema_rmsprop", "lp", "mbstd", "spectral", "simloss"])
def test_the_switches_it_must_work_with(ngan, variant, monkeypatch):
    """four iterations eager and replayed, bit-equal, under the least-squares objective (threshold 0.5, mode 0), in the bf16 storage mode
    (the scores handed to the kernel are fp32), with R1 every second iteration, EMA and RMSprop, with the one-sided penalty, with a minibatch standard-deviation
    channel in the critic's head, with the spectral term and with the similarity term on the generated images"""
    kw = {"lsgan": dict(objective="lsgan"), "bf16": {},
          "r1_lazy_ema_rmsprop": dict(grad_pen_mode="r1", grad_pen_interval=2, ema_beta=0.99, optimizer="rmsprop"),
          "lp": dict(grad_pen_mode="lp"),
          "mbstd": dict(nets=lambda: small_nets(ngan, mbstd_group=4)),
          "spectral": dict(spec_loss_lambda=1.0, setup=lambda t: t.set_spectral_target(16, target16())),
          "simloss": dict(sim_loss_on="generated", sim_loss_center=True, setup=lambda t: t.set_sim_lambda(0.5))}[variant]
    calls, plain = [], ngan.ops.ada_accumulate

    def spy(real, fake, counters, mode=0, threshold=0.0):
        calls.append((real.dtype, None if fake is None else fake.dtype, tuple(real.shape), mode, threshold))
        return plain(real, fake, counters, mode, threshold)
    monkeypatch.setattr(ngan.ops, "ada_accumulate", spy)
    if variant == "bf16":
        ngan.ops.set_conv_precision("bf16")
    try:
        eager, tr = run_pair(ngan, 4, **ADA, **kw)
        assert same(state_of(eager), state_of(tr)) and ada_of(eager) == ada_of(tr)
        assert ada_of(tr)[0][3] == 2 and ada_of(tr)[2] == 4
    finally:
        ngan.ops.set_conv_precision("f32")
    want_mode = (0, 0.5) if variant == "lsgan" else (1, 0.0)
    assert calls and all(c[0] is torch.float32 and c[2] == (4,) and c[3:] == want_mode for c in calls), calls
    assert all((c[1] is None) == (variant == "lsgan") for c in calls)


# ---- epoch driver and checkpoint ---------------------------------------------------------------------------------------------------
def driver_run(ngan, f, epochs=(1, 11), resume=False, ada=True, **kw):
    """pggan_train on four synthetic 16 x 16 images, one batch per epoch, replayed graphs, given latents, a checkpoint every fifth
    epoch (ten epochs: the status line is printed every tenth): epoch 1 at 8 x 8, the growth step to 16 x 16 at epoch 2, its fade-in
    complete at epoch 4, as in the older drivers' tests; the controller updates every second iteration"""
    cfg = types.SimpleNamespace(**dict(DRIVER_CFG, N_epochs=10, checkpointing_period=5, ID="ada"))
    G, D = small_nets(ngan, res=8)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, device_latents=True, alpha_step=cfg.alpha_step,
                                 **(dict(ADA, **kw) if ada else dict(diffaug=POLICY)))
    data = ngan.train.TensorImageDataset.synthetic(4, 16, device=DEV, seed=8)
    ck = ngan.utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=torch.device(DEV), trainer=tr,
                                 extra_checkpoint_period=1e3)
    if resume:
        ck.load_state()
    lines = []
    series = ngan.train.pggan_train(tr, data, cfg, checkpoint=ck, epoch_init=epochs[0], epoch_final=epochs[1], use_graph=True,
                                    log=lambda *a: lines.append(" ".join(map(str, a))), draws=driver_draws,
                                    on_epoch=lambda ep, t: torch.manual_seed(100 + ep))
    torch.cuda.synchronize()
    return series, live_state_of(tr), tr, lines, ck


def live_state_of(tr):
    """state_of(tr) with the parameter values of RETIRED layers zeroed.  A layer that a completed transition retired (the smaller
    resolution's ToImage / FromImage) leaves the modules' state_dict, so no checkpoint has ever held its last values: a run resumed
    after the transition keeps the constructor's values in those dead segments, which nothing reads again.  Measured with this
    driver and a default-argument trainer, and alike with a diffaug policy and with the controller: 32 generator and 64 critic
    elements differ, all in inactive segments; optimiser state, step counts and monitors are equal.  What a resumed run guarantees,
    and what this compares bit for bit, is every live parameter, all optimiser state, and the controller."""
    state = state_of(tr)
    for k, flat in ((0, tr.flat_g), (1, tr.flat_d)):
        for off, p, active in zip(flat.offsets, flat.params, flat.active_host):
            if not active:
                state[k][off:off + p.numel()] = 0.0
    return state


def test_epoch_driver_status_line_checkpoint_and_resume(ngan, tmp_path, capsys):
    f = str(tmp_path / "a.pth")
    series, state, tr, lines, ck = driver_run(ngan, f)
    status = [ln for ln in lines if ln.startswith("Epoch:10,")]
    assert len(status) == 1 and "ada_p:" in status[0] and "ada_rt:" in status[0], lines
    saved = ngan.utils.load_checkpoint_dict(f)
    assert set(ngan.utils.ADA_KEYS) <= set(saved) and (saved["ada_target"], saved["ada_interval"], saved["ada_kimg"]) == (0.6, 2, 0.064)
    assert saved["ada_iteration"] == 10 == tr.ada_iteration and saved["ada_counters"].tolist() == [0, 0, 0, 5] == ada_of(tr)[0]
    assert np.array_equal(A.bits(saved["ada_p"].numpy()), A.bits(tr._ada.p.cpu().numpy()))
    ada = saved["ADA"]
    assert [e[0] for e in ada] == list(range(1, 11)) and all(0.0 <= e[1] <= 1.0 and -1.0 <= e[2] <= 1.0 for e in ada)
    assert ada[-1][1:] == tuple(tr._ada.p.tolist()) and len({e[1] for e in ada}) > 2, ada        # the last epoch's pair; p moved
    assert "{:#7.4g}".format(ada[-1][1]).strip() in status[0]
    g = str(tmp_path / "b.pth")
    head = driver_run(ngan, g, epochs=(1, 6))
    capsys.readouterr()                                                          # resuming under other settings is allowed, and said
    other = driver_run(ngan, g, epochs=(6, 7), resume=True, ada_target=0.5, diffaug_p=0.25, ada_p_init=0.0)      # (epoch 6: no checkpoint)
    assert "ada_target=0.6" in capsys.readouterr().out and float(other[2]._ada.p[0]) <= 0.25       # p carried over, under the new clamp
    assert other[2].ada_iteration == 6
    tail = driver_run(ngan, g, epochs=(6, 11), resume=True)
    assert {k: head[0][k] + tail[0][k] for k in series} == series, "the resumed run's monitors do not continue bit-equal"
    assert same(state, tail[1]), ("the resumed run's live state differs in", [i for i, (u, v) in enumerate(zip(state, tail[1])) if not np.array_equal(u, v)])
    assert tr.G.image_size == 16 and tr.G.alpha_value() >= 1 and not all(tr.flat_g.active_host), "the run did not cross a completed transition"
    assert ada_of(tail[2]) == ada_of(tr) and ngan.utils.load_checkpoint_dict(g)["ADA"] == ada
    h = str(tmp_path / "c.pth")                                                  # a file without the keys is off; eval-side readers see extras only
    driver_run(ngan, h, epochs=(1, 6), ada=False)
    assert not any(k.startswith("ada") or k == "ADA" for k in ngan.utils.load_checkpoint_dict(h))


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, q):
    """a batch of 8 in shares 4 + 4 and 5 + 3, four iterations each with an update every second: after every update both ranks hold the
    same p and last_r bit for bit, and the reduced n is the global count of reals seen"""
    import datetime
    import os
    import sys
    import traceback
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        from __graft_entry__ import load_package
        ngan = load_package()
        seen, plain = [], ngan.ops.ada_update

        def spy(counters, p, target, span, p_max=1.0):
            torch.cuda.synchronize()
            n = int(counters[2])
            plain(counters, p, target, span, p_max)
            torch.cuda.synchronize()
            seen.append((n, [int(v) for v in A.bits(p.cpu().numpy())]))
        ngan.ops.ada_update = spy
        report = []
        for shares in ([4, 4], [5, 3]):
            tr = ngan.train.PGGANTrainer(*small_nets(ngan), learning_rate=1e-3, **ADA)
            assert tr.world == world
            cut = slice(sum(shares[:rank]), sum(shares[:rank + 1]))
            del seen[:]
            for i in range(4):
                d = batch_draws(ngan, 80 + i, 8)
                tr.train_iteration(d["real"][cut], d["z_d"][cut], d["z_gp"][cut], d["eps"][cut], d["z_g"][cut], global_batch=shares)
            assert len(seen) == 2 and all(n == 16 for n, _ in seen), (shares, seen)       # 2 iterations x the global batch of 8
            mine = torch.tensor([b for _, bits in seen for b in bits], dtype=torch.int64)
            both = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(both, mine)
            assert torch.equal(both[0], both[1]), (shares, both)
            assert tr._ada.counters.tolist() == [0, 0, 0, 2] and tr.ada_iteration == 4
            report.append((shares, seen[-1][1]))
        torch.cuda.synchronize()
        q.put((rank, "ok", report))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_hold_the_same_p_after_every_update():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    results = sorted(q.get(timeout=5) for _ in range(2))
    assert [r[:2] for r in results] == [(0, "ok"), (1, "ok")], results
    assert results[0][2] == results[1][2] and all(p.exitcode == 0 for p in procs)
