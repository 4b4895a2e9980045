"""A training run over N ranks is the one-rank run of the same configuration: the share weight that makes
unequal shares of a global batch exact, cached graphs under changing shares, both epoch drivers on two ranks against the oracle / the
fp64 loop / one rank, rank 0's checkpoint resumed by every rank, and one launched rank for real.

Two gloo ranks share the one GPU (the collectives travel through the host; the real thing is RCCL, one rank per GPU), as in
test_gpu_dist.py; all two-rank cases run in ONE pair of processes, one after the other, and every test below reads that pair's
results.  The one-rank sides of the comparisons run in the pytest process: three processes hold the GPU at most."""
import datetime
import os
import socket
import subprocess
import sys
import traceback
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
FIXTURE = "small_res16_fade_warm"          # share weight, graphs (a fade-in stage: every kind of parameter is active)
ORACLE_FIXTURE = "small_res8_warm"         # the driver against the oracle (no growth)
SHARES = [(3, 1), (4, 3), (5, 1)]          # of the fixture's own batch of 4, and of drawn batches of 7 and 6
BOUND = 2e-4                               # tests/test_gpu_dist.py, equal split: the weight adds one fp32 multiplication per root
WGAN_SHARES = SHARES + [(2, 2)]            # (the equal split, which needs no weight, beside them: the same figures)
WGAN_CFG = dict(gw=[16, 8, 8], dw=[8, 8, 16], latent=8, size=64, colors=1)      # wgan_small's widths


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _np(t):
    return t.detach().cpu().numpy().copy()


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _unit(g, n, latent):
    v = torch.randn(n, latent, generator=g)
    return v / v.norm(dim=1, keepdim=True)


def draw_batch(seed, n, latent, res, colors=1):
    """reals, latents and epsilon of one global batch from a seeded host generator (as tests/test_gpu_dist.py draws them)"""
    g = torch.Generator().manual_seed(seed)
    return dict(real=torch.rand(n, colors, res, res, generator=g) * 2 - 1, z_d=_unit(g, n, latent), z_gp=_unit(g, n, latent),
                eps=torch.rand(n, 1, 1, 1, generator=g), z_g=_unit(g, n, latent))


def pg_draws(latent):
    def draws(epoch, k, n):
        d = draw_batch(10007 * epoch + k, n, latent, 1)
        d.pop("real")
        return d
    return draws


def wgan_draws(latent):
    def draws(epoch, k, n):
        g = torch.Generator().manual_seed(20011 * epoch + k)
        return dict(z_d=[torch.randn(n, latent, generator=g)], z_g=torch.randn(n, latent, generator=g))
    return draws


def flipped(draws):
    """the same global draws with every batch in reversed sample order"""
    def f(epoch, k, n):
        return {name: ([x.flip(0) for x in v] if isinstance(v, list) else v.flip(0)) for name, v in draws(epoch, k, n).items()}
    return f


def share_inputs(fix, n, latent, res):
    if n == int(fix["meta"][4]):
        return {k: torch.from_numpy(fix[k]) for k in ("real", "z_d", "z_gp", "eps", "z_g")}
    return draw_batch(500 + n, n, latent, res)


# ---------------------------------------------------------------------------------------------------------------------
# share weight, one iteration
# ---------------------------------------------------------------------------------------------------------------------
def grad_error(flat, flat_ref, world, skip=()):
    """tests/test_gpu_dist.py's measure: per tensor, against the tensor's own scale plus 1e-3 of the net's largest gradient"""
    worst = 0.0
    top = max(float(q.grad.abs().max()) for q in flat_ref.params)
    for p, pr, a in zip(flat.params, flat_ref.params, flat.active_host):
        if not a or id(p) in skip:
            continue
        got, want = p.grad / world, pr.grad                      # the fused optimiser launch applies the 1/world factor
        worst = max(worst, float((got - want).abs().max()) / (float(want.abs().max()) + 1e-3 * top))
    return worst


def param_error(tr, ref, skip=()):
    return max(float((p - pr).abs().max()) for flat, flat_ref in ((tr.flat_g, ref.flat_g), (tr.flat_d, ref.flat_d))
               for p, pr in zip(flat.params, flat_ref.params) if id(p) not in skip)


def biases_in_front_of_batchnorm(*nets):
    """ids of the conv biases that feed a BatchNorm2d directly.  BatchNorm subtracts the batch mean, so their exact gradient is zero:
    what the kernels (and torch) compute for them is rounding residue, unrelated between two summation orders, and Adam's first steps
    turn its sign into +-lr.  They are held to the residue's size instead (`residue_error`)."""
    out = {}
    for net in nets:
        mods = list(net.layers)
        for m, nxt in zip(mods[:-1], mods[1:]):
            if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)) and m.bias is not None and isinstance(nxt, torch.nn.BatchNorm2d):
                out[id(m.bias)] = m.bias
    return out


def residue_error(flat, flat_ref, world, only):
    """for the tensors whose exact gradient is zero: the largest |gradient| on either side, relative to the net's largest gradient"""
    top = max(float(q.grad.abs().max()) for q in flat_ref.params)
    worst = 0.0
    for p, pr in zip(flat.params, flat_ref.params):
        if id(p) in only:
            worst = max(worst, float(p.grad.abs().max()) / world / top, float(pr.grad.abs().max()) / top)
    return worst


def pggan_share_case(ngan, T, fix, own, rank, world, shares, precision, fused, weighted=True):
    """one critic and one generator half-step on this rank's share against the whole batch on a one-rank trainer; returns
    {critic grad, generator grad, parameters}: errors.  weighted=False: without the global batch, i.e. every rank's loss weighted
    1/world as before the share weight existed."""
    ngan.ops.set_conv_precision(precision)
    try:
        res, latent = int(fix["meta"][0]), int(fix["meta"][3])
        n = sum(shares)
        lo = sum(shares[:rank])
        data = {k: v.to(DEV) for k, v in share_inputs(fix, n, latent, res).items()}
        mine = {k: v[lo:lo + shares[rank]] for k, v in data.items()}
        # (the sharding rule would cut 4 into 2 + 2: any other split is stated share by share)
        gb = (n if shares == tuple(b - a for a, b in (ngan.launch.shard_bounds(n, world, r) for r in range(world))) else shares) \
            if weighted else None
        G, D = T.build_small(ngan, fix)
        tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3, fused_stem=fused)
        Gr, Dr = T.build_small(ngan, fix)
        ref = ngan.train.PGGANTrainer(Gr, Dr, learning_rate=1e-3, process_group=own, fused_stem=fused)
        assert tr.world == world and ref.world == 1 and tr.fused_stem == fused
        out = {}
        tr.d_compute(mine["real"], mine["z_d"], mine["z_gp"], mine["eps"], global_batch=gb)
        tr._exchange(tr.flat_d)
        ref.d_compute(data["real"], data["z_d"], data["z_gp"], data["eps"])
        out["critic grad"] = grad_error(tr.flat_d, ref.flat_d, world)
        if not weighted:         # (the stem's factor gather needs the global batch once the shares differ: critic only)
            torch.cuda.synchronize()
            return out
        tr.g_compute(mine["real"], mine["z_g"], skip_stem_grad=fused, global_batch=gb)
        tr._exchange(tr.flat_g)
        tr.materialize_stem_grad()           # fused stem: the update reads the gathered factors; form the gradient for the comparison
        ref.g_compute(data["real"], data["z_g"])
        out["generator grad"] = grad_error(tr.flat_g, ref.flat_g, world)
        tr.opt_d.step()
        tr.g_adam()
        ref.opt_d.step()
        ref.g_adam()
        out["parameters"] = param_error(tr, ref)
        torch.cuda.synchronize()
        return out
    finally:
        ngan.ops.set_conv_precision("f32")


def wgan_share_case(ngan, TW, own, rank, world, shares):
    c = WGAN_CFG
    n = sum(shares)
    lo = sum(shares[:rank])
    g = torch.Generator().manual_seed(900 + n)
    real = (torch.rand(n, c["colors"], c["size"], c["size"], generator=g) * 2 - 1).to(DEV)
    z_d, z_g = torch.randn(n, c["latent"], generator=g).to(DEV), torch.randn(n, c["latent"], generator=g).to(DEV)
    sl = slice(lo, lo + shares[rank])
    G, D = TW.make_nets(c["gw"], c["dw"], c["latent"], c["size"], c["colors"])
    Gr, Dr = TW.make_nets(c["gw"], c["dw"], c["latent"], c["size"], c["colors"])
    tr = ngan.train.WGANTrainer(G.to(DEV), D.to(DEV), learning_rate=1e-3, sync_batchnorm=True)
    ref = ngan.train.WGANTrainer(Gr.to(DEV), Dr.to(DEV), learning_rate=1e-3, process_group=own)
    assert tr.world == world and ref.world == 1
    out = {}
    rule = tuple(b - a for a, b in (ngan.launch.shard_bounds(n, world, r) for r in range(world)))
    gb = n if shares == rule else shares
    zero = biases_in_front_of_batchnorm(tr.G, tr.D)
    tr.d_compute(real[sl], z_d[sl], global_batch=gb)
    tr._exchange(tr.flat_d)
    ref.d_compute(real, z_d)
    out["critic grad"] = grad_error(tr.flat_d, ref.flat_d, world, skip=zero)
    out["critic zero-gradient residue"] = residue_error(tr.flat_d, ref.flat_d, world, zero)
    out["critic grad, residue tensors included (not asserted)"] = grad_error(tr.flat_d, ref.flat_d, world)
    tr.g_compute(real[sl], z_g[sl], global_batch=gb)
    tr._exchange(tr.flat_g)
    ref.g_compute(real, z_g)
    out["generator grad"] = grad_error(tr.flat_g, ref.flat_g, world, skip=zero)
    out["generator zero-gradient residue"] = residue_error(tr.flat_g, ref.flat_g, world, zero)
    for t in (tr, ref):
        t.opt_d.step()
        t.opt_g.step()
    out["parameters"] = param_error(tr, ref, skip=zero)
    out["parameters, residue tensors included (not asserted)"] = param_error(tr, ref)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# graphs under changing shares
# ---------------------------------------------------------------------------------------------------------------------
def graphs_case(ngan, T, fix, rank, world):
    """global batches 4, 3, 4 (shares 2 + 2, 2 + 1, 2 + 2): cached graphs replayed against the same ranks running eagerly on the same
    draws.  Returns the names of the parameters that differ (none: replay == eager bit for bit, with the weight in device memory)."""
    res, latent = int(fix["meta"][0]), int(fix["meta"][3])
    make = lambda: ngan.train.PGGANTrainer(*T.build_small(ngan, fix), learning_rate=1e-3)      # noqa: E731
    eager, tr = make(), make()
    statics, captures = {}, 0
    for step, n in enumerate((4, 3, 4)):
        lo, hi = ngan.launch.shard_bounds(n, world, rank)
        data = {k: v[lo:hi].to(DEV) for k, v in draw_batch(700 + step, n, latent, res).items()}
        real = data.pop("real")
        eager.train_iteration(real, **data, global_batch=n)
        if not tr.has_graph(real.shape, n):
            key = tr._graph_key(real.shape, n)
            statics[key] = {k: v.clone() for k, v in data.items()}
            tr.capture(real, draws=statics[key], global_batch=n)
            captures += 1
        for k, v in statics[tr._graph_key(real.shape, n)].items():
            v.copy_(data[k])
        tr.replay(real, global_batch=n)
    torch.cuda.synchronize()
    names = tr.flat_g.names + tr.flat_d.names
    differing = [k for k, p, pe in zip(names, tr.flat_g.params + tr.flat_d.params, eager.flat_g.params + eager.flat_d.params)
                 if not torch.equal(p, pe)]
    return dict(differing=differing, captures=captures)


# ---------------------------------------------------------------------------------------------------------------------
# drivers
# ---------------------------------------------------------------------------------------------------------------------
def recorded(tr, names):
    """wrap the trainer's step entry points: per call the batch size, n_critic and (host reads: test only) the scalars"""
    log = []
    for name in names:
        inner = getattr(tr, name)

        def wrapper(real, *a, _inner=inner, **k):
            out = _inner(real, *a, **k)
            log.append(dict(b=int(real.size(0)), n_critic=tr.n_critic, stats={s: float(v) for s, v in out.items()},
                            flat=(tr.flat_g.flat.clone(), tr.flat_d.flat.clone()) if not log else None))
            return out
        setattr(tr, name, wrapper)
    return log


def oracle_driver_run(ngan, T, world, rank):
    """pggan_train, one epoch, 11 images in global batches of 4 (4, 4, 3), eager, given draws"""
    from conftest import load_golden
    fix = load_golden(ORACLE_FIXTURE)
    res, latent = int(fix["meta"][0]), int(fix["meta"][3])
    G, D = T.build_small(ngan, fix)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-3)
    assert tr.world == world
    log = recorded(tr, ["train_iteration"])
    cfg = types.SimpleNamespace(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[], N_epochs=1,
                                alpha_step=0.5, learning_rate=1e-3, checkpointing_period=10, ID="orc", seed=17)
    data = ngan.train.TensorImageDataset.synthetic(11, res, device=DEV, seed=5)
    series = ngan.train.pggan_train(tr, data, cfg, use_graph=False, log=lambda *a: None, draws=pg_draws(latent))
    torch.cuda.synchronize()
    return dict(log=[dict(b=e["b"], stats=e["stats"]) for e in log], series=series,
                G={k: _np(p) for k, p in G.named_parameters()}, D={k: _np(p) for k, p in D.named_parameters()})


GROWTH_CFG = dict(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=8, transit_sch=[2], N_epochs=6, alpha_step=0.5,
                  learning_rate=1e-3, checkpointing_period=2, ID="grow", seed=3)


class ReversedBatches:
    """a TensorImageDataset that serves every batch in reversed sample order"""

    def __init__(self, inner):
        self.inner = inner

    def __len__(self):
        return len(self.inner)

    def set_image_size(self, size):
        self.inner.set_image_size(size)

    def batch(self, indices):
        return torch.stack([self.inner[j] for j in reversed(indices)])


def growth_nets(ngan):
    torch.manual_seed(5)
    G = ngan.models.Generator_PG([32, 16, 16], image_size_init=4, latent_dim=32).to(DEV)
    D = ngan.models.Discriminator_PG([16, 16, 32], image_size_init=4).to(DEV)
    return G, D


def growth_driver_run(ngan, world, rank, ckpt_dir=None, reverse=False, sim_lambda=0.0):
    """pggan_train over a growth event: 11 images in global batches of 8 (8, 3), epochs 1 - 4 with growth at epoch 2, replayed graphs,
    given draws.  ckpt_dir: rank 0 checkpoints there (epochs 2 and 4, one file); every rank then resumes from it for one more epoch."""
    cfg = types.SimpleNamespace(**dict(GROWTH_CFG, sim_loss_lambda=sim_lambda))
    G, D = growth_nets(ngan)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, alpha_step=cfg.alpha_step)
    assert tr.world == world
    log = recorded(tr, ["replay"])
    data = ngan.train.TensorImageDataset.synthetic(11, 16, device=DEV, seed=8)
    draws = pg_draws(32)
    if reverse:
        data, draws = ReversedBatches(data), flipped(draws)
    epochs = []
    on_epoch = lambda ep, t: epochs.append((ep, t.G.alpha_value(), t.G.image_size, t.opt_g.param_groups[0]["lr"]))   # noqa: E731
    ck = None
    if ckpt_dir is not None:
        f = os.path.join(ckpt_dir, "GenDisc_grow.pth")
        ck = ngan.utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=DEV, trainer=tr,
                                     extra_checkpoint_period=1e3)
    series = ngan.train.pggan_train(tr, data, cfg, checkpoint=ck, epoch_final=5, use_graph=True, log=lambda *a: None, draws=draws,
                                    on_epoch=on_epoch)
    torch.cuda.synchronize()
    out = dict(series=series, epochs=epochs, n_critic=[e["n_critic"] for e in log], first=[_np(t) for t in log[0]["flat"]],
               flat=[_np(tr.flat_g.flat), _np(tr.flat_d.flat)], seg_step=[_np(tr.flat_g.seg_step), _np(tr.flat_d.seg_step)])
    if ckpt_dir is not None:
        out["files"] = sorted(os.listdir(ckpt_dir))
        G2, D2 = growth_nets(ngan)
        tr2 = ngan.train.PGGANTrainer(G2, D2, learning_rate=cfg.learning_rate, alpha_step=cfg.alpha_step)
        ck2 = ngan.utils.Checkpointer(G2, D2, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=DEV, trainer=tr2,
                                      extra_checkpoint_period=1e3)
        ck2.load_state()
        out["resumed_epoch"] = (ck2.epoch, G2.image_size)
        out["resumed_equal"] = all(torch.equal(a, b) for net, net2 in ((G, G2), (D, D2))
                                   for a, b in zip(net.state_dict().values(), net2.state_dict().values()))
        more = ngan.train.pggan_train(tr2, data, cfg, checkpoint=ck2, epoch_init=5, epoch_final=6, use_graph=True, log=lambda *a: None,
                                      draws=draws)
        torch.cuda.synchronize()
        out["more"] = more
        state = torch.cat([tr2.flat_g.flat, tr2.flat_d.flat, tr2.flat_g.exp_avg, tr2.flat_d.exp_avg_sq]).cpu()
        if world > 1:
            every = [torch.empty_like(state) for _ in range(world)]
            dist.all_gather(every, state)
            out["resumed_ranks_equal"] = all(torch.equal(every[0], x) for x in every[1:])
    return out


def wgan_driver_run(ngan, TW, world, rank, sync):
    """wgan_train, one epoch of 11 images in global batches of 4 (4, 4, 3), n_critic 1, given draws, eager"""
    c = WGAN_CFG
    G, D = TW.make_nets(c["gw"], c["dw"], c["latent"], c["size"], c["colors"])
    tr = ngan.train.WGANTrainer(G.to(DEV), D.to(DEV), learning_rate=1e-3, n_critic=1, sync_batchnorm=sync)
    assert tr.world == world
    cfg = types.SimpleNamespace(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, N_epochs=1, learning_rate=1e-3,
                                checkpointing_period=10, ID="wg", seed=29)
    data = ngan.train.TensorImageDataset.synthetic(11, c["size"], device=DEV, seed=6)
    lines = []
    hist = ngan.train.wgan_train(tr, data, cfg, use_graph=True, log=lines.append, eval_noise=torch.zeros(16, c["latent"], device=DEV),
                                 draws=wgan_draws(c["latent"]))
    torch.cuda.synchronize()
    return dict(history=hist, lines=lines, G={k: _np(v) for k, v in G.layers.state_dict().items()},
                D={k: _np(v) for k, v in D.layers.state_dict().items()})


# ---------------------------------------------------------------------------------------------------------------------
# the pair of ranks
# ---------------------------------------------------------------------------------------------------------------------
def _two_rank_worker(rank, world, port, q, ckpt_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(4)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=240))
    out = {}
    try:
        from __graft_entry__ import load_package
        from conftest import load_golden
        import test_gpu_models as T
        import test_gpu_wgan as TW
        import test_gpu_epoch_dist as E
        ngan = load_package()
        fix = load_golden(FIXTURE)
        own = [dist.new_group([r]) for r in range(world)][rank]
        for precision in ("f32", "bf16"):
            for fused in (True, False):
                for shares in SHARES:
                    out[("pggan", precision, fused, shares)] = E.pggan_share_case(ngan, T, fix, own, rank, world, shares, precision, fused)
        out["unweighted 3 + 1"] = E.pggan_share_case(ngan, T, fix, own, rank, world, (3, 1), "f32", True, weighted=False)
        for shares in WGAN_SHARES:
            out[("wgan", shares)] = E.wgan_share_case(ngan, TW, own, rank, world, shares)
        out["graphs"] = E.graphs_case(ngan, T, fix, rank, world)
        out["oracle"] = E.oracle_driver_run(ngan, T, world, rank)
        out["growth"] = E.growth_driver_run(ngan, world, rank, ckpt_dir=ckpt_dir)
        out["wgan_driver"] = E.wgan_driver_run(ngan, TW, world, rank, sync=True)
        out["similarity"] = E.growth_driver_run(ngan, world, rank, sim_lambda=0.5)["series"]
    except Exception:  # noqa: BLE001
        out["exception"] = traceback.format_exc()
    finally:
        q.put((rank, out))
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """both ranks' results; a phase that raised ends its rank there (its traceback is under "exception"), and nothing is started again"""
    world = 2
    ckpt_dir = str(tmp_path_factory.mktemp("ckpt"))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, world, port, q, ckpt_dir)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(world):
            r, out = q.get(timeout=840)
            got[r] = out
    finally:
        for p in procs:
            p.join(60)
            if p.is_alive():
                p.terminate()
    assert sorted(got) == [0, 1] and all(p.exitcode == 0 for p in procs), ([p.exitcode for p in procs], sorted(got))
    return got


def phase(pair, key):
    for r in (0, 1):
        assert key in pair[r], f"rank {r} never reached {key!r}: " + pair[r].get("exception", "(no traceback)")
    return pair[0][key], pair[1][key]


@pytest.mark.parametrize("shares", SHARES)
@pytest.mark.parametrize("fused", [True, False], ids=["fused_stem", "plain_stem"])
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_share_weight_gives_the_whole_batch_gradient(pair, precision, fused, shares):
    for r, errs in enumerate(phase(pair, ("pggan", precision, fused, shares))):
        print(f"rank {r} {precision} fused={fused} shares {shares}: {errs}")
        for what, e in errs.items():
            assert e < BOUND, (r, what, e)


def test_without_the_share_weight_unequal_shares_miss_the_bound(pair):
    """3 + 1 with every rank weighted 1/world -- (mean_a + mean_b) / 2 instead of the batch mean, what the trainers did before they
    knew the global batch: far outside the bound, so the test above shows something"""
    for r, errs in enumerate(phase(pair, "unweighted 3 + 1")):
        print(f"rank {r}: unweighted shares 3 + 1: {errs}")
        assert errs["critic grad"] > 10 * BOUND, errs


@pytest.mark.parametrize("shares", WGAN_SHARES)
def test_share_weight_wgan_sync_batchnorm(pair, shares):
    """The conv biases in front of a BatchNorm have an exact gradient of zero (`biases_in_front_of_batchnorm`): both sides must keep
    them at rounding residue -- below 1e-5 of the net's largest gradient: an fp32 sum of up to 4 x 64 x 64 = 16384 terms that cancel
    keeps about eps * sqrt(16384) = 8e-6 of the terms' magnitude, which is at most the magnitude of a weight gradient's terms -- and
    they are left out of the element-wise comparison, which would compare the residue of one summation order with that of another.
    Measured on an MI355X: residue 1.7e-7 - 4.2e-6; without them critic gradient 3.0e-6 - 5.3e-6, generator gradient 1.2e-6 - 4.1e-6,
    parameters 7.5e-7 - 1.1e-5; with them 2.3e-3 - 3.0e-3 (gradient measure) and 1.7e-3 - 1.9e-3 (parameters, Adam at lr 1e-3 turning
    the residue's sign into +-lr) -- for the equal split 2 + 2, which involves no weight, exactly as for 3 + 1."""
    for r, errs in enumerate(phase(pair, ("wgan", shares))):
        print(f"rank {r} wgan shares {shares}: {errs}")
        for what, e in errs.items():
            if "not asserted" in what:
                continue
            assert e < (1e-5 if "residue" in what else BOUND), (r, what, e)


def test_cached_graphs_replay_eager_under_changing_shares(pair):
    r0, r1 = phase(pair, "graphs")
    # every rank captures at the same steps (a capture holds collectives): twice, or three times when the ragged shape registered
    # new packed weight copies and all graphs were forgotten on both ranks
    assert r0["captures"] == r1["captures"] and r0["captures"] in (2, 3), (r0["captures"], r1["captures"])
    assert r0["differing"] == [] and r1["differing"] == [], (r0["differing"], r1["differing"])


# ---- the PGGAN driver against the oracle -------------------------------------------------------------------------------
def _check_against_oracle(ngan, runs, order):
    """runs: one result of oracle_driver_run per rank; order: the epoch's permutation.  Bounds: test_gpu_train.py's
    test_three_iterations_follow_the_oracle, unchanged."""
    from conftest import load_golden, split_state
    from oracle import pggan_oracle as O
    fix = load_golden(ORACLE_FIXTURE)
    res, alpha, init, latent = int(fix["meta"][0]), float(fix["meta"][1]), int(fix["meta"][2]), int(fix["meta"][3])
    pg, pd = O.as_leaf_params(split_state(fix, "G/")), O.as_leaf_params(split_state(fix, "D/"))
    spec = O.NetSpec(image_size_init=init, slope=0.2, alpha=alpha)
    og, od = O.make_adam(pg, 1e-3), O.make_adam(pd, 1e-3)
    images = ngan.train.TensorImageDataset.synthetic(11, res, seed=5).full
    draws = pg_draws(latent)
    for k, i in enumerate(range(0, 11, 4)):
        idx = order[i:i + 4]
        d = draws(1, k, len(idx))
        want = O.train_step(pg, spec, pd, spec, og, od, images[idx], d["z_d"], d["z_gp"], d["eps"], d["z_g"])
        assert sum(run["log"][k]["b"] for run in runs) == len(idx)
        for k_w, k_g in (("D_loss", "D_loss"), ("score_real", "score_real"), ("score_fake", "score_fake"), ("GP", "D_grad_pen"),
                         ("G_loss", "G_loss")):
            got = sum(run["log"][k]["b"] * run["log"][k]["stats"][k_g] for run in runs) / len(idx)      # rank-weighted mean
            print(f"iteration {k} {k_w}: {got} (oracle {want[k_w]})")
            assert abs(got - want[k_w]) < 2e-3 * abs(want[k_w]) + 2e-4, (k, k_w, got, want[k_w])
    for run in runs:
        for tag, ref in (("G", pg), ("D", pd)):
            for name, p in run[tag].items():
                if name in ref and ref[name].grad is not None:
                    assert float(np.abs(p - ref[name].detach().numpy()).max()) < 2e-4, (tag, name)


def test_pggan_driver_follows_the_oracle_on_one_rank(ngan, monkeypatch):
    """(one rank draws its permutation from torch's global generator, whose state at that point depends on everything before; the
    test hands the driver a known permutation instead)"""
    import test_gpu_models as T
    order = ngan.train.epoch_order(11, 17, 1, 2)
    monkeypatch.setattr(ngan.train, "epoch_order", lambda n, seed, epoch, world=1: list(order))
    _check_against_oracle(ngan, [oracle_driver_run(ngan, T, 1, 0)], order)


def test_pggan_driver_follows_the_oracle_on_two_ranks(ngan, pair):
    runs = phase(pair, "oracle")
    assert runs[0]["series"] == runs[1]["series"]
    assert [e["b"] for e in runs[0]["log"]] == [2, 2, 2] and [e["b"] for e in runs[1]["log"]] == [2, 2, 1]
    _check_against_oracle(ngan, list(runs), ngan.train.epoch_order(11, 17, 1, 2))


# ---- the PGGAN driver across a growth event ----------------------------------------------------------------------------
def _deviation(a, b):
    params = max(float(np.abs(x - y).max()) for x, y in zip(a["flat"], b["flat"]))
    series = max(abs(x - y) for k in a["series"] for x, y in zip(a["series"][k], b["series"][k]))
    return params, series


@pytest.fixture(scope="module")
def one_rank_growth(ngan):
    """the one-rank run on the two-rank run's permutations, and the same with every batch reversed: the same mathematics in another
    summation order, on the one-rank code path -- the yardstick for how far two correct fp32 runs drift apart"""
    orig = ngan.train.epoch_order
    ngan.train.epoch_order = lambda n, seed, epoch, world=1: orig(n, seed, epoch, 2)
    try:
        out = {}
        for sim in (0.0, 0.5):
            out[sim] = (growth_driver_run(ngan, 1, 0, sim_lambda=sim), growth_driver_run(ngan, 1, 0, reverse=True, sim_lambda=sim))
        return out
    finally:
        ngan.train.epoch_order = orig


def test_pggan_driver_across_a_growth_event(pair, one_rank_growth):
    """Measured on the MI355X: the figures are printed before they are asserted."""
    r0, r1 = phase(pair, "growth")
    one, rev = one_rank_growth[0.0]
    for r in (r0, r1):                       # exact: the schedule and the update counts
        assert r["epochs"] == one["epochs"] and r["n_critic"] == one["n_critic"] == [1] * 8
        for a, b in zip(r["seg_step"], one["seg_step"]):
            assert np.array_equal(a, b)
    assert [e[2] for e in one["epochs"]] == [4, 8, 8, 8] and one["epochs"][1][1] < 1 <= one["epochs"][3][1]      # it did grow and fade in
    assert all(np.array_equal(a, b) for a, b in zip(r0["flat"], r1["flat"])), "the ranks' parameters differ"
    assert r0["series"] == r1["series"]
    first = max(float(np.abs(a - b).max()) for a, b in zip(r0["first"], one["first"]))
    print(f"after the first update: two ranks against one rank {first:.3e}")
    assert first < BOUND
    yard, got = _deviation(one, rev), _deviation(r0, one)
    print(f"end of run, parameters: reversed batches {yard[0]:.3e}, two ranks {got[0]:.3e}; series: reversed {yard[1]:.3e}, two ranks {got[1]:.3e}")
    # measured on an MI355X: parameters 6.5e-7 (reversed batches) / 1.0e-6 (two ranks), series 7.2e-7 / 1.05e-6
    assert got[0] <= 2 * yard[0] and got[1] <= 2 * yard[1], (got, yard)


def test_rank_0_writes_and_every_rank_resumes(pair):
    for r in phase(pair, "growth"):
        assert r["files"] == ["GenDisc_grow.pth"]
        assert r["resumed_epoch"] == (4, 8) and r["resumed_equal"] and r["resumed_ranks_equal"]
        assert len(r["more"]["G_loss"]) == 1 and np.isfinite(r["more"]["G_loss"][0])


def test_similarity_monitor_couples_the_global_batch(pair, one_rank_growth):
    s0, s1 = phase(pair, "similarity")
    assert s0 == s1
    one, rev = one_rank_growth[0.5]
    base = one_rank_growth[0.0][0]["series"]["G_loss"]
    assert max(abs(a - b) for a, b in zip(one["series"]["G_loss"], base)) > 1e-3, "the monitor adds nothing: the case shows nothing"
    yard = max(abs(a - b) for a, b in zip(one["series"]["G_loss"], rev["series"]["G_loss"]))
    got = max(abs(a - b) for a, b in zip(s0["G_loss"], one["series"]["G_loss"]))
    print(f"G_loss with the similarity monitor: reversed batches {yard:.3e}, two ranks {got:.3e}")      # measured: 6.7e-7 / 1.05e-6
    assert got <= 2 * yard, (got, yard)


# ---- the WGAN driver ---------------------------------------------------------------------------------------------------
def test_wgan_driver_on_two_ranks_follows_the_fp64_loop(ngan, pair):
    """wgan_train on two ranks against the fp64 whole-batch loop of test_gpu_wgan over the same global batches and draws; bound and
    yardsticks as in test_gpu_wgan_sync_bn (`_state_errors`): 3 x the fp32 loop's own deviation, 3 x the one-rank HIP driver's, and a
    floor of 1e-5 max|ref| + 1e-7"""
    import copy
    import test_gpu_wgan as TW
    runs = phase(pair, "wgan_driver")
    c = WGAN_CFG
    G, D = TW.make_nets(c["gw"], c["dw"], c["latent"], c["size"], c["colors"])
    G64, D64, G32, D32 = copy.deepcopy(G.layers).double(), copy.deepcopy(D.layers).double(), copy.deepcopy(G.layers), copy.deepcopy(D.layers)
    o64, o32 = TW.ref_opts(G64, D64, "adam", 1e-3), TW.ref_opts(G32, D32, "adam", 1e-3)
    images = ngan.train.TensorImageDataset.synthetic(11, c["size"], seed=6).full
    order, draws = ngan.train.epoch_order(11, 29, 1, 2), wgan_draws(c["latent"])
    sums = {}
    for k, i in enumerate(range(0, 11, 4)):
        idx = order[i:i + 4]
        d = draws(1, k, len(idx))
        want = TW.ref_iteration(G64, D64, *o64, images[idx].double(), [z.double() for z in d["z_d"]], d["z_g"].double(), 1)
        TW.ref_iteration(G32, D32, *o32, images[idx], d["z_d"], d["z_g"], 1)
        for name, v in want.items():
            sums[name] = sums.get(name, 0.0) + v
    orig = ngan.train.epoch_order
    ngan.train.epoch_order = lambda n, seed, epoch, world=1: orig(n, seed, epoch, 2)
    try:
        single = wgan_driver_run(ngan, TW, 1, 0, sync=False)
    finally:
        ngan.train.epoch_order = orig
    assert runs[0]["history"] == runs[1]["history"]
    assert sum("run eagerly" in ln for ln in runs[0]["lines"]) == 1 and not any("run eagerly" in ln for ln in runs[1]["lines"])
    for name, v in sums.items():                      # the per-epoch sums of the per-batch means
        got = runs[0]["history"][0][name]
        print(f"{name}: two ranks {got}, fp64 loop {v}, one rank {single['history'][0][name]}")
        assert abs(got - v) <= 1e-3 * max(abs(v), 1e-2), (name, got, v)
    errs = []
    for run in runs:
        for tag, r64, r32 in (("G", G64, G32), ("D", D64, D32)):
            rd, sd32 = r64.state_dict(), r32.state_dict()
            for k in rd:
                if k.endswith("num_batches_tracked"):
                    if int(run[tag][k]) != int(rd[k]):
                        errs.append((tag, k, int(run[tag][k]), int(rd[k])))
                    continue
                ref = rd[k].numpy()
                err = float(np.abs(run[tag][k].astype(np.float64) - ref).max())
                bound = max(3 * float(np.abs(sd32[k].double().numpy() - ref).max()), 1e-5 * float(np.abs(ref).max()) + 1e-7,
                            3 * float(np.abs(single[tag][k].astype(np.float64) - ref).max()))
                if not err <= bound:
                    errs.append((tag, k, err, bound))
        assert all(np.array_equal(run[t][k], runs[0][t][k]) for t in ("G", "D") for k in run[t]), "the ranks' states differ"
    assert errs == [], errs


# ---- one rank, a real RCCL group -----------------------------------------------------------------------------------------
def _one_rank_worker(port, q):
    """trainers made before the process group exists (no group, no communication stream) and after (a one-rank `nccl` group,
    global_batch=None): three iterations, eager and replayed, must leave bit-equal parameters"""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    try:
        from __graft_entry__ import load_package
        from conftest import load_golden
        import test_gpu_models as T
        import test_gpu_epoch_dist as E
        ngan = load_package()
        fix = load_golden(FIXTURE)
        res, latent, batch = int(fix["meta"][0]), int(fix["meta"][3]), int(fix["meta"][4])
        torch.cuda.set_device(DEV)
        make = lambda **kw: ngan.train.PGGANTrainer(*T.build_small(ngan, fix), learning_rate=1e-3, **kw)      # noqa: E731
        steps = [{k: v.to(DEV) for k, v in E.draw_batch(300 + i, batch, latent, res).items()} for i in range(3)]

        def run(eager, replayed):
            for s in steps:
                eager.train_iteration(s["real"], s["z_d"], s["z_gp"], s["eps"], s["z_g"])
            static = {k: steps[0][k].clone() for k in ("z_d", "z_gp", "eps", "z_g")}
            replayed.capture(steps[0]["real"], draws=static)
            for s in steps:
                for k, v in static.items():
                    v.copy_(s[k])
                replayed.replay(s["real"])
            torch.cuda.synchronize()

        plain = [make(), make()]         # no group: everything they do happens before a process group exists
        assert all(t.world == 1 and t._comm_stream is None for t in plain)
        run(*plain)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
        try:
            grouped = [make(process_group=dist.group.WORLD) for _ in range(2)]
            assert all(t.world == 1 and t._comm_stream is not None and t._root is t._one for t in grouped)
            run(*grouped)
            bad = []
            for tag, a, b in (("eager", plain[0], grouped[0]), ("replayed", plain[1], grouped[1]), ("eager/replayed", plain[0], plain[1])):
                if not (torch.equal(a.flat_g.flat, b.flat_g.flat) and torch.equal(a.flat_d.flat, b.flat_d.flat)):
                    bad.append(tag)
            q.put("ok" if not bad else "not bit-equal: " + ", ".join(bad))
        finally:
            dist.destroy_process_group()
    except Exception:  # noqa: BLE001
        q.put(traceback.format_exc())
        raise


def test_one_rank_is_untouched():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_one_rank_worker, args=(_free_port(), q))
    p.start()
    p.join(300)
    if p.is_alive():
        p.terminate()
        pytest.fail("the one-rank worker did not finish in 300 s")
    assert q.get(timeout=5) == "ok"
    assert p.exitcode == 0


# ---- the launcher, for real, once ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["pggan", "wgan"])
def test_a_launched_rank_trains_and_checkpoints(tmp_path, path):
    """the path every rank of `--gpus N` takes, with N = 1: RANK / LOCAL_RANK / WORLD_SIZE in the environment, a one-rank `nccl` group,
    the synthetic dataset, two epochs at the smallest preset.  (`--gpus 2` needs two GPUs: not run here.)"""
    conf = tmp_path / "tiny.py"
    lines = [f"{d}_dir = {str(tmp_path / d)!r}" for d in ("images", "weights", "plots", "logs")]
    lines += ["ID = 'ln01'", "N_epochs = 2", "checkpointing_period = 2", "batch_size = 8", "n_critic = 1", "learning_rate = 1e-3"]
    if path == "pggan":
        lines += ["pggan = True", "wgan = False", "image_size = 8", "N_gen_features = [32, 16]", "N_dis_features = [16, 32]",
                  "transit_sch = [1]", "alpha_step = 1.0", "grad_pen_lambda = 10.0"]
    else:
        lines += ["pggan = False", "wgan = True", "image_size = 64", "latent_dim = 8", "N_gen_features = [16, 8, 8]",
                  "N_dis_features = [8, 8, 16]"]
    conf.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    cmd = [sys.executable, os.path.join(ROOT, "neuron-gan_amd", "launch.py"), "--configs", str(conf)]
    out = subprocess.run(cmd, env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    found = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs if f == "GenDisc_ln01.pth"]
    assert len(found) == 1, found
