"""Synchronised BatchNorm for the data-parallel WGAN trainer (WGANTrainer(sync_batchnorm=True); csrc/stride2.hip: ngan_bn_moments ->
ngan_bn_merge_fold forward, ngan_bn_act_bwd_partial -> ngan_bn_act_bwd_merged backward) against torch fp64 on the CPU.

Kernel level: a tensor's pixel range cut into 1 - 4 unequal contiguous parts (what the ranks hold), one record per part, the records
concatenated (what all_gather yields) and merged, against fp64 BatchNorm2d over the whole tensor.  Trainer level, in spawned processes:
two gloo ranks on one GPU against the fp64 whole-batch reference loop of test_gpu_wgan (equal halves) and against a one-rank trainer on
the whole batch (a ragged 3 / 5 split), and one rank in a real RCCL group with its communication stream."""
import copy
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

import __graft_entry__ as graft

pkg = graft.load_package()
from neuron_gan_amd import train  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
TOL = 5e-5
SLOPE = 0.2


def rel_err(got, ref):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-30))


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------------
# kernel level
# ------------------------------------------------------------------------------------------------------------------
SHAPES = [(4, 8, 16), (3, 64, 8), (16, 1024, 2), (1, 32, 64), (8, 16, 128)]     # those of test_gpu_wgan's BatchNorm test
FAR_MEAN = (4, 16, 16)                                                           # |mean| = 1e3 std
CUTS = {1: [], 2: [0.3], 3: [0.5, 0.7], 4: [0.1, 0.5, 0.65]}                    # cumulative cut points of the pixel range


def make_case(shape, far=False):
    b, c, h = shape
    g = torch.Generator().manual_seed(c + h + (7 if far else 0))
    y = torch.randn(b, c, h, h, generator=g, dtype=torch.float64)
    y = y * 0.5 + 500.0 if far else y * 2 + 3
    y = y.float().double()              # the kernels read y in fp32: compare on the same values
    bn_ref = torch.nn.BatchNorm2d(c).double()
    with torch.no_grad():
        bn_ref.weight.normal_(1.0, 0.1, generator=g)
        bn_ref.bias.normal_(0.0, 0.1, generator=g)
        bn_ref.running_var.uniform_(0.5, 1.5, generator=g)
    bn = copy.deepcopy(bn_ref).float().to(DEV)
    return y, bn_ref, bn, g


def edges(npix, parts):
    e = [0] + [int(f * npix) for f in CUTS[parts]] + [npix]
    assert all(a < b for a, b in zip(e[:-1], e[1:])), e
    return e


def work(npix, c):
    return torch.empty(pkg._C.lib().ngan_chan_reduce_workspace_floats(npix, c), device=DEV)


def merged_forward(yd, bn, parts):
    """per-part moments records, concatenated, merged: (scale, shift, mean, rstd, n_total, pixel slices)"""
    c = yd.shape[-1]
    npix = yd.numel() // c
    flat = yd.view(npix, c)
    e = edges(npix, parts)
    sl = [flat[a:b] for a, b in zip(e[:-1], e[1:])]
    recs = []
    for p in sl:
        rec = torch.empty(1 + 2 * c, device=DEV, dtype=torch.float64)
        pkg._C.call("ngan_bn_moments", p, p.shape[0], c, rec, work(p.shape[0], c))
        recs.append(rec)
    scale, shift, mean, rstd = (torch.empty(c, device=DEV) for _ in range(4))
    n_total = torch.empty(1, device=DEV, dtype=torch.float64)
    pkg._C.call("ngan_bn_merge_fold", torch.cat(recs), parts, c, bn.weight.detach(), bn.bias.detach(), mean, rstd, scale, shift,
                bn.running_mean, bn.running_var, bn.num_batches_tracked, float(bn.momentum), float(bn.eps), n_total)
    return scale, shift, mean, rstd, n_total, sl


@pytest.mark.parametrize("parts", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES + ["far"])
def test_forward_partition_invariance(shape, parts):
    far = shape == "far"
    y, bn_ref, bn, _ = make_case(FAR_MEAN if far else shape, far)
    c = y.shape[1]
    act_ref = F.leaky_relu(bn_ref(y), SLOPE)
    yd = nhwc(y.float().to(DEV))
    npix = yd.numel() // c
    scale, shift, mean, rstd, n_total, _ = merged_forward(yd, bn, parts)
    a = torch.empty_like(yd)
    pkg._C.call("ngan_bn_act_apply", yd, scale, shift, 1, SLOPE, npix, c, a)
    assert rel_err(nchw(a), act_ref) < TOL, rel_err(nchw(a), act_ref)
    assert rel_err(bn.running_mean, bn_ref.running_mean) < 1e-6
    assert rel_err(bn.running_var, bn_ref.running_var) < 1e-5
    assert int(bn.num_batches_tracked) == int(bn_ref.num_batches_tracked) == 1
    assert float(n_total) == npix


@pytest.mark.parametrize("parts", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_partition_invariance(shape, parts):
    y, bn_ref, bn, g = make_case(shape)
    c = y.shape[1]
    yr = y.clone().requires_grad_(True)
    z_ref = bn_ref(yr)
    act_ref = F.leaky_relu(z_ref, SLOPE)
    go = torch.randn(act_ref.shape, generator=g, dtype=torch.float64)
    act_ref.backward(go)
    yd = nhwc(y.float().to(DEV))
    scale, shift, mean, rstd, n_total, ys = merged_forward(yd, bn, parts)
    gd = nhwc(go.float().to(DEV)).view(-1, c)
    gs = [gd[p0:p0 + p.shape[0]] for p0, p in zip(edges(gd.shape[0], parts)[:-1], ys)]
    recs = []
    for p, gp in zip(ys, gs):
        rec = torch.empty(2 * c, device=DEV, dtype=torch.float64)
        pkg._C.call("ngan_bn_act_bwd_partial", p, gp, scale, shift, mean, rstd, 1, SLOPE, p.shape[0], c, rec, work(p.shape[0], c))
        recs.append(rec)
    recs = torch.cat(recs)
    gy, dg, db = [], [], []
    for r, (p, gp) in enumerate(zip(ys, gs)):
        out, dgr, dbr = torch.empty_like(p), torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        pkg._C.call("ngan_bn_act_bwd_merged", p, gp, scale, shift, mean, rstd, bn.weight.detach(), 1, SLOPE, p.shape[0], c, recs, parts, r,
                    n_total, out, dgr, dbr, torch.empty(3 * c, device=DEV))
        gy.append(out)
        dg.append(dgr)
        db.append(dbr)
    gy = torch.cat(gy).view(yd.shape)
    assert rel_err(nchw(gy), yr.grad) < 1e-4, rel_err(nchw(gy), yr.grad)
    assert rel_err(sum(dg), bn_ref.weight.grad) < TOL and rel_err(sum(db), bn_ref.bias.grad) < TOL
    # each part's own share: the fp64 sums over that part's pixels alone, taken with the whole tensor's statistics
    var = y.var(dim=(0, 2, 3), unbiased=False)
    xhat = nhwc((y - y.mean(dim=(0, 2, 3), keepdim=True)) / torch.sqrt(var + bn.eps).view(1, -1, 1, 1)).view(-1, c)
    gz = nhwc(torch.where(z_ref.detach() > 0, go, SLOPE * go)).view(-1, c)
    e = edges(gd.shape[0], parts)
    for r, (a, b) in enumerate(zip(e[:-1], e[1:])):
        want_g, want_b = (gz[a:b] * xhat[a:b]).sum(0), gz[a:b].sum(0)
        assert rel_err(dg[r], want_g) < TOL, (r, rel_err(dg[r], want_g))
        assert rel_err(db[r], want_b) < TOL, (r, rel_err(db[r], want_b))
        if parts > 1:     # a share, not the whole
            assert rel_err(dg[r], bn_ref.weight.grad) > 1e-3


# ------------------------------------------------------------------------------------------------------------------
# trainer level, spawned ranks
# ------------------------------------------------------------------------------------------------------------------
TRAIN_CFGS = [dict(gw=[32, 16, 8], dw=[8, 16, 32], latent=16, size=64, b=8, n_critic=2, colors=1),
              dict(gw=[16, 8], dw=[8, 16], latent=32, size=32, b=6, n_critic=1, colors=3)]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _env(port):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(4)


def _state_errors(tag, nets, refs, refs32, single=None):
    """test_gpu_wgan's bound per tensor, max(3 * |ref32 - ref64|, 1e-5 max|ref| + 1e-7), num_batches_tracked exact.  With `single`
    (the one-GPU HIP trainer on the whole batch) the bound also admits 3 x that path's own deviation: the data-parallel run is held to
    the fidelity of the single-GPU path on the same batch, whose summation order differs from the fp32 reference loop's as much"""
    errs = []
    for i, (net, ref, r32) in enumerate(zip(nets, refs, refs32)):
        sd, rd, sd32 = net.layers.state_dict(), ref.state_dict(), r32.state_dict()
        s1 = single[i].layers.state_dict() if single is not None else None
        for k in rd:
            if k.endswith("num_batches_tracked"):
                if int(sd[k]) != int(rd[k]):
                    errs.append((tag, k, int(sd[k]), int(rd[k])))
                continue
            err = float((sd[k].double().cpu() - rd[k]).abs().max())
            bound = max(3 * float((sd32[k].double() - rd[k]).abs().max()), 1e-5 * float(rd[k].abs().max()) + 1e-7)
            if s1 is not None:
                bound = max(bound, 3 * float((s1[k].double().cpu() - rd[k]).abs().max()))
            if not err <= bound:
                errs.append((tag, k, err, bound))
    return errs


def _gather_cpu(t, world):
    t = t.detach().reshape(-1).cpu().contiguous()
    if world == 1:           # (an RCCL group takes no CPU tensors)
        return [t]
    out = [torch.empty_like(t) for _ in range(world)]
    dist.all_gather(out, t)
    return out


def _differs_across_ranks(tr, world):
    """names of the training-state tensors that are not bit-identical on every rank"""
    named = [("G.flat", tr.flat_g.flat), ("D.flat", tr.flat_d.flat), ("G.step", tr.flat_g.seg_step), ("D.step", tr.flat_d.seg_step)]
    for tag, flat in (("G", tr.flat_g), ("D", tr.flat_d)):
        named += [(f"{tag}.{s}", getattr(flat, s)) for s in flat.state_names]
    named += [(f"G.{k}", v) for k, v in tr.G.named_buffers()] + [(f"D.{k}", v) for k, v in tr.D.named_buffers()]
    bad = []
    for name, t in named:
        got = _gather_cpu(t, world)
        if not all(torch.equal(got[0], x) for x in got[1:]):
            bad.append(name)
    return bad


def _reference_run(T, cfg, kind, lr, world, rank, tr_kw, own=None):
    """2 x train_iteration of this rank's slice against the fp64 (and fp32) whole-batch reference loop; returns the error list.
    own: a one-rank group; the one-GPU trainer then runs the whole batch alongside (the second yardstick of _state_errors)"""
    G, D = T.make_nets(cfg["gw"], cfg["dw"], cfg["latent"], cfg["size"], cfg["colors"])
    Gl, Dl = copy.deepcopy(G.layers).double(), copy.deepcopy(D.layers).double()
    G32, D32 = copy.deepcopy(G.layers), copy.deepcopy(D.layers)
    optG, optD = T.ref_opts(Gl, Dl, kind, lr)
    optG32, optD32 = T.ref_opts(G32, D32, kind, lr)
    G.to(DEV)
    D.to(DEV)
    tr = train.WGANTrainer(G, D, learning_rate=lr, optimizer=kind, n_critic=cfg["n_critic"], sync_batchnorm=True, **tr_kw)
    assert tr.world == world
    single = None
    if own is not None:
        Gs, Ds = T.make_nets(cfg["gw"], cfg["dw"], cfg["latent"], cfg["size"], cfg["colors"])
        single = train.WGANTrainer(Gs.to(DEV), Ds.to(DEV), learning_rate=lr, optimizer=kind, n_critic=cfg["n_critic"], process_group=own)
        assert single.world == 1 and not single.sync_batchnorm
    tag = (kind, cfg["size"])
    errs = []
    g = torch.Generator().manual_seed(7)
    b = cfg["b"]
    sl = slice(rank * b // world, (rank + 1) * b // world)
    for it in range(2):
        real = torch.rand(b, cfg["colors"], cfg["size"], cfg["size"], generator=g, dtype=torch.float64) * 2 - 1
        zs = [torch.randn(b, cfg["latent"], generator=g, dtype=torch.float64) for _ in range(cfg["n_critic"])]
        zg = torch.randn(b, cfg["latent"], generator=g, dtype=torch.float64)
        want = T.ref_iteration(Gl, Dl, optG, optD, real, zs, zg, cfg["n_critic"])
        T.ref_iteration(G32, D32, optG32, optD32, real.float(), [z.float() for z in zs], zg.float(), cfg["n_critic"])
        got = tr.train_iteration(real[sl].float().to(DEV), [z[sl].float().to(DEV) for z in zs], zg[sl].float().to(DEV))
        if single is not None:
            single.train_iteration(real.float().to(DEV), [z.float().to(DEV) for z in zs], zg.float().to(DEV))
        for k, v in want.items():
            mean = float(sum(_gather_cpu(got[k].float(), world))) / world
            if not abs(mean - v) <= 1e-3 * max(abs(v), 1e-2):
                errs.append((tag, it, k, mean, v))
    torch.cuda.synchronize()
    errs += _state_errors(tag, (G, D), (Gl, Dl), (G32, D32), None if single is None else (single.G, single.D))
    bad = _differs_across_ranks(tr, world)
    if bad:
        errs.append((tag, "not bit-identical across ranks", bad))
    return errs, tr


def _ragged(T, world, rank, own):
    """ranks hold 3 and 5 samples: one d_compute against a one-rank trainer on all 8.  running_mean within 1e-5 (not the kernel test's
    1e-6): the stage-1 partial sums are fp32 on either side, so a batch mean carries ~1e-7 of the channel's spread, and the G stem's
    channel means are small against their spread (measured: 1.9e-6 of max|running_mean|)"""
    counts = [3, 5]
    n = sum(counts)
    G, D = T.make_nets([32, 16, 8], [8, 16, 32], 16, 64)
    Gr, Dr = T.make_nets([32, 16, 8], [8, 16, 32], 16, 64)
    for m in (G, D, Gr, Dr):
        m.to(DEV)
    tr = train.WGANTrainer(G, D, learning_rate=1e-3, sync_batchnorm=True)
    ref = train.WGANTrainer(Gr, Dr, learning_rate=1e-3, process_group=own)
    assert ref.world == 1 and not ref.sync_batchnorm
    g = torch.Generator().manual_seed(11)
    real = (torch.rand(n, 1, 64, 64, generator=g) * 2 - 1).to(DEV)
    z = torch.randn(n, 16, generator=g).to(DEV)
    start = sum(counts[:rank])
    sl = slice(start, start + counts[rank])
    got = tr.d_compute(real[sl], z[sl])
    want = ref.d_compute(real, z)
    torch.cuda.synchronize()
    errs = []
    weighted = float(sum(_gather_cpu(got["score_real"].double() * counts[rank], world))) / n
    if not abs(weighted - float(want["score_real"])) <= 1e-5 * abs(float(want["score_real"])):
        errs.append(("ragged score_real", weighted, float(want["score_real"])))
    for ours, theirs in ((G, Gr), (D, Dr)):
        for (k, a), (_, w) in zip(ours.named_buffers(), theirs.named_buffers()):
            if k.endswith("num_batches_tracked"):
                ok = int(a) == int(w)
            else:
                ok = rel_err(a, w) < 1e-5
            if not ok:
                errs.append(("ragged buffer", k, rel_err(a, w) if a.is_floating_point() else (int(a), int(w))))
    bad = []
    for net in (G, D):
        for k, v in net.named_buffers():
            every = _gather_cpu(v, world)          # one collective per buffer on every rank, whatever the outcome
            if not all(torch.equal(every[0], x) for x in every[1:]):
                bad.append(k)
    if bad:
        errs.append(("ragged buffers not bit-identical across ranks", bad))
    return errs


def _two_rank_worker(rank, world, port, q):
    _env(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import test_gpu_wgan as T
        own = [dist.new_group([r]) for r in range(world)][rank]
        out = {}
        for i, cfg in enumerate(TRAIN_CFGS):
            for kind in ("adam", "rmsprop"):
                out[f"cfg{i}-{kind}"] = _reference_run(T, cfg, kind, 1e-3 if kind == "adam" else 1e-4, world, rank, {}, own)[0]
        out["ragged"] = _ragged(T, world, rank, own)
        q.put((rank, out))
    except Exception as e:  # noqa: BLE001
        q.put((rank, {"exception": [repr(e)]}))
        raise
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_rank_results():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
    for p in procs:
        if p.is_alive():     # a rank that died leaves its peer waiting in a collective
            p.kill()
            p.join()
    results = dict(q.get(timeout=5) for _ in range(2))
    assert all(p.exitcode == 0 for p in procs), ([p.exitcode for p in procs], results)
    return results


@pytest.mark.parametrize("check", ["cfg0-adam", "cfg0-rmsprop", "cfg1-adam", "cfg1-rmsprop"])
def test_two_ranks_on_one_gpu_match_the_whole_batch_fp64_loop(two_rank_results, check):
    """each rank holds half of `real` and of every latent batch; 2 x train_iteration; parameters, optimiser state and BatchNorm
    buffers bit-identical across ranks and within test_gpu_wgan's bound of the fp64 reference loop on the whole batch"""
    for rank in (0, 1):
        assert "exception" not in two_rank_results[rank], two_rank_results[rank]
    assert all(two_rank_results[r][check] == [] for r in (0, 1)), {r: two_rank_results[r][check] for r in (0, 1)}


def test_ragged_split_keeps_exact_statistics(two_rank_results):
    for rank in (0, 1):
        assert "exception" not in two_rank_results[rank], two_rank_results[rank]
    assert all(two_rank_results[r]["ragged"] == [] for r in (0, 1)), {r: two_rank_results[r]["ragged"] for r in (0, 1)}


def _rccl_worker(port, q):
    """one rank, a real RCCL process group: BatchNorm collectives and gradient exchanges on the communication stream"""
    _env(port)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        import test_gpu_wgan as T
        cfg = TRAIN_CFGS[1]
        errs, tr = _reference_run(T, cfg, "adam", 1e-3, 1, 0, dict(device_latents=True))
        if tr._comm_stream is None:
            errs.append("no communication stream")
        real = (torch.rand(cfg["b"], cfg["colors"], cfg["size"], cfg["size"]) * 2 - 1).to(dev)
        try:
            tr.capture(real)
            errs.append("capture() did not raise")
        except NotImplementedError:
            pass
        tr.comm_timing = []
        nbt = int(tr.D.layers[3].num_batches_tracked)
        st = tr.step(real, use_graph=True)
        torch.cuda.synchronize()
        tags = [t for t, _, _ in tr.comm_timing]
        # G [16, 8]: 2 BatchNorms, D [8, 16]: 1.  Forwards: D(real) 1 + G 2 + D(fake) 1, then G 2 + D 1; backwards: D 1 + D 1, D 1 + G 2
        if tags.count("batchnorm") != 12 or tags.count("critic") != 1 or tags.count("generator") != 1:
            errs.append(("collectives of one eager step", tags))
        if tr.has_graph(real.shape) or int(tr.D.layers[3].num_batches_tracked) != nbt + 3:
            errs.append("step(use_graph=True) did not run eagerly")
        if not all(torch.isfinite(v).all() for v in st.values()):
            errs.append(("step stats", {k: float(v) for k, v in st.items()}))
        q.put(errs)
    except Exception as e:  # noqa: BLE001
        q.put([repr(e)])
        raise
    finally:
        dist.destroy_process_group()


def test_one_rank_rccl_group_eager_only():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_worker, args=(_free_port(), q))
    p.start()
    p.join(600)
    if p.is_alive():
        p.kill()
        p.join()
    assert p.exitcode == 0, f"worker exit code {p.exitcode}"
    assert q.get(timeout=5) == []
