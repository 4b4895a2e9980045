"""RMSprop through the data-parallel paths, in spawned processes as test_gpu_dist.py does: two gloo ranks on one GPU against one rank
on the whole batch (critic all-reduce, generator stem exchanged as gathered factors into ngan_linear_wgrad_rmsprop, 1/world in
grad_scale), and the three-segment capture of one rank with a live RCCL group against the eager trajectory."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_gpu_dist import _free_port

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(port):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)


def _dp_worker(rank, world, port, fixture, q):
    """Rule, stated before the first run: after one iteration the parameters of a rank and of the whole-batch rank agree by the share
    rule of test_gpu_rmsprop.rmsprop_close -- fewer than 2e-3 of each tensor's elements differ by more than a tenth of a first
    RMSprop step (lr).  The two gradients agree to fp32 summation order (2e-4 of the max-norm in test_gpu_dist.py), and the first
    step is 10 lr sign(g), so only elements whose gradient is at rounding level can differ, by a whole step."""
    _setup(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from __graft_entry__ import load_package
        from conftest import load_golden
        import test_gpu_models as T
        from test_gpu_rmsprop import rmsprop_close
        ngan = load_package()
        dev = torch.device("cuda:0")
        fix = load_golden(fixture)
        own = [dist.new_group([r]) for r in range(world)][rank]
        t = lambda k: torch.from_numpy(fix[k]).to(dev)
        batch = int(fix["meta"][4])
        half = batch // world
        sl = slice(rank * half, (rank + 1) * half)
        lr = 1e-4
        G, D = T.build_small(ngan, fix)
        tr = ngan.train.PGGANTrainer(G, D, learning_rate=lr, optimizer="rmsprop")
        assert tr.world == world and tr.stem is not None and tr.fused_stem
        assert tr.opt_g.hyper_host[3] == 1.0 / world and tr.opt_d.hyper_host[3] == 1.0 / world
        Gr, Dr = T.build_small(ngan, fix)
        ref = ngan.train.PGGANTrainer(Gr, Dr, learning_rate=lr, optimizer="rmsprop", process_group=own)
        assert ref.world == 1
        tr.train_iteration(t("real")[sl], t("z_d")[sl], t("z_gp")[sl], t("eps")[sl], t("z_g")[sl])
        ref.train_iteration(t("real"), t("z_d"), t("z_gp"), t("eps"), t("z_g"))
        torch.cuda.synchronize()
        for flat, flat_ref in ((tr.flat_g, ref.flat_g), (tr.flat_d, ref.flat_d)):
            assert torch.equal(flat.seg_step, flat_ref.seg_step)
            for name, p, pr, a in zip(flat.names, flat.params, flat_ref.params, flat.active_host):
                if a:
                    assert rmsprop_close(p.detach().cpu().numpy(), pr.detach().cpu().numpy(), lr), name
            assert float((flat.square_avg - flat_ref.square_avg).abs().max()) <= 1e-2 * float(flat_ref.square_avg.abs().max())
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_match_the_whole_batch():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, "small_res16_fade_warm", q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    results = sorted(q.get(timeout=5) for _ in range(2))
    assert results == [(0, "ok"), (1, "ok")], results
    assert all(p.exitcode == 0 for p in procs)


def _capture_worker(port, q):
    """force_exchange with one rank and a real RCCL group: the three-segment capture (the RMSprop launches of both nets in their own
    segments, the stem's factors exchanged eagerly in between) replayed three times equals the eager trajectory bit for bit --
    parameters, square_avg and step counts -- in the f32 and bf16 modes."""
    _setup(port)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        from __graft_entry__ import load_package
        import test_gpu_rmsprop as R
        ngan = load_package()
        for mode in ("f32", "bf16"):
            ngan.ops.set_conv_precision(mode)
            seq = R.draws_32(5)

            def make():
                tr = R.make_32(ngan)
                tr.force_exchange = True
                tr.enable_stem_exchange()
                assert tr.stem is not None and tr._comm_stream is not None
                return tr
            eager, tr = make(), make()
            static = {k: seq[0][k].clone() for k in ("z_d", "z_gp", "eps", "z_g")}
            tr.capture(seq[0]["real"], draws=static)
            assert len(tr._graph) == 3
            for s in seq:
                eager.train_iteration(s["real"], s["z_d"], s["z_gp"], s["eps"], s["z_g"])
                for k, v in static.items():
                    v.copy_(s[k])
                tr.replay(s["real"])
            torch.cuda.synchronize()
            R.assert_same_training_state(tr, eager)
        ngan.ops.set_conv_precision("f32")
        q.put("ok")
    except Exception as e:  # noqa: BLE001
        q.put(repr(e))
        raise
    finally:
        dist.destroy_process_group()


def test_segmented_capture_replays_the_eager_rmsprop_trajectory():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_capture_worker, args=(_free_port(), q))
    p.start()
    p.join(600)
    assert p.exitcode == 0, f"worker exit code {p.exitcode}"
    assert q.get(timeout=5) == "ok"
