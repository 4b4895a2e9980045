"""Time one WGAN training iteration at the default widths (G [128..16], D [16..128]), 512^2, batch 8: the HIP path's replayed graph
(WGANTrainer.capture / replay) against the same nets' `self.layers` run as stock PyTorch modules in eager mode on the same GPU with
torch.optim and the reference's loop (train.py:470-506) -- the yardstick, a measurement only.  n_critic 1 and 5, Adam and RMSprop.
Then a per-kernel breakdown of one eager HIP iteration (torch.profiler), n_critic 1, Adam.

--sync: in a spawned child holding a one-rank RCCL group, n_critic 1, Adam: the replayed graph, the eager iteration, and the eager
iteration with sync_batchnorm=True (every training-mode BatchNorm call all-gathers its statistics on the communication stream, plus the
two gradient all-reduces), and the time inside those collectives (events around each communication-stream section).  One rank: what
this measures is the cost of the synchronised path itself, not an interconnect.

    python tools/wgan_time.py [--iters 20] [--warmup 5] [--sync]      (record: profiles/wgan_time.txt)
"""
import argparse
import copy
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

pkg = graft.load_package()
from neuron_gan_amd import models, train, utils  # noqa: E402

GW, DW, LATENT, SIZE, B = [128, 64, 32, 32, 16, 16], [16, 16, 32, 32, 64, 128], 512, 512, 8
DEV = torch.device("cuda:0")


def nets():
    torch.manual_seed(1)
    G = models.Generator_wgan(GW, latent_dim=LATENT, image_size=SIZE)
    D = models.Discriminator_wgan(DW, image_size=SIZE)
    G.apply(utils.init_weights)
    D.apply(utils.init_weights)
    return G.to(DEV), D.to(DEV)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def hip_replay(kind, n_critic, real, iters, warmup):
    G, D = nets()
    tr = train.WGANTrainer(G, D, optimizer=kind, n_critic=n_critic, device_latents=True)
    tr.capture(real)
    return timed(lambda: tr.replay(real), iters, warmup)


def torch_eager(kind, n_critic, real, iters, warmup):
    G, D = nets()
    Gl, Dl = copy.deepcopy(G.layers), copy.deepcopy(D.layers)
    if kind == "adam":
        oG, oD = torch.optim.Adam(Gl.parameters(), lr=1e-4, betas=(0.5, 0.999)), torch.optim.Adam(Dl.parameters(), lr=1e-4, betas=(0.5, 0.999))
    else:
        oG, oD = torch.optim.RMSprop(Gl.parameters(), lr=1e-4), torch.optim.RMSprop(Dl.parameters(), lr=1e-4)

    def it():
        for _ in range(n_critic):
            rs = Dl(real)
            z = torch.randn(B, LATENT, device=DEV)
            sf = Dl(Gl(z).detach()).mean()
            loss = -rs.mean() + sf + 0.001 * torch.square(rs).mean()
            Dl.zero_grad()
            loss.backward()
            oD.step()
            for p in Dl.parameters():
                p.data.clamp_(-0.01, 0.01)
        Gl.zero_grad()
        gl = -Dl(Gl(torch.randn(B, LATENT, device=DEV))).mean()
        gl.backward()
        oG.step()
    return timed(it, iters, warmup)


def breakdown(real):
    from torch.profiler import ProfilerActivity, profile
    G, D = nets()
    tr = train.WGANTrainer(G, D, optimizer="adam", n_critic=1, device_latents=True)
    for _ in range(2):
        tr.train_iteration(real)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        tr.train_iteration(real)
        torch.cuda.synchronize()
    rows = sorted(prof.key_averages(), key=lambda e: -e.device_time_total)
    total = sum(e.device_time_total for e in rows)
    lines = [f"  device time of one eager HIP iteration (n_critic 1, Adam): {total / 1e3:.3f} ms over {sum(e.count for e in rows)} launches"]
    for e in rows[:16]:
        lines.append(f"  {e.device_time_total / 1e3:8.3f} ms  {e.count:5d}x  {e.key[:100]}")
    return lines


def sync_child(port, iters, warmup, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(DEV)
    real = (torch.rand(B, 1, SIZE, SIZE, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(DEV)
    G, D = nets()
    tr = train.WGANTrainer(G, D, optimizer="adam", n_critic=1, device_latents=True)
    tr.capture(real)          # before the process group exists: WGANTrainer.capture is a GLOBAL-mode capture
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=DEV)
    try:
        graph = timed(lambda: tr.replay(real), iters, warmup)
        G, D = nets()
        tr = train.WGANTrainer(G, D, optimizer="adam", n_critic=1, device_latents=True)
        eager = timed(lambda: tr.train_iteration(real), iters, warmup)
        G, D = nets()
        tr = train.WGANTrainer(G, D, optimizer="adam", n_critic=1, device_latents=True, sync_batchnorm=True)
        synced = timed(lambda: tr.train_iteration(real), iters, warmup)
        tr.comm_timing = []                     # a window of its own: the events are not part of the timings above
        for _ in range(iters):
            tr.train_iteration(real)
        torch.cuda.synchronize()
        per_tag = {}
        for tag, e0, e1 in tr.comm_timing:
            n, ms = per_tag.get(tag, (0, 0.0))
            per_tag[tag] = (n + 1, ms + e0.elapsed_time(e1))
        n_bn, ms_bn = per_tag.get("batchnorm", (0, 0.0))
        n_ex = sum(per_tag.get(t, (0, 0.0))[0] for t in ("critic", "generator"))
        ms_ex = sum(per_tag.get(t, (0, 0.0))[1] for t in ("critic", "generator"))
        q.put([f"  sync_batchnorm, one-rank RCCL group, adam n_critic 1: HIP graph replay {graph:8.3f} ms   eager {eager:8.3f} ms   "
               f"eager + sync_batchnorm {synced:8.3f} ms",
               f"    inside the collectives per iteration: {n_bn / iters:.0f} BatchNorm all-gathers {ms_bn / iters:7.3f} ms, "
               f"{n_ex / iters:.0f} gradient all-reduces {ms_ex / iters:7.3f} ms"])
    except Exception as e:      # noqa: BLE001
        q.put([f"  (sync measurement failed: {type(e).__name__}: {e})"])
        raise
    finally:
        dist.destroy_process_group()


def sync_lines(iters, warmup):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=sync_child, args=(port, iters, warmup, q))
    p.start()
    p.join(900)
    if p.is_alive():
        p.kill()
        p.join()
    try:
        return q.get(timeout=5)
    except Exception:       # noqa: BLE001 (queue.Empty: the child died before reporting)
        return [f"  (sync measurement: child exit code {p.exitcode})"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sync", action="store_true", help="only the sync_batchnorm comparison (one-rank RCCL group, spawned child)")
    a = ap.parse_args()
    if a.sync:
        print(f"WGAN iteration, G {GW} D {DW}, {SIZE}^2, batch {B}, fp32, {torch.cuda.get_device_name(0)}", flush=True)
        print("\n".join(sync_lines(a.iters, a.warmup)))
        return
    real = (torch.rand(B, 1, SIZE, SIZE, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(DEV)
    print(f"WGAN iteration, G {GW} D {DW}, {SIZE}^2, batch {B}, fp32, {torch.cuda.get_device_name(0)}")
    for kind in ("adam", "rmsprop"):
        for n_critic in (1, 5):
            h = hip_replay(kind, n_critic, real, a.iters, a.warmup)
            t = torch_eager(kind, n_critic, real, a.iters, a.warmup)
            print(f"  {kind:8s} n_critic {n_critic}: HIP graph replay {h:8.3f} ms   torch eager (self.layers) {t:8.3f} ms   "
                  f"ratio {t / h:5.2f}x", flush=True)
    try:
        print("\n".join(breakdown(real)))
    except Exception as e:      # the profiler is a diagnostic: its absence must not hide the timings above
        print(f"  (no per-kernel breakdown: {type(e).__name__}: {e})")


if __name__ == "__main__":
    main()
