"""Replayed-iteration time with Adam against RMSprop at the bench's headline configuration (512 x 512, batch 16, fp32, one GPU, HIP-graph
replay of the whole iteration, weights from torch.manual_seed(1)).  One trainer per optimiser in the same process; rounds alternate
between them (Adam, RMSprop, Adam, ...) so that clock and thermal drift fall on both.  Per round: `--steps` replays after one
warm-up replay, timed with events around the whole batch of replays.
    python tools/optimizer_time.py --rounds 6 --steps 20 > profiles/optimizer_time.txt
Per-kernel times come from a kernel trace of the same tool with fewer rounds:
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/optimizer_time.py --rounds 1 --steps 5"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(os.path.join(__file__, os.pardir)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    pkg = load_package()
    dev = torch.device("cuda:0")
    pkg.ops.set_conv_precision("f32")
    torch.manual_seed(123)
    pool = [(torch.rand(args.batch, 1, args.res, args.res) * 2 - 1).to(dev) for _ in range(4)]
    trainers = {}
    for kind in ("adam", "rmsprop"):
        G, D = bench.build_nets(pkg, args.res, 1.0, dev)
        tr = pkg.train.PGGANTrainer(G, D, learning_rate=1e-4, beta1=0.5, grad_pen_lambda=10.0, drift_epsilon=0.001,
                                    device_latents=True, optimizer=kind)
        assert tr.fused_stem
        tr.capture(pool[0], warmup=2)
        trainers[kind] = tr
    times = {k: [] for k in trainers}
    for _ in range(args.rounds):
        for kind, tr in trainers.items():
            tr.replay(pool[0])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.steps):
                tr.replay(pool[i % len(pool)])
            e1.record()
            torch.cuda.synchronize()
            times[kind].append(e0.elapsed_time(e1) / args.steps)
    print(f"replayed iteration, {args.res}x{args.res}, batch {args.batch}, fp32, one GPU: ms per iteration, {args.rounds} alternating "
          f"rounds of {args.steps} replays")
    for kind, ts in times.items():
        print(f"{kind:8s} median {statistics.median(ts):.3f}  min {min(ts):.3f}  max {max(ts):.3f}  rounds " +
              " ".join(f"{t:.3f}" for t in ts))
    d = [r - a for a, r in zip(times["adam"], times["rmsprop"])]
    print(f"rmsprop - adam per round: median {statistics.median(d):+.3f} ms  min {min(d):+.3f}  max {max(d):+.3f}")
    for kind, tr in trainers.items():
        for tag, flat in (("G", tr.flat_g), ("D", tr.flat_d)):
            assert bool(torch.isfinite(flat.flat).all()), (kind, tag)


if __name__ == "__main__":
    main()
