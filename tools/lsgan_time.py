"""Cost of the least-squares objective (PGGANTrainer(objective="lsgan")) against the Wasserstein objective on one MI355X, in one
process, on the same commit:
  1. the graph-replayed iteration at the bench's headline configuration (512 x 512, batch 16, default widths, fp32), under both
     objectives, at grad_pen_lambda 10 and at 0: alternating rounds of `--steps` replays, device events around each round; the spread
     of the Wasserstein rounds goes alongside.  The launch counts of the two objectives are equal (one scalar-head launch each way
     per loss), so the expectation is no difference beyond that spread.
  2. PER-CALL times of the two new launches, ngan_lsloss_head and ngan_lsloss_head_bwd, next to the W heads they stand in for, at the
     critic's 2 x 16 scores and the generator's 16: device events around `--reps` back-to-back eager calls after a warm-up, median of
     `--rounds`.  A call cannot go faster than the host issues it, so these are upper bounds on the kernel times.
    python tools/lsgan_time.py --rounds 6 --steps 20 > profiles/lsgan_time.txt"""
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
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lsgan_time.py measures on a GPU; none found")
    pkg = load_package()
    dev = torch.device("cuda:0")
    pkg.ops.set_conv_precision("f32")

    def timed(fn, n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n          # ms per call

    # ---- 1. the replayed iteration under both objectives -------------------------------------------------------------------------
    torch.manual_seed(123)
    pool = [(torch.rand(args.batch, 1, args.res, args.res) * 2 - 1).to(dev) for _ in range(4)]
    for lam in (10.0, 0.0):
        trainers = {}
        for objective in ("wasserstein", "lsgan"):
            G, D = bench.build_nets(pkg, args.res, 1.0, dev)
            tr = pkg.train.PGGANTrainer(G, D, learning_rate=1e-4, beta1=0.5, grad_pen_lambda=lam, drift_epsilon=0.001,
                                        device_latents=True, objective=objective)
            tr.capture(pool[0], warmup=2)
            trainers[objective] = tr
        times = {k: [] for k in trainers}
        for _ in range(args.rounds):
            for objective, tr in trainers.items():
                tr.replay(pool[0])
                times[objective].append(timed(lambda i, tr=tr: tr.replay(pool[i % len(pool)]), args.steps))
        print(f"replayed iteration, {args.res}x{args.res}, batch {args.batch}, fp32, one GPU, grad_pen_lambda {lam:g}: ms per iteration, "
              f"{args.rounds} alternating rounds of {args.steps} replays")
        for objective, ts in times.items():
            print(f"  {objective:11s} median {statistics.median(ts):.4f}  min {min(ts):.4f}  max {max(ts):.4f}  rounds " + " ".join(f"{t:.4f}" for t in ts))
        spread = max(times["wasserstein"]) - min(times["wasserstein"])
        d = [b - a for a, b in zip(times["wasserstein"], times["lsgan"])]
        print(f"  wasserstein spread (max - min over the rounds): {spread * 1e3:.1f} us")
        print(f"  lsgan - wasserstein per round: median {statistics.median(d) * 1e3:+.1f} us  min {min(d) * 1e3:+.1f}  max {max(d) * 1e3:+.1f}")
        for objective, tr in trainers.items():
            for tag, flat in (("G", tr.flat_g), ("D", tr.flat_d)):
                assert bool(torch.isfinite(flat.flat).all()), (lam, objective, tag)
        del trainers

    # ---- 2. the two launches alone -------------------------------------------------------------------------------------------------
    print(f"per-call times (upper bounds on the kernel times): device events around {args.reps} back-to-back eager calls, median of "
          f"{args.rounds} rounds")
    call = pkg._C.call
    g = torch.Generator(device=dev).manual_seed(1)
    one = torch.ones((), device=dev)
    for n_real, n_fake in ((args.batch, args.batch), (args.batch, 0)):
        scores = torch.randn(n_real + n_fake, generator=g, device=dev)
        loss, mr, mf = (torch.empty((), device=dev) for _ in range(3))
        gs = torch.empty_like(scores)
        calls = {
            "lsloss_head": lambda i: call("ngan_lsloss_head", scores, n_real, n_fake, 1.0, 0.0, loss, mr, mf),
            "lsloss_head_bwd": lambda i: call("ngan_lsloss_head_bwd", scores, n_real, n_fake, 1.0, 0.0, one, None, None, gs),
            "wloss_head": lambda i: call("ngan_wloss_head", scores, n_real, n_fake, 0.001, loss, mr, mf),
            "wloss_head_bwd": lambda i: call("ngan_wloss_head_bwd", scores, n_real, n_fake, 0.001, one, None, None, gs),
        }
        for name, fn in calls.items():
            timed(fn, 5)
            ts = [timed(fn, args.reps) * 1e3 for _ in range(args.rounds)]
            print(f"  n_real {n_real:3d} n_fake {n_fake:3d} {name:16s} median {statistics.median(ts):7.2f} us  min {min(ts):7.2f}  max {max(ts):7.2f}")


if __name__ == "__main__":
    main()
