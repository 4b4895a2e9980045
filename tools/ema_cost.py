"""Cost of the averaged generator (ema_beta) at the bench's headline configuration (512 x 512, batch 16, fp32, one GPU, HIP-graph
replay of the whole iteration, weights from torch.manual_seed(1)): three trainers in one process --
    off        ema_beta = 0: the launches of a build without the feature
    folded     ema_beta = 0.999, the average updated inside the optimiser launches (ngan_adam_step_ema + ngan_linear_wgrad_adam_ema)
    separate   ema_beta = 0.999, the plain launches followed by ngan_ema_step over the whole generator (opt_g.ema_fold = False)
Rounds alternate between them so that clock and thermal drift fall on all three.  Per round: `--steps` replays after one warm-up
replay, timed with events around the whole batch of replays.  Then the generator's optimiser step alone (opt_g.step with the last
step's stem factors, eager, events around `--steps` calls), the same three forms.
    python tools/ema_cost.py --rounds 6 --steps 20 >> profiles/ema_cost.txt"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(os.path.join(__file__, os.pardir)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
import bench  # noqa: E402

FORMS = {"off": (0.0, True), "folded": (0.999, True), "separate": (0.999, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--optimizer", default="adam", choices=["adam", "rmsprop"])
    args = ap.parse_args()
    pkg = load_package()
    dev = torch.device("cuda:0")
    pkg.ops.set_conv_precision("f32")
    torch.manual_seed(123)
    pool = [(torch.rand(args.batch, 1, args.res, args.res) * 2 - 1).to(dev) for _ in range(4)]
    trainers = {}
    for form, (beta, fold) in FORMS.items():
        G, D = bench.build_nets(pkg, args.res, 1.0, dev)
        tr = pkg.train.PGGANTrainer(G, D, learning_rate=1e-4, beta1=0.5, grad_pen_lambda=10.0, drift_epsilon=0.001,
                                    device_latents=True, optimizer=args.optimizer, ema_beta=beta)
        tr.opt_g.ema_fold = fold
        assert tr.fused_stem and tr.ema_enabled == (beta > 0)
        tr.capture(pool[0], warmup=2)
        trainers[form] = tr

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(args.steps):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    def report(title, times, unit):
        print(title)
        for form, ts in times.items():
            print(f"{form:9s} median {statistics.median(ts):.4f}  min {min(ts):.4f}  max {max(ts):.4f}  rounds " +
                  " ".join(f"{t:.4f}" for t in ts))
        for form in ("folded", "separate"):
            d = [b - a for a, b in zip(times["off"], times[form])]
            print(f"{form} - off per round: median {statistics.median(d):+.4f} {unit}  min {min(d):+.4f}  max {max(d):+.4f}")
        d = [b - a for a, b in zip(times["folded"], times["separate"])]
        print(f"separate - folded per round: median {statistics.median(d):+.4f} {unit}  min {min(d):+.4f}  max {max(d):+.4f}")

    times = {k: [] for k in trainers}
    for _ in range(args.rounds):
        for form, tr in trainers.items():
            tr.replay(pool[0])
            times[form].append(timed(lambda i, tr=tr: tr.replay(pool[i % len(pool)])))
    n_g = sum(p.numel() for p in trainers["off"].flat_g.params)
    print(f"generator parameters: {n_g} ({4 * n_g / 1e6:.1f} MB); optimiser {args.optimizer}")
    report(f"replayed iteration, {args.res}x{args.res}, batch {args.batch}, fp32, one GPU: ms per iteration, {args.rounds} alternating "
           f"rounds of {args.steps} replays", times, "ms")
    # the generator's optimiser step alone: the stem launch from the last replay's factors + the flat tail (+ ngan_ema_step) + re-pack
    steps = {k: [] for k in trainers}
    for _ in range(args.rounds):
        for form, tr in trainers.items():
            assert tr.stem.factors is not None
            tr.opt_g.step(tr.stem.factors)
            steps[form].append(timed(lambda i, tr=tr: tr.opt_g.step(tr.stem.factors)) * 1e3)
    report(f"generator optimiser step alone (eager launches, events around {args.steps} calls): us per step", steps, "us")
    for form, tr in trainers.items():
        for tag, flat in (("G", tr.flat_g), ("D", tr.flat_d)):
            assert bool(torch.isfinite(flat.flat).all()), (form, tag)
        if tr.ema_enabled:
            assert bool(torch.isfinite(tr.flat_g.ema).all()) and not torch.equal(tr.flat_g.ema, tr.flat_g.flat)


if __name__ == "__main__":
    main()
