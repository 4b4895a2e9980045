"""Cost of differentiable augmentation (PGGANTrainer(diffaug=...)) on one MI355X, in one process:
  1. PER-CALL times of the four entry points -- ngan_diffaug_params, the forward and adjoint with the colour group (two launches
     each) and without (one) -- at (16, 1, 512, 512) and (32, 1, 512, 512): device events around `--reps` back-to-back eager calls
     after a warm-up, median of `--rounds`.  A call cannot go faster than the host issues it (about 9 us here: what the 64-byte
     parameter launch measures), so these are upper bounds on the kernel times and the rates are lower bounds; kernel times proper
     need `rocprofv3 --kernel-trace --stats` in a run of its own.  Bytes/s over the ALGORITHMIC bytes (12 B per element with the colour group: x read by the sum pass, read
     again and y written by the map pass; 8 B per element without) next to the HBM peak (8.0 TB/s specified, 6.3 TB/s achieved by a
     float4 copy).  The batches fit the 256 MiB Infinity Cache, so a rate above the HBM peak is the cache's, not an error.
  2. the graph-replayed iteration at the bench's headline configuration (512 x 512, batch 16, fp32), policy off and on
     (color,translation,cutout, p = 1), alternating rounds of `--steps` replays; the spread of the off rounds goes alongside.
  3. the acceptance figure: on - off against the summed kernel times of one iteration (reals b + generated 2 b forward in the critic
     step, b forward + b adjoint in the generator step, one parameter launch) -- what exceeds them by more than the off spread is a
     host-side cost; less than them is expected, they are upper bounds.  The eager uniform draw and parameter launch of every replay are inside the "on" time, as in training.
    python tools/diffaug_time.py --rounds 6 --steps 20 > profiles/diffaug_time.txt"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(os.path.join(__file__, os.pardir)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
import bench  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12
POLICY = "color,translation,cutout"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diffaug_time.py measures on a GPU; none found")
    pkg = load_package()
    ops = pkg.ops
    dev = torch.device("cuda:0")
    ops.set_conv_precision("f32")

    def timed(fn, n):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n          # ms per call

    # ---- 1. kernels ----------------------------------------------------------------------------------------------------------
    print(f"per-call times (upper bounds on the kernel times; rates are lower bounds): device events around {args.reps} back-to-back "
          f"eager calls, median of {args.rounds} rounds; bytes = algorithmic bytes")
    kernel_us = {}
    g = torch.Generator(device=dev).manual_seed(1)
    for B in (args.batch, 2 * args.batch):
        R = args.res
        x = torch.rand((B, 1, R, R), generator=g, device=dev) * 2 - 1
        y = torch.empty_like(x)
        u = torch.rand((B, 8), generator=g, device=dev)
        table = torch.empty((B, 8), dtype=torch.int32, device=dev)
        ops.diffaug_params(u, table, R, 7, 1.0)
        nocol = torch.empty((B, 8), dtype=torch.int32, device=dev)
        ops.diffaug_params(u, nocol, R, 6, 1.0)
        ws = torch.empty(int(pkg._C.lib().ngan_diffaug_workspace_bytes(B, 1, R)) // 8, dtype=torch.float64, device=dev)
        calls = {
            "params": (lambda i: ops.diffaug_params(u, table, R, 7, 1.0), 32 * B + 32 * B),
            "fwd colour": (lambda i: pkg._C.call("ngan_diffaug_fwd", x, table, y, ws, B, 1, R, R, B, 1, -1.0), 12 * x.numel()),
            "bwd colour": (lambda i: pkg._C.call("ngan_diffaug_bwd", x, table, y, ws, B, 1, R, R, B, 1), 12 * x.numel()),
            "fwd no colour": (lambda i: pkg._C.call("ngan_diffaug_fwd", x, nocol, y, None, B, 1, R, R, B, 0, -1.0), 8 * x.numel()),
            "bwd no colour": (lambda i: pkg._C.call("ngan_diffaug_bwd", x, nocol, y, None, B, 1, R, R, B, 0), 8 * x.numel()),
        }
        for name, (fn, nbytes) in calls.items():
            timed(fn, 5)
            ts = [timed(fn, args.reps) * 1e3 for _ in range(args.rounds)]
            med = statistics.median(ts)
            kernel_us[(B, name)] = med
            rate = nbytes / (med * 1e-6)
            print(f"  ({B}, 1, {R}, {R}) {name:14s} median {med:8.2f} us  min {min(ts):8.2f}  max {max(ts):8.2f}   {nbytes / 1e6:8.2f} MB  "
                  f">= {rate / 1e12:6.3f} TB/s = {rate / HBM_SPEC:5.2f} of the 8.0 TB/s HBM peak, {rate / HBM_COPY:5.2f} of a float4 copy's 6.3 TB/s")

    # ---- 2. the replayed iteration, off and on ---------------------------------------------------------------------------------
    torch.manual_seed(123)
    pool = [(torch.rand(args.batch, 1, args.res, args.res) * 2 - 1).to(dev) for _ in range(4)]
    trainers = {}
    for form, policy in (("off", ""), ("on", POLICY)):
        G, D = bench.build_nets(pkg, args.res, 1.0, dev)
        tr = pkg.train.PGGANTrainer(G, D, learning_rate=1e-4, beta1=0.5, grad_pen_lambda=10.0, drift_epsilon=0.001,
                                    device_latents=True, diffaug=policy)
        assert tr.diffaug_enabled == (policy != "")
        tr.capture(pool[0], warmup=2)
        trainers[form] = tr
    times = {k: [] for k in trainers}
    for _ in range(args.rounds):
        for form, tr in trainers.items():
            tr.replay(pool[0])
            times[form].append(timed(lambda i, tr=tr: tr.replay(pool[i % len(pool)]), args.steps))
    print(f"replayed iteration, {args.res}x{args.res}, batch {args.batch}, fp32, one GPU: ms per iteration, {args.rounds} alternating "
          f"rounds of {args.steps} replays")
    for form, ts in times.items():
        print(f"  {form:3s} median {statistics.median(ts):.4f}  min {min(ts):.4f}  max {max(ts):.4f}  rounds " + " ".join(f"{t:.4f}" for t in ts))
    spread = max(times["off"]) - min(times["off"])
    d = [b - a for a, b in zip(times["off"], times["on"])]
    diff = statistics.median(d)
    print(f"  off spread (max - min over the rounds): {spread * 1e3:.1f} us")
    print(f"  on - off per round: median {diff * 1e3:+.1f} us  min {min(d) * 1e3:+.1f}  max {max(d) * 1e3:+.1f}")

    # ---- 3. acceptance -----------------------------------------------------------------------------------------------------------
    b = args.batch
    if (2 * b, "fwd colour") in kernel_us:
        # critic step: reals (b) and generated (2 b) forward; generator step: b forward, b adjoint; one parameter launch.  The
        # (3 b)-sample critic work is counted as one b-launch plus one 2b-launch, as the trainer issues it.
        kernels = kernel_us[(b, "fwd colour")] + kernel_us[(2 * b, "fwd colour")] + kernel_us[(b, "fwd colour")] + \
            kernel_us[(b, "bwd colour")] + kernel_us[(b, "params")]
        elems = 5 * b * args.res * args.res
        print(f"summed per-call times of one iteration (3 forward calls, 1 adjoint, 1 parameter launch): {kernels:.1f} us "
              f"for {12 * elems / 1e6:.0f} MB algorithmic")
        extra = diff * 1e3 - kernels
        # the per-call times are upper bounds on the kernel times, so only an excess over them points at the host; on also saves
        # the W-loss's concatenation of 2 b images, which the off path pays
        if extra > spread * 1e3:
            verdict = "MORE than the calls cost by more than the off spread: look for a host-side cost"
        elif extra >= -spread * 1e3:
            verdict = "explained by the calls within the off spread"
        else:
            verdict = ("less than the calls cost alone: inside the graph the kernels are not held to the host's issue rate, and the "
                       "on path does not concatenate the W-loss's 2 b images; no host-side cost")
        print(f"on - off - per-call sum = {extra:+.1f} us against an off spread of {spread * 1e3:.1f} us: {verdict}")
    for form, tr in trainers.items():
        for tag, flat in (("G", tr.flat_g), ("D", tr.flat_d)):
            assert bool(torch.isfinite(flat.flat).all()), (form, tag)


if __name__ == "__main__":
    main()
