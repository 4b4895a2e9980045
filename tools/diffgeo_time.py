"""Cost of the geometric augmentation groups (PGGANTrainer(diffaug="blit,geometry")) on one MI355X, in one process:
  1. PER-CALL times of ngan_diffgeo_fwd and ngan_diffgeo_bwd at (16, 1, 512, 512) and (32, 1, 512, 512), rows drawn by
     ngan_diffgeo_params with both groups at p = 1, next to a plain-torch restatement on the same GPU: F.affine_grid + F.grid_sample
     (bilinear, zero padding, align_corners=True) on the matching matrices, and its autograd backward (the cotangent through
     grid_sample alone: the grid is built once, outside the timed region).  Device events around `--reps` back-to-back eager calls
     after a warm-up, median of `--rounds`.  A call cannot go faster than the host issues it (about 8 us here), so these are upper
     bounds on the kernel times.  Next to each time: the fraction of the byte floor, 8 B per element (one read, one write) at the
     6.3 TB/s a float4 copy achieves; the batches fit the 256 MiB Infinity Cache, so a fraction above 1 is the cache's, not an error.
     Condition: neither launch is slower than torch's.
  2. the graph-replayed iteration at the bench's headline configuration (512 x 512, batch 16, default widths, fp32), policy off and
     on (blit,geometry, p = 1), alternating rounds of `--steps` replays; the spread of the off rounds goes alongside.  `--off-only`
     measures the off trainer alone -- the form to run on the parent commit, whose figures go next to these.
    python tools/diffgeo_time.py --rounds 6 --steps 20 > profiles/diffgeo_time.txt"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.abspath(os.path.join(__file__, os.pardir)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
import bench  # noqa: E402

HBM_COPY = 6.3e12
POLICY = "blit,geometry"


def grid_theta(table, R):
    """(B, 2, 3) matrices of F.affine_grid(align_corners=True) for the affine rows: normalised (x, y) = (column, row) / c - 1"""
    a = table.double()
    c = 0.5 * (R - 1)
    th = torch.stack([torch.stack([a[:, 4], a[:, 3], a[:, 3] + a[:, 4] + a[:, 5] / c - 1], 1),
                      torch.stack([a[:, 1], a[:, 0], a[:, 0] + a[:, 1] + a[:, 2] / c - 1], 1)], 1)
    return th.float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--off-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diffgeo_time.py measures on a GPU; none found")
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

    # ---- 1. kernels against torch ------------------------------------------------------------------------------------------------
    if not args.off_only:
        print(f"per-call times (upper bounds on the kernel times): device events around {args.reps} back-to-back eager calls, median of "
              f"{args.rounds} rounds; floor = 8 B per element at a float4 copy's 6.3 TB/s")
        g = torch.Generator(device=dev).manual_seed(1)
        ok = True
        for B in (args.batch, 2 * args.batch):
            R = args.res
            x = torch.rand((B, 1, R, R), generator=g, device=dev) * 2 - 1
            y = torch.empty_like(x)
            u = torch.rand((B, 8), generator=g, device=dev)
            table = torch.empty((B, 8), dtype=torch.float32, device=dev)
            ops.diffgeo_params(u, table, R, 24, 1.0)
            grid = F.affine_grid(grid_theta(table, R), list(x.shape), align_corners=True)
            xr = x.clone().requires_grad_()
            yt = F.grid_sample(xr, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
            worst = float((yt.detach() - ops.diffgeo(x, table)).abs().max())
            print(f"  ({B}, 1, {R}, {R}) largest |kernel - grid_sample| (fp32 both): {worst:.2e}")

            def torch_bwd(i):
                torch.autograd.grad(yt, xr, x, retain_graph=True)

            calls = {
                "fwd": (lambda i: pkg._C.call("ngan_diffgeo_fwd", x, table, y, B, 1, R, R, B, -1.0)),
                "torch fwd": (lambda i: F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)),
                "bwd": (lambda i: pkg._C.call("ngan_diffgeo_bwd", x, table, y, B, 1, R, R, B)),
                "torch bwd": torch_bwd,
            }
            med = {}
            floor_us = 8 * x.numel() / HBM_COPY * 1e6
            for name, fn in calls.items():
                timed(fn, 5)
                ts = [timed(fn, args.reps) * 1e3 for _ in range(args.rounds)]
                med[name] = statistics.median(ts)
                print(f"  ({B}, 1, {R}, {R}) {name:10s} median {med[name]:8.2f} us  min {min(ts):8.2f}  max {max(ts):8.2f}   floor {floor_us:6.2f} us "
                      f"= {floor_us / med[name]:5.2f} of the time")
            for k in ("fwd", "bwd"):
                verdict = "not slower than torch's" if med[k] <= med["torch " + k] else "SLOWER than torch's"
                ok = ok and med[k] <= med["torch " + k]
                print(f"  ({B}, 1, {R}, {R}) {k}: {med[k]:.2f} us against {med['torch ' + k]:.2f} us: {verdict} ({med['torch ' + k] / med[k]:.2f} x)")
        print("condition (neither launch slower than torch's): " + ("met" if ok else "NOT met"))

    # ---- 2. the replayed iteration, off and on ---------------------------------------------------------------------------------
    torch.manual_seed(123)
    pool = [(torch.rand(args.batch, 1, args.res, args.res) * 2 - 1).to(dev) for _ in range(4)]
    trainers = {}
    for form, policy in (("off", ""),) + (() if args.off_only else (("on", POLICY),)):
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
    print(f"  off spread (max - min over the rounds): {(max(times['off']) - min(times['off'])) * 1e3:.1f} us")
    if "on" in times:
        d = [b - a for a, b in zip(times["off"], times["on"])]
        print(f"  on - off per round: median {statistics.median(d) * 1e3:+.1f} us  min {min(d) * 1e3:+.1f}  max {max(d) * 1e3:+.1f}  "
              f"(three forward calls on b, 2 b and b samples, one adjoint on b, one parameter launch and its uniform draw)")
    for form, tr in trainers.items():
        for tag, flat in (("G", tr.flat_g), ("D", tr.flat_d)):
            assert bool(torch.isfinite(flat.flat).all()), (form, tag)


if __name__ == "__main__":
    main()
