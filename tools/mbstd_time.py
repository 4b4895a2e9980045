"""Cost of the critic's minibatch standard-deviation channel (Discriminator_PG(mbstd_group=4)) against the default critic on one MI355X,
in one process, on the same commit:
  1. the graph-replayed iteration at the bench's headline configuration (512 x 512, batch 16, default widths, fp32, grad_pen_lambda
     10), with mbstd_group 4 and 0: alternating rounds of `--steps` replays, device events around each round; the spread of the off
     rounds goes alongside.  The head then runs unfused (Conv, StdFieldAdd, LReLUPN) and the statistic adds its launches in each of the
     critic's passes: a few tens of launches on tensors of at most 32 x 16 x 16 x 128 floats, bound by latency.
  2. PER-CALL times of every new launch at the head's shapes (the critic pass's 2 x 16 samples in two segments, and the penalty /
     generator passes' 16), each next to a plain-torch restatement of the same operator on the same GPU: device events around `--reps`
     back-to-back eager calls after a warm-up, median of `--rounds`.  A call cannot go faster than the host issues it, so these are
     upper bounds on the kernel times; torch's restatements are several launches each and are timed the same way.
    python tools/mbstd_time.py --rounds 6 --steps 20 > profiles/mbstd_time.txt"""
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
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mbstd_time.py measures on a GPU; none found")
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

    # ---- 1. the replayed iteration with and without the channel ------------------------------------------------------------------------
    torch.manual_seed(123)
    pool = [(torch.rand(args.batch, 1, args.res, args.res) * 2 - 1).to(dev) for _ in range(4)]
    trainers = {}
    for group in (0, 4):
        G, _ = bench.build_nets(pkg, args.res, 1.0, dev)
        torch.manual_seed(2)
        D = pkg.models.Discriminator_PG(bench.D_WIDTHS, image_size_init=16, mbstd_group=group)
        D.set_resolution(args.res, 1.0)
        tr = pkg.train.PGGANTrainer(G, D.to(dev), learning_rate=1e-4, beta1=0.5, grad_pen_lambda=10.0, drift_epsilon=0.001, device_latents=True)
        tr.capture(pool[0], warmup=2)
        trainers[group] = tr
    times = {k: [] for k in trainers}
    for _ in range(args.rounds):
        for group, tr in trainers.items():
            tr.replay(pool[0])
            times[group].append(timed(lambda i, tr=tr: tr.replay(pool[i % len(pool)]), args.steps))
    print(f"replayed iteration, {args.res}x{args.res}, batch {args.batch}, fp32, one GPU, grad_pen_lambda 10: ms per iteration, "
          f"{args.rounds} alternating rounds of {args.steps} replays")
    for group, ts in times.items():
        print(f"  mbstd_group {group}  median {statistics.median(ts):.4f}  min {min(ts):.4f}  max {max(ts):.4f}  rounds " + " ".join(f"{t:.4f}" for t in ts))
    d = [b - a for a, b in zip(times[0], times[4])]
    print(f"  off spread (max - min over the rounds): {(max(times[0]) - min(times[0])) * 1e3:.1f} us")
    print(f"  on - off per round: median {statistics.median(d) * 1e3:+.1f} us  min {min(d) * 1e3:+.1f}  max {max(d) * 1e3:+.1f}")
    for group, tr in trainers.items():
        for tag, flat in (("G", tr.flat_g), ("D", tr.flat_d)):
            assert bool(torch.isfinite(flat.flat).all()), (group, tag)
    del trainers

    # ---- 2. the launches alone, each against torch's restatement ----------------------------------------------------------------------
    print(f"per-call times (upper bounds on the kernel times): device events around {args.reps} back-to-back eager calls, median of "
          f"{args.rounds} rounds; hip / torch in us")
    call = pkg._C.call
    gen = torch.Generator(device=dev).manual_seed(1)
    hh, ch, scale, eps = 16, bench.D_WIDTHS[-1], 0.05, 1e-8
    for b, seg in ((2 * args.batch, 2), (args.batch, 1)):
        ge = pkg.ops.mbstd_group_size(b // seg, 4)
        x, h, c, g = (torch.randn(b, hh, hh, ch, generator=gen, device=dev) for _ in range(4))
        gs, s = torch.randn(b, generator=gen, device=dev), torch.rand(b, generator=gen, device=dev)
        w_std = torch.randn(ch, 1, 3, 3, generator=gen, device=dev)
        ws = torch.empty(pkg._C.mbstd_workspace_doubles(b, hh, hh, ch, ge), device=dev, dtype=torch.float64)
        so, dgs, gso = (torch.empty(b, device=dev) for _ in range(3))
        gx, dx, out = (torch.empty_like(x) for _ in range(3))
        gw = torch.empty_like(w_std)
        J = hh * hh * ch
        ones = torch.ones(1, 1, hh, hh, device=dev)
        # (3, 3, H, W): 1 where tap (ky, kx) at (y, x) reads a pixel inside the image
        masks = torch.stack([torch.stack([torch.nn.functional.pad(ones[0, 0], (1, 1, 1, 1))[ky:ky + hh, kx:kx + hh] for kx in range(3)])
                             for ky in range(3)])

        def stats():
            xg = x.reshape(b // ge, ge, J)
            d = xg - xg.mean(1, keepdim=True)
            return d, torch.sqrt((d * d).mean(1, keepdim=True) + eps)

        def t_fwd(i):
            return stats()[1].mean((1, 2)).repeat_interleave(ge)

        def t_bwd(i):
            d, sigma = stats()
            return (gs.reshape(-1, ge, 1).sum(1, keepdim=True) / (ge * J)) * d / sigma

        def t_bwdbwd(i):
            d, sigma = stats()
            hg = h.reshape(b // ge, ge, J)
            coef = gs.reshape(-1, ge, 1).sum(1, keepdim=True) / (ge * J)
            hd = (hg * d).sum(1, keepdim=True)
            return (hd / sigma).sum((1, 2)) / (ge * J), coef * ((hg - hg.mean(1, keepdim=True)) / sigma - d * hd / (ge * sigma ** 3))

        def field():           # T (1, H, W, C): the constant plane through the zero-padded conv
            return torch.nn.functional.conv2d(ones, w_std, padding=1).permute(0, 2, 3, 1)

        pairs = {
            "mbstd_fwd": (lambda i: call("ngan_mbstd_fwd", x, so, ws, b, hh, hh, ch, seg, ge), t_fwd),
            "mbstd_bwd": (lambda i: call("ngan_mbstd_bwd", gs, x, gx, b, hh, hh, ch, seg, ge), t_bwd),
            "mbstd_bwdbwd": (lambda i: call("ngan_mbstd_bwdbwd", h, gs, x, dgs, dx, ws, b, hh, hh, ch, seg, ge), t_bwdbwd),
            "stdfield_add": (lambda i: call("ngan_stdfield_add", c, s, w_std, out, b, hh, hh, ch, scale),
                             lambda i: c + (scale * s)[:, None, None, None] * field()),
            "stdfield_ds": (lambda i: call("ngan_stdfield_ds", g, w_std, gso, b, hh, hh, ch, scale), lambda i: scale * (g * field()).sum((1, 2, 3))),
            "stdfield_dw": (lambda i: call("ngan_stdfield_dw", g, s, gw, b, hh, hh, ch, scale),
                            lambda i: scale * torch.einsum("nyxc,ijyx->cij", s[:, None, None, None] * g, masks)),
        }
        for name, (hip, ref) in pairs.items():
            row = []
            for fn in (hip, ref):
                timed(fn, 5)
                ts = [timed(fn, args.reps) * 1e3 for _ in range(args.rounds)]
                row.append(statistics.median(ts))
            verdict = "" if row[0] <= row[1] else f"   SLOWER than torch's restatement by {row[0] - row[1]:.2f} us"
            print(f"  B {b:3d} segments {seg} G_eff {ge} {hh}x{hh}x{ch}  {name:13s} hip {row[0]:8.2f}  torch {row[1]:8.2f}{verdict}")


if __name__ == "__main__":
    main()
