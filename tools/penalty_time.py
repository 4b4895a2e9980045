"""Cost of the penalty's forms and of lazy regularisation (PGGANTrainer(grad_pen_mode=, grad_pen_interval=)) on one MI355X, in one
process, by the protocol of tools/lsgan_time.py:
  1. the graph-replayed iteration at the bench's headline configuration (512 x 512, batch 16, default widths, fp32, grad_pen_lambda 10)
     for modes gp, lp and r1 at intervals 1, 4 and 16: alternating rounds of `--steps` replays, device events around each round (an
     interval above 1 replays the due and the other graphs in their schedule, so a round of 20 holds 5 due iterations at interval 4 and
     1 or 2 at interval 16).  Expected, from the README's two figures t1 (lambda 10) and t0 (lambda 0): gp at interval k near
     (t1 + (k - 1) t0) / k; r1 at interval 1 below gp by one generator pass on the batch and the interpolate's launch.
  2. with `--parent DIR` (a checkout of the parent commit with its library built): the default-argument trainer of this tree against
     the parent's, alternating in the same rounds; the condition is a difference within the spread of the parent's own rounds.
  3. PER-CALL times at (batch, 1, 512, 512) of ngan_penalty_head against the ngan_sample_l2norm + ngan_gp_head chain and of
     ngan_penalty_bwd against ngan_gp_coef + ngan_scale_rows: device events around `--reps` back-to-back eager calls after a warm-up,
     median of `--rounds`, with each chain's spread (max - min).  A call cannot go faster than the host issues it: upper bounds.
    python tools/penalty_time.py --rounds 6 --steps 20 [--parent DIR] > profiles/penalty_time.txt"""
import argparse
import importlib.util
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(os.path.join(__file__, os.pardir)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402
import bench  # noqa: E402


def load_other(root, name):
    """the package of another checkout (`root`/neuron-gan_amd) under the module name `name`, with that checkout's library"""
    pkg_dir = os.path.join(root, "neuron-gan_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    assert os.path.dirname(mod._C.LIB_PATH) == pkg_dir, mod._C.LIB_PATH
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=1000)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--parent", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("penalty_time.py measures on a GPU; none found")
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

    def line(tag, ts):
        return (f"  {tag:22s} median {statistics.median(ts):.4f}  min {min(ts):.4f}  max {max(ts):.4f}  rounds " + " ".join(f"{t:.4f}" for t in ts))

    torch.manual_seed(123)
    pool = [(torch.rand(args.batch, 1, args.res, args.res) * 2 - 1).to(dev) for _ in range(4)]

    def trainer(package, **kw):
        G, D = bench.build_nets(package, args.res, 1.0, dev)
        return package.train.PGGANTrainer(G, D, learning_rate=1e-4, beta1=0.5, grad_pen_lambda=10.0, drift_epsilon=0.001, device_latents=True, **kw)

    def rounds_of(trainers):
        for tr in trainers.values():
            for i in range(2 * getattr(tr, "grad_pen_interval", 1) + 2):       # every phase's graphs exist before anything is timed
                tr.step(pool[i % len(pool)])
        times = {k: [] for k in trainers}
        for _ in range(args.rounds):
            for k, tr in trainers.items():
                times[k].append(timed(lambda i, tr=tr: tr.step(pool[i % len(pool)]), args.steps))
        for k, tr in trainers.items():
            assert bool(torch.isfinite(tr.flat_g.flat).all()) and bool(torch.isfinite(tr.flat_d.flat).all()), k
        return times

    # ---- 1. modes and intervals --------------------------------------------------------------------------------------------------------
    print(f"replayed iteration, {args.res}x{args.res}, batch {args.batch}, fp32, one GPU, grad_pen_lambda 10: ms per iteration, "
          f"{args.rounds} alternating rounds of {args.steps} replays")
    for k in (1, 4, 16):
        times = rounds_of({mode: trainer(pkg, grad_pen_mode=mode, grad_pen_interval=k) for mode in ("gp", "lp", "r1")})
        print(f" grad_pen_interval {k}")
        for mode, ts in times.items():
            print(line(mode, ts))
        if k == 1:
            d = [b - a for a, b in zip(times["gp"], times["r1"])]
            print(f"  gp spread (max - min over the rounds): {(max(times['gp']) - min(times['gp'])) * 1e3:.1f} us;  r1 - gp per round: median "
                  f"{statistics.median(d) * 1e3:+.1f} us  min {min(d) * 1e3:+.1f}  max {max(d) * 1e3:+.1f}")

    # ---- 2. the default-argument trainer against the parent commit's ---------------------------------------------------------------------
    if args.parent:
        parent = load_other(os.path.abspath(args.parent), "neuron_gan_amd_parent")
        parent.ops.set_conv_precision("f32")
        times = rounds_of({"parent": trainer(parent), "this tree, defaults": trainer(pkg)})
        print("the default-argument trainer against the parent commit's, same rounds")
        for tag, ts in times.items():
            print(line(tag, ts))
        spread = max(times["parent"]) - min(times["parent"])
        d = [b - a for a, b in zip(times["parent"], times["this tree, defaults"])]
        print(f"  parent spread (max - min over the rounds): {spread * 1e3:.1f} us;  this tree - parent per round: median "
              f"{statistics.median(d) * 1e3:+.1f} us  min {min(d) * 1e3:+.1f}  max {max(d) * 1e3:+.1f}")
        print(f"  condition (the default-argument trainer times as the parent within the parent's own spread): "
              f"{'met' if abs(statistics.median(d)) <= spread else 'NOT met'}")

    # ---- 3. the fused launches against the chains they stand beside ----------------------------------------------------------------------
    print(f"per-call times at ({args.batch}, 1, {args.res}, {args.res}) (upper bounds on the kernel times): device events around {args.reps} "
          f"back-to-back eager calls, median of {args.rounds} rounds")
    call = pkg._C.call
    B, n = args.batch, args.res * args.res
    gen = torch.Generator(device=dev).manual_seed(1)
    g = torch.randn(B, n, generator=gen, device=dev) * (2.0 / n ** 0.5)          # norms near 2: every row of form 1 is live
    norms, ws, coef = torch.empty(B, device=dev), torch.empty(64 * B, device=dev), torch.empty(B, device=dev)
    out1, one, grad = torch.empty((), device=dev), torch.ones((), device=dev), torch.empty_like(g)

    def chain_head(i):
        call("ngan_sample_l2norm", g, norms, ws, B, n)
        call("ngan_gp_head", norms, B, 10.0, out1)

    def chain_bwd(i):
        call("ngan_gp_coef", norms, B, 10.0, one, coef)
        call("ngan_scale_rows", g, coef, grad, B, n)

    calls = {"l2norm + gp_head": chain_head, "gp_coef + scale_rows": chain_bwd}
    for form in (1, 2):
        calls[f"penalty_head form {form}"] = lambda i, form=form: call("ngan_penalty_head", g, B, n, form, 10.0, ws, norms, out1)
        calls[f"penalty_bwd form {form}"] = lambda i, form=form: call("ngan_penalty_bwd", g, norms, B, n, form, 10.0, one, grad)
    per_call = {}
    for name, fn in calls.items():
        timed(fn, 5)
        ts = per_call[name] = [timed(fn, args.reps) * 1e3 for _ in range(args.rounds)]
        print(f"  {name:22s} median {statistics.median(ts):7.2f} us  min {min(ts):7.2f}  max {max(ts):7.2f}  spread {max(ts) - min(ts):6.2f}")
    for fused, chain in (("penalty_head", "l2norm + gp_head"), ("penalty_bwd", "gp_coef + scale_rows")):
        limit = statistics.median(per_call[chain]) + max(per_call[chain]) - min(per_call[chain])
        slower = [f for f in per_call if f.startswith(fused) and statistics.median(per_call[f]) > limit]
        print(f"  condition ({fused} no slower than {chain} by more than that chain's spread): {'NOT met: ' + ', '.join(slower) if slower else 'met'}")
    print("not measured: whether any mode or interval samples better (that needs the micrograph folder and a long run; the seven checkpoint "
          "metrics are the instruments); kernel times proper (a kernel trace in a run of its own)")


if __name__ == "__main__":
    main()
