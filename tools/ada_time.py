"""Cost of the adaptive augmentation probability (PGGANTrainer(ada_target > 0)) on one MI355X, in one process, by the protocol of
tools/simloss_time.py:
  (a) with `--parent DIR` (a checkout of the parent commit with its library built): the default-argument trainer of this tree against
      the parent's -- the graph-replayed iteration at the bench's headline configuration (512 x 512, batch 16, default widths, fp32,
      grad_pen_lambda 10), alternating rounds of `--steps` replays, device events around each round.  The condition is a median
      difference within the spread of the parent's own rounds.
  (b) `diffaug="color,translation,cutout"` at a fixed probability against the same policy with ada_target = 0.6, ada_interval = 4, in
      the same kind of rounds.  No number is fixed in advance; the expectation on record is one one-workgroup launch per critic step
      plus one one-thread launch every fourth iteration.  The difference is set beside the sum of the per-call times of the launches
      added per iteration.
  (c) PER-CALL times of each new entry point -- ngada_accumulate (both modes, 16 scores), ngada_update, ngada_diffaug_params and
      ngada_diffgeo_params (64 rows: the rows of an iteration at batch 16) -- beside the existing ngan_diffaug_params / ngan_diffgeo_params:
      device events around `--reps` back-to-back eager calls after a warm-up, median of `--rounds`.  A call cannot go faster than the
      host issues it: upper bounds on the kernel times.
  With `--bench`: `python bench.py --gpus 1 --steps 20 --warmup 5` on this tree and on the parent, each in a fresh child process before
  this process touches the GPU; their result lines go into the same file.
    python tools/ada_time.py --rounds 6 --steps 20 [--parent DIR] [--bench] --out profiles/ada_time.txt"""
import argparse
import importlib.util
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.abspath(os.path.join(__file__, os.pardir)))
sys.path.insert(0, ROOT)

POLICY = "color,translation,cutout"


def load_other(root, name):
    """the package of another checkout (`root`/neuron-gan_amd) under the module name `name`, with that checkout's library"""
    pkg_dir = os.path.join(root, "neuron-gan_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg_dir, "__init__.py"), submodule_search_locations=[pkg_dir])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    assert os.path.dirname(mod._C.LIB_PATH) == pkg_dir, mod._C.LIB_PATH
    return mod


def bench_line(root):
    """the JSON result line of bench.py in the checkout `root`, run in a fresh child process"""
    print(f"bench.py in {root} ...", flush=True)
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=root, capture_output=True,
                         text=True, timeout=900)
    rows = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode != 0 or not rows:
        raise SystemExit(f"bench.py in {root} failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
    return rows[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--parent", type=str, default="")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    bench_rows = []
    if args.bench:                                   # child processes first: this one has not touched the GPU yet
        bench_rows.append(("this tree", bench_line(ROOT)))
        if args.parent:
            bench_rows.append(("parent", bench_line(os.path.abspath(args.parent))))

    import torch
    from __graft_entry__ import load_package
    import bench
    if not torch.cuda.is_available():
        raise SystemExit("ada_time.py measures on a GPU; none found")
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
        return (f"  {tag:26s} median {statistics.median(ts):.4f}  min {min(ts):.4f}  max {max(ts):.4f}  rounds " + " ".join(f"{t:.4f}" for t in ts))

    torch.manual_seed(123)
    pool = [(torch.rand(args.batch, 1, args.res, args.res) * 2 - 1).to(dev) for _ in range(4)]

    def trainer(package, **kw):
        G, D = bench.build_nets(package, args.res, 1.0, dev)
        return package.train.PGGANTrainer(G, D, learning_rate=1e-4, beta1=0.5, grad_pen_lambda=10.0, drift_epsilon=0.001, device_latents=True, **kw)

    def rounds_of(trainers):
        for tr in trainers.values():
            for i in range(4):                   # the graphs exist before anything is timed
                tr.step(pool[i % len(pool)])
        times = {k: [] for k in trainers}
        for _ in range(args.rounds):
            for k, tr in trainers.items():
                times[k].append(timed(lambda i, tr=tr: tr.step(pool[i % len(pool)]), args.steps))
        for k, tr in trainers.items():
            assert bool(torch.isfinite(tr.flat_g.flat).all()) and bool(torch.isfinite(tr.flat_d.flat).all()), k
        return times

    say(f"replayed iteration, {args.res}x{args.res}, batch {args.batch}, fp32, one GPU, grad_pen_lambda 10: ms per iteration, "
        f"{args.rounds} alternating rounds of {args.steps} replays")
    # ---- (a) the default-argument trainer against the parent commit's ------------------------------------------------------------------
    spread_a = None
    if args.parent:
        parent = load_other(os.path.abspath(args.parent), "neuron_gan_amd_parent")
        parent.ops.set_conv_precision("f32")
        times = rounds_of({"parent": trainer(parent), "this tree, defaults": trainer(pkg)})
        say("(a) the default-argument trainer against the parent commit's, same rounds")
        for tag, ts in times.items():
            say(line(tag, ts))
        spread_a = max(times["parent"]) - min(times["parent"])
        d = [b - a for a, b in zip(times["parent"], times["this tree, defaults"])]
        say(f"  parent spread (max - min over the rounds): {spread_a * 1e3:.1f} us;  this tree - parent per round: median "
            f"{statistics.median(d) * 1e3:+.1f} us  min {min(d) * 1e3:+.1f}  max {max(d) * 1e3:+.1f}")
        say(f"  condition (the default-argument trainer times as the parent within the parent's own spread): "
            f"{'met' if abs(statistics.median(d)) <= spread_a else 'NOT met'}")

    # ---- (b) a fixed probability against the adaptive one -------------------------------------------------------------------------------
    fixed = trainer(pkg, diffaug=POLICY, diffaug_p=0.5)
    adaptive = trainer(pkg, diffaug=POLICY, ada_target=0.6, ada_interval=4, ada_kimg=500.0, ada_p_init=0.5)
    times = rounds_of({"diffaug, fixed p = 0.5": fixed, "diffaug, ada_target 0.6": adaptive})
    say(f"(b) diffaug={POLICY} at a fixed probability against the same policy with ada_target = 0.6, ada_interval = 4 (p starts at 0.5)")
    for tag, ts in times.items():
        say(line(tag, ts))
    d_b = [b - a for a, b in zip(times["diffaug, fixed p = 0.5"], times["diffaug, ada_target 0.6"])]
    spread_b = max(times["diffaug, fixed p = 0.5"]) - min(times["diffaug, fixed p = 0.5"])
    say(f"  adaptive - fixed per round: median {statistics.median(d_b) * 1e3:+.1f} us  min {min(d_b) * 1e3:+.1f}  max {max(d_b) * 1e3:+.1f};  "
        f"spread of the fixed-p rounds {spread_b * 1e3:.1f} us")
    torch.cuda.synchronize()
    say(f"  the controller after the run: counters {adaptive._ada.counters.tolist()}, p {adaptive._ada.p.tolist()}, "
        f"ada_iteration {adaptive.ada_iteration}")

    # ---- (c) the new launches per eager call -----------------------------------------------------------------------------------------
    say(f"(c) per-call times (upper bounds on the kernel times): device events around {args.reps} back-to-back eager calls, median of "
        f"{args.rounds} rounds")
    ops, B, rows = pkg.ops, args.batch, 4 * args.batch
    real, fake = torch.randn(B, device=dev), torch.randn(B, device=dev)
    counters, p = ops.ada_state(dev, 0.5)
    u = torch.rand(rows, 8, device=dev)
    table = ops.diffaug_table([ops.DIFFAUG_IDENTITY], dev).repeat(rows, 1).contiguous()
    geo = ops.diffgeo_table([ops.DIFFGEO_IDENTITY], dev).repeat(rows, 1).contiguous()
    calls = {"ngan_diffaug_params": lambda i: ops.diffaug_params(u, table, args.res, 7, 0.5),
             "ngada_diffaug_params": lambda i: ops.diffaug_params_live(u, table, args.res, 7, p),
             "ngan_diffgeo_params": lambda i: ops.diffgeo_params(u, geo, args.res, 24, 0.5),
             "ngada_diffgeo_params": lambda i: ops.diffgeo_params_live(u, geo, args.res, 24, p),
             "ngada_accumulate mode 1": lambda i: ops.ada_accumulate(real, fake, counters, ops.ADA_MODE_MIDPOINT),
             "ngada_accumulate mode 0": lambda i: ops.ada_accumulate(real, None, counters, ops.ADA_MODE_THRESHOLD, 0.5),
             "ngada_update": lambda i: ops.ada_update(counters, p, 0.6, 5e5, 1.0)}
    med = {}
    for name, fn in calls.items():
        timed(fn, 5)
        ts = [timed(fn, args.reps) * 1e3 for _ in range(args.rounds)]
        med[name] = statistics.median(ts)
        say(f"  {name:26s} median {med[name]:8.2f} us  min {min(ts):8.2f}  max {max(ts):8.2f}  spread {max(ts) - min(ts):6.2f}")
    added = med["ngada_accumulate mode 1"] + med["ngada_update"] / 4 + (med["ngada_diffaug_params"] - med["ngan_diffaug_params"])
    say(f"  launches (b) adds per iteration at n_critic = 1: one ngada_accumulate, a quarter of an ngada_update, and the live mapping in "
        f"place of the by-value one: {added:.2f} us by these per-call times")
    if spread_a is not None:
        excess = statistics.median(d_b) * 1e3 - spread_a * 1e3
        say(f"  (b)'s median difference less (a)'s spread: {excess:+.1f} us against {added:.2f} us of added launches: "
            f"{'within' if excess <= added else 'ABOVE -- to be explained before shipping'}")
    for tag, row in bench_rows:
        say(f"bench.py --gpus 1 --steps 20 --warmup 5, {tag}: {row}")
    say("not measured: whether adaptive augmentation improves samples on the micrographs (that needs the image folder and a long run, with "
        "MS-SSIM, SWD and the arbor scores as instruments); whether 0.6 is a sensible target for the midpoint statistic of a Wasserstein "
        "critic; kernel times proper (a kernel trace in a run of its own)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
