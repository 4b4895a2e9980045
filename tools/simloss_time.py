"""Cost of the similarity loss on the generated images (PGGANTrainer(sim_loss_on="generated")) on one MI355X, in one process, by the
protocol of tools/specloss_time.py:
  1. the graph-replayed iteration at the bench's headline configuration (512 x 512, batch 16, default widths, fp32, grad_pen_lambda 10)
     with sim_loss_on="generated" (weight 0.5) against the default on this tree: alternating rounds of `--steps` replays, device
     events around each round.
  2. with `--parent DIR` (a checkout of the parent commit with its library built): the default-argument trainer of this tree against
     the parent's, alternating in the same rounds; the condition is a median difference within the spread of the parent's own rounds.
  3. PER-CALL times at (batch, 1, 512, 512) of each new entry point -- nganx_pair_gram (two launches, on the images),
     nganx_simloss_head (one) and nganx_pair_mix (one) -- against the reference's own similarity_loss (utils.similarity_loss: two norm
     divisions, two matmuls, the squared difference) and its autograd backward in plain torch on the same GPU.  Device events around
     `--reps` back-to-back eager calls after a warm-up, median of `--rounds`.  A call cannot go faster than the host issues it: upper
     bounds.  The condition is that no new entry point is slower than the torch pass it replaces, with the share of the byte floor
     (forward reads B N 4 bytes; backward reads the same plus the addend and writes B N 4 bytes) at 8 TB/s beside it.
    python tools/simloss_time.py --rounds 6 --steps 20 [--parent DIR] --out profiles/simloss_time.txt"""
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

HBM_PEAK = 8.0e12       # bytes per second


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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--parent", type=str, default="")
    ap.add_argument("--out", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("simloss_time.py measures on a GPU; none found")
    pkg = load_package()
    dev = torch.device("cuda:0")
    pkg.ops.set_conv_precision("f32")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

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
        tr = package.train.PGGANTrainer(G, D, learning_rate=1e-4, beta1=0.5, grad_pen_lambda=10.0, drift_epsilon=0.001, device_latents=True, **kw)
        if kw.get("sim_loss_on") == "generated":
            tr.set_sim_lambda(0.5)
        return tr

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

    # ---- 1. the term on against the term off ---------------------------------------------------------------------------------------------
    say(f"replayed iteration, {args.res}x{args.res}, batch {args.batch}, fp32, one GPU, grad_pen_lambda 10: ms per iteration, "
        f"{args.rounds} alternating rounds of {args.steps} replays")
    times = rounds_of({"sim_loss_on real": trainer(pkg), "sim_loss_on generated": trainer(pkg, sim_loss_on="generated", sim_loss_center=True)})
    for tag, ts in times.items():
        say(line(tag, ts))
    d = [b - a for a, b in zip(times["sim_loss_on real"], times["sim_loss_on generated"])]
    say(f"  the term's cost per iteration (on - off per round): median {statistics.median(d) * 1e3:+.1f} us  min {min(d) * 1e3:+.1f}  "
        f"max {max(d) * 1e3:+.1f};  spread of the rounds without it {(max(times['sim_loss_on real']) - min(times['sim_loss_on real'])) * 1e3:.1f} us")

    # ---- 2. the default-argument trainer against the parent commit's ---------------------------------------------------------------------
    if args.parent:
        parent = load_other(os.path.abspath(args.parent), "neuron_gan_amd_parent")
        parent.ops.set_conv_precision("f32")
        times = rounds_of({"parent": trainer(parent), "this tree, defaults": trainer(pkg)})
        say("the default-argument trainer against the parent commit's, same rounds")
        for tag, ts in times.items():
            say(line(tag, ts))
        spread = max(times["parent"]) - min(times["parent"])
        d = [b - a for a, b in zip(times["parent"], times["this tree, defaults"])]
        say(f"  parent spread (max - min over the rounds): {spread * 1e3:.1f} us;  this tree - parent per round: median "
            f"{statistics.median(d) * 1e3:+.1f} us  min {min(d) * 1e3:+.1f}  max {max(d) * 1e3:+.1f}")
        say(f"  condition (the default-argument trainer times as the parent within the parent's own spread): "
            f"{'met' if abs(statistics.median(d)) <= spread else 'NOT met'}")

    # ---- 3. the new entry points against the reference's similarity_loss in plain torch --------------------------------------------------
    say(f"per-call times at ({args.batch}, 1, {args.res}, {args.res}) (upper bounds on the kernel times): device events around {args.reps} "
        f"back-to-back eager calls, median of {args.rounds} rounds")
    call, lib = pkg._C.call, pkg._C.lib()
    B, N = args.batch, args.res * args.res
    x = pool[0].view(B, N)
    z = pkg.utils.sample_latent_vec((B, 512), seed=5).to(dev)
    gx, sx = torch.empty(B, B, device=dev, dtype=torch.float64), torch.empty(B, device=dev, dtype=torch.float64)
    gz, sz = pkg.ops.pair_gram(z)
    ws_z = torch.empty(lib.nganx_pair_gram_workspace_bytes(B, 512) // 8, device=dev, dtype=torch.float64)
    ws = torch.empty(lib.nganx_pair_gram_workspace_bytes(B, N) // 8, device=dev, dtype=torch.float64)
    lam, one = torch.full((), 0.5, device=dev), torch.ones((), device=dev)
    loss, sim = torch.empty((), device=dev), torch.empty(B, B, device=dev, dtype=torch.float64)
    mix, shift = torch.empty(B, B, device=dev), torch.empty(B, device=dev)
    grad, addend = torch.empty(B, N, device=dev), torch.randn(B, N, device=dev)
    xg = x.clone().requires_grad_(True)
    state = {}

    def torch_both(i):
        state["loss"] = pkg.utils.similarity_loss(xg, z, 0.5)
        (g,) = torch.autograd.grad(state["loss"], xg)
        state["grad"] = addend + g

    calls = {"pair_gram (images)": lambda i: call("nganx_pair_gram", x, gx, sx, ws, B, N),
             "pair_gram (latents)": lambda i: call("nganx_pair_gram", z, gz, sz, ws_z, B, 512),
             "simloss_head": lambda i: call("nganx_simloss_head", gx, sx, gz, lam, B, N, 0, loss, sim, mix, shift),
             "torch similarity_loss": lambda i: pkg.utils.similarity_loss(x, z, 0.5),
             "pair_mix": lambda i: call("nganx_pair_mix", x, mix, shift, one, addend, grad, B, N),
             "torch fwd+bwd": torch_both}
    per_call = {}
    for name, fn in calls.items():
        timed(fn, 5)
        ts = per_call[name] = [timed(fn, args.reps) * 1e3 for _ in range(args.rounds)]
        say(f"  {name:26s} median {statistics.median(ts):8.2f} us  min {min(ts):8.2f}  max {max(ts):8.2f}  spread {max(ts) - min(ts):6.2f}")
    med = {k: statistics.median(ts) for k, ts in per_call.items()}
    torch_both(0)
    agree_l = abs(float(loss) - float(state["loss"])) / abs(float(state["loss"]))
    agree_g = float((grad - state["grad"]).abs().max() / state["grad"].abs().max())
    say(f"  (the two losses agree to {agree_l:.1e} relative, the two gradients to {agree_g:.1e} of the largest element; torch works in fp32)")
    torch_bwd = med["torch fwd+bwd"] - med["torch similarity_loss"]
    say(f"  torch backward alone (fwd+bwd minus its forward): {torch_bwd:.2f} us")
    floor_f, floor_b = B * N * 4 / HBM_PEAK * 1e6, 3 * B * N * 4 / HBM_PEAK * 1e6
    say(f"  byte floor at 8 TB/s: forward {floor_f:.2f} us ({B * N * 4 / 1e6:.1f} MB read) -> pair_gram runs at {floor_f / med['pair_gram (images)']:.3f} of it;  "
        f"backward {floor_b:.2f} us ({3 * B * N * 4 / 1e6:.1f} MB) -> pair_mix runs at {floor_b / med['pair_mix']:.3f} of it")
    rows = (("pair_gram", med["pair_gram (images)"], med["torch similarity_loss"]), ("simloss_head", med["simloss_head"], med["torch similarity_loss"]),
            ("the whole forward (both pair_gram calls + simloss_head)", med["pair_gram (images)"] + med["pair_gram (latents)"] + med["simloss_head"],
             med["torch similarity_loss"]), ("pair_mix", med["pair_mix"], torch_bwd))
    slower = [name for name, mine, theirs in rows if mine > theirs]
    say(f"  condition (no new entry point slower than the torch pass it replaces): {'NOT met: ' + ', '.join(slower) if slower else 'met'}")
    say("not measured: whether either form of the term (raw or centred) improves samples (that needs the micrograph folder and a long "
        "run, with MS-SSIM as the instrument); kernel times proper (a kernel trace in a run of its own)")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
