"""Cost of the generator's spectral regularisation (PGGANTrainer(spec_loss_lambda=)) on one MI355X, in one process, by the protocol of
tools/penalty_time.py:
  1. the graph-replayed iteration at the bench's headline configuration (512 x 512, batch 16, default widths, fp32, grad_pen_lambda 10)
     with spec_loss_lambda 1 against spec_loss_lambda 0 on this tree: alternating rounds of `--steps` replays, device events around
     each round.
  2. with `--parent DIR` (a checkout of the parent commit with its library built): the default-argument trainer of this tree against
     the parent's, alternating in the same rounds; the condition is a difference within the spread of the parent's own rounds.
  3. PER-CALL times at (batch, 1, 512, 512) of each new entry point -- ngan_specloss_fwd (three launches), ngan_specloss_head (one),
     ngan_specloss_bwd (two) -- against a plain-torch restatement on the same GPU: torch.fft.rfft2 of the windowed images and the ring
     means by index_add in fp32 (forward), the logarithm, square and mean (head), and autograd through both (backward).  Device events
     around `--reps` back-to-back eager calls after a warm-up, median of `--rounds`.  A call cannot go faster than the host issues it:
     upper bounds.  The condition is that no new entry point is slower than its restatement.
    python tools/specloss_time.py --rounds 6 --steps 20 [--parent DIR] > profiles/specloss_time.txt"""
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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--parent", type=str, default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("specloss_time.py measures on a GPU; none found")
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
    target = pkg.metrics.radial_spectrum(pkg.metrics.channels_last(torch.cat(pool)), True).mean(0)      # white noise: about 1/3 per bin

    def trainer(package, **kw):
        G, D = bench.build_nets(package, args.res, 1.0, dev)
        tr = package.train.PGGANTrainer(G, D, learning_rate=1e-4, beta1=0.5, grad_pen_lambda=10.0, drift_epsilon=0.001, device_latents=True, **kw)
        if kw.get("spec_loss_lambda"):
            tr.set_spectral_target(args.res, target)
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
    print(f"replayed iteration, {args.res}x{args.res}, batch {args.batch}, fp32, one GPU, grad_pen_lambda 10: ms per iteration, "
          f"{args.rounds} alternating rounds of {args.steps} replays")
    times = rounds_of({"spec_loss_lambda 0": trainer(pkg, spec_loss_lambda=0.0), "spec_loss_lambda 1": trainer(pkg, spec_loss_lambda=1.0)})
    for tag, ts in times.items():
        print(line(tag, ts))
    d = [b - a for a, b in zip(times["spec_loss_lambda 0"], times["spec_loss_lambda 1"])]
    print(f"  the term's cost per iteration (on - off per round): median {statistics.median(d) * 1e3:+.1f} us  min {min(d) * 1e3:+.1f}  "
          f"max {max(d) * 1e3:+.1f};  spread of the rounds without it {(max(times['spec_loss_lambda 0']) - min(times['spec_loss_lambda 0'])) * 1e3:.1f} us")

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

    # ---- 3. the new entry points against a plain-torch restatement -----------------------------------------------------------------------
    print(f"per-call times at ({args.batch}, 1, {args.res}, {args.res}) (upper bounds on the kernel times): device events around {args.reps} "
          f"back-to-back eager calls, median of {args.rounds} rounds")
    call, lib = pkg._C.call, pkg._C.lib()
    B, R = args.batch, args.res
    K, half = R // 2 + 1, R // 2
    x = pool[0]
    radial = torch.empty(B, K, device=dev, dtype=torch.float64)
    transform = torch.empty(B, K, R, 2, device=dev)
    ws_f = torch.empty(lib.ngan_specloss_fwd_workspace_bytes(B, R, 1) // 8, device=dev, dtype=torch.float64)
    ws_b = torch.empty(lib.ngan_specloss_bwd_workspace_bytes(B, R, 1) // 8, device=dev, dtype=torch.float64)
    per_image = torch.empty(B, device=dev, dtype=torch.float64)
    loss, one = torch.empty((), device=dev), torch.ones((), device=dev)
    c, coef = torch.empty(B, K, device=dev), torch.empty(B, K, device=dev)
    skipped = torch.empty(1, device=dev, dtype=torch.int32)
    grad, addend = torch.empty(B, 1, R, R, device=dev), torch.randn(B, 1, R, R, device=dev)
    # the restatement's constants: the window, the ring of every half-plane frequency with its Hermitian weight over n_k norm
    h = pkg.metrics.spectrum_window(R).to(dev)
    w = (h[:, None] * h[None, :])[None, None]
    norm = float((h.double() ** 2).sum() ** 2)
    f = torch.arange(R, device=dev)
    u = torch.where(f < half, f, f - R)[:, None].double()
    v = torch.arange(K, device=dev)[None, :].double()
    ring = torch.floor(torch.sqrt(u * u + v * v) + 0.5).long()
    keep = ring <= half
    ring = torch.where(keep, ring, torch.zeros_like(ring)).reshape(-1)
    herm = torch.where((torch.arange(K, device=dev) == 0) | (torch.arange(K, device=dev) == half), 1.0, 2.0)[None, :].expand(R, K)
    n_k = pkg.metrics.spectrum_ring_counts(R).to(dev).float()
    weight = (torch.where(keep, herm, torch.zeros_like(herm)).reshape(-1) / (n_k[ring] * norm)).float()
    t32 = target.float()

    def torch_forward(images):
        F = torch.fft.rfft2(images * w)
        P = (F.real * F.real + F.imag * F.imag).reshape(B, -1) * weight
        return torch.zeros(B, K, device=dev).index_add(1, ring, P)

    def torch_head(S):
        q = torch.log((S[:, 1:] / t32[1:] + 1e-3) / (1.0 + 1e-3))
        return (q * q).mean(1).sum() / B

    xg = x.clone().requires_grad_(True)
    state = {}

    def torch_backward(i):
        state["loss"] = torch_head(torch_forward(xg))
        (g,) = torch.autograd.grad(state["loss"], xg)
        state["grad"] = addend + g

    S_t = torch_forward(x)
    ring_norm = torch.empty(K, device=dev, dtype=torch.float64)
    calls = {"specloss_fwd": lambda i: call("ngan_specloss_fwd", x, radial, transform, ring_norm, ws_f, B, R, 1, 1),
             "torch forward": lambda i: torch_forward(x),
             "specloss_head": lambda i: call("ngan_specloss_head", radial, target, ring_norm, B, R, 1.0 / B, 1e-3, per_image, loss, c, coef, skipped),
             "torch head": lambda i: torch_head(S_t),
             "specloss_bwd": lambda i: call("ngan_specloss_bwd", transform, coef, one, addend, grad, ws_b, B, R, 1, 1),
             "torch fwd+head+bwd": torch_backward}
    per_call = {}
    for name, fn in calls.items():
        timed(fn, 5)
        ts = per_call[name] = [timed(fn, args.reps) * 1e3 for _ in range(args.rounds)]
        print(f"  {name:22s} median {statistics.median(ts):8.2f} us  min {min(ts):8.2f}  max {max(ts):8.2f}  spread {max(ts) - min(ts):6.2f}")
    med = {k: statistics.median(ts) for k, ts in per_call.items()}
    agree = float((radial.float() - S_t).abs().max() / S_t.abs().max())
    print(f"  (the two forwards agree to {agree:.1e} of the largest bin; the restatement works in fp32 throughout)")
    torch_bwd_alone = med["torch fwd+head+bwd"] - med["torch forward"] - med["torch head"]
    print(f"  torch backward alone (fwd+head+bwd minus its forward and head): {torch_bwd_alone:.2f} us")
    rows = (("specloss_fwd", med["specloss_fwd"], med["torch forward"]), ("specloss_head", med["specloss_head"], med["torch head"]),
            ("specloss_bwd", med["specloss_bwd"], torch_bwd_alone))
    slower = [name for name, mine, theirs in rows if mine > theirs]
    print(f"  condition (no new entry point slower than torch's restatement): {'NOT met: ' + ', '.join(slower) if slower else 'met'}")
    print("not measured: whether the term improves samples (that needs the micrograph folder and a long run, with the spectrum metric's "
          "high_db as the instrument); kernel times proper (a kernel trace in a run of its own)")


if __name__ == "__main__":
    main()
