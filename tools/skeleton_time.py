"""Time the arbor-skeleton metric on one GPU.  Without a data folder the inputs are the micrograph-like fields of
tests/multiotsu_ref.py (64 seeds at 512 x 512, mapped to [-1, 1]); the report says so.

  1. `thin` alone (with and without writing the skeleton) and all of `skeleton_statistics` for 64 images at 512 x 512 through the
     kernels, next to a plain-torch restatement of the same sweeps on the same GPU (the eight neighbour planes as shifted views of a
     padded boolean tensor, both sub-iterations, one host read-back per pair for "until nothing changes"; the counts from the same
     planes), with the bytes the thinning has to move at least -- one mask read and one skeleton write -- over the measured time, and
     the pass counts seen;
  2. the metric's own work in one evaluation at the default setting: 8192 images per side in minibatches of 64, i.e. 256 calls of
     `skeleton_statistics` and one `Skeleton.result()`;
  3. `evaluate_skeleton` itself at that setting with an untrained generator and a synthetic data set, as tools/morph_time.py does.

HIP events, three warm calls, the median of --runs runs.  A record, not a gate.

    python tools/skeleton_time.py [--images 8192] [--runs 3] [--out profiles/skeleton_time.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import multiotsu_ref as OT  # noqa: E402

pkg = g.load_package()
M = pkg.metrics
DEV = torch.device("cuda:0")
parser = argparse.ArgumentParser()
parser.add_argument("--images", type=int, default=8192)
parser.add_argument("--runs", type=int, default=3)
parser.add_argument("--out", type=str, default="")
ARGS = parser.parse_args()
R, BATCH, RUNS = 512, 64, ARGS.runs
PEAK = 5e12                                          # bytes / s the floor is taken against


def timed(fn, reps=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / reps)
    return statistics.median(times)


# ---- the plain-torch restatement ---------------------------------------------------------------------------------------------------------
def ring(m):
    """P2 .. P9 of a boolean (B, R, R) tensor, background outside"""
    p = F.pad(m, (1, 1, 1, 1))
    at = lambda dy, dx: p[:, 1 + dy:1 + dy + R, 1 + dx:1 + dx + R]   # noqa: E731
    return at(-1, 0), at(-1, 1), at(0, 1), at(1, 1), at(1, 0), at(1, -1), at(0, -1), at(-1, -1)


def torch_thin(mask):
    """(skeleton bool, sub-iterations run for the whole batch): Guo-Hall A1 on every image at once"""
    m = mask != 0
    i8 = lambda b: b.to(torch.int8)   # noqa: E731
    passes = 0
    while True:
        before = m
        for sub in (0, 1):
            P2, P3, P4, P5, P6, P7, P8, P9 = ring(m)
            C = i8(~P2 & (P3 | P4)) + i8(~P4 & (P5 | P6)) + i8(~P6 & (P7 | P8)) + i8(~P8 & (P9 | P2))
            N1 = i8(P9 | P2) + i8(P3 | P4) + i8(P5 | P6) + i8(P7 | P8)
            N2 = i8(P2 | P3) + i8(P4 | P5) + i8(P6 | P7) + i8(P8 | P9)
            N = torch.minimum(N1, N2)
            side = ((P2 | P3 | ~P5) & P4) if sub == 0 else ((P6 | P7 | ~P9) & P8)
            m = m & ~((C == 1) & (N >= 2) & (N <= 3) & ~side)
            passes += 1
        if torch.equal(m, before):                   # one host read-back per pair
            return m, passes


def torch_counts(m):
    """(B, 6) int64 {pixels, tips, junctions, isolated, orth, diag} of a boolean (B, R, R) tensor"""
    r = ring(m)
    P2, P3, P4, P5, P6, P7, P8, P9 = r
    B = sum(x.to(torch.int8) for x in r)
    X = sum((~r[k] & r[(k + 1) % 8]).to(torch.int8) for k in range(8))
    n = lambda b: b.sum((1, 2))   # noqa: E731
    return torch.stack([n(m), n(m & (X == 1) & (B <= 2)), n(m & (X >= 3)), n(m & (B == 0)), n(m & P4) + n(m & P6),
                        n(m & P5 & ~P4 & ~P6) + n(m & P7 & ~P8 & ~P6)], 1)


def torch_skeleton_statistics(x):
    """skeleton_statistics with the thinning in plain torch and the front end through the kernels (tools/morph_time.py times that)"""
    r, ok, stats, kept = M._kept_mask(x, 1, 1, None)
    sk, _ = torch_thin(kept)
    s, k = torch_counts(sk).double(), stats.double()
    return {"length": (s[:, 4] + 2.0 ** 0.5 * s[:, 5]) / r, "tips": s[:, 1], "junctions": s[:, 2], "width": k[:, 3] / s[:, 0]}


def main():
    out = []
    t0 = time.time()
    img = np.stack([OT.micrograph(seed, R) for seed in range(BATCH)])
    x = torch.from_numpy((img.astype(np.float64) / 127.5 - 1.0).astype(np.float32)[..., None]).to(DEV)
    print(f"{BATCH} micrograph fields in {time.time() - t0:.1f} s", flush=True)
    _, _, _, kept = M._kept_mask(x, 1, 1, None)
    skeleton, stats = M.thin(kept)
    tsk, tpasses = torch_thin(kept)
    agree = {"skeleton": torch.equal(tsk.to(torch.uint8), skeleton), "counts": torch.equal(torch_counts(tsk), stats[:, :6].long()),
             "pass count (the batch's largest)": tpasses == int(stats[:, 6].max())}
    s = stats.double().mean(0).tolist()
    passes = stats[:, 6].tolist()
    out.append(f"input: {BATCH} micrograph-like fields of tests/multiotsu_ref.py (seeds 0 .. {BATCH - 1}) at {R} x {R}, mapped to [-1, 1]; no data "
               f"folder on this machine.  Per image on average: kept mask {s[7]:.0f} pixels ({100 * s[7] / R / R:.1f} %), skeleton {s[0]:.0f} "
               f"pixels, {s[1]:.1f} tips, {s[2]:.1f} junctions, {s[3]:.1f} isolated, width {s[7] / max(s[0], 1):.2f}")
    out.append(f"passes (sub-iterations, the last empty pair included): min {min(passes)}, median {statistics.median(passes):.0f}, max {max(passes)}")
    out.append("the torch restatement gives the same " + ", ".join(k for k, v in agree.items() if v)
               + ("; it DIFFERS in " + ", ".join(k for k, v in agree.items() if not v) if not all(agree.values()) else ""))
    px = BATCH * R * R
    stages = [
        ("thin, skeleton written", lambda: M.thin(kept), lambda: torch_thin(kept), px * 2, "1 B read, 1 B written per pixel"),
        ("thin, stats only", lambda: M.thin(kept, want_skeleton=False), None, px, "1 B read"),
        ("skeleton_counts", lambda: M.skeleton_counts(skeleton), lambda: torch_counts(tsk), px, "1 B read"),
        ("arbor front end (existing)", lambda: M._kept_mask(x, 1, 1, None), None, 0, ""),
        ("skeleton_statistics (all)", lambda: M.skeleton_statistics(x), lambda: torch_skeleton_statistics(x), px * (4 + 1 + 2 + 5 + 1),
         "the front end's bytes and 1 B read"),
    ]
    out.append("")
    out.append(f"stages, {BATCH} images at {R} x {R}; MI355X, HIP events, median of {RUNS} x 10 calls, ms; floor = least bytes / 5 TB/s")
    out.append(f"{'stage':<28}{'kernels':>10}{'torch':>10}{'torch / kernels':>17}{'MB':>9}{'floor':>9}{'floor / kernels':>17}  least traffic")
    slower = []
    for name, fn, tfn, nbytes, what in stages:
        a = timed(fn)
        b = timed(tfn, reps=2) if tfn is not None else None
        floor = nbytes / PEAK * 1e3
        out.append(f"{name:<28}{a:>10.4f}" + (f"{b:>10.4f}{b / a:>17.1f}" if b is not None else f"{'-':>10}{'-':>17}")
                   + (f"{nbytes / 1e6:>9.1f}{floor:>9.4f}{floor / a:>17.3f}  {what}" if nbytes else ""))
        if b is not None and a > b:
            slower.append(name)
        print(out[-1], flush=True)
    out.append(f"(torch's thinning ran {tpasses} sub-iterations for the whole batch, with one host read-back per pair; the kernel stops each "
               f"image on its own)")
    out.append("no stage is slower than torch's" if not slower else "SLOWER than torch: " + ", ".join(slower))

    n_batches = (ARGS.images + BATCH - 1) // BATCH

    def metric_alone():
        m = M.Skeleton(R, device=DEV)
        for _ in range(n_batches):
            m.feed("real", x)
            m.feed("fake", x)
        return m.result()
    t = timed(metric_alone, reps=1)
    out.append("")
    out.append(f"the metric's own work in one evaluation at the default setting ({ARGS.images} images per side, minibatches of {BATCH}: "
               f"{2 * n_batches} calls of skeleton_statistics and one result(); every call is fed the same {BATCH} fields above, on both "
               f"sides, not {ARGS.images} distinct images): {t:.1f} ms")

    torch.manual_seed(1)
    G = pkg.models.Generator_PG([128, 64, 32, 32, 16, 16], image_size_init=16).to(DEV)
    G.set_resolution(R, 1.0)
    data = pkg.data.NeuronDataset(torch.from_numpy(img[:, None].astype(np.float32) / 255.0), augmentations=True, im_translation=0.05,
                                  device=DEV, seed=3)
    res = {}

    def whole():
        res["r"], res["m"] = M.evaluate_skeleton(G, data, n_images=ARGS.images, batch_size=BATCH, return_metric=True)
    t2 = timed(whole, reps=1)
    out.append(f"evaluate_skeleton at that setting, untrained generator, the same fields as the data set through its augmentation chain: "
               f"{t2:.1f} ms (the metric's share {100 * t / t2:.0f} %)")
    out.append(M.format_skeleton(res["r"], "its table"))
    text = "\n".join(out)
    print(text)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
