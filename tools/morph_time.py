"""Time the arbor-morphology metric on one GPU.  Without a data folder the inputs are the micrograph-like fields of
tests/multiotsu_ref.py (64 seeds at 512 x 512, mapped to [-1, 1]); the report says so.

  1. every stage for 64 images at 512 x 512 through the kernels of csrc/morph.hip, next to a plain-torch restatement on the same GPU
     (levels by the same arithmetic and a one-hot histogram; labels by iterated 3 x 3 max-pool propagation of the pixel index until
     nothing changes, which converges to the largest index of the component instead of the smallest; box counts by a max_pool2d
     pyramid), with the bytes each kernel has to move at least over the measured time;
  2. the metric's own work in one evaluation at the default setting: 8192 images per side in minibatches of 64, i.e. 256 calls of
     `arbor_statistics` and one `Morphology.result()`;
  3. `evaluate_morphology` itself at that setting with an untrained generator and a synthetic data set, as tools/spectrum_time.py does.

HIP events, three warm calls, the median of --runs runs.  A record, not a gate.

    python tools/morph_time.py [--images 8192] [--runs 3] [--out profiles/morph_time.txt]
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
PEAK = 5e12                                          # bytes / s the floors are taken against


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
def torch_levels(x):
    lv = torch.clamp(torch.addcmul(torch.full_like(x, 128.0), x, torch.full_like(x, 127.5)), 0.0, 255.0).to(torch.uint8)[..., 0]
    hist = torch.zeros(x.shape[0], 256, device=x.device, dtype=torch.int32)
    hist.scatter_add_(1, lv.reshape(x.shape[0], -1).long(), torch.ones(1, device=x.device, dtype=torch.int32).expand(x.shape[0], R * R))
    return lv, hist


def torch_mask(levels, cut):
    return (levels.to(torch.int32) > cut.view(-1, 1, 1)).to(torch.uint8)


def torch_labels(mask):
    """every foreground pixel ends with the largest linear index of its component; returns (labels, sweeps)"""
    fg = mask.bool().unsqueeze(1)
    idx = torch.arange(R * R, device=mask.device, dtype=torch.float32).view(1, 1, R, R)         # exact below 2^24
    lab = torch.where(fg, idx.expand(mask.shape[0], -1, -1, -1), torch.full((), -1.0, device=mask.device))
    sweeps = 0
    while True:
        new = torch.where(fg, F.max_pool2d(lab, 3, stride=1, padding=1), lab)
        sweeps += 1
        if torch.equal(new, lab):                    # one host read-back per sweep: the price of "until nothing changes"
            return lab[:, 0].to(torch.int32), sweeps
        lab = new


def torch_boxes(mask):
    m = mask.float().unsqueeze(1)
    out = [m.sum((1, 2, 3))]
    while m.shape[-1] > 1:
        m = F.max_pool2d(m, 2)
        out.append(m.sum((1, 2, 3)))
    return torch.stack(out, 1).to(torch.int32)


def main():
    out = []
    t0 = time.time()
    img = np.stack([OT.micrograph(seed, R) for seed in range(BATCH)])
    x = torch.from_numpy((img.astype(np.float64) / 127.5 - 1.0).astype(np.float32)[..., None]).to(DEV)
    print(f"{BATCH} micrograph fields in {time.time() - t0:.1f} s", flush=True)
    levels, hist = M.morph_levels(x)
    thresholds, status = M.otsu_thresholds(hist)
    cut = thresholds[:, 0].contiguous()
    mask = M.morph_mask(levels, cut)
    labels, stats, kept = M.connected_components(mask)
    counts = M.box_counts(kept)
    # does the restatement agree?  (labels: the same partition seen from its other end; said in the report, not asserted)
    tl, th = torch_levels(x)
    tlab, sweeps = torch_labels(mask)
    off = (torch.arange(BATCH, device=DEV) * R * R).view(-1, 1, 1)
    fg = labels >= 0
    a, b = (labels + off)[fg].long(), (tlab + off)[fg].long()
    n_pairs = torch.unique(torch.stack([a, b]), dim=1).shape[1]
    agree = {"levels": torch.equal(tl, levels), "histogram": torch.equal(th, hist), "mask": torch.equal(torch_mask(levels, cut), mask),
             "labels (partition)": torch.equal(tlab >= 0, fg) and n_pairs == torch.unique(a).numel() == torch.unique(b).numel(),
             "box counts": torch.equal(torch_boxes(kept), counts)}
    s = stats.double().mean(0).tolist()
    out.append(f"input: {BATCH} micrograph-like fields of tests/multiotsu_ref.py (seeds 0 .. {BATCH - 1}) at {R} x {R}, mapped to [-1, 1]; no data "
               f"folder on this machine.  Per image on average: foreground {s[0]:.0f} pixels ({100 * s[0] / R / R:.1f} %), {s[1]:.0f} components, "
               f"largest {s[2]:.0f} pixels; status 0 for {int((status == 0).sum())} of {BATCH}")
    out.append("the torch restatement gives the same " + ", ".join(k for k, v in agree.items() if v)
               + ("; it DIFFERS in " + ", ".join(k for k, v in agree.items() if not v) if not all(agree.values()) else ""))
    px = BATCH * R * R
    stages = [
        ("levels + histogram", lambda: M.morph_levels(x), lambda: torch_levels(x), px * (4 + 1), "4 B read, 1 B written per pixel"),
        ("multi-Otsu (existing)", lambda: M.otsu_thresholds(hist), None, 0, ""),
        ("mask", lambda: M.morph_mask(levels, cut), lambda: torch_mask(levels, cut), px * 2, "1 B read, 1 B written"),
        ("labels + stats + kept", lambda: M.connected_components(mask), lambda: torch_labels(mask), px * (1 + 4), "1 B read, 4 B written"),
        ("box counts", lambda: M.box_counts(kept), lambda: torch_boxes(kept), px, "1 B read"),
        ("arbor_statistics (all)", lambda: M.arbor_statistics(x), None, px * (4 + 1 + 2 + 5 + 1), "the sum of the above"),
    ]
    out.append("")
    out.append(f"stages, {BATCH} images at {R} x {R}; MI355X, HIP events, median of {RUNS} x 10 calls, ms; floor = least bytes / 5 TB/s")
    out.append(f"{'stage':<26}{'kernels':>10}{'torch':>10}{'torch / kernels':>17}{'MB':>9}{'floor':>9}{'floor / kernels':>17}  least traffic")
    slower = []
    for name, fn, tfn, nbytes, what in stages:
        a = timed(fn)
        b = timed(tfn, reps=2) if tfn is not None else None
        floor = nbytes / PEAK * 1e3
        out.append(f"{name:<26}{a:>10.4f}" + (f"{b:>10.4f}{b / a:>17.1f}" if b is not None else f"{'-':>10}{'-':>17}")
                   + (f"{nbytes / 1e6:>9.1f}{floor:>9.4f}{floor / a:>17.3f}  {what}" if nbytes else ""))
        if b is not None and a > b:
            slower.append(name)
        print(out[-1], flush=True)
    out.append(f"(torch's labelling took {sweeps} sweeps of a 3 x 3 max-pool on this input, with one host read-back each)")
    out.append("no stage is slower than torch's" if not slower else "SLOWER than torch: " + ", ".join(slower))

    n_batches = (ARGS.images + BATCH - 1) // BATCH

    def metric_alone():
        m = M.Morphology(R, device=DEV)
        for _ in range(n_batches):
            m.feed("real", x)
            m.feed("fake", x)
        return m.result()
    t = timed(metric_alone, reps=1)
    out.append("")
    out.append(f"the metric's own work in one evaluation at the default setting ({ARGS.images} images per side, minibatches of {BATCH}: "
               f"{2 * n_batches} calls of arbor_statistics and one result(); every call is fed the same {BATCH} fields above, on both sides, "
               f"not {ARGS.images} distinct images): {t:.1f} ms")

    torch.manual_seed(1)
    G = pkg.models.Generator_PG([128, 64, 32, 32, 16, 16], image_size_init=16).to(DEV)
    G.set_resolution(R, 1.0)
    data = pkg.data.NeuronDataset(torch.from_numpy(img[:, None].astype(np.float32) / 255.0), augmentations=True, im_translation=0.05,
                                  device=DEV, seed=3)
    res = {}

    def whole():
        res["r"] = M.evaluate_morphology(G, data, n_images=ARGS.images, batch_size=BATCH)
    t2 = timed(whole, reps=1)
    out.append(f"evaluate_morphology at that setting, untrained generator, the same fields as the data set through its augmentation chain: "
               f"{t2:.1f} ms (the metric's share {100 * t / t2:.0f} %)")
    out.append(M.format_morphology(res["r"], "its table"))
    text = "\n".join(out)
    print(text)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
