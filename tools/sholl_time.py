"""Time the arbor-geometry metric on one GPU.  Without a data folder the inputs are the micrograph-like fields of
tests/multiotsu_ref.py (64 seeds at 512 x 512, mapped to [-1, 1]); the report says so.

  1. `distance_transform`, `sholl_crossings` and all of `sholl_statistics` for 64 images at 512 x 512 through the kernels, next to a
     plain-torch restatement on the same GPU: the column distances by cumulative maxima of the last background row, the row
     minimisation as a broadcast (R, R) min-plus per block of rows, the soma by argmax, the crossings by shifted views of a padded ring
     map and `bincount`, the roots by a masked sum.  The restatement of `sholl_statistics` keeps the front end and the thinning on the
     kernels (tools/morph_time.py and tools/skeleton_time.py time those against torch) and does the geometry in torch.  Each stage is
     put next to the bytes it has to move at least: the transform reads 1 B and writes 4 B per pixel, plus its 2 B workspace written
     and read; the Sholl pass reads 5 B per pixel;
  2. the metric's own work in one evaluation at the default setting: 8192 images per side in minibatches of 64, i.e. 256 calls of
     `sholl_statistics` and one `Sholl.result()`;
  3. `evaluate_sholl` itself at that setting with an untrained generator and a synthetic data set, as tools/skeleton_time.py does.

HIP events, three warm calls, the median of --runs runs.  A record, not a gate.

    python tools/sholl_time.py [--images 8192] [--runs 3] [--out profiles/sholl_time.txt]
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
ROWS = 8                                             # rows per min-plus block: (64, 8, 512, 512) int32 is 537 MB


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
def torch_edt(mask):
    """(dist2 (B, R, R) int32, soma (B, 3) int32)"""
    m = mask != 0
    b = m.shape[0]
    rows = torch.arange(R, device=m.device, dtype=torch.int32)[None, :, None]
    last = torch.where(m, torch.full_like(rows, -1), rows).cummax(dim=1).values            # the last background row at or above, -1 outside
    nxt = torch.where(m, torch.full_like(rows, R), rows).flip(1).cummin(dim=1).values.flip(1)
    col = torch.minimum(rows - last, nxt - rows)
    g2 = col * col
    xs = torch.arange(R, device=m.device, dtype=torch.int32)
    apart = (xs[:, None] - xs[None, :]) ** 2                                                # [x, x']
    edge = torch.minimum((xs + 1) ** 2, (R - xs) ** 2)                                      # the columns -1 and R, where g is 0
    dist2 = torch.empty(b, R, R, device=m.device, dtype=torch.int32)
    for y in range(0, R, ROWS):
        dist2[:, y:y + ROWS] = torch.minimum((g2[:, y:y + ROWS, None, :] + apart).amin(dim=3), edge)
    flat = dist2.view(b, -1)
    best = flat.argmax(dim=1)                                                               # (the first of the largest)
    d = flat.gather(1, best[:, None])[:, 0]
    soma = torch.stack([best // R, best % R, d.long()], 1)
    return dist2, torch.where(d[:, None] > 0, soma, torch.tensor([-1, -1, 0], device=m.device)).to(torch.int32)


def torch_sholl(skeleton, dist2, centre):
    """(crossings (B, 91) int64, roots (B) fp64)"""
    m = skeleton != 0
    b = m.shape[0]
    s = M.sholl_step(R)
    c = centre.long()
    pos = torch.arange(-1, R + 1, device=m.device)
    d2 = (pos[None, :, None] - c[:, 0, None, None]) ** 2 + (pos[None, None, :] - c[:, 1, None, None]) ** 2
    root = d2.double().sqrt().floor().long()
    root = root - (root * root > d2).long() + ((root + 1) * (root + 1) <= d2).long()
    k = root // s
    p = F.pad(m, (1, 1, 1, 1))
    at = lambda t, dy, dx: t[:, 1 + dy:1 + dy + R, 1 + dx:1 + dx + R]   # noqa: E731
    P4, P5, P6, P7, P8 = at(p, 0, 1), at(p, 1, 1), at(p, 1, 0), at(p, 1, -1), at(p, 0, -1)
    image = torch.arange(b, device=m.device)[:, None, None] * M.SHOLL_BINS
    hits = []
    for edge, (dy, dx) in ((m & P4, (0, 1)), (m & P6, (1, 0)), (m & P5 & ~P4 & ~P6, (1, 1)), (m & P7 & ~P8 & ~P6, (1, -1))):
        ka, kb = at(k, 0, 0), at(k, dy, dx)
        sel = edge & (ka != kb)
        hits.append((image + torch.maximum(ka, kb))[sel])
    valid = (c[:, 0] >= 0)
    crossings = torch.bincount(torch.cat(hits), minlength=b * M.SHOLL_BINS).view(b, M.SHOLL_BINS) * valid[:, None]
    return crossings, (dist2.double().sqrt() * m).sum((1, 2)) * valid


def torch_sholl_statistics(x):
    """sholl_statistics with the geometry in plain torch; the front end and the thinning through the kernels"""
    r, ok, stats, kept = M._kept_mask(x, 1, 1, None)
    skeleton, sk = M.thin(kept)
    dist2, soma = torch_edt(kept)
    crossings, roots = torch_sholl(skeleton, dist2, soma)
    peak = crossings.max(dim=1).values
    return {"calibre": 2.0 * roots / sk[:, 0].double() - 1.0, "soma": soma[:, 2].double().sqrt(), "sholl_peak": peak.double(),
            "crossings": crossings}


def main():
    out = []
    t0 = time.time()
    img = np.stack([OT.micrograph(seed, R) for seed in range(BATCH)])
    x = torch.from_numpy((img.astype(np.float64) / 127.5 - 1.0).astype(np.float32)[..., None]).to(DEV)
    print(f"{BATCH} micrograph fields in {time.time() - t0:.1f} s", flush=True)
    _, _, _, kept = M._kept_mask(x, 1, 1, None)
    skeleton, stats = M.thin(kept)
    dist2, soma = M.distance_transform(kept)
    crossings, roots = M.sholl_crossings(skeleton, dist2, soma)
    td, ts = torch_edt(kept)
    tc, tr = torch_sholl(skeleton, dist2, soma)
    agree = {"dist2": torch.equal(td, dist2), "soma": torch.equal(ts, soma), "crossings": torch.equal(tc, crossings.long()),
             "roots (to 1e-12)": bool(((tr - roots).abs() <= 1e-12 * roots.abs().clamp(min=1.0)).all())}
    st = M.sholl_statistics(x)
    mean = lambda name: float(st[name][st["scored"]].mean())   # noqa: E731
    out.append(f"input: {BATCH} micrograph-like fields of tests/multiotsu_ref.py (seeds 0 .. {BATCH - 1}) at {R} x {R}, mapped to [-1, 1]; no data "
               f"folder on this machine.  Per image on average: kept mask {float(stats[:, 7].double().mean()):.0f} pixels, skeleton "
               f"{float(stats[:, 0].double().mean()):.0f} pixels, calibre {mean('calibre'):.2f} pixels, soma radius {mean('soma'):.2f} pixels, "
               f"Sholl peak {mean('sholl_peak'):.1f} at {mean('sholl_radius'):.3f}, reach {mean('reach'):.3f} image widths; largest dist2 "
               f"{int(dist2.max())}")
    out.append("the torch restatement gives the same " + ", ".join(k for k, v in agree.items() if v)
               + ("; it DIFFERS in " + ", ".join(k for k, v in agree.items() if not v) if not all(agree.values()) else ""))
    px = BATCH * R * R
    stages = [
        ("distance_transform", lambda: M.distance_transform(kept), lambda: torch_edt(kept), px * (1 + 4 + 2 + 2 + 2),
         "1 B read, 4 B written, workspace 2 B written, read and written"),
        ("sholl_crossings", lambda: M.sholl_crossings(skeleton, dist2, soma), lambda: torch_sholl(skeleton, dist2, soma), px * 5, "5 B read per pixel"),
        ("front end + thin (existing)", lambda: M.thin(M._kept_mask(x, 1, 1, None)[3]), None, 0, ""),
        ("sholl_statistics (all)", lambda: M.sholl_statistics(x), lambda: torch_sholl_statistics(x), px * (4 + 1 + 2 + 5 + 1 + 1 + 11 + 5),
         "the front end's and the thinning's bytes and the two above"),
    ]
    out.append("")
    out.append(f"stages, {BATCH} images at {R} x {R}; MI355X, HIP events, median of {RUNS} x 10 calls, ms; floor = least bytes / 5 TB/s")
    out.append(f"{'stage':<30}{'kernels':>10}{'torch':>10}{'torch / kernels':>17}{'MB':>9}{'floor':>9}{'floor / kernels':>17}  least traffic")
    slower = []
    for name, fn, tfn, nbytes, what in stages:
        a = timed(fn)
        b = timed(tfn, reps=2) if tfn is not None else None
        floor = nbytes / PEAK * 1e3
        out.append(f"{name:<30}{a:>10.4f}" + (f"{b:>10.4f}{b / a:>17.1f}" if b is not None else f"{'-':>10}{'-':>17}")
                   + (f"{nbytes / 1e6:>9.1f}{floor:>9.4f}{floor / a:>17.3f}  {what}" if nbytes else ""))
        if b is not None and a > b:
            slower.append(name)
        print(out[-1], flush=True)
    out.append("no stage is slower than torch's" if not slower else "SLOWER than torch: " + ", ".join(slower))

    n_batches = (ARGS.images + BATCH - 1) // BATCH

    def metric_alone():
        m = M.Sholl(R, device=DEV)
        for _ in range(n_batches):
            m.feed("real", x)
            m.feed("fake", x)
        return m.result()
    t = timed(metric_alone, reps=1)
    out.append("")
    out.append(f"the metric's own work in one evaluation at the default setting ({ARGS.images} images per side, minibatches of {BATCH}: "
               f"{2 * n_batches} calls of sholl_statistics and one result(); every call is fed the same {BATCH} fields above, on both "
               f"sides, not {ARGS.images} distinct images): {t:.1f} ms")

    torch.manual_seed(1)
    G = pkg.models.Generator_PG([128, 64, 32, 32, 16, 16], image_size_init=16).to(DEV)
    G.set_resolution(R, 1.0)
    data = pkg.data.NeuronDataset(torch.from_numpy(img[:, None].astype(np.float32) / 255.0), augmentations=True, im_translation=0.05,
                                  device=DEV, seed=3)
    res = {}

    def whole():
        res["r"], res["m"] = M.evaluate_sholl(G, data, n_images=ARGS.images, batch_size=BATCH, return_metric=True)
    t2 = timed(whole, reps=1)
    out.append(f"evaluate_sholl at that setting, untrained generator, the same fields as the data set through its augmentation chain: "
               f"{t2:.1f} ms (the metric's share {100 * t / t2:.0f} %)")
    out.append(M.format_sholl(res["r"], "its table"))
    text = "\n".join(out)
    print(text)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
