"""Time the arbor-branch metric on one GPU.  Without a data folder the inputs are the micrograph-like fields of
tests/multiotsu_ref.py (64 seeds at 512 x 512, mapped to [-1, 1]); the report says so.

  1. `branch_graph` and all of `branch_statistics` for 64 images at 512 x 512 through the kernels, next to a plain-torch restatement on
     the same GPU: the edges and degrees from shifted views of the padded skeleton, the labels by iterated min-propagation over the
     node edges and branch edges (every pixel takes the smallest label among itself and its neighbours of the same kind, until nothing
     changes; the check for that is made every eighth sweep), the records of branches and nodes by `bincount`.  The restatement of
     `branch_statistics` keeps the front end and the thinning on the kernels (tools/morph_time.py and tools/skeleton_time.py time those
     against torch) and cuts the skeleton in torch.  Each stage is put next to the bytes it has to move at least: the graph reads 1 B
     per pixel and writes 84 integers per image (4 more bytes per pixel with labels);
  2. the metric's own work in one evaluation at the default setting: 8192 images per side in minibatches of 64, i.e. 256 calls of
     `branch_statistics` and one `Branches.result()`;
  3. `evaluate_branches` itself at that setting with an untrained generator and a synthetic data set, as tools/sholl_time.py does.

HIP events, three warm calls, the median of --runs runs.  A record, not a gate.

    python tools/branch_time.py [--images 8192] [--runs 3] [--out profiles/branch_time.txt]
"""
import argparse
import math
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
DIRS = ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1))     # E, SE, S, SW, W, NW, N, NE
S = {name: i for i, name in enumerate(M.BRANCH_STATS)}


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
def shifted(t, dy, dx, fill):
    """t[b, y + dy, x + dx], `fill` outside"""
    r = t.shape[1]
    return F.pad(t, (1, 1, 1, 1), value=fill)[:, 1 + dy:1 + dy + r, 1 + dx:1 + dx + r]


def torch_branch_graph(skeleton, spur):
    """(labels (B, R, R) int32, stats (B, 20) int64, hist (B, 64) int64)"""
    m = skeleton != 0
    b, r, _ = m.shape
    P = r * r
    nb = [shifted(m, dy, dx, False) for dy, dx in DIRS]
    edge = [m & nb[k] if k % 2 == 0 else m & nb[k] & ~nb[k - 1] & ~nb[(k + 1) % 8] for k in range(8)]
    deg = sum(e.to(torch.int32) for e in edge)
    node = m & (deg >= 3)
    node_nb = [shifted(node, dy, dx, False) for dy, dx in DIRS]
    same = [edge[k] & (node == node_nb[k]) for k in range(8)]                  # node edges and branch edges
    BIG = P
    index = torch.arange(P, device=m.device, dtype=torch.int32).view(1, r, r).expand(b, r, r)
    lab = torch.where(m, index, torch.full_like(index, BIG))
    while True:
        before = lab
        for _ in range(8):
            best = lab
            for k, (dy, dx) in enumerate(DIRS):
                best = torch.minimum(best, torch.where(same[k], shifted(lab, dy, dx, BIG), BIG))
            lab = best
        if torch.equal(lab, before):
            break
    labels = torch.where(m, torch.where(node, -2 - lab, lab), torch.full_like(lab, -1))
    image = torch.arange(b, device=m.device)[:, None, None] * P
    root = image + lab.long()                                                # of every set pixel, over the batch
    branch = m & ~node
    attach = [edge[k] & branch & node_nb[k] for k in range(8)]
    inner = [edge[k] & branch & ~node_nb[k] for k in range(4)]                # every branch edge once, at its smaller end
    orth = sum(attach[k].long() for k in (0, 2, 4, 6)) + sum(inner[k].long() for k in (0, 2))
    diag = sum(attach[k].long() for k in (1, 3, 5, 7)) + sum(inner[k].long() for k in (1, 3))
    atts = sum(a.long() for a in attach)
    at = root[branch]
    count = lambda w: torch.bincount(at, weights=w[branch].double(), minlength=b * P).long()   # noqa: E731
    n, o, d, a = count(torch.ones_like(orth)), count(orth), count(diag), count(atts)
    is_spur = (a == 1) & (n < spur)
    strong = torch.zeros(b * P, device=m.device, dtype=torch.long)
    for k, (dy, dx) in enumerate(DIRS):
        sel = attach[k] & ~is_spur[root.clamp(max=b * P - 1)]
        strong += torch.bincount((image + shifted(lab, dy, dx, BIG).long())[sel], minlength=b * P)
    is_root = (lab == index)
    node_root, branch_root = (is_root & node).view(b, P), (is_root & branch).view(b, P)
    n, o, d, a, strong, is_spur = (t.view(b, P) for t in (n, o, d, a, strong, is_spur))
    lo = (2.0 * d.double() * d.double()).sqrt().floor().long()
    lo = lo - (lo * lo > 2 * d * d).long() + ((lo + 1) * (lo + 1) <= 2 * d * d).long()
    L = o + lo
    cls = {"free": branch_root & (a == 0), "links": branch_root & (a == 2), "spurs": branch_root & is_spur,
           "terminal": branch_root & (a == 1) & ~is_spur}
    stats = torch.zeros(b, 20, device=m.device, dtype=torch.long)
    stats[:, S["pixels"]], stats[:, S["node_pixels"]] = m.view(b, P).sum(1), node.view(b, P).sum(1)
    stats[:, S["nodes"]], stats[:, S["branches"]] = node_root.sum(1), branch_root.sum(1)
    for name, short in (("terminal", "term"), ("links", "link"), ("free", "free"), ("spurs", "spur")):
        stats[:, S[name]] = cls[name].sum(1)
        stats[:, S[short + "_orth"]], stats[:, S[short + "_diag"]] = (o * cls[name]).sum(1), (d * cls[name]).sum(1)
    node_edge = [edge[k] & node & node_nb[k] for k in range(4)]
    stats[:, S["node_orth"]] = (node_edge[0].view(b, P).sum(1) + node_edge[2].view(b, P).sum(1))
    stats[:, S["node_diag"]] = (node_edge[1].view(b, P).sum(1) + node_edge[3].view(b, P).sum(1))
    stats[:, S["longest"]] = (L * (branch_root & ~is_spur)).max(dim=1).values
    stats[:, S["forks"]] = (node_root & (strong >= 3)).sum(1)
    binned = cls["terminal"] | cls["links"]
    bins = (L // max(1, r // 128)).clamp(max=M.BRANCH_BINS - 1) + torch.arange(b, device=m.device)[:, None] * M.BRANCH_BINS
    hist = torch.bincount(bins[binned], minlength=b * M.BRANCH_BINS).view(b, M.BRANCH_BINS)
    return labels, stats, hist


def torch_branch_statistics(x):
    """branch_statistics with the graph in plain torch; the front end and the thinning through the kernels"""
    r, ok, stats, kept = M._kept_mask(x, 1, 1, None)
    skeleton, sk = M.thin(kept)
    _, st, hist = torch_branch_graph(skeleton, M.default_spur(r))
    s = st.double()
    return {"forks": s[:, 19], "nodes": s[:, 2], "terminal_length": (s[:, 8] + math.sqrt(2.0) * s[:, 9]) / s[:, 4].clamp(min=1.0) / r, "hist": hist}


def main():
    out = []
    t0 = time.time()
    img = np.stack([OT.micrograph(seed, R) for seed in range(BATCH)])
    x = torch.from_numpy((img.astype(np.float64) / 127.5 - 1.0).astype(np.float32)[..., None]).to(DEV)
    print(f"{BATCH} micrograph fields in {time.time() - t0:.1f} s", flush=True)
    _, _, _, kept = M._kept_mask(x, 1, 1, None)
    skeleton, sk = M.thin(kept)
    spur = M.default_spur(R)
    labels, stats, hist = M.branch_graph(skeleton, spur, want_labels=True)
    tl, ts, th = torch_branch_graph(skeleton, spur)
    agree = {"labels": torch.equal(tl, labels), "stats": torch.equal(ts, stats.long()), "hist": torch.equal(th, hist.long())}
    st = M.branch_statistics(x)
    mean = lambda name: float(st[name][st["scored"]].mean())   # noqa: E731
    out.append(f"input: {BATCH} micrograph-like fields of tests/multiotsu_ref.py (seeds 0 .. {BATCH - 1}) at {R} x {R}, mapped to [-1, 1]; no data "
               f"folder on this machine.  Per image on average: skeleton {float(sk[:, 0].double().mean()):.0f} pixels with "
               f"{float(sk[:, 2].double().mean()):.1f} junction pixels (X >= 3); spur {spur}: nodes {mean('nodes'):.1f}, forks {mean('forks'):.1f}, "
               f"terminals {mean('terminals'):.1f} of {mean('terminal_length'):.4f}, spurs {mean('spurs'):.1f}, links of {mean('link_length'):.4f}, "
               f"longest {mean('longest'):.3f} image widths")
    out.append("the torch restatement gives the same " + ", ".join(k for k, v in agree.items() if v)
               + ("; it DIFFERS in " + ", ".join(k for k, v in agree.items() if not v) if not all(agree.values()) else ""))
    px = BATCH * R * R
    small = BATCH * 84 * 4
    stages = [
        ("branch_graph", lambda: M.branch_graph(skeleton, spur), lambda: torch_branch_graph(skeleton, spur), px + small,
         "1 B read per pixel, 84 integers written per image"),
        ("branch_graph with labels", lambda: M.branch_graph(skeleton, spur, want_labels=True), None, px * 5 + small, "and 4 B written per pixel"),
        ("front end + thin (existing)", lambda: M.thin(M._kept_mask(x, 1, 1, None)[3]), None, 0, ""),
        ("branch_statistics (all)", lambda: M.branch_statistics(x), lambda: torch_branch_statistics(x), px * (4 + 1 + 2 + 5 + 1 + 1 + 1) + small,
         "the front end's and the thinning's bytes and the graph's"),
    ]
    out.append("")
    out.append(f"stages, {BATCH} images at {R} x {R}; MI355X, HIP events, median of {RUNS} x 10 calls, ms; floor = least bytes / 5 TB/s")
    out.append(f"{'stage':<30}{'kernels':>10}{'torch':>10}{'torch / kernels':>17}{'MB':>9}{'floor':>9}{'floor / kernels':>17}  least traffic")
    slower = []
    for name, fn, tfn, nbytes, what in stages:
        a = timed(fn)
        b = timed(tfn, reps=1) if tfn is not None else None
        floor = nbytes / PEAK * 1e3
        out.append(f"{name:<30}{a:>10.4f}" + (f"{b:>10.4f}{b / a:>17.1f}" if b is not None else f"{'-':>10}{'-':>17}")
                   + (f"{nbytes / 1e6:>9.1f}{floor:>9.4f}{floor / a:>17.3f}  {what}" if nbytes else ""))
        if b is not None and a > b:
            slower.append(name)
        print(out[-1], flush=True)
    out.append("no stage is slower than torch's" if not slower else "SLOWER than torch: " + ", ".join(slower))

    n_batches = (ARGS.images + BATCH - 1) // BATCH

    def metric_alone():
        m = M.Branches(R, device=DEV)
        for _ in range(n_batches):
            m.feed("real", x)
            m.feed("fake", x)
        return m.result()
    t = timed(metric_alone, reps=1)
    out.append("")
    out.append(f"the metric's own work in one evaluation at the default setting ({ARGS.images} images per side, minibatches of {BATCH}: "
               f"{2 * n_batches} calls of branch_statistics and one result(); every call is fed the same {BATCH} fields above, on both "
               f"sides, not {ARGS.images} distinct images): {t:.1f} ms")

    torch.manual_seed(1)
    G = pkg.models.Generator_PG([128, 64, 32, 32, 16, 16], image_size_init=16).to(DEV)
    G.set_resolution(R, 1.0)
    data = pkg.data.NeuronDataset(torch.from_numpy(img[:, None].astype(np.float32) / 255.0), augmentations=True, im_translation=0.05,
                                  device=DEV, seed=3)
    res = {}

    def whole():
        res["r"], res["m"] = M.evaluate_branches(G, data, n_images=ARGS.images, batch_size=BATCH, return_metric=True)
    t2 = timed(whole, reps=1)
    out.append(f"evaluate_branches at that setting, untrained generator, the same fields as the data set through its augmentation chain: "
               f"{t2:.1f} ms (the metric's share {100 * t / t2:.0f} %)")
    out.append(M.format_branches(res["r"], "its table"))
    text = "\n".join(out)
    print(text)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
