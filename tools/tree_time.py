"""Time the arbor-tree tracing on one GPU.  Without a data folder the inputs are the micrograph-like fields of tests/multiotsu_ref.py
(64 seeds at 512 x 512, mapped to [-1, 1]); the report says so.

  1. `arbor_tree` and all of `tree_statistics` for 64 images at 512 x 512 through the kernels, next to a plain-torch restatement on the
     same GPU: the edges from shifted views of the padded skeleton, the components by iterated min-propagation of labels, the roots by
     a scatter-min of (d2 << 32 | index) per label, the costs by iterated min-plus propagation over the shifted views (every pixel takes
     the smallest cost + weight among its neighbours, until nothing changes; the check for that is made every eighth sweep), the parents
     from the converged costs in the order of the neighbours' indices, the orders by iterated propagation along the parents.  The
     restatement of `tree_statistics` keeps the front end, the thinning and the distance transform on the kernels (their own tools time
     those against torch) and traces in torch.  Each stage is put next to the bytes it has to move at least, and the sweeps the kernels
     made (the workspace keeps the two counts of every image) are reported;
  2. the metric's own work in one evaluation at the default setting: 8192 images per side in minibatches of 64, i.e. 256 calls of
     `tree_statistics` and one `Tree.result()`; and `evaluate_tree` itself at that setting with an untrained generator and a synthetic
     data set, as tools/branch_time.py does;
  3. with --snake, instead: ONE call on one `snake` image at 512 x 512, the known worst case (a path of R^2 / 2 edges, as many sweeps),
     timed once with the host's clock.  Run it as a process of its own under its own time limit.

HIP events, warm calls first, the median of --runs runs.  A record, not a gate.

    python tools/tree_time.py [--images 8192] [--runs 3] [--out profiles/tree_time.txt]
    python tools/tree_time.py --snake [--out profiles/tree_time_snake.txt]
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
import morph_cases as MC  # noqa: E402
import multiotsu_ref as OT  # noqa: E402

pkg = g.load_package()
M = pkg.metrics
DEV = torch.device("cuda:0")
parser = argparse.ArgumentParser()
parser.add_argument("--images", type=int, default=8192)
parser.add_argument("--runs", type=int, default=3)
parser.add_argument("--snake", action="store_true")
parser.add_argument("--out", type=str, default="")
ARGS = parser.parse_args()
R, BATCH, RUNS = 512, 64, ARGS.runs
PEAK = 5e12                                          # bytes / s the floor is taken against
DIRS = ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1))     # E, SE, S, SW, W, NW, N, NE
BY_INDEX = (5, 6, 7, 4, 0, 3, 2, 1)                                                 # the directions in the order of the neighbour's index
FAR = 1 << 40


def timed(fn, reps=10, warm=3):
    for _ in range(warm):
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


def until_stable(t, sweep):
    sweeps = 0
    while True:
        before = t
        for _ in range(8):
            t = sweep(t)
        sweeps += 8
        if torch.equal(t, before):
            return t, sweeps


def torch_arbor_tree(skeleton, centre):
    """{cost, parent, order (B, R, R) int32, stats (B, 12) int64, sums (B, 2) fp64, sweeps}; every centre inside its image"""
    m = skeleton != 0
    b, r, _ = m.shape
    P = r * r
    nb = [shifted(m, dy, dx, False) for dy, dx in DIRS]
    edge = [m & nb[k] if k % 2 == 0 else m & nb[k] & ~nb[k - 1] & ~nb[(k + 1) % 8] for k in range(8)]
    weight = [408 if k % 2 == 0 else 577 for k in range(8)]
    deg = sum(e.to(torch.int32) for e in edge)
    index = torch.arange(P, device=m.device, dtype=torch.int64).view(1, r, r).expand(b, r, r)
    image = torch.arange(b, device=m.device)[:, None, None] * P

    def label_sweep(lab):
        best = lab
        for k, (dy, dx) in enumerate(DIRS):
            best = torch.minimum(best, torch.where(edge[k], shifted(lab, dy, dx, FAR), FAR))
        return best
    lab, s0 = until_stable(torch.where(m, index, torch.full_like(index, FAR)), label_sweep)
    yy, xx = index // r, index % r
    d2 = (yy - centre[:, 0].long()[:, None, None]) ** 2 + (xx - centre[:, 1].long()[:, None, None]) ** 2
    key = (d2 << 32) | index
    flat = (image + lab.clamp(max=P - 1))
    best = torch.full((b * P,), 1 << 62, device=m.device, dtype=torch.int64).scatter_reduce(0, flat[m], key[m], "amin")
    root = torch.where(m, best[flat] & 0xffffffff, torch.full_like(index, -1))
    is_root = m & (root == index)

    def cost_sweep(cost):
        best = cost
        for k, (dy, dx) in enumerate(DIRS):
            best = torch.minimum(best, torch.where(edge[k], shifted(cost, dy, dx, FAR) + weight[k], FAR))
        return best
    cost, s1 = until_stable(torch.where(is_root, torch.zeros_like(index), torch.full_like(index, FAR)), cost_sweep)
    parent = torch.where(is_root, torch.full_like(index, -1), torch.full_like(index, -2))
    for k in BY_INDEX:
        dy, dx = DIRS[k]
        hit = edge[k] & ~is_root & (parent == -2) & (shifted(cost, dy, dx, FAR) + weight[k] == cost)
        parent = torch.where(hit, index + dy * r + dx, parent)
    kids = sum((edge[k] & (shifted(parent, dy, dx, -9) == index)).to(torch.int32) for k, (dy, dx) in enumerate(DIRS))
    up = parent.clamp(min=0).view(b, P)
    step = (kids >= 2).view(b, P).gather(1, up).view(b, r, r).long()
    settled = m & ~is_root

    def order_sweep(order):
        above = order.view(b, P).gather(1, up).view(b, r, r)
        return torch.where(settled & (order < 0) & (above >= 0), above + step, order)
    order, s2 = until_stable(torch.where(is_root, torch.zeros_like(index), torch.full_like(index, -1)), order_sweep)
    tip = m & (kids == 0) & (deg <= 1)
    n = lambda t: t.view(b, P).sum(1)   # noqa: E731
    orth, diag = n(edge[0]) + n(edge[2]), n(edge[1]) + n(edge[3])
    reach = torch.where(m, cost, torch.zeros_like(cost))
    main = best.view(b, P).min(dim=1).values & 0xffffffff
    stats = torch.stack([n(m), n(is_root), orth, diag, orth + diag - n(m) + n(is_root), n(m & (kids == 0)), n(tip), n(m & (kids >= 2)),
                         reach.view(b, P).max(1).values, order.view(b, P).max(1).values.clamp(min=0), main, n(root == main[:, None, None])], dim=1)
    ry, rx = root // r, root % r
    term = torch.where(tip & (cost > 0), ((yy - ry) ** 2 + (xx - rx) ** 2).double().sqrt() / (cost.double().clamp(min=1.0) / 408.0), 0.0)
    sums = torch.stack([n(torch.where(tip, cost, torch.zeros_like(cost))).double(), n(term)], dim=1)
    back = torch.full_like(index, -1)
    return {"cost": torch.where(m, cost, back).int(), "parent": parent.int(), "order": torch.where(m, order, back).int(), "stats": stats,
            "sums": sums, "sweeps": (s0, s1, s2)}


def torch_tree_statistics(x):
    """tree_statistics with the tracing in plain torch; the front end, the thinning and the distance transform through the kernels"""
    r, ok, stats, kept = M._kept_mask(x, 1, 1, None)
    skeleton, sk = M.thin(kept)
    _, soma = M.distance_transform(kept)
    t = torch_arbor_tree(skeleton, soma)
    s = t["stats"].double()
    tips = s[:, 6].clamp(min=1.0)
    return {"trees": s[:, 1], "cycles": s[:, 4], "path_max": s[:, 8] / 408.0 / r, "path_mean": t["sums"][:, 0] / tips / 408.0 / r,
            "contraction": t["sums"][:, 1] / tips}


def sweeps_of(ws, b):
    """the relaxation's and the order's sweep counts of every image, left in the first two int32 of its slice of the workspace"""
    notes = ws[:b * R * R * 8].view(torch.int32).view(b, -1)[:, :2].cpu().numpy()
    return notes[:, 0], notes[:, 1]


def snake():
    mask = torch.from_numpy(MC.family("snake", R)).to(DEV)[None].contiguous()
    centre = torch.tensor([[0, 0, 1]], device=DEV, dtype=torch.int32)
    torch.cuda.synchronize()
    t0 = time.time()
    t, ws = M._trace(mask, centre, True)
    torch.cuda.synchronize()
    dt = time.time() - t0
    st = dict(zip(M.TREE_STATS, t["stats"][0].tolist()))
    a, b = sweeps_of(ws, 1)
    pixels = int(mask.sum())
    ok = st["pixels"] == pixels and st["path_max"] == 408 * (pixels - 1) and st["tips"] == 1 and st["cycles"] == 0 and st["trees"] == 1
    return (f"the known worst case: one `snake` image at {R} x {R} about its first pixel, a single path of {pixels} pixels; one call, the first "
            f"of its process, host clock: {dt * 1e3:.0f} ms; {int(a[0])} relaxation sweeps and {int(b[0])} order sweeps; path_max "
            f"{st['path_max']} = 408 x {st['path_max'] // 408}, one tip, no cycle: {'as expected' if ok else 'NOT as expected ' + str(st)}")


def main():
    if ARGS.snake:
        text = snake()
        print(text)
        if ARGS.out:
            with open(ARGS.out, "w") as f:
                f.write(text + "\n")
        return
    out = []
    t0 = time.time()
    img = np.stack([OT.micrograph(seed, R) for seed in range(BATCH)])
    x = torch.from_numpy((img.astype(np.float64) / 127.5 - 1.0).astype(np.float32)[..., None]).to(DEV)
    print(f"{BATCH} micrograph fields in {time.time() - t0:.1f} s", flush=True)
    _, _, _, kept = M._kept_mask(x, 1, 1, None)
    skeleton, sk = M.thin(kept)
    _, soma = M.distance_transform(kept)
    assert bool((soma[:, 0] >= 0).all())
    t, ws = M._trace(skeleton, soma, True)
    relax, order = sweeps_of(ws, BATCH)
    tt = torch_arbor_tree(skeleton, soma)
    agree = {k: torch.equal(tt[k], t[k]) for k in ("cost", "parent", "order")}
    agree["stats"] = torch.equal(tt["stats"], t["stats"].long())
    agree["tip_cost"] = torch.equal(tt["sums"][:, 0], t["sums"][:, 0])
    agree["contraction to 1e-12"] = bool(((tt["sums"][:, 1] - t["sums"][:, 1]).abs() <= 1e-12 * t["sums"][:, 1].abs()).all())
    st = M.tree_statistics(x)
    mean = lambda name: float(st[name][st["scored"]].mean())   # noqa: E731
    out.append(f"input: {BATCH} micrograph-like fields of tests/multiotsu_ref.py (seeds 0 .. {BATCH - 1}) at {R} x {R}, mapped to [-1, 1]; no data "
               f"folder on this machine.  Per image on average: skeleton {float(sk[:, 0].double().mean()):.0f} pixels in {mean('trees'):.1f} trees "
               f"with {mean('cycles'):.1f} cycles, {mean('tips'):.1f} tips and {mean('forks'):.1f} forks; longest path {mean('path_max'):.3f} and mean "
               f"path {mean('path_mean'):.3f} image widths, contraction {mean('contraction'):.3f}, largest order {mean('max_order'):.1f}")
    out.append(f"sweeps per image, one workgroup each: relaxation {int(relax.min())} .. {int(relax.max())} (mean {relax.mean():.0f}), order "
               f"{int(order.min())} .. {int(order.max())} (mean {order.mean():.0f}); the torch restatement, which sweeps the whole batch until its "
               f"slowest image stands and checks every eighth sweep: labels {tt['sweeps'][0]}, costs {tt['sweeps'][1]}, orders {tt['sweeps'][2]}")
    out.append("the torch restatement gives the same " + ", ".join(k for k, v in agree.items() if v)
               + ("; it DIFFERS in " + ", ".join(k for k, v in agree.items() if not v) if not all(agree.values()) else ""))
    px = BATCH * R * R
    small = BATCH * (12 * 4 + 16)
    stages = [
        ("arbor_tree", lambda: M.arbor_tree(skeleton, soma, want_order=False), lambda: torch_arbor_tree(skeleton, soma), px * 9 + small,
         "1 B read and 8 B written per pixel, 12 integers and 2 doubles per image"),
        ("arbor_tree with order", lambda: M.arbor_tree(skeleton, soma), None, px * 13 + small, "and 4 B more written per pixel"),
        ("front end + thin + edt (existing)", lambda: (M.thin(M._kept_mask(x, 1, 1, None)[3]), M.distance_transform(kept)), None, 0, ""),
        ("tree_statistics (all)", lambda: M.tree_statistics(x), lambda: torch_tree_statistics(x), px * (4 + 1 + 2 + 5 + 1 + 6 + 9) + small,
         "the front end's, the thinning's and the distance transform's bytes and the tracing's"),
    ]
    out.append("")
    out.append(f"stages, {BATCH} images at {R} x {R}; MI355X, HIP events, median of {RUNS} x 10 calls (torch: {RUNS} x 1), ms; floor = least bytes / 5 TB/s")
    out.append(f"{'stage':<36}{'kernels':>10}{'torch':>11}{'torch / kernels':>17}{'MB':>9}{'floor':>9}{'floor / kernels':>17}  least traffic")
    slower = []
    for name, fn, tfn, nbytes, what in stages:
        a = timed(fn)
        b = timed(tfn, reps=1, warm=1) if tfn is not None else None
        floor = nbytes / PEAK * 1e3
        out.append(f"{name:<36}{a:>10.4f}" + (f"{b:>11.4f}{b / a:>17.1f}" if b is not None else f"{'-':>11}{'-':>17}")
                   + (f"{nbytes / 1e6:>9.1f}{floor:>9.4f}{floor / a:>17.3f}  {what}" if nbytes else ""))
        if b is not None and a > b:
            slower.append(name)
        print(out[-1], flush=True)
    out.append("no stage is slower than torch's" if not slower else "SLOWER than torch: " + ", ".join(slower))

    n_batches = (ARGS.images + BATCH - 1) // BATCH

    def metric_alone():
        m = M.Tree(R, device=DEV)
        for _ in range(n_batches):
            m.feed("real", x)
            m.feed("fake", x)
        return m.result()
    t1 = timed(metric_alone, reps=1, warm=1)
    out.append("")
    out.append(f"the metric's own work in one evaluation at --tree {ARGS.images} ({ARGS.images} images per side, minibatches of {BATCH}: "
               f"{2 * n_batches} calls of tree_statistics and one result(); every call is fed the same {BATCH} fields above, on both "
               f"sides, not {ARGS.images} distinct images): {t1:.1f} ms")
    torch.manual_seed(1)
    G = pkg.models.Generator_PG([128, 64, 32, 32, 16, 16], image_size_init=16).to(DEV)
    G.set_resolution(R, 1.0)
    data = pkg.data.NeuronDataset(torch.from_numpy(img[:, None].astype(np.float32) / 255.0), augmentations=True, im_translation=0.05,
                                  device=DEV, seed=3)
    res = {}

    def whole():
        res["r"] = M.evaluate_tree(G, data, n_images=ARGS.images, batch_size=BATCH)
    t2 = timed(whole, reps=1, warm=1)
    out.append(f"evaluate_tree at that setting, untrained generator, the same fields as the data set through its augmentation chain: "
               f"{t2:.1f} ms (the metric's share {100 * t1 / t2:.0f} %)")
    out.append(M.format_tree(res["r"], "its table"))
    text = "\n".join(out)
    print(text)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
