"""Time `evaluate_swd` at the default setting (512 x 512, C = 1, 8192 images per side, 128 patches, 4 x 128 directions) two ways: through
the kernels of csrc/swd.hip, and through a plain-torch fp32 restatement on the GPU (F.conv2d pyramid, indexed gather, materialised
normalised matrix, matmul, torch.sort).  HIP events around every stage, one warm run, the median of --runs runs.  A record, not a gate.

    python tools/swd_time.py [--images 8192] [--runs 5] [--out profiles/swd_time.txt]
    python tools/swd_time.py --micro      # sort_columns and project alone on 2^20 descriptors x 512 directions, next to torch's
                                          # (NGAN_LIB_PATH picks the library: builds with -DNGAN_SWD_SORT_BLOCK=... are measured this way)
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
M = pkg.metrics
DEV = torch.device("cuda:0")
parser = argparse.ArgumentParser()
parser.add_argument("--images", type=int, default=8192)
parser.add_argument("--runs", type=int, default=5)
parser.add_argument("--out", type=str, default="")
parser.add_argument("--micro", action="store_true")
ARGS = parser.parse_args()
R, C, N_IMAGES, BATCH, NH, REPS, DPR = 512, 1, ARGS.images, 64, 128, 4, 128
RUNS = ARGS.runs
STAGES = ["reals", "fakes", "pyramid", "descriptors", "project", "sort", "l1"]


class Clock:
    def __init__(self):
        self.ev = {s: [] for s in STAGES}

    def __call__(self, stage):
        clock = self

        class _Ctx:
            def __enter__(self):
                self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                self.a.record()

            def __exit__(self, *exc):
                self.b.record()
                clock.ev[stage].append((self.a, self.b))
        return _Ctx()

    def totals(self):
        torch.cuda.synchronize()
        return {s: sum(a.elapsed_time(b) for a, b in v) for s, v in self.ev.items()}


def make_inputs():
    torch.manual_seed(1)
    G = pkg.models.Generator_PG([128, 64, 32, 32, 16, 16], image_size_init=16).to(DEV)
    G.set_resolution(R, 1.0)
    gen = torch.Generator().manual_seed(2)
    data = pkg.data.NeuronDataset(torch.rand(64, 1, R, R, generator=gen), augmentations=True, im_translation=0.05, device=DEV, seed=3)
    return G, data


def batches(G, data, clock):
    n_data = len(data)
    for k, i in enumerate(range(0, N_IMAGES, BATCH)):
        b = min(BATCH, N_IMAGES - i)
        with clock("reals"):
            reals = data.batch([(i + j) % n_data for j in range(b)])
        z = pkg.utils.sample_latent_vec((b, G.latent_dim), seed=k, device=DEV)
        with clock("fakes"), torch.no_grad():
            fakes = G(z).detach()
        yield reals, fakes


def run_kernels(G, data):
    clock = Clock()
    m = M.SWD(R, n_colors=C, nhoods_per_image=NH, dir_repeats=REPS, dirs_per_repeat=DPR, seed=0, device=DEV, n_images=N_IMAGES)
    for reals, fakes in batches(G, data, clock):
        for which, x in (("real", reals), ("fake", fakes)):
            x = M.channels_last(x)
            with clock("pyramid"):
                pyr = M.laplacian_pyramid(x, len(m.levels))
            for l, level in enumerate(pyr):
                pos = m.draw_positions(x.shape[0], m.levels[l])
                out = m._room(which, l, pos.shape[0])
                used = m.count[which][l]
                with clock("descriptors"):
                    M.patch_descriptors(level, pos, out=out, sums=m.sums[which][l], row_offset=used, accumulate=used > 0)
                m.count[which][l] = used + pos.shape[0]
    vals = []
    for l in range(len(m.levels)):
        n = m.count["real"][l]
        d = m.dirs[l].to(DEV)
        proj = {}
        for which in ("real", "fake"):
            with clock("project"):
                p = M.project(m.desc[which][l][:n], m.sums[which][l], d)
            with clock("sort"):
                M.sort_columns(p)
            proj[which] = p
        with clock("l1"):
            vals.append(M.sorted_l1(proj["real"], proj["fake"], n))
        del proj
    res = [v * 1e3 for v in torch.cat(vals).tolist()]
    return clock.totals(), res


K1 = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


def t_down(x, k2):      # x (B, C, H, W)
    return F.conv2d(F.pad(x, (2, 2, 2, 2), mode="reflect"), k2, stride=2, groups=x.shape[1])


def t_up(c, k2):
    b, ch, h, w = c.shape
    z = torch.zeros(b, ch, 2 * h, 2 * w, device=c.device)
    z[:, :, ::2, ::2] = c
    return F.conv2d(F.pad(z, (2, 2, 2, 2), mode="reflect"), 4.0 * k2, groups=ch)


def run_torch(G, data):
    clock = Clock()
    k2 = (K1[:, None] * K1[None, :]).expand(C, 1, 5, 5).contiguous().to(DEV)
    m = M.SWD(R, n_colors=C, nhoods_per_image=NH, dir_repeats=REPS, dirs_per_repeat=DPR, seed=0, device=DEV)
    n_total = N_IMAGES * NH
    desc = {w: [torch.empty(n_total, 49 * C, device=DEV) for _ in m.levels] for w in ("real", "fake")}
    count = {w: [0] * len(m.levels) for w in ("real", "fake")}
    d7 = torch.arange(7, device=DEV)
    for reals, fakes in batches(G, data, clock):
        for which, x in (("real", reals), ("fake", fakes)):
            with clock("pyramid"):
                pyr, cur = [], x
                for _ in range(len(m.levels) - 1):
                    nxt = t_down(cur, k2)
                    pyr.append(cur - t_up(nxt, k2))
                    cur = nxt
                pyr.append(cur)
            for l, level in enumerate(pyr):
                pos = m.draw_positions(x.shape[0], m.levels[l]).to(DEV).long()
                with clock("descriptors"):
                    rows = (pos[:, 1, None] + d7)[:, None, :, None]
                    cols = (pos[:, 2, None] + d7)[:, None, None, :]
                    ch = torch.arange(C, device=DEV)[None, :, None, None]
                    patch = level[pos[:, 0, None, None, None], ch, rows, cols]            # (n, C, 7, 7)
                    n = pos.shape[0]
                    desc[which][l][count[which][l]:count[which][l] + n] = patch.reshape(n, -1)
                count[which][l] += n
    vals = []
    for l in range(len(m.levels)):
        d = m.dirs[l].to(DEV)
        srt = {}
        for which in ("real", "fake"):
            with clock("project"):
                dd = desc[which][l].view(n_total, C, 49)
                mean = dd.mean((0, 2), keepdim=True)
                std = (dd - mean).square().mean((0, 2), keepdim=True).sqrt()
                v = ((dd - mean) / std).view(n_total, 49 * C)                             # materialised
                p = d.t() @ v.t()                                                        # (n_dirs, n): contiguous columns for the sort
            with clock("sort"):
                srt[which] = torch.sort(p, dim=1).values
            del p, v
        with clock("l1"):
            vals.append((srt["real"] - srt["fake"]).abs().mean().reshape(1))
        del srt
    res = [v * 1e3 for v in torch.cat(vals).tolist()]
    return clock.totals(), res


def main():
    G, data = make_inputs()
    out = []
    results = {}
    for name, fn in (("kernels", run_kernels), ("torch fp32", run_torch)):
        t0 = time.time()
        fn(G, data)                     # warm
        torch.cuda.synchronize()
        print(f"{name}: warm run {time.time() - t0:.1f} s wall", flush=True)
        runs = []
        for _ in range(RUNS):
            tot, res = fn(G, data)
            runs.append(tot)
            print(f"  {name}: {sum(tot.values()):.1f} ms", flush=True)
        med = {s: statistics.median(r[s] for r in runs) for s in STAGES}
        med["total"] = statistics.median(sum(r.values()) for r in runs)
        results[name] = (med, res)
    out.append(f"evaluate_swd, {R} x {R}, C = {C}, {N_IMAGES} images per side in minibatches of {BATCH}, {NH} patches per image and level, "
               f"{REPS} x {DPR} directions, levels 512 .. 16; MI355X, HIP events around the stages, one warm run, median of {RUNS} runs, ms")
    out.append(f"{'stage':<14}{'kernels':>12}{'torch fp32':>12}")
    for s in STAGES + ["total"]:
        out.append(f"{s:<14}{results['kernels'][0][s]:>12.2f}{results['torch fp32'][0][s]:>12.2f}")
    mt = {k: sum(v[0][s] for s in ("pyramid", "descriptors", "project", "sort", "l1")) for k, v in results.items()}
    out.append(f"{'metric only':<14}{mt['kernels']:>12.2f}{mt['torch fp32']:>12.2f}   (without producing the images, which both ways share)")
    out.append("SWD x 1e3 per level, kernels:    " + " ".join(f"{v:.4f}" for v in results["kernels"][1]))
    out.append("SWD x 1e3 per level, torch fp32: " + " ".join(f"{v:.4f}" for v in results["torch fp32"][1]))
    text = "\n".join(out)
    print(text)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            f.write(text + "\n")


def micro():
    n_dirs, n = 512, 1 << 20
    torch.manual_seed(0)
    src = torch.randn(n_dirs, n, device=DEV)
    work = torch.empty_like(src)
    ts = []
    for i in range(7):
        work.copy_(src)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        M.sort_columns(work)
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ok = bool((work[:, 1:] >= work[:, :-1]).all())
    print(f"block {M.sort_block_elements()}: sort (512, 2^20) median {statistics.median(ts[2:]):.2f} ms (runs {' '.join(f'{t:.2f}' for t in ts)}), ascending {ok}")
    desc = torch.randn(n, 49, device=DEV)
    sums = M.descriptor_sums(desc)
    dirs = torch.randn(49, n_dirs, device=DEV)
    tp = []
    for i in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        p = M.project(desc, sums, dirs)
        b.record()
        torch.cuda.synchronize()
        tp.append(a.elapsed_time(b))
    t = statistics.median(tp[2:])
    print(f"project (2^20, 49) x (49, 512): median {t:.2f} ms = {2 * n * 49 * n_dirs / t / 1e9:.1f} TFLOP/s, {n * n_dirs * 4 / t / 1e6:.0f} GB/s stored")
    tm = []
    for i in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        q = dirs.t() @ desc.t()
        b.record()
        torch.cuda.synchronize()
        tm.append(a.elapsed_time(b))
    print(f"torch matmul of the same shape (no normalisation, no tail): median {statistics.median(tm[2:]):.2f} ms")
    tt = []
    for i in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        s = torch.sort(src, dim=1).values
        b.record()
        torch.cuda.synchronize()
        tt.append(a.elapsed_time(b))
    print(f"torch.sort (512, 2^20): median {statistics.median(tt[1:]):.2f} ms; equal to ours {bool((s == work).all())}")


if __name__ == "__main__":
    micro() if ARGS.micro else main()
