"""Time `evaluate_msssim` at the default setting (512 x 512, C = 1, 10000 pairs per side, five scales) two ways: through the kernels of
csrc/msssim.hip, and through a plain-torch fp32 restatement on the GPU (the five moments stacked as channels, the 11-tap window as
two grouped F.conv2d passes, pointwise torch for cs and ssim, F.avg_pool2d for the next scale).  HIP events around every stage, one warm
run, the median of --runs runs.  A record, not a gate.

    python tools/msssim_time.py [--pairs 10000] [--runs 3] [--out profiles/msssim_time.txt]
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
parser.add_argument("--pairs", type=int, default=10000)
parser.add_argument("--runs", type=int, default=3)
parser.add_argument("--out", type=str, default="")
ARGS = parser.parse_args()
R, C, N_PAIRS, BATCH, RUNS = 512, 1, ARGS.pairs, 64, ARGS.runs
SCALES = M.msssim_scales(R)
SIZES = [R >> s for s in range(SCALES)]
STAGES = ["fakes", "reals"] + [f"scale {h}" for h in SIZES] + ["pool"]


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
    """(side, a, b): channels-last pairs, batch by batch, first the generated side, then the data's, as evaluate_msssim produces them"""
    lat = torch.Generator(device="cpu").manual_seed(2)
    n_data = len(data)
    for i in range(0, N_PAIRS, BATCH):
        n = 2 * min(BATCH, N_PAIRS - i)
        z = torch.randn(n, G.latent_dim, generator=lat).clamp(-5, 5)
        z = (z / z.norm(p=2, dim=1, keepdim=True)).to(DEV)
        with clock("fakes"), torch.no_grad():
            x = M.channels_last(G(z).detach())
            a, b = x[0::2].contiguous(), x[1::2].contiguous()
        yield "fake", a, b
    for i in range(0, N_PAIRS, BATCH):
        n = 2 * min(BATCH, N_PAIRS - i)
        with clock("reals"):
            x = M.channels_last(data.batch([(2 * i + j) % n_data for j in range(n)]))
            a, b = x[0::2].contiguous(), x[1::2].contiguous()
        yield "real", a, b


def combine(vals):
    w = M.msssim_weights(SCALES)
    out = None
    for s, v in enumerate(vals):
        f = v.clamp_min(0.0).pow(w[s])
        out = f if out is None else out * f
    return out


def run_kernels(G, data):
    clock = Clock()
    per = {"fake": [], "real": []}
    for side, a, b in batches(G, data, clock):
        vals = []
        for s, h in enumerate(SIZES):
            with clock(f"scale {h}"):
                vals.append(M.msssim_scale(a, b)[:, 1 if s == SCALES - 1 else 0])
            if s < SCALES - 1:
                with clock("pool"):
                    a, b = M.msssim_pool2(a, b)
        per[side].append(combine(vals))
    return clock.totals(), {k: float(torch.cat(v).mean()) for k, v in per.items()}


def run_torch(G, data):
    clock = Clock()
    win = M.msssim_window().to(DEV)
    kx = win.view(1, 1, 1, 11).expand(5 * C, 1, 1, 11).contiguous()
    ky = win.view(1, 1, 11, 1).expand(5 * C, 1, 11, 1).contiguous()
    c1, c2 = (0.01 * M.DATA_RANGE) ** 2, (0.03 * M.DATA_RANGE) ** 2
    per = {"fake": [], "real": []}
    for side, a, b in batches(G, data, clock):
        a, b = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)              # (P, C, H, H); a view for one colour
        vals = []
        for s, h in enumerate(SIZES):
            with clock(f"scale {h}"):
                mom = F.conv2d(F.conv2d(torch.cat([a, b, a * a, b * b, a * b], 1), kx, groups=5 * C), ky, groups=5 * C)
                ma, mb, eaa, ebb, eab = mom.split(C, 1)
                cs = (2 * (eab - ma * mb) + c2) / ((eaa - ma * ma) + (ebb - mb * mb) + c2)
                if s == SCALES - 1:
                    cs = cs * (2 * ma * mb + c1) / (ma * ma + mb * mb + c1)
                vals.append(cs.double().mean((1, 2, 3)))
            if s < SCALES - 1:
                with clock("pool"):
                    a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
        per[side].append(combine(vals))
    return clock.totals(), {k: float(torch.cat(v).mean()) for k, v in per.items()}


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
    out.append(f"evaluate_msssim, {R} x {R}, C = {C}, {N_PAIRS} pairs per side (generated and data) in minibatches of {BATCH} pairs, "
               f"{SCALES} scales; MI355X, HIP events around the stages, one warm run, median of {RUNS} runs, ms")
    out.append(f"{'stage':<14}{'kernels':>12}{'torch fp32':>12}")
    for s in STAGES + ["total"]:
        out.append(f"{s:<14}{results['kernels'][0][s]:>12.2f}{results['torch fp32'][0][s]:>12.2f}")
    mt = {k: sum(v[0][s] for s in STAGES[2:]) for k, v in results.items()}
    out.append(f"{'metric only':<14}{mt['kernels']:>12.2f}{mt['torch fp32']:>12.2f}   (without producing the images, which both ways share)")
    slower = [s for s in STAGES[2:] if results["kernels"][0][s] > results["torch fp32"][0][s]]
    out.append("stages where the kernels are slower than torch: " + (", ".join(slower) if slower else "none"))
    for k, (_, res) in results.items():
        out.append(f"mean MS-SSIM, {k}: generated {res['fake']:.6f}, data {res['real']:.6f}")
    text = "\n".join(out)
    print(text)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
