"""Time `evaluate_spectrum` at the default setting (512 x 512, C = 1, 8192 images per side) two ways: through the kernels of
csrc/spectrum.hip, and through a plain-torch fp32 restatement on the GPU (torch.fft.rfft2 of the windowed images, |F|^2, index_add_
over a precomputed ring index with the Hermitian weights).  HIP events around every stage, one warm run, the median of --runs runs.
Then `radial_spectrum` alone at (64, 512, 512, 1) and (64, 64, 64, 1), both ways, with the bytes the kernels must move (the image
read once, the half spectrum written and read back) over the measured time.  A record, not a gate.

    python tools/spectrum_time.py [--images 8192] [--runs 3] [--out profiles/spectrum_time.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

pkg = g.load_package()
M = pkg.metrics
DEV = torch.device("cuda:0")
parser = argparse.ArgumentParser()
parser.add_argument("--images", type=int, default=8192)
parser.add_argument("--runs", type=int, default=3)
parser.add_argument("--out", type=str, default="")
ARGS = parser.parse_args()
R, C, N_IMAGES, BATCH, RUNS = 512, 1, ARGS.images, 64, ARGS.runs
STAGES = ["fakes", "reals", "spectrum"]


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
    """(side, images): channels-last minibatches, a real one and a generated one in turn, as evaluate_spectrum produces them"""
    lat = torch.Generator(device="cpu").manual_seed(2)
    n_data = len(data)
    for i in range(0, N_IMAGES, BATCH):
        n = min(BATCH, N_IMAGES - i)
        with clock("reals"):
            x = M.channels_last(data.batch([(i + j) % n_data for j in range(n)]))
        yield "real", x
        z = torch.randn(n, G.latent_dim, generator=lat).clamp(-5, 5)
        z = (z / z.norm(p=2, dim=1, keepdim=True)).to(DEV)
        with clock("fakes"), torch.no_grad():
            x = M.channels_last(G(z).detach())
        yield "fake", x


class TorchSpectrum:
    """the plain-torch fp32 restatement for one image size: rfft2, |F|^2, index_add_ over the ring index"""

    def __init__(self, size):
        self.size, self.bins = size, size // 2 + 1
        h = M.spectrum_window(size).to(DEV)
        self.w = (h[:, None] * h[None, :]).view(1, size, size, 1)
        self.norm = float(h.double().square().sum() ** 2)
        fy = torch.arange(size, device=DEV)
        fy = torch.where(fy < size // 2, fy, fy - size)
        fx = torch.arange(self.bins, device=DEV)
        d = fy[:, None] ** 2 + fx[None, :] ** 2
        k = torch.floor(torch.sqrt(d.double()) + 0.5).long()
        self.keep = (k <= size // 2).view(-1)
        self.index = k.clamp_max(size // 2).view(-1)
        wt = torch.full((self.bins,), 2.0, device=DEV)
        wt[0] = wt[-1] = 1.0
        self.weight = (wt.view(1, -1).expand(size, -1).reshape(-1) * self.keep).view(1, 1, -1)
        self.counts = M.spectrum_ring_counts(size).to(DEV).double()

    def __call__(self, x):
        f = torch.fft.rfft2((x * self.w).permute(0, 3, 1, 2))
        p = (f.real.square() + f.imag.square()).reshape(x.shape[0], x.shape[3], -1) * self.weight
        out = torch.zeros(x.shape[0], self.bins, device=DEV, dtype=torch.float32)
        out.index_add_(1, self.index, p.sum(1))
        return out.double() / (x.shape[3] * self.counts * self.norm)


def run(G, data, spectrum):
    clock = Clock()
    sums = {"real": 0.0, "fake": 0.0}
    for side, x in batches(G, data, clock):
        with clock("spectrum"):
            s = spectrum(x)
            sums[side] = sums[side] + s.sum(0)
    tot = clock.totals()
    ratio = 10.0 * torch.log10(sums["fake"] / sums["real"])
    return tot, float(ratio[R // 4 + 1:].mean())


def time_alone(fn, x, reps=20):
    for _ in range(3):
        fn(x)
    torch.cuda.synchronize()
    times = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn(x)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / reps)
    return statistics.median(times)


def main():
    G, data = make_inputs()
    out = []
    ways = [("kernels", M.radial_spectrum)]
    try:
        torch_way = TorchSpectrum(R)
        torch_way(torch.zeros(2, R, R, C, device=DEV))
        torch.cuda.synchronize()
        ways.append(("torch fp32", torch_way))
    except Exception as e:                                   # no usable torch.fft on this machine: the kernel path alone, and said
        out.append(f"torch.fft is not usable here ({type(e).__name__}: {e}): the kernel path alone")
    results = {}
    for name, fn in ways:
        t0 = time.time()
        run(G, data, fn)                # warm
        torch.cuda.synchronize()
        print(f"{name}: warm run {time.time() - t0:.1f} s wall", flush=True)
        runs = []
        for _ in range(RUNS):
            tot, high = run(G, data, fn)
            runs.append(tot)
            print(f"  {name}: {sum(tot.values()):.1f} ms", flush=True)
        med = {s: statistics.median(r[s] for r in runs) for s in STAGES}
        med["total"] = statistics.median(sum(r.values()) for r in runs)
        results[name] = (med, high)
    names = [n for n, _ in ways]
    out.append(f"evaluate_spectrum, {R} x {R}, C = {C}, {N_IMAGES} images per side (data and generated) in minibatches of {BATCH}; "
               f"MI355X, HIP events around the stages, one warm run, median of {RUNS} runs, ms")
    out.append(f"{'stage':<14}" + "".join(f"{n:>12}" for n in names))
    for s in STAGES + ["total"]:
        out.append(f"{s:<14}" + "".join(f"{results[n][0][s]:>12.2f}" for n in names))
    share = results["kernels"][0]["spectrum"] / results["kernels"][0]["total"]
    out.append(f"the metric's own share of an evaluation through the kernels: {100 * share:.1f} % (the rest produces the images)")
    for n in names:
        out.append(f"high_db, {n}: {results[n][1]:+.4f}")
    out.append("")
    out.append(f"radial_spectrum alone, median of {RUNS} x 20 calls, ms; floor = bytes / 5 TB/s, bytes = image read + half spectrum "
               "written and read back")
    out.append(f"{'shape':<20}" + "".join(f"{n:>12}" for n in names) + f"{'MB':>10}{'floor':>10}{'floor / kernels':>18}")
    for shape in ((64, 512, 512, 1), (64, 64, 64, 1)):
        b, r, _, c = shape
        x = torch.rand(*shape, device=DEV) * 2 - 1
        fns = [M.radial_spectrum] + ([TorchSpectrum(r)] if len(ways) > 1 else [])
        ms = [time_alone(f, x) for f in fns]
        nbytes = b * c * (r * r * 4 + 2 * (r // 2 + 1) * r * 8)
        floor = nbytes / 5e12 * 1e3
        out.append(f"{str(shape):<20}" + "".join(f"{t:>12.4f}" for t in ms) + f"{nbytes / 1e6:>10.1f}{floor:>10.4f}{floor / ms[0]:>18.3f}")
        if len(ms) > 1 and ms[0] > ms[1]:
            out.append(f"  the kernels are slower than torch at {shape}: {ms[0] / ms[1]:.2f} x")
    text = "\n".join(out)
    print(text)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
