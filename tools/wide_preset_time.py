"""One training iteration (PGGANTrainer.train_iteration, eager) with the generator / critic widths of the reference's wide presets
(configs/config.py:87-98) at 32 x 32, batch 4, in the f32 and bf16 modes: median wall time of 10 iterations after 3 warm-up ones.
Informational: the wide layers are a compatibility path in both modes, not a tuned one.
    python tools/wide_preset_time.py > profiles/wide_preset_time.txt"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

PRESETS = {"0004": ([1024, 512, 256, 128, 64, 32, 16, 8], [16, 32, 64, 128, 128, 128, 128]),
           "0008": ([512, 256, 128, 64], [64, 128, 256, 512])}
DEV = "cuda:0"


def main():
    ngan = load_package()
    gen = torch.Generator().manual_seed(3)
    z = [torch.randn(4, 64, generator=gen) for _ in range(3)]
    z = [(v / v.norm(dim=1, keepdim=True)).to(DEV) for v in z]
    real = (torch.rand(4, 1, 32, 32, generator=gen) * 2 - 1).to(DEV)
    eps = torch.rand(4, 1, 1, 1, generator=gen).to(DEV)
    print("preset  mode  ms/iteration (median of 10, eager, 32x32, batch 4)", flush=True)
    for name, (gw, dw) in PRESETS.items():
        for mode in ("f32", "bf16"):
            ngan.ops.set_conv_precision(mode)
            torch.manual_seed(23)
            G = ngan.models.Generator_PG(gw, image_size_init=4, latent_dim=64)
            D = ngan.models.Discriminator_PG(dw, image_size_init=4)
            G.set_resolution(32, 1.0)
            D.set_resolution(32, 1.0)
            tr = ngan.train.PGGANTrainer(G.to(DEV), D.to(DEV), learning_rate=1e-4)
            times = []
            for i in range(13):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.train_iteration(real, z[0], z[1], eps, z[2])
                torch.cuda.synchronize()
                if i >= 3:
                    times.append((time.perf_counter() - t0) * 1e3)
            times.sort()
            print(f"{name}    {mode:5s} {times[len(times) // 2]:.2f}", flush=True)
    ngan.ops.set_conv_precision("f32")


if __name__ == "__main__":
    main()
