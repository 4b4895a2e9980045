"""Time the image-folder load path on N synthetic 512^2 micrograph-like images: NeuronDataset.from_arrays as a whole (upload, noise
statistics, pad-and-fill, device-synchronised, after a warm-up call) and its three entry points separately (HIP events around each:
ngan_u8_histogram, ngan_multiotsu4_noise_stats, ngan_u8_pad_noise_fill in chunks of 32 with the draws already made), next to the
fp64 numpy search of tests/multiotsu_ref.py on the same host for a few of the images.  A record, not a gate.

    python tools/dataset_time.py [--images 64] [--size 512] [--repeats 5] [--host-images 4]   (record: profiles/dataset_dir_time.txt)
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import multiotsu_ref as M  # noqa: E402

pkg = graft.load_package()
from neuron_gan_amd import _C, data  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, repeats):
    """milliseconds of `repeats` runs of fn between HIP events, after one warm-up run"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=4)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "dataset_dir_time.txt"))
    a = ap.parse_args()
    n, r = a.images, a.size
    base = [M.micrograph(100 + i, r) for i in range(min(n, 8))]                      # eight distinct images, repeated
    images = np.stack([base[i % len(base)] for i in range(n)])
    lines = [f"python tools/dataset_time.py --images {n} --size {r} --repeats {a.repeats} --host-images {a.host_images}",
             f"{n} images of {r} x {r} bytes ({len(base)} distinct generator images, repeated), {torch.cuda.get_device_name(0)}", ""]
    fmt = lambda name, ms: f"{name:<44s} median {np.median(ms):9.3f} ms   min {min(ms):9.3f}   max {max(ms):9.3f}"

    def whole():
        data.NeuronDataset.from_arrays(images, device=DEV, fill_seed=1)
        torch.cuda.synchronize()
    whole()                                                                           # warm-up: library load, allocator
    wall = []
    for _ in range(a.repeats):
        t = time.perf_counter()
        whole()
        wall.append(1e3 * (time.perf_counter() - t))
    lines.append(fmt("from_arrays, host bytes -> canvases (wall)", wall))

    dev_images = torch.from_numpy(images).to(DEV)
    hist = torch.empty(n, 256, device=DEV, dtype=torch.int32)
    ws = torch.empty(_C.lib().ngan_multiotsu_workspace_bytes(n), device=DEV, dtype=torch.uint8)
    thr = torch.empty(n, 3, device=DEV, dtype=torch.int32)
    rec = torch.empty(n, 3, device=DEV, dtype=torch.float64)
    status = torch.empty(n, device=DEV, dtype=torch.int32)
    p = r + 2 * (r // 4)
    canvases = torch.empty(n, p, p, device=DEV, dtype=torch.float32)
    chunk = data._FILL_CHUNK
    draws = torch.randn(min(n, chunk), p, p, device=DEV)

    def fill():
        for i in range(0, n, chunk):
            c = min(chunk, n - i)
            _C.call("ngan_u8_pad_noise_fill", dev_images[i:i + c], draws[:c], rec[i:i + c], canvases[i:i + c], c, r)
    lines.append(fmt("ngan_u8_histogram", timed(lambda: _C.call("ngan_u8_histogram", dev_images, hist, n, r * r), a.repeats)))
    lines.append(fmt("ngan_multiotsu4_noise_stats (search + finish)",
                     timed(lambda: _C.call("ngan_multiotsu4_noise_stats", hist, ws, thr, rec, status, n), a.repeats)))
    lines.append(fmt(f"ngan_u8_pad_noise_fill ({-(-n // chunk)} launches)", timed(fill, a.repeats)))
    lines.append(fmt(f"torch.randn of one chunk ({draws.shape[0]} x {p} x {p})",
                     timed(lambda: torch.randn(draws.shape, device=DEV), a.repeats)))
    assert int(status.abs().sum()) == 0

    host = []
    thr_host = thr.cpu().numpy()
    for i in range(min(a.host_images, n)):
        h = np.bincount(images[i].ravel(), minlength=256)
        t = time.perf_counter()
        triplet, _, _ = M.multiotsu4(h)
        host.append(1e3 * (time.perf_counter() - t))
        assert tuple(int(v) for v in thr_host[i]) == triplet
    lines.append(fmt("numpy fp64 search, ONE image, this host", host))
    lines.append("")
    lines.append(f"thresholds of image 0: {tuple(int(v) for v in thr_host[0])}; noise mean / std {float(rec[0, 1]):.4f} / {float(rec[0, 2]):.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
