"""The image-folder data set on the GPU (csrc/dataset.hip, data.noise_statistics, NeuronDataset.from_arrays / from_directory and the
command line's --dataset_dir) against numpy: np.bincount for the histogram, tests/multiotsu_ref.py (the definition of include/ngan.h
in fp64 numpy) for the thresholds, np.mean / np.std of the selected pixels for the noise record, and a numpy restatement of the
reference's Pad + replace_zero_with_noise + ToTensor for the canvases.

Thresholds are compared for equality, which is fair only where fp64 rounding cannot decide the winner: every generator image used
below has a relative gap of at least 1e-9 between its best and its second-best distinct partition (asserted on the reference's own
output before the kernel is looked at; fp64 evaluation noise of a four-term sum is about 1e-15)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import multiotsu_ref as M
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MIN_GAP = 1e-9
# (size, seeds) of the generator images of the statistics test: ten of 64^2 / 128^2 and two of 512^2
STAT_BATCHES = ((64, (1, 2, 3, 4, 5)), (128, (11, 12, 13, 14, 16)), (512, (22, 23)))


def _histogram(ngan, images):
    """ngan_u8_histogram of a (N, R, R) uint8 device tensor -> (N, 256) numpy counts; the output starts as garbage (overwritten)"""
    n, r, _ = images.shape
    hist = torch.full((n, 256), 12345, device=images.device, dtype=torch.int32)
    ngan._C.call("ngan_u8_histogram", images, hist, n, r * r)
    return hist.cpu().numpy()


def _bincounts(images):
    return np.stack([np.bincount(im.ravel(), minlength=256) for im in images])


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("r", [64, 100, 512])
def test_histogram_equals_bincount(ngan, n, r):
    rng = np.random.default_rng(100 * r + n)
    cases = {
        "random": rng.integers(0, 256, (n, r, r), dtype=np.uint8),
        "micrograph": np.stack([M.micrograph(1000 + r + i, r) for i in range(n)]),
        "one level": np.full((n, r, r), 0 if n == 1 else 137, dtype=np.uint8),
    }
    for name, images in cases.items():
        got = _histogram(ngan, torch.from_numpy(images).to(DEV))
        assert np.array_equal(got, _bincounts(images)), name
        assert got.sum() == n * r * r


@pytest.mark.parametrize("r,offset", [(37, 0), (37, 5), (64, 3), (3, 1)])
def test_histogram_of_unaligned_images(ngan, r, offset):
    """pixels a multiple of nothing and a base address off the 16-byte grid: the scalar head and tail around the 16-byte loads"""
    n = 3
    images = np.random.default_rng(r + offset).integers(0, 256, (n, r, r), dtype=np.uint8)
    flat = torch.zeros(offset + n * r * r, device=DEV, dtype=torch.uint8)
    view = flat[offset:].view(n, r, r)
    view.copy_(torch.from_numpy(images))
    assert view.data_ptr() % 16 == offset % 16
    assert np.array_equal(_histogram(ngan, view), _bincounts(images))


@pytest.mark.parametrize("size,seeds", STAT_BATCHES)
def test_thresholds_and_noise_record_equal_the_reference(ngan, size, seeds):
    images = np.stack([M.micrograph(s, size) for s in seeds])
    want = []
    for seed, img in zip(seeds, images):
        triplet, best, second = M.multiotsu4(np.bincount(img.ravel(), minlength=256))
        gap = M.relative_gap(best, second)
        print(f"size {size} seed {seed}: reference thresholds {triplet}, relative gap to the next distinct partition {gap:.3e}")
        assert gap >= MIN_GAP, (seed, gap)                    # a condition on the input, checked before the kernel is looked at
        want.append((triplet,) + M.noise_record(img, triplet[0]))
    thresholds, count, mean, std = ngan.data.noise_statistics(torch.from_numpy(images).to(DEV))
    for i, (triplet, n, m, s) in enumerate(want):
        rel_m, rel_s = abs(mean[i] - m) / m, abs(std[i] - s) / s
        print(f"size {size} seed {seeds[i]}: kernel thresholds {tuple(int(t) for t in thresholds[i])}, count {int(count[i])} (reference {n}), "
              f"relative error of mean {rel_m:.2e}, of std {rel_s:.2e}")
        assert tuple(int(t) for t in thresholds[i]) == triplet
        assert int(count[i]) == n
        assert rel_m <= 1e-12 and rel_s <= 1e-12
    assert mean.dtype == np.float64 and std.dtype == np.float64


def test_tie_classes_resolve_to_the_smallest_triplet(ngan):
    """sparse histograms: many triplets cut the occupied levels the same way and score bit-identically; the smallest one wins,
    whichever workgroup found it"""
    rng = np.random.default_rng(9)
    images = []
    for levels in ([1, 2, 3, 60, 61, 140, 141, 250], [0, 5, 6, 7, 90, 170, 171, 255], [4, 5, 6, 7, 8, 9, 10, 11],
                   [2, 3, 120, 121, 122, 200, 201, 202, 203, 254]):
        images.append(rng.choice(np.array(levels, dtype=np.uint8), size=(32, 32)))
    images = np.stack(images)
    thresholds, count, mean, std = ngan.data.noise_statistics(torch.from_numpy(images).to(DEV))
    for i, img in enumerate(images):
        triplet, best, second = M.multiotsu4(np.bincount(img.ravel(), minlength=256))
        assert M.relative_gap(best, second) >= MIN_GAP
        assert tuple(int(t) for t in thresholds[i]) == triplet, i
        n, m, s = M.noise_record(img, triplet[0])
        assert int(count[i]) == n and abs(mean[i] - m) <= 1e-12 * m and abs(std[i] - s) <= 1e-12 * s


def test_images_without_thresholds_or_noise_floor_are_refused(ngan):
    rng = np.random.default_rng(3)
    good = [M.micrograph(1, 64), M.micrograph(2, 64)]
    three = rng.choice(np.array([0, 40, 90], dtype=np.uint8), size=(64, 64))
    floorless = rng.choice(np.array([0, 50, 100, 200], dtype=np.uint8), size=(64, 64))
    stats = lambda imgs: ngan.data.noise_statistics(torch.from_numpy(np.stack(imgs)).to(DEV))
    with pytest.raises(ValueError, match=r"image 1\b.*four grey levels"):
        stats([good[0], three, good[1]])
    with pytest.raises(ValueError, match=r"image 2\b.*no pixel lies strictly between 0 and its lowest threshold"):
        stats([good[0], good[1], floorless])
    with pytest.raises(ValueError, match=r"image 0\b"):
        ngan.data.NeuronDataset.from_arrays(np.stack([three, good[0]]), device=DEV)
    # the other images of those batches, on their own: unaffected
    thresholds, count, mean, std = stats(good)
    for i, img in enumerate(good):
        triplet, _, _ = M.multiotsu4(np.bincount(img.ravel(), minlength=256))
        n, m, s = M.noise_record(img, triplet[0])
        assert tuple(int(t) for t in thresholds[i]) == triplet and int(count[i]) == n
        assert abs(mean[i] - m) <= 1e-12 * m and abs(std[i] - s) <= 1e-12 * s


def _fill(ngan, images, normals, record):
    n, r, _ = images.shape
    p = r + 2 * (r // 4)
    out = torch.full((n, p, p), -7.0, device=DEV, dtype=torch.float32)
    ngan._C.call("ngan_u8_pad_noise_fill", torch.from_numpy(images).to(DEV), torch.from_numpy(normals).to(DEV),
                 torch.from_numpy(record).to(DEV), out, n, r)
    return out.cpu().numpy()


@pytest.mark.parametrize("r,n", [(64, 3), (100, 2), (5, 3), (16, 33)])
def test_pad_and_fill_equals_the_reference_bit_for_bit(ngan, r, n):
    """(5, 3): 147 canvas pixels, not a multiple of four -- the scalar tail after the 16-byte stores.  The records put the noise
    inside the range, mostly below 0 and mostly above 255 in turn, so that both clamps act."""
    rng = np.random.default_rng(r * 10 + n)
    if r >= 64:
        images = np.stack([M.micrograph(50 + i, r) for i in range(n)])
    else:
        images = rng.integers(0, 4, (n, r, r)).astype(np.uint8) * rng.integers(1, 86, (n, r, r)).astype(np.uint8)
    pad = r // 4
    p = r + 2 * pad
    normals = rng.standard_normal((n, p, p)).astype(np.float32)
    record = np.zeros((n, 3), dtype=np.float64)
    record[:, 0] = 1000.0
    record[:, 1] = np.resize([18.037, 1.5, 251.25], n) + rng.uniform(0, 0.5, n)
    record[:, 2] = np.resize([4.0123, 6.0, 9.5], n) + rng.uniform(0, 0.5, n)
    got = _fill(ngan, images, normals, record)
    want = M.pad_noise_fill(images, normals, record[:, 1], record[:, 2])
    assert got.dtype == np.float32 and got.shape == (n, p, p)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    levels = np.rint(got.astype(np.float64) * 255.0)
    assert np.array_equal(got, levels.astype(np.float32) / np.float32(255.0))          # multiples of 1/255 as float32 divisions
    inner = got[:, pad:pad + r, pad:pad + r]
    assert np.array_equal(inner[images != 0], images[images != 0].astype(np.float32) / np.float32(255.0))   # no non-zero pixel changed
    ring = np.ones((p, p), dtype=bool)
    ring[pad:pad + r, pad:pad + r] = False
    noise = np.trunc(np.clip(record[:, 2, None, None] * normals.astype(np.float64) + record[:, 1, None, None], 0.0, 255.0))
    assert np.array_equal(levels[:, ring], noise[:, ring])                              # the pad ring is noise
    assert np.array_equal(levels[:, pad:pad + r, pad:pad + r][images == 0], noise[:, pad:pad + r, pad:pad + r][images == 0])
    if n >= 3:
        assert (levels[1] == 0).any() and (levels[2] == 255).any() and 0 < np.median(levels[0][ring]) < 255


def test_from_arrays_feeds_the_augmentation_kernel(ngan):
    r, seeds = 64, (1, 2, 3)
    images = np.stack([M.micrograph(s, r) for s in seeds])
    pad = r // 4
    p = r + 2 * pad
    normals = torch.from_numpy(np.random.default_rng(4).standard_normal((len(seeds), p, p)).astype(np.float32))
    ds = ngan.data.NeuronDataset.from_arrays(images, augmentations=False, device=DEV, normals=normals, filenames=["a", "b", "c"])
    assert len(ds) == 3 and ds.image_size == ds.image_size_max == r and ds.canvas == p and ds.load_all
    assert list(ds.filenames) == ["a", "b", "c"]
    # the canvases are the reference's, from the statistics the data set reports
    assert ds.images_noise_mean.dtype == np.float64 and ds.images_noise_std.shape == (3,) and ds.noise_thresholds.shape == (3, 3)
    want = M.pad_noise_fill(images, normals.numpy(), ds.images_noise_mean, ds.images_noise_std)
    canvases = ds.images.cpu()
    assert np.array_equal(canvases.numpy(), want)
    for i, img in enumerate(images):
        triplet, _, _ = M.multiotsu4(np.bincount(img.ravel(), minlength=256))
        assert tuple(int(t) for t in ds.noise_thresholds[i]) == triplet
    crop = canvases[:, pad:pad + r, pad:pad + r] * 2 - 1
    full = ds.batch([2, 0]).cpu()
    assert torch.allclose(full[:, 0], crop[[2, 0]], atol=1e-6)
    ds.set_image_size(16)
    small = ds.batch([1]).cpu()
    ref = F.interpolate(crop[1][None, None], size=(16, 16), mode="bilinear", antialias=True, align_corners=False)
    assert torch.allclose(small, ref, atol=1e-5)
    # the device generator of the draws: the same fill_seed gives the same canvases, another one does not; chunks of 32 images
    many = np.stack([images[i % 3] for i in range(35)])
    a = ngan.data.NeuronDataset.from_arrays(many, device=DEV, fill_seed=11)
    b = ngan.data.NeuronDataset.from_arrays(many, device=DEV, fill_seed=11)
    c = ngan.data.NeuronDataset.from_arrays(many, device=DEV, fill_seed=12)
    assert torch.equal(a.images, b.images) and not torch.equal(a.images, c.images)
    inner = a.images[:, pad:pad + r, pad:pad + r].cpu().numpy()
    assert np.array_equal(inner[many != 0], many[many != 0].astype(np.float32) / np.float32(255.0))
    assert float(a.images.min()) >= 0.0 and float(a.images[34, :pad].mean()) > 10.0 / 255.0     # the last chunk's ring is filled


def _tiny_image(seed):
    """16 x 16 bytes: a zero border, a noise floor of levels 14..22 and three brighter clusters, so that every status is 0"""
    rng = np.random.default_rng(seed)
    a = np.zeros((16, 16), dtype=np.uint8)
    a[2:14, 2:14] = rng.integers(14, 23, (12, 12))
    a[3:6, 3:8] = rng.integers(57, 64, (3, 5))
    a[7:10, 4:9] = rng.integers(117, 124, (3, 5))
    a[10:13, 6:11] = rng.integers(197, 204, (3, 5))
    return a


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_a_folder_of_pngs_loads_and_trains_from_the_command_line(ngan, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    folder = tmp_path / "real_images"
    folder.mkdir()
    images = np.stack([_tiny_image(s) for s in range(8)])
    for i in (5, 0, 3, 7, 1, 6, 2, 4):
        Image.fromarray(images[i]).save(folder / f"neuron_{i:02d}.png")
    (folder / ".hidden").write_bytes(b"not an image")
    a = ngan.data.NeuronDataset.from_directory(str(folder), image_size=16, device=DEV, fill_seed=3, seed=1)
    b = ngan.data.NeuronDataset.from_arrays(images, device=DEV, fill_seed=3, seed=1)
    assert len(a) == 8 and [os.path.basename(f) for f in a.filenames] == [f"neuron_{i:02d}.png" for i in range(8)]
    assert torch.equal(a.images, b.images) and a.images.shape == (8, 24, 24)
    assert np.array_equal(a.images_noise_mean, b.images_noise_mean) and np.array_equal(a.noise_thresholds, b.noise_thresholds)

    conf = tmp_path / "tiny.py"
    lines = [f"{d}_dir = {str(tmp_path / d)!r}" for d in ("images", "weights", "plots", "logs")]
    lines += ["ID = 'dd01'", "N_epochs = 2", "checkpointing_period = 2", "batch_size = 8", "n_critic = 1", "learning_rate = 1e-3",
              "pggan = True", "wgan = False", "image_size = 16", "N_gen_features = [32, 16]", "N_dis_features = [16, 32]",
              "transit_sch = [1]", "alpha_step = 1.0", "grad_pen_lambda = 10.0"]
    conf.write_text("\n".join(lines) + "\n")
    cmd = [sys.executable, os.path.join(ROOT, "neuron-gan_amd", "launch.py"), "--configs", str(conf), "--dataset_dir"]

    def run(directory):
        env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
        return subprocess.run(cmd + [str(directory)], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)

    out = run(folder)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    found = [os.path.join(d, f) for d, _, fs in os.walk(tmp_path) for f in fs if f == "GenDisc_dd01.pth"]
    assert len(found) == 1, found
    line = [l for l in out.stdout.splitlines() if l.startswith("Dataset:")]
    assert len(line) == 1 and str(folder) in line[0] and "8 images" in line[0], out.stdout[-2000:]

    missing = tmp_path / "no_such_folder"
    out = run(missing)
    assert out.returncode != 0
    assert "The dataset path {} does not exist.".format(missing) in out.stderr, out.stderr[-4000:]
