"""Device-resident dataset with the reference's augmentation chain.

Restates /root/reference/data/NeuronDataset.py for the HIP path: `NeuronDataset` keeps every image on the GPU (the reference's
`load_all` mode, which its on-device `DatasetIterator` requires, NeuronDataset.py:171-175) already padded by image_size // 4
(NeuronDataset.py:70-71) and, when noise statistics are given, with the zero pixels replaced by Gaussian noise (13-21).  A batch
is produced by ONE call of `ngan_augment_batch` (csrc/augment.hip): RandomAffine(degrees=180, translate=(t, t), nearest, fill 0),
RandomVerticalFlip, ColorJitter(brightness 0.25, contrast 0.25, random order), CenterCrop, Renormalize((0,1) -> (-1,1)) and the
antialiased Resize to the current stage's resolution (112-126, 149-164) -- instead of the reference's per-image Python loop
(NeuronDataset.py:199-207), which could not feed a step that consumes ~2 000 images per second.

A folder of images is loaded by `NeuronDataset.from_directory` (the reference's constructor surface, NeuronDataset.py:46-110): PIL
decodes the 8-bit greyscale files on the host, and the arithmetic of the load loop runs on the device for the whole folder at once
(csrc/dataset.hip): `ngan_u8_histogram`, `ngan_multiotsu4_noise_stats` (the 4-class multi-Otsu thresholds that
`skimage.filters.threshold_multiotsu(img, classes=4)` searches for, and the mean / standard deviation of the pixels between zero and
the lowest threshold, NeuronDataset.py:93-97) and `ngan_u8_pad_noise_fill` (Pad + replace_zero_with_noise + ToTensor, 13-19, 100-107).
`noise_statistics` and `NeuronDataset.from_arrays` are the same path for bytes that are already in memory.  Deviations from the
reference, all stated in INTEGRATION.md: files are read in sorted order; class scores are fp64 where skimage's table is float32;
noise outside [0, 255] is clamped where the reference's uint8 assignment wraps; 8-bit mode `L` images only.

Neither skimage nor torchvision is installed here, so parity with the libraries themselves is unpinned: the thresholds are pinned
against a numpy fp64 restatement of the definition in include/ngan.h (tests/multiotsu_ref.py), the augmentation chain against a
plain-torch CPU restatement of torchvision's tensor code path (tests/test_gpu_data.py).
"""
import math
import os

import numpy as np
import torch

from . import _C


def _as_images(images):
    if images.dim() == 3:
        images = images.unsqueeze(1)
    if images.dim() != 4 or images.shape[1] != 1 or images.shape[2] != images.shape[3]:
        raise ValueError(f"expected square single-colour images (N, 1, R, R) or (N, R, R), got {tuple(images.shape)}")
    return images.float()


_FILL_CHUNK = 32     # images per launch of the pad-and-fill: bounds the normal draws held at once (32 x 768^2 fp32 = 75 MB at R = 512)


def _as_bytes(images_u8, device):
    """(N, R, R) 8-bit images, numpy or torch, host or device -> a contiguous torch.uint8 tensor on `device`"""
    if isinstance(images_u8, np.ndarray):
        if images_u8.dtype != np.uint8:
            raise ValueError(f"expected 8-bit images (uint8), got {images_u8.dtype}")
        images_u8 = torch.from_numpy(np.ascontiguousarray(images_u8))
    if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8:
        raise ValueError(f"expected a uint8 array or tensor, got {getattr(images_u8, 'dtype', type(images_u8))}")
    if images_u8.dim() != 3 or images_u8.shape[0] == 0 or images_u8.shape[1] != images_u8.shape[2]:
        raise ValueError(f"expected square single-colour 8-bit images (N, R, R), got {tuple(images_u8.shape)}")
    return images_u8.to(device).contiguous()


def _noise_statistics(images_u8):
    """the two launches and the one read-back of `noise_statistics`; also returns the device-resident (N, 3) fp64 records"""
    n, r, _ = images_u8.shape
    dev = images_u8.device
    hist = torch.empty(n, 256, device=dev, dtype=torch.int32)
    ws = torch.empty(_C.lib().ngan_multiotsu_workspace_bytes(n), device=dev, dtype=torch.uint8)
    thresholds = torch.empty(n, 3, device=dev, dtype=torch.int32)
    record = torch.empty(n, 3, device=dev, dtype=torch.float64)
    status = torch.empty(n, device=dev, dtype=torch.int32)
    _C.call("ngan_u8_histogram", images_u8, hist, n, r * r)
    _C.call("ngan_multiotsu4_noise_stats", hist, ws, thresholds, record, status, n)
    host = torch.cat([thresholds.double(), record, status.double().unsqueeze(1)], dim=1).cpu().numpy()   # the one read-back
    for i in np.flatnonzero(host[:, 6]):
        why = ("fewer than four grey levels occur in it (threshold_multiotsu needs four classes)" if host[i, 6] == 1 else
               "no pixel lies strictly between 0 and its lowest threshold: there is no noise floor to measure")
        raise ValueError(f"image {int(i)}: {why}")
    return host[:, 0:3].astype(np.int64), host[:, 3].astype(np.int64), host[:, 4].copy(), host[:, 5].copy(), record


def noise_statistics(images_u8):
    """(thresholds (N, 3) int, count (N,) int, mean (N,), std (N,) float64, in grey levels) of (N, R, R) torch.uint8 images on the
    GPU: per image the 4-class multi-Otsu thresholds and the statistics of the pixels 0 < v < thresholds[0] (reference
    NeuronDataset.py:93-97).  ValueError names the first image that has fewer than four grey levels or no such pixel."""
    if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() != 3:
        raise ValueError("expected a (N, R, R) torch.uint8 tensor")
    return _noise_statistics(images_u8.contiguous())[:4]


def read_image_folder(directory, image_size=None):
    """((N, R, R) uint8 array, file names) of every regular file of `directory` whose name does not start with a dot, in sorted order
    (the reference takes os.listdir's order, NeuronDataset.py:63-64), decoded by PIL on the host: 8-bit greyscale (mode `L`), square,
    all of one size (`image_size` when given).  Anything else is a ValueError that names the file."""
    if not os.path.exists(directory):
        raise ValueError('The dataset path {} does not exist.'.format(directory))
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("reading an image folder needs PIL (the `pillow` package); without it, decode the files yourself and "
                          "use NeuronDataset.from_arrays") from e
    names = sorted(f for f in os.listdir(directory) if not f.startswith('.') and os.path.isfile(os.path.join(directory, f)))
    if not names:
        raise ValueError('The dataset path {} holds no image file.'.format(directory))
    filenames = [os.path.join(directory, f) for f in names]
    arrays = []
    for filename in filenames:
        with Image.open(filename) as img:
            if img.mode != 'L':
                raise ValueError(f"{filename}: mode {img.mode!r}; only 8-bit greyscale (mode 'L') images are supported")
            arr = np.array(img)
        if arr.ndim != 2 or arr.shape[0] != arr.shape[1]:
            raise ValueError(f"{filename}: {arr.shape[1]} x {arr.shape[0]} pixels; images must be square")
        want = int(image_size) if image_size else arrays[0].shape[0] if arrays else arr.shape[0]
        if arr.shape[0] != want:
            raise ValueError(f"{filename}: {arr.shape[0]} pixels wide, expected {want}" +
                             (" (image_size)" if image_size else f" as {filenames[0]}"))
        arrays.append(arr)
    return np.stack(arrays), filenames


class NeuronDataset:
    def __init__(self, images, image_size=None, augmentations=True, im_translation=0.0, device="cuda", noise_mean=None,
                 noise_std=None, seed=None):
        images = _as_images(images)
        n, _, r, _ = images.shape
        self.image_size = self.image_size_max = int(image_size or r)
        if self.image_size_max != r:
            raise ValueError(f"images are {r} pixels wide, image_size is {self.image_size_max}")
        self.augmentations = bool(augmentations)
        self.im_translation = float(im_translation)
        self.device = torch.device(device)
        self.load_all = True
        pad = r // 4                                                            # NeuronDataset.py:70
        self.canvas = r + 2 * pad
        padded = torch.zeros(n, self.canvas, self.canvas)
        padded[:, pad:pad + r, pad:pad + r] = images[:, 0]
        self.gen = torch.Generator(device="cpu")
        if seed is not None:
            self.gen.manual_seed(int(seed))
        if noise_mean is not None:                                              # replace_zero_with_noise, NeuronDataset.py:13-21
            mean = torch.as_tensor(noise_mean, dtype=torch.float32).reshape(-1, 1, 1)
            std = torch.as_tensor(noise_std, dtype=torch.float32).reshape(-1, 1, 1)
            noise = torch.randn(padded.shape, generator=self.gen) * std + mean
            padded = torch.where(padded == 0, noise, padded)
        self.images = padded.to(self.device).contiguous()
        self._ws = None

    @classmethod
    def from_arrays(cls, images_u8, augmentations=True, im_translation=0.0, device="cuda", seed=None, fill_seed=None, normals=None,
                    filenames=None):
        """The reference's load loop (NeuronDataset.py:84-107) for (N, R, R) 8-bit images in memory: noise statistics by multi-Otsu,
        pad by R // 4, Gaussian noise of those statistics in every zero pixel -- all on the device.  `fill_seed` seeds the device
        generator of the normal draws; `normals` (N, P, P), P = R + 2 * (R // 4), replaces them.  `seed` seeds the augmentation
        stream, as in the constructor."""
        device = torch.device(device)
        images_u8 = _as_bytes(images_u8, device)
        n, r, _ = images_u8.shape
        pad = r // 4                                                            # NeuronDataset.py:70
        canvas = r + 2 * pad
        if normals is not None and tuple(normals.shape) != (n, canvas, canvas):
            raise ValueError(f"normals must be {(n, canvas, canvas)}, got {tuple(normals.shape)}")
        thresholds, _, mean, std, record = _noise_statistics(images_u8)
        self = cls.__new__(cls)
        self.image_size = self.image_size_max = r
        self.augmentations = bool(augmentations)
        self.im_translation = float(im_translation)
        self.device = device
        self.load_all = True
        self.canvas = canvas
        self.gen = torch.Generator(device="cpu")
        if seed is not None:
            self.gen.manual_seed(int(seed))
        fill_gen = torch.Generator(device=device)
        if fill_seed is not None:
            fill_gen.manual_seed(int(fill_seed))
        self.images = torch.empty(n, canvas, canvas, device=device, dtype=torch.float32)
        for i in range(0, n, _FILL_CHUNK):
            c = min(_FILL_CHUNK, n - i)
            if normals is None:
                draws = torch.randn(c, canvas, canvas, generator=fill_gen, device=device, dtype=torch.float32)
            else:
                draws = normals[i:i + c].to(device=device, dtype=torch.float32).contiguous()
            _C.call("ngan_u8_pad_noise_fill", images_u8[i:i + c], draws, record[i:i + c], self.images[i:i + c], c, r)
        self.images_noise_mean, self.images_noise_std = mean, std             # NeuronDataset.py:86-97, grey levels
        self.noise_thresholds = thresholds
        self.filenames = None if filenames is None else np.array(list(filenames))
        self._ws = None
        return self

    @classmethod
    def from_directory(cls, directory, image_size=None, augmentations=True, im_translation=0.0, device="cuda", seed=None,
                       fill_seed=None, normals=None):
        """NeuronDataset(directory=...) of the reference (NeuronDataset.py:46-110): every regular file of the folder whose name does
        not start with a dot, in sorted order, decoded by PIL; 8-bit greyscale (mode `L`), square, all of one size."""
        arrays, filenames = read_image_folder(directory, image_size)
        return cls.from_arrays(arrays, augmentations=augmentations, im_translation=im_translation, device=device, seed=seed,
                               fill_seed=fill_seed, normals=normals, filenames=filenames)

    def __len__(self):
        return self.images.shape[0]

    def set_image_size(self, size: int):
        assert size <= self.image_size_max, 'The image size ({}) must be < {}.'.format(size, self.image_size_max)
        assert self.image_size_max % size == 0, 'The image size ({}) must divide {}.'.format(size, self.image_size_max)
        self.image_size = int(size)

    # ---- random draws of one batch (torchvision's distributions: RandomAffine.get_params, RandomVerticalFlip, ColorJitter) ----
    def draw_params(self, batch):
        g = self.gen
        if not self.augmentations:
            z, o = torch.zeros(batch), torch.ones(batch)
            return dict(angle=z, tx=z, ty=z, flip=z.int(), brightness=o, contrast=o, contrast_first=z.int())
        u = lambda lo, hi: torch.empty(batch).uniform_(lo, hi, generator=g)
        max_d = self.im_translation * self.canvas
        return dict(angle=u(-180.0, 180.0), tx=torch.round(u(-max_d, max_d)) if max_d > 0 else torch.zeros(batch),
                    ty=torch.round(u(-max_d, max_d)) if max_d > 0 else torch.zeros(batch),
                    flip=(torch.rand(batch, generator=g) < 0.5).int(),
                    brightness=u(0.75, 1.25), contrast=u(0.75, 1.25),
                    contrast_first=(torch.rand(batch, generator=g) < 0.5).int())

    @staticmethod
    def pack_params(p):
        """host dict of per-sample tensors -> the (B, 8) record array of include/ngan.h"""
        b = p["angle"].shape[0]
        rad = p["angle"].double() * (math.pi / 180.0)
        rec = torch.zeros(b, 8, dtype=torch.float32)
        rec[:, 0], rec[:, 1] = torch.cos(rad).float(), torch.sin(rad).float()
        rec[:, 2], rec[:, 3] = p["tx"].float(), p["ty"].float()
        rec[:, 4], rec[:, 5] = p["brightness"].float(), p["contrast"].float()
        ints = rec.view(torch.int32)
        ints[:, 6], ints[:, 7] = p["flip"].int(), p["contrast_first"].int()
        return rec

    def batch(self, indices, params=None):
        """(B, 1, S, S) augmented images in [-1, 1] at the current stage resolution for the given image indices."""
        idx = torch.as_tensor(indices, dtype=torch.int32)
        b = idx.numel()
        if b == 0:
            raise ValueError("empty batch")
        if int(idx.min()) < 0 or int(idx.max()) >= len(self):
            raise IndexError("image index out of range")
        rec = self.pack_params(params if params is not None else self.draw_params(b)).to(self.device, non_blocking=True)
        idx = idx.to(self.device, non_blocking=True)
        need = _C.lib().ngan_augment_workspace_bytes(b, self.canvas) // 4
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, device=self.device, dtype=torch.float32)
        s = self.image_size
        out = torch.empty(b, 1, s, s, device=self.device, dtype=torch.float32)
        _C.call("ngan_augment_batch", self.images, idx, rec, self._ws, out, len(self), b, self.canvas, self.image_size_max, s)
        return out

    def __getitem__(self, i):
        return self.batch([int(i)])[0]


class DatasetIterator:
    """Sequential batches over a device dataset (reference NeuronDataset.py:170-207): the last batch may be short."""

    def __init__(self, dataset: NeuronDataset, batch_size: int, device=None):
        if not dataset.load_all:
            raise Exception('On-device iteration is only possible when all images are loaded.')
        self.dataset = dataset
        self.N_images = len(dataset)
        self.batch_size = batch_size
        self.device = dataset.device
        self.image_ind = 0

    def __iter__(self):
        self.image_ind = 0
        return self

    def __next__(self):
        if self.image_ind < self.N_images:
            last = min(self.image_ind + self.batch_size, self.N_images)
            out = self.dataset.batch(list(range(self.image_ind, last)))
            self.image_ind = last
            return out
        raise StopIteration
