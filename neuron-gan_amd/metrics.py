"""Sample quality: the sliced Wasserstein distance (SWD) on Laplacian-pyramid patches (Karras et al. 2018, section 5) -- an addition of
this implementation, the reference has no quality metric.  Every stage is a kernel of csrc/swd.hip (include/ngan.h, last section):

    pyr_down / laplacian / laplacian_pyramid   the pyramid, channels-last fp32
    patch_descriptors                          7 x 7 x C neighbourhoods -> rows of a descriptor matrix, fp64 channel sums alongside
    project                                    per-channel normalisation and the random projections, direction-major, +inf padded
    sort_columns                               bitonic sort of every projected column
    sliced_wasserstein                         mean |sorted A - sorted B| over all directions and descriptors

`SWD` feeds minibatches of real and generated images and reports one value (x 1e3) per pyramid level R, R/2, ..., 16;
`evaluate_swd` drives it from a generator and a dataset.  All randomness (patch corners, directions, augmentation draws) comes from
private host generators seeded by `seed`: torch's global generator is never consumed, so a run trains the same with the metric on.

Sample diversity, the other half of that paper's evaluation: the mean multi-scale structural similarity (MS-SSIM, Wang, Simoncelli
and Bovik 2003) between random pairs of samples, which rises towards 1 when the generator collapses -- kernels of csrc/msssim.hip:

    msssim_scale / msssim_pool2 / msssim       per-pair (cs, ssim) of one scale, the next scale, the whole metric
    MSSSIM, evaluate_msssim                    accumulation over minibatches of pairs; generated pairs next to pairs of augmented reals

Spectral fidelity: the radial power spectrum of samples against the data's (Durall et al. 2020: generators that upsample and convolve
fall short at the high-frequency end, which is where this data keeps its noise texture) -- kernels of csrc/spectrum.hip:

    radial_spectrum / power_spectrum           per image the ring means of |F|^2 of the (Hann-windowed) image; the half-plane power
    Spectrum, evaluate_spectrum                accumulation over minibatches of both sets; per-bin ratio in dB, distance_db, high_db

Arbor morphology, the statistics people take from these micrographs: is the dendrite one connected tree, how much of the field does it
cover, how does it fill space across scales -- integer kernels of csrc/morph.hip on the image thresholded at the data loader's own
multi-Otsu level (csrc/dataset.hip):

    morph_levels / morph_mask                  8-bit levels with their histogram; the mask level > cut
    connected_components                       8-connected labels (smallest pixel index of the component), {area, components, largest,
                                               kept_area}, the mask of the components of at least min_size pixels
    box_counts / box_dimension                 occupied aligned boxes of side 1, 2, ..., R; the least-squares slope over 1 .. R/4
    arbor_statistics                           per image: fill, components, largest_share, dimension, scored
    Morphology, evaluate_morphology            per-image values of both sets; means, standard errors and the Kolmogorov-Smirnov distance

Arbor skeleton, what a neuroscientist reads off an arbor -- how much cable, how many endings and branch points, how thick the
processes are -- on the same kept mask, thinned in one launch of csrc/skeleton.hip (Guo and Hall 1989, the whole iteration in LDS):

    thin / skeleton_counts                     the skeleton and {pixels, tips, junctions, isolated, orth, diag, passes, area}; the
                                               six counts of any mask
    skeleton_statistics                        per image: length, tips, junctions, width, scored
    Skeleton, evaluate_skeleton                per-image values of both sets, summarised as Morphology does

Arbor geometry, where in the image the branches lie and how thick they are locally -- the exact Euclidean distance transform of the
kept mask and the Sholl histogram of its skeleton about the soma (csrc/sholl.hip):

    distance_transform                         squared distance to the nearest background pixel; the soma {y, x, dist2}, centre and
                                               radius of the largest inscribed disc
    sholl_crossings / sholl_step               skeleton edges that cross the circles of radius k s about a centre, 91 bins; the sum of
                                               the skeleton's local half-calibres
    sholl_statistics                           per image: calibre, soma, sholl_peak, sholl_radius, reach, scored, crossings
    Sholl, evaluate_sholl                      per-image values of both sets as above, and the mean Sholl profile of each side

Arbor branches, the skeleton cut into nodes and branches -- junction pixels merged into branch points, thinning spurs told apart from
real endings, the lengths of terminal and internal branches (csrc/branch.hip):

    branch_graph / default_spur                labels of nodes and branches, the 20 integers of BRANCH_STATS and the branch-length
                                               histogram of any mask, for a spur length in pixels
    branch_statistics                          per image: forks, nodes, terminals, spurs, terminal_length, link_length, longest, scored,
                                               hist
    Branches, evaluate_branches                per-image values of both sets as above, and the mean branch-length histogram of each side"""
import contextlib
import math

import torch

from . import _C

NHOOD = 7                     # the kernels' patch size
MIN_LEVEL = 16                # the coarsest pyramid level of the published metric


def _images(x):
    if not (isinstance(x, torch.Tensor) and x.dim() == 4 and x.dtype == torch.float32):
        raise TypeError("expected a 4-d fp32 tensor of channels-last images (B, H, W, C)")
    if x.shape[3] not in (1, 3):
        raise ValueError(f"C={x.shape[3]}: 1 or 3 colour channels")
    return x.contiguous()


def channels_last(images):
    """(B, C, R, R) or (B, R, R, C) images -> contiguous fp32 (B, R, R, C); one colour channel needs no copy"""
    if images.dim() != 4:
        raise ValueError(f"images must have 4 dimensions, got {tuple(images.shape)}")
    images = images.detach().float()
    if images.shape[3] in (1, 3) and images.shape[1] == images.shape[2]:
        return images.contiguous()
    if images.shape[1] not in (1, 3) or images.shape[2] != images.shape[3]:
        raise ValueError(f"images must be (B, C, R, R) or (B, R, R, C) with C in (1, 3), got {tuple(images.shape)}")
    if images.shape[1] == 1:
        return images.contiguous().view(images.shape[0], images.shape[2], images.shape[3], 1)
    return images.permute(0, 2, 3, 1).contiguous()


def pyr_down(x):
    """Gaussian [1 4 6 4 1] / 16 per axis, mirror boundary, sampled at the even rows and columns: (B, H, W, C) -> (B, H/2, W/2, C)"""
    x = _images(x)
    b, h, w, c = x.shape
    out = torch.empty(b, h // 2, w // 2, c, device=x.device, dtype=torch.float32)
    _C.call("ngan_swd_pyr_down", x, out, b, h, w, c)
    return out


def laplacian(fine, coarse):
    """fine - up(coarse), up = zero-insert x2 filtered with 4 x the Gaussian (mirror boundary on the fine grid)"""
    fine, coarse = _images(fine), _images(coarse)
    b, h, w, c = fine.shape
    if tuple(coarse.shape) != (b, h // 2, w // 2, c):
        raise ValueError(f"coarse must be {(b, h // 2, w // 2, c)}, got {tuple(coarse.shape)}")
    out = torch.empty_like(fine)
    _C.call("ngan_swd_laplacian", fine, coarse, out, b, h, w, c)
    return out


def laplacian_pyramid(images, num_levels):
    """[lap_0, ..., lap_{L-2}, gauss_{L-1}] of channels-last images: level l is H / 2^l pixels wide; the last keeps the low-pass"""
    if num_levels < 1:
        raise ValueError("num_levels must be at least 1")
    cur = _images(images)
    out = []
    for _ in range(num_levels - 1):
        nxt = pyr_down(cur)
        out.append(laplacian(cur, nxt))
        cur = nxt
    out.append(cur)
    return out


def _positions(positions):
    pos = torch.as_tensor(positions).to(dtype=torch.int32, device="cpu").contiguous()
    if pos.dim() != 2 or pos.shape[1] != 3 or pos.shape[0] == 0:
        raise ValueError(f"positions must be (n, 3) triples (image, top row, left column), got {tuple(pos.shape)}")
    return pos


def patch_descriptors(images, positions, out=None, sums=None, row_offset=0, accumulate=False):
    """Rows row_offset .. row_offset + n of `out` (any rows x 49 C; default a new (n, 49 C) matrix) = the 7 x 7 x C neighbourhoods
    at `positions` ((n, 3) int triples: image, top row, left column; validated by the entry point on the host), channel-major;
    `sums` (2 C doubles) = per-channel sum and sum of squares, added to when accumulate.  Returns (out, sums)."""
    x = _images(images)
    b, h, w, c = x.shape
    pos = _positions(positions)
    n = pos.shape[0]
    if out is None:
        out = torch.empty(row_offset + n, 49 * c, device=x.device, dtype=torch.float32)
    if out.dim() != 2 or out.shape[1] != 49 * c or out.shape[0] < row_offset + n or out.dtype != torch.float32:
        raise ValueError(f"out must be fp32 (>= {row_offset + n}, {49 * c}), got {tuple(out.shape)}")
    if sums is None:
        if accumulate:
            raise ValueError("accumulate needs the sums to add to")
        sums = torch.empty(2 * c, device=x.device, dtype=torch.float64)
    ws = torch.empty(max(1, _C.lib().ngan_swd_descriptors_workspace_bytes(n, c) // 8), device=x.device, dtype=torch.float64)
    _C.call("ngan_swd_descriptors", x, pos.data_ptr(), pos.to(x.device), out, sums, ws, n, int(row_offset), int(bool(accumulate)),
            b, h, w, c)
    return out, sums


def descriptor_sums(desc):
    """what patch_descriptors returns as `sums`, for a descriptor matrix that came from elsewhere"""
    d = desc.double().view(desc.shape[0], -1, 49)
    return torch.cat([d.sum((0, 2)), (d * d).sum((0, 2))])


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def project(desc, sums, dirs, n_pad=None):
    """(n_dirs, n_pad) projections of the normalised descriptors on the columns of dirs (49 C, n_dirs); columns n .. n_pad are +inf"""
    n, k = desc.shape
    c = k // 49
    if k != 49 * c or tuple(dirs.shape[:1]) != (k,) or dirs.dim() != 2:
        raise ValueError(f"desc (n, 49 C) and dirs (49 C, n_dirs) expected, got {tuple(desc.shape)} and {tuple(dirs.shape)}")
    n_pad = next_pow2(n) if n_pad is None else int(n_pad)
    proj = torch.empty(dirs.shape[1], n_pad, device=desc.device, dtype=torch.float32)
    _C.call("ngan_swd_project", desc, sums, dirs.contiguous(), proj, n, n_pad, dirs.shape[1], c)
    return proj


def sort_columns(cols):
    """ascending, in place, every row of the direction-major (n_dirs, n_pad) matrix; n_pad a power of two"""
    _C.call("ngan_swd_sort_columns", cols, cols.shape[0], cols.shape[1])
    return cols


def sort_block_elements():
    return int(_C.lib().ngan_swd_sort_block_elements())


def sorted_l1(a, b, n):
    """one fp64 device scalar: mean |a - b| over the first n entries of every sorted column"""
    out = torch.empty(1, device=a.device, dtype=torch.float64)
    ws = torch.empty(max(1, _C.lib().ngan_swd_l1_workspace_bytes(n, a.shape[0]) // 8), device=a.device, dtype=torch.float64)
    _C.call("ngan_swd_l1", a, b, out, ws, n, a.shape[1], a.shape[0])
    return out


def sliced_wasserstein(descA, descB, dirs, sumsA=None, sumsB=None):
    """fp64 device scalar: the sliced Wasserstein distance of two descriptor sets of equal size, each normalised by its own per-channel
    mean and population standard deviation; dirs (49 C, n_dirs) holds the unit directions of all repeats side by side (the mean over
    repeats of the per-repeat mean is the mean over all columns)"""
    if descA.shape != descB.shape:
        raise ValueError(f"the two sets need the same number of descriptors, got {tuple(descA.shape)} and {tuple(descB.shape)}")
    n = descA.shape[0]
    sumsA = descriptor_sums(descA) if sumsA is None else sumsA
    sumsB = descriptor_sums(descB) if sumsB is None else sumsB
    pa = sort_columns(project(descA, sumsA, dirs))
    pb = sort_columns(project(descB, sumsB, dirs))
    return sorted_l1(pa, pb, n)


def draw_directions(n_features, dir_repeats, dirs_per_repeat, generator):
    """per repeat randn(n_features, dirs_per_repeat) with unit columns, fp32; the repeats side by side"""
    reps = []
    for _ in range(dir_repeats):
        d = torch.randn(n_features, dirs_per_repeat, generator=generator, dtype=torch.float32)
        reps.append(d / d.square().sum(0, keepdim=True).sqrt())
    return torch.cat(reps, 1)


class SWD:
    """Accumulates the descriptors of real and generated minibatches and reports the distance per pyramid level.

        m = SWD(image_size=64); m.feed('real', x); m.feed('fake', G(z)); m.result()

    Levels are image_size, image_size / 2, ..., 16 (none below 16 x 16: `result()` then says so).  Per image and level
    nhoods_per_image patches with top-left corners uniform in [0, H - 7], drawn independently for the two sets unless feed() is
    given `positions` (one (n, 3) int tensor per level); dir_repeats x dirs_per_repeat unit directions per level, drawn at
    construction.  n_images: how many images each set will hold, if known -- the descriptor matrices are then allocated once."""

    def __init__(self, image_size, n_colors=1, nhood_size=NHOOD, nhoods_per_image=128, dir_repeats=4, dirs_per_repeat=128, seed=0,
                 device="cuda", n_images=None):
        if nhood_size != NHOOD:
            raise ValueError(f"nhood_size={nhood_size}: the kernels gather {NHOOD} x {NHOOD} patches")
        if n_colors not in (1, 3):
            raise ValueError(f"n_colors={n_colors}: 1 or 3")
        if image_size < 1 or image_size & (image_size - 1):
            raise ValueError(f"image_size={image_size} must be a power of two")
        self.image_size, self.n_colors, self.nhoods_per_image = int(image_size), int(n_colors), int(nhoods_per_image)
        self.device = torch.device(device)
        self.levels = []
        r = self.image_size
        while r >= MIN_LEVEL:
            self.levels.append(r)
            r //= 2
        self.gen = torch.Generator(device="cpu").manual_seed(int(seed))
        self.dirs = [draw_directions(49 * self.n_colors, dir_repeats, dirs_per_repeat, self.gen) for _ in self.levels]
        self._capacity = None if n_images is None else int(n_images) * self.nhoods_per_image
        self.desc = {w: [None] * len(self.levels) for w in ("real", "fake")}
        self.sums = {w: [None] * len(self.levels) for w in ("real", "fake")}
        self.count = {w: [0] * len(self.levels) for w in ("real", "fake")}

    def draw_positions(self, batch, size):
        yx = torch.randint(0, size - NHOOD + 1, (batch, self.nhoods_per_image, 2), generator=self.gen, dtype=torch.int32)
        idx = torch.arange(batch, dtype=torch.int32).view(batch, 1, 1).expand(batch, self.nhoods_per_image, 1)
        return torch.cat([idx, yx], 2).reshape(-1, 3)

    def _room(self, which, level, n):
        k = 49 * self.n_colors
        have, used = self.desc[which][level], self.count[which][level]
        if have is None or have.shape[0] < used + n:
            rows = max(used + n, self._capacity or 0, 2 * (0 if have is None else have.shape[0]))
            grown = torch.empty(rows, k, device=self.device, dtype=torch.float32)
            if used:
                grown[:used].copy_(have[:used])
            self.desc[which][level] = grown
        if self.sums[which][level] is None:
            self.sums[which][level] = torch.zeros(2 * self.n_colors, device=self.device, dtype=torch.float64)
        return self.desc[which][level]

    def feed(self, which, images, positions=None):
        if which not in self.desc:
            raise ValueError(f"which={which!r}: 'real' or 'fake'")
        x = channels_last(images.to(self.device))
        if tuple(x.shape[1:]) != (self.image_size, self.image_size, self.n_colors):
            raise ValueError(f"images must be {self.image_size} pixels wide with {self.n_colors} colours, got {tuple(images.shape)}")
        if not self.levels:
            return
        if positions is not None and len(positions) != len(self.levels):
            raise ValueError(f"positions: one (n, 3) tensor per level, {len(self.levels)} levels")
        for l, level in enumerate(laplacian_pyramid(x, len(self.levels))):
            pos = self.draw_positions(x.shape[0], self.levels[l]) if positions is None else _positions(positions[l])
            out = self._room(which, l, pos.shape[0])
            used = self.count[which][l]
            patch_descriptors(level, pos, out=out, sums=self.sums[which][l], row_offset=used, accumulate=used > 0)
            self.count[which][l] = used + pos.shape[0]

    def result(self, dirs=None):
        """{'levels': [R, R/2, ..., 16], 'swd': [per level, x 1e3], 'mean': their mean}; no level (a stage below 16 x 16): empty lists,
        mean None and a 'note'.  dirs: optional (49 C, n_dirs) directions per level instead of the drawn ones."""
        if not self.levels:
            return {"levels": [], "swd": [], "mean": None,
                    "note": f"{self.image_size} x {self.image_size} images are below {MIN_LEVEL} x {MIN_LEVEL}: no pyramid level to score"}
        vals = []
        for l, size in enumerate(self.levels):
            n = self.count["real"][l]
            if n == 0 or n != self.count["fake"][l]:
                raise ValueError(f"level {size}: {n} real and {self.count['fake'][l]} generated descriptors; feed both sets equally")
            for which in ("real", "fake"):
                s = self.sums[which][l].tolist()
                c = self.n_colors
                for ch in range(c):
                    mean = s[ch] / (49.0 * n)
                    if not s[c + ch] / (49.0 * n) - mean * mean > 0.0:
                        raise ValueError(f"level {size}: channel {ch} of the {which} set has zero variance")
            d = (self.dirs[l] if dirs is None else dirs[l]).to(self.device, torch.float32)
            vals.append(sliced_wasserstein(self.desc["real"][l][:n], self.desc["fake"][l][:n], d, self.sums["real"][l],
                                           self.sums["fake"][l]))
        swd = [v * 1e3 for v in torch.cat(vals).tolist()]
        return {"levels": list(self.levels), "swd": swd, "mean": sum(swd) / len(swd)}


@contextlib.contextmanager
def _private_stream(dataset, size, seed):
    """for the duration, `dataset` (None: nothing to do) serves images `size` pixels wide and draws its augmentations from a private
    generator seeded seed + 1; its own generator, left where it was, and its image size are restored afterwards"""
    if dataset is None:
        yield
        return
    aug = torch.Generator(device="cpu").manual_seed(int(seed) + 1)
    old_size = dataset.image_size
    own_gen = getattr(dataset, "gen", None)
    dataset.set_image_size(size)
    if own_gen is not None:
        dataset.gen = aug
    try:
        yield
    finally:
        if own_gen is not None:
            dataset.gen = own_gen
        dataset.set_image_size(old_size)


def _real_batch(dataset, idx, device):
    """the images `idx` through the data set's own augmentation chain, on the device"""
    if hasattr(dataset, "batch"):
        return dataset.batch(idx)
    return torch.stack([dataset[j] for j in idx]).to(device)


def _latents(generator, n, lat, device):
    """n latents of the sampler's distribution (utils.sample_latent_vec, 'randn': normal draws clamped to [-5, 5], projected on the unit
    sphere) from the private generator `lat`"""
    z = torch.randn(n, generator.latent_dim, generator=lat).clamp(-5, 5)
    return (z / z.norm(p=2, dim=1, keepdim=True)).to(device)


def _feed_two_sets(metric, generator, dataset, n_images, batch_size, seed):
    """the loop of evaluate_swd, evaluate_spectrum and the arbor metrics: per minibatch, feed `metric` the reals (indices cycled, under
    _private_stream; dataset None: the data side is already there) and then the fakes under no_grad from latents of a private generator
    seeded seed + 2; one minibatch of images alive at a time"""
    lat = torch.Generator(device="cpu").manual_seed(int(seed) + 2)
    with _private_stream(dataset, metric.image_size, seed):
        for i in range(0, n_images, batch_size):
            b = min(batch_size, n_images - i)
            if dataset is not None:
                metric.feed("real", _real_batch(dataset, [(i + j) % len(dataset) for j in range(b)], metric.device))
            with torch.no_grad():
                fakes = generator(_latents(generator, b, lat, metric.device)).detach()
            metric.feed("fake", fakes)
            del fakes


def evaluate_swd(generator, dataset, n_images=8192, batch_size=64, seed=0, nhoods_per_image=128, dir_repeats=4, dirs_per_repeat=128):
    """SWD of `generator` against `dataset` at the generator's current resolution: n_images reals through the dataset's own
    augmentation chain (its indices cycled, its random draws taken from a private generator so that the training stream is left
    where it was), n_images fakes under no_grad from latents of the sampler's distribution (utils.sample_latent_vec, 'randn': normal
    draws clamped to [-5, 5], projected on the unit sphere) drawn from a private generator -- the sampler's own seeded form calls
    torch.manual_seed, which reseeds the device generator that a trainer's device latents come from; one minibatch of images per
    side alive at a time."""
    device = next(generator.parameters()).device
    size = int(generator.image_size)
    metric = SWD(size, n_colors=int(getattr(generator, "N_colors", 1)), nhoods_per_image=nhoods_per_image, dir_repeats=dir_repeats,
                 dirs_per_repeat=dirs_per_repeat, seed=seed, device=device, n_images=n_images)
    if not metric.levels:
        return metric.result()
    _feed_two_sets(metric, generator, dataset, n_images, batch_size, seed)
    return metric.result()


# ---- sample diversity: multi-scale structural similarity between pairs (csrc/msssim.hip; include/ngan.h, last section) -----------------
MSSSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)     # Wang, Simoncelli and Bovik 2003
MSSSIM_WINDOW = 11                                              # taps of the Gaussian window, sigma = 1.5
DATA_RANGE = 2.0              # width of [-1, 1]: data.py's batches ("augmented images in [-1, 1]") and ToImage's tanh live there


def msssim_scales(image_size):
    """S = min(5, 1 + floor(log2(R / 11))): 16 -> 1, 32 -> 2, 64 -> 3, 128 -> 4, 256 and above -> 5, below 16 -> 0"""
    s, r = 0, int(image_size)
    while r >= 16 and s < len(MSSSIM_WEIGHTS):
        s, r = s + 1, r // 2
    return s


def msssim_weights(scales):
    """the first `scales` of the published exponents, renormalised to sum 1"""
    w = MSSSIM_WEIGHTS[:scales]
    return [v / sum(w) for v in w]


def msssim_window():
    """the 11 fp32 taps the kernel filters with (normalised in fp64, then rounded)"""
    import ctypes
    buf = (ctypes.c_float * MSSSIM_WINDOW)()
    if _C.lib().ngan_msssim_window(ctypes.cast(buf, ctypes.c_void_p)) != 0:
        raise RuntimeError(_C.lib().ngan_last_error().decode())
    return torch.tensor(list(buf), dtype=torch.float32)


def _pair(a, b):
    a, b = _images(a), _images(b)
    if a.shape != b.shape or a.shape[1] != a.shape[2]:
        raise ValueError(f"two equal stacks of square images (P, R, R, C) expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.shape[0] == 0:
        raise ValueError("no pair to score")
    return a, b


def msssim_scale(a, b, data_range=DATA_RANGE):
    """(P, 2) fp64 on the device: the mean cs and the mean ssim of one scale for every pair (a[p], b[p]); channels-last fp32 images
    at least 16 pixels wide; the means run over the (R - 10)^2 C entries of the unpadded 11 x 11 Gaussian filtering"""
    a, b = _pair(a, b)
    p, r, _, c = a.shape
    out = torch.empty(p, 2, device=a.device, dtype=torch.float64)
    ws = torch.empty(max(1, _C.lib().ngan_msssim_workspace_bytes(p, r) // 8), device=a.device, dtype=torch.float64)
    _C.call("ngan_msssim_scale", a, b, out, ws, p, r, c, float(data_range))
    return out


def msssim_pool2(a, b):
    """the next scale of both stacks: 2 x 2 averages, (P, R, R, C) -> (P, R/2, R/2, C)"""
    a, b = _pair(a, b)
    p, r, _, c = a.shape
    ao = torch.empty(p, r // 2, r // 2, c, device=a.device, dtype=torch.float32)
    bo = torch.empty_like(ao)
    _C.call("ngan_msssim_pool2", a, b, ao, bo, p, r, c)
    return ao, bo


def msssim(a, b, data_range=DATA_RANGE):
    """(P,) fp64 on the device: MS-SSIM of every pair (a[p], b[p]) of channels-last fp32 images (P, R, R, C), R a power of two >= 16,
    C in (1, 3).  S = msssim_scales(R) scales, each the 2 x 2 average of the one before; with w = msssim_weights(S)

        MS-SSIM = prod_{s < S} max(cs_s, 0)^w_s * max(ssim_S, 0)^w_S        (combined in fp64)

    data_range: the width of the interval the images live in, 2 by default ([-1, 1], the data set loader's and the generator's range);
    C1 = (0.01 data_range)^2 and C2 = (0.03 data_range)^2."""
    a, b = _pair(a, b)
    scales = msssim_scales(a.shape[1])
    if scales == 0:
        raise ValueError(f"{a.shape[1]} x {a.shape[1]} images are below 16 x 16: the 11 x 11 window has no scale to score")
    w = msssim_weights(scales)
    value = None
    for s in range(scales):
        v = msssim_scale(a, b, data_range)[:, 1 if s == scales - 1 else 0].clamp_min(0.0).pow(w[s])
        value = v if value is None else value * v
        if s < scales - 1:
            a, b = msssim_pool2(a, b)
    return value


class MSSSIM:
    """Accumulates MS-SSIM over pairs of generated and, optionally, of real images and reports the means.

        m = MSSSIM(image_size=64); m.feed('fake', G(z0), G(z1)); m.feed('real', x0, x1); m.result()

    A collapsed generator shows as a 'fake' mean clearly above the 'real' one (the data's own pair similarity under its augmentations).
    data_range: see msssim().  A stage below 16 x 16 has no scale: feed() does nothing and result() says so."""

    def __init__(self, image_size, n_colors=1, data_range=DATA_RANGE, device="cuda"):
        if n_colors not in (1, 3):
            raise ValueError(f"n_colors={n_colors}: 1 or 3")
        if image_size < 1 or image_size & (image_size - 1):
            raise ValueError(f"image_size={image_size} must be a power of two")
        if not data_range > 0:
            raise ValueError(f"data_range={data_range!r} must be positive")
        self.image_size, self.n_colors, self.data_range = int(image_size), int(n_colors), float(data_range)
        self.device = torch.device(device)
        self.scales = msssim_scales(self.image_size)
        self.weights = msssim_weights(self.scales) if self.scales else []
        self.values = {"fake": [], "real": []}

    def feed(self, which, a, b):
        if which not in self.values:
            raise ValueError(f"which={which!r}: 'fake' or 'real'")
        a, b = channels_last(a.to(self.device)), channels_last(b.to(self.device))
        want = (self.image_size, self.image_size, self.n_colors)
        if tuple(a.shape[1:]) != want or a.shape != b.shape:
            raise ValueError(f"two equal stacks of {self.image_size} pixel wide images with {self.n_colors} colours expected, "
                             f"got {tuple(a.shape)} and {tuple(b.shape)}")
        if self.scales:
            self.values[which].append(msssim(a, b, self.data_range))

    def per_pair(self, which):
        """(n,) fp64: every value fed so far, in feeding order"""
        v = self.values[which]
        return torch.cat(v) if v else torch.empty(0, dtype=torch.float64, device=self.device)

    @staticmethod
    def _mean_sem(v):
        n = v.numel()
        mean = float(v.mean())
        return mean, (float(v.std(unbiased=True)) / n ** 0.5 if n > 1 else None)

    def result(self):
        """{'scales': S, 'weights': [...], 'fake': mean, 'fake_sem': standard error of the mean (None for one pair), 'real': mean or
        None, 'real_sem': ..., 'pairs': generated pairs}; a stage below 16 x 16: scales 0, no number and a 'note'"""
        if not self.scales:
            return {"scales": 0, "weights": [], "fake": None, "fake_sem": None, "real": None, "real_sem": None, "pairs": 0,
                    "note": f"{self.image_size} x {self.image_size} images are below 16 x 16: the 11 x 11 window has no scale to score"}
        fake, real = self.per_pair("fake"), self.per_pair("real")
        if fake.numel() == 0:
            raise ValueError("no generated pair was fed")
        out = {"scales": self.scales, "weights": list(self.weights), "real": None, "real_sem": None, "pairs": int(fake.numel())}
        out["fake"], out["fake_sem"] = self._mean_sem(fake)
        if real.numel():
            out["real"], out["real_sem"] = self._mean_sem(real)
        return out


def evaluate_msssim(generator, dataset=None, n_pairs=10000, batch_size=64, seed=0, data_range=DATA_RANGE):
    """Mean MS-SSIM over n_pairs pairs of samples of `generator` at its current resolution and, with a data set, over n_pairs pairs
    of its images for comparison.  2 n_pairs images are generated under no_grad, pair i = images (2 i, 2 i + 1); the latents follow
    the sampler's distribution (normal draws clamped to [-5, 5], projected on the unit sphere) and come from a private generator, as
    in evaluate_swd.  The reals are 2 n_pairs draws through the data set's own augmentation chain (indices cycled, paired the same
    way), its generator swapped for a private one and its image size set for the duration, both restored afterwards.  batch_size
    pairs per side are alive at a time; torch's global and device generators are never consumed."""
    device = next(generator.parameters()).device
    size = int(generator.image_size)
    metric = MSSSIM(size, n_colors=int(getattr(generator, "N_colors", 1)), data_range=data_range, device=device)
    if not metric.scales:
        return metric.result()
    n_pairs, batch_size = int(n_pairs), int(batch_size)
    if n_pairs < 1 or batch_size < 1:
        raise ValueError(f"n_pairs={n_pairs} and batch_size={batch_size} must be positive")
    lat = torch.Generator(device="cpu").manual_seed(int(seed) + 2)
    for i in range(0, n_pairs, batch_size):
        with torch.no_grad():
            fakes = channels_last(generator(_latents(generator, 2 * min(batch_size, n_pairs - i), lat, device)).detach())
        metric.feed("fake", fakes[0::2].contiguous(), fakes[1::2].contiguous())
        del fakes
    if dataset is not None:
        with _private_stream(dataset, size, seed):
            for i in range(0, n_pairs, batch_size):
                idx = [(2 * i + j) % len(dataset) for j in range(2 * min(batch_size, n_pairs - i))]
                reals = channels_last(_real_batch(dataset, idx, device))
                metric.feed("real", reals[0::2].contiguous(), reals[1::2].contiguous())
                del reals
    return metric.result()


def format_msssim(result, title="MS-SSIM between pairs"):
    """the table eval.py prints: one row per side, mean +- standard error"""
    if not result["scales"]:
        return f"{title}: {result['note']}"
    pm = lambda m, s: f"{m:9.5f}" + (f" +- {s:.5f}" if s is not None else "")   # noqa: E731
    rows = [f"{title} ({result['scales']} scale{'s' if result['scales'] > 1 else ''}, {result['pairs']} pairs)",
            f"{'generated':>10s} {pm(result['fake'], result['fake_sem'])}"]
    if result["real"] is not None:
        rows.append(f"{'data':>10s} {pm(result['real'], result['real_sem'])}")
    return "\n".join(rows)


# ---- spectral fidelity: radial power spectrum of samples against the data's (csrc/spectrum.hip; include/ngan.h, last section) ---------
SPECTRUM_MIN, SPECTRUM_MAX = 16, 1024        # image sizes the kernels transform


def _host_array(entry, ctype, n, *args):
    import ctypes
    buf = (ctype * n)()
    if getattr(_C.lib(), entry)(ctypes.cast(buf, ctypes.c_void_p), *args) != 0:
        raise RuntimeError(_C.lib().ngan_last_error().decode())
    return list(buf)


def spectrum_window(R):
    """the R fp32 taps of the periodic Hann window the kernels apply (formed in fp64, then rounded)"""
    import ctypes
    return torch.tensor(_host_array("ngan_spectrum_window", ctypes.c_float, max(int(R), 1), int(R)), dtype=torch.float32)


def spectrum_ring_counts(R):
    """n_0 .. n_{R/2}: the number of frequencies of the R x R plane in every ring"""
    import ctypes
    return torch.tensor(_host_array("ngan_spectrum_ring_counts", ctypes.c_int, max(int(R) // 2 + 1, 1), int(R)), dtype=torch.int64)


def _spectrum(images, window, want_power):
    x = _images(images)
    b, r, r2, c = x.shape
    if r != r2:
        raise ValueError(f"square images (B, R, R, C) expected, got {tuple(x.shape)}")
    if b == 0:
        raise ValueError("no image to transform")
    radial = torch.empty(b, r // 2 + 1, device=x.device, dtype=torch.float64)
    power = torch.empty(b, c, r, r // 2 + 1, device=x.device, dtype=torch.float32) if want_power else None
    ws = torch.empty(max(1, _C.lib().ngan_spectrum_workspace_bytes(b, r, c) // 8), device=x.device, dtype=torch.float64)
    _C.call("ngan_spectrum_radial", x, radial, power, ws, b, r, c, int(bool(window)))
    return radial, power


def radial_spectrum(images, window=True):
    """(B, R/2 + 1) fp64 on the device: per image the mean over the colour channels and over ring k (signed frequencies with
    floor(sqrt(u^2 + v^2) + 1/2) = k, decided in integers; the corners beyond R/2 are dropped) of |F|^2 / sum w^2, F the 2-D DFT of
    the image under the periodic Hann window w (window=False: none).  Channels-last fp32 images (B, R, R, C), R a power of two in
    16 .. 1024, C in (1, 3).  White noise of variance s^2 gives s^2 in every bin."""
    return _spectrum(images, window, False)[0]


def power_spectrum(images, window=True):
    """(radial, power): radial_spectrum's result, the same bits, and the power of the half plane, (B, C, R, R/2 + 1) fp32 with the
    x frequency 0 .. R/2 last and the y frequency in DFT order"""
    return _spectrum(images, window, True)


class Spectrum:
    """Accumulates the radial power spectra of real and generated images and compares their means bin by bin.

        m = Spectrum(image_size=64); m.feed('real', x); m.feed('fake', G(z)); m.result()

    ratio_db[k] = 10 log10(generated / data); distance_db is the mean |ratio_db| over k = 1 .. R/2 (bin 0, the windowed mean level,
    is reported but not scored); high_db the signed mean over the top octave R/4 < k <= R/2: negative when the samples lack fine
    texture (the upsampling deficit), positive when they are noisier than the data.  A stage below 16 x 16 has no bins: feed() does
    nothing and result() says so."""

    def __init__(self, image_size, n_colors=1, window=True, device="cuda"):
        if n_colors not in (1, 3):
            raise ValueError(f"n_colors={n_colors}: 1 or 3")
        if image_size < 1 or image_size & (image_size - 1):
            raise ValueError(f"image_size={image_size} must be a power of two")
        if image_size > SPECTRUM_MAX:
            raise ValueError(f"image_size={image_size}: the kernels transform up to {SPECTRUM_MAX} x {SPECTRUM_MAX}")
        self.image_size, self.n_colors, self.window = int(image_size), int(n_colors), bool(window)
        self.device = torch.device(device)
        self.bins = self.image_size // 2 + 1 if self.image_size >= SPECTRUM_MIN else 0
        self.count = {"real": 0, "fake": 0}
        self.sums = {"real": None, "fake": None}          # (2, bins) fp64 on the device: sum S, sum S^2

    def feed(self, which, images):
        if which not in self.count:
            raise ValueError(f"which={which!r}: 'real' or 'fake'")
        x = channels_last(images.to(self.device))
        if tuple(x.shape[1:]) != (self.image_size, self.image_size, self.n_colors):
            raise ValueError(f"images must be {self.image_size} pixels wide with {self.n_colors} colours, got {tuple(images.shape)}")
        if not self.bins:
            return
        s = radial_spectrum(x, self.window)
        both = torch.stack([s.sum(0), s.square().sum(0)])
        self.sums[which] = both if self.sums[which] is None else self.sums[which] + both
        self.count[which] += x.shape[0]

    def _mean_sem(self, which):
        n = self.count[which]
        tot, sq = self.sums[which].tolist()
        mean = [t / n for t in tot]
        if n < 2:
            return mean, [None] * len(mean)
        return mean, [math.sqrt(max(q - n * m * m, 0.0) / (n - 1) / n) for q, m in zip(sq, mean)]

    def result(self):
        """{'k': [0 .. R/2], 'real': [mean S per bin], 'fake': [...], 'real_sem', 'fake_sem': standard errors of those means (None for
        one image), 'ratio_db': [per bin; None where either mean is 0], 'distance_db', 'high_db', 'skipped_bins': scored bins left
        out for that reason, 'images': n per side}; a stage below 16 x 16: empty lists, no number and a 'note'"""
        if not self.bins:
            return {"k": [], "real": [], "fake": [], "real_sem": [], "fake_sem": [], "ratio_db": [], "distance_db": None,
                    "high_db": None, "skipped_bins": 0, "images": 0,
                    "note": f"{self.image_size} x {self.image_size} images are below {SPECTRUM_MIN} x {SPECTRUM_MIN}: no ring to score"}
        n = self.count["real"]
        if n == 0 or n != self.count["fake"]:
            raise ValueError(f"{n} real and {self.count['fake']} generated images; feed both sets equally")
        real, real_sem = self._mean_sem("real")
        fake, fake_sem = self._mean_sem("fake")
        ratio = [10.0 * math.log10(f / r) if f > 0.0 and r > 0.0 else None for f, r in zip(fake, real)]
        scored = [v for v in ratio[1:] if v is not None]
        high = [v for v in ratio[self.image_size // 4 + 1:] if v is not None]
        return {"k": list(range(self.bins)), "real": real, "fake": fake, "real_sem": real_sem, "fake_sem": fake_sem, "ratio_db": ratio,
                "distance_db": sum(abs(v) for v in scored) / len(scored) if scored else None,
                "high_db": sum(high) / len(high) if high else None,
                "skipped_bins": len(ratio) - 1 - len(scored), "images": n}


def evaluate_spectrum(generator, dataset, n_images=8192, batch_size=64, seed=0, window=True, real_from=None, return_metric=False):
    """The radial power spectrum of `generator`'s samples against `dataset`'s images at the generator's current resolution, built
    like evaluate_swd: n_images reals through the data set's own augmentation chain (its indices cycled, its generator swapped for a
    private one and its image size set for the duration, both restored afterwards), n_images fakes under no_grad from latents of the
    sampler's distribution (normal draws clamped to [-5, 5], projected on the unit sphere) drawn from a private generator; one
    minibatch of images per side alive at a time; torch's global and device generators are never consumed.
    real_from: a Spectrum that an earlier call returned (return_metric=True: the call then returns (result, metric)) with the same
    settings -- its data side is taken over instead of being computed again, and `dataset` is not touched (it may be None)."""
    device = next(generator.parameters()).device
    size = int(generator.image_size)
    metric = Spectrum(size, n_colors=int(getattr(generator, "N_colors", 1)), window=window, device=device)
    if not metric.bins:
        return (metric.result(), metric) if return_metric else metric.result()
    if real_from is not None:
        if (real_from.image_size, real_from.n_colors, real_from.window, real_from.count["real"]) != \
                (metric.image_size, metric.n_colors, metric.window, int(n_images)):
            raise ValueError("real_from was fed with other settings")
        metric.count["real"], metric.sums["real"] = real_from.count["real"], real_from.sums["real"]
    n_images, batch_size = int(n_images), int(batch_size)
    if n_images < 1 or batch_size < 1:
        raise ValueError(f"n_images={n_images} and batch_size={batch_size} must be positive")
    _feed_two_sets(metric, generator, dataset if real_from is None else None, n_images, batch_size, seed)
    return (metric.result(), metric) if return_metric else metric.result()


def spectral_target(dataset, image_size, n_images=256, seed=0, batch_size=64, device="cuda"):
    """The data's mean radial spectrum at `image_size`, fp64 (R/2 + 1,) on `device`: the target of the generator's spectral loss
    (loss_functions.G_spectral_loss).  Taken the way evaluate_spectrum takes its data side: n_images images through the data set's
    own augmentation chain, its indices cycled, its random draws from a private generator seeded seed + 1, its image size and its
    own generator restored afterwards; torch's global and device generators are never consumed.  Every rank of a data-parallel run
    computes the same bits from the whole data set."""
    size, n_images, batch_size = int(image_size), int(n_images), int(batch_size)
    if n_images < 1 or batch_size < 1:
        raise ValueError(f"n_images={n_images} and batch_size={batch_size} must be positive")
    if size < SPECTRUM_MIN or size > SPECTRUM_MAX or size & (size - 1):
        raise ValueError(f"image_size={size}: the kernels transform powers of two from {SPECTRUM_MIN} to {SPECTRUM_MAX}")
    total = None
    with _private_stream(dataset, size, seed):
        for i in range(0, n_images, batch_size):
            b = min(batch_size, n_images - i)
            x = _real_batch(dataset, [(i + j) % len(dataset) for j in range(b)], torch.device(device))
            s = radial_spectrum(channels_last(x.to(device)), True).sum(0)
            total = s if total is None else total + s
    return total / n_images


def format_spectrum(result, title="Radial power spectrum"):
    """the table eval.py prints: data, generated and their ratio in dB at the octave edges k = 1, 2, 4, ..., R/2, the two summaries
    below it"""
    if not result["k"]:
        return f"{title}: {result['note']}"
    rows = [f"{title} ({result['images']} images per side)", f"{'k':>6s} {'data':>12s} {'generated':>12s} {'dB':>8s}"]
    k = 1
    while k < len(result["k"]):
        db = result["ratio_db"][k]
        rows.append(f"{k:6d} {result['real'][k]:12.5e} {result['fake'][k]:12.5e} " + (f"{db:8.2f}" if db is not None else f"{'-':>8s}"))
        k *= 2
    num = lambda v: "-" if v is None else f"{v:.2f}"   # noqa: E731
    rows.append(f"distance_db {num(result['distance_db'])}   high_db {num(result['high_db'])}"
                + (f"   ({result['skipped_bins']} bins without power left out)" if result["skipped_bins"] else ""))
    return "\n".join(rows)


# ---- arbor morphology: connectivity and box-counting dimension (csrc/morph.hip; include/ngan.h, last section) ---------------------------
MORPH_MIN, MORPH_MAX = 16, 1024              # image sizes the kernels take
MORPH_STATISTICS = ("fill", "components", "largest_share", "dimension")


def _square_bytes(t, what):
    if not (isinstance(t, torch.Tensor) and t.dim() == 3 and t.dtype == torch.uint8 and t.shape[1] == t.shape[2] and t.shape[0] > 0):
        raise TypeError(f"{what}: expected a uint8 tensor (B, R, R) with B >= 1")
    return t.contiguous()


def morph_levels(images):
    """(levels, hist): the 8-bit level of every pixel of channels-last fp32 images (B, R, R, C) in [-1, 1] -- trunc(clamp(fmaf(g, 127.5,
    128), 0, 255)) with g the pixel or, for C = 3, (x0 + x1 + x2) * (1 / 3) in fp32 -- as (B, R, R) uint8, and their (B, 256) int32
    histograms"""
    x = _images(images)
    b, r, r2, c = x.shape
    if r != r2 or b == 0:
        raise ValueError(f"square images (B, R, R, C) with B >= 1 expected, got {tuple(x.shape)}")
    levels = torch.empty(b, r, r, device=x.device, dtype=torch.uint8)
    hist = torch.empty(b, 256, device=x.device, dtype=torch.int32)
    _C.call("ngan_morph_levels", x, levels, hist, b, r, c)
    return levels, hist


def otsu_thresholds(hist):
    """(thresholds (B, 3) int32, status (B) int32) of (B, 256) int32 histograms: the data loader's 4-class multi-Otsu search
    (ngan_multiotsu4_noise_stats); status 0 ok, otherwise the thresholds are zeros"""
    n = hist.shape[0]
    dev = hist.device
    ws = torch.empty(_C.lib().ngan_multiotsu_workspace_bytes(n), device=dev, dtype=torch.uint8)
    thresholds = torch.empty(n, 3, device=dev, dtype=torch.int32)
    record = torch.empty(n, 3, device=dev, dtype=torch.float64)
    status = torch.empty(n, device=dev, dtype=torch.int32)
    _C.call("ngan_multiotsu4_noise_stats", hist.contiguous(), ws, thresholds, record, status, n)
    return thresholds, status


def morph_mask(levels, cut):
    """(B, R, R) uint8 0 / 1: level > cut; cut one level for all images or a (B) integer tensor (255: an empty mask)"""
    levels = _square_bytes(levels, "levels")
    b, r, _ = levels.shape
    if not isinstance(cut, torch.Tensor):
        cut = torch.full((b,), int(cut), dtype=torch.int32)
    if cut.numel() != b:
        raise ValueError(f"cut must hold one level per image ({b}), got {tuple(cut.shape)}")
    cut = cut.to(device=levels.device, dtype=torch.int32).contiguous()
    mask = torch.empty_like(levels)
    _C.call("ngan_morph_mask", levels, cut, mask, b, r)
    return mask


def connected_components(mask, min_size=1, want_kept=True):
    """(labels, stats, kept) of (B, R, R) uint8 masks (non-zero: foreground) under 8-connectivity.  labels (B, R, R) int32: -1 on the
    background, otherwise the smallest linear index row * R + col of the pixel's component.  stats (B, 4) int32: {area, components of
    at least min_size pixels, pixels of the largest component, pixels in the counted components}.  kept (B, R, R) uint8: the mask
    restricted to the counted components (None with want_kept=False; labels and stats are the same bits either way)."""
    mask = _square_bytes(mask, "mask")
    b, r, _ = mask.shape
    labels = torch.empty(b, r, r, device=mask.device, dtype=torch.int32)
    stats = torch.empty(b, 4, device=mask.device, dtype=torch.int32)
    kept = torch.empty_like(mask) if want_kept else None
    ws = torch.empty(max(1, _C.lib().ngan_morph_workspace_bytes(b, r) // 4), device=mask.device, dtype=torch.int32)
    _C.call("ngan_morph_label", mask, labels, stats, kept, ws, b, r, int(min_size))
    return labels, stats, kept


def box_counts(mask):
    """(B, log2 R + 1) int32: the number of aligned 2^k x 2^k boxes that hold a foreground pixel, k = 0 (the area) .. log2 R (0 or 1)"""
    mask = _square_bytes(mask, "mask")
    b, r, _ = mask.shape
    counts = torch.empty(b, max(r.bit_length(), 1), device=mask.device, dtype=torch.int32)
    _C.call("ngan_morph_boxcount", mask, counts, b, r)
    return counts


def box_dimension(counts, R):
    """(B) fp64: the box-counting dimension, the least-squares slope of ln N(s) against ln(1 / s) over the box sides s = 1, 2, ...,
    R / 4, in closed form from the integer counts of `box_counts`; NaN for an empty mask"""
    n = int(R).bit_length() - 2                      # sides 2^0 .. 2^(n-1) = R / 4
    if n < 2 or counts.dim() != 2 or counts.shape[1] < n:
        raise ValueError(f"R={R} with counts {tuple(counts.shape)}: at least two box sides up to R / 4 are needed")
    c = counts[:, :n].to(torch.float64)
    y = torch.where(c > 0, c, torch.full_like(c, float("nan"))).log()
    x = -math.log(2.0) * torch.arange(n, device=counts.device, dtype=torch.float64)
    xc = x - x.mean()
    return (y * xc).sum(1) / (xc * xc).sum()


def _kept_mask(images, otsu_class, min_size, threshold):
    """the front end arbor_statistics and skeleton_statistics share: levels -> cut -> mask -> components -> kept mask.  Returns
    (R, ok (B) bool: the threshold search succeeded, stats (B, 4) int32 of connected_components, kept (B, R, R) uint8)"""
    if otsu_class not in (1, 2, 3):
        raise ValueError(f"otsu_class={otsu_class}: 1, 2 or 3 (the classes above t0, t1, t2)")
    if int(min_size) < 1:
        raise ValueError(f"min_size={min_size} must be at least 1")
    levels, hist = morph_levels(images)
    b, r, _ = levels.shape
    if threshold is None:
        thresholds, status = otsu_thresholds(hist)
        ok = status == 0
        cut = torch.where(ok, thresholds[:, otsu_class - 1], torch.full_like(status, 255))
    else:
        if not 0 <= int(threshold) <= 255:
            raise ValueError(f"threshold={threshold}: a level in 0 .. 255")
        cut = torch.full((b,), int(threshold), device=levels.device, dtype=torch.int32)
        ok = torch.ones(b, device=levels.device, dtype=torch.bool)
    mask = morph_mask(levels, cut)
    _, stats, kept = connected_components(mask, min_size)
    return r, ok, stats, kept


def arbor_statistics(images, otsu_class=1, min_size=1, threshold=None):
    """Per-image morphology of channels-last fp32 images (B, R, R, C) in [-1, 1], fp64 tensors on the device (no host read-back):
    the foreground is level > t, t the upper end of multi-Otsu class otsu_class - 1 of the image's own histogram (otsu_class=1: above
    t0, the data loader's signal / noise split) or the fixed level `threshold`; components below min_size pixels are dropped.
        fill            kept pixels / R^2                         components      counted components
        largest_share   largest component / kept pixels           dimension       box-counting dimension of the kept mask
        scored          False where the threshold search failed (fewer than four grey levels, no noise floor) or nothing is kept:
                        the other four are then not to be used (fill 0, the ratios NaN)"""
    r, ok, stats, kept = _kept_mask(images, otsu_class, min_size, threshold)
    counts = box_counts(kept)
    s = stats.to(torch.float64)
    return {"fill": s[:, 3] / float(r * r), "components": s[:, 1], "largest_share": s[:, 2] / s[:, 3],
            "dimension": box_dimension(counts, r), "scored": ok & (stats[:, 3] > 0)}


def ks_distance(a, b):
    """two-sample Kolmogorov-Smirnov distance sup |F_a - F_b| of two 1-d fp64 tensors, by sorting"""
    a, b = a.to(torch.float64).sort().values, b.to(torch.float64).sort().values
    at = torch.cat([a, b])
    fa = torch.searchsorted(a, at, right=True).to(torch.float64) / a.numel()
    fb = torch.searchsorted(b, at, right=True).to(torch.float64) / b.numel()
    return float((fa - fb).abs().max())


class Morphology:
    """Collects the per-image arbor statistics of real and generated images and compares their distributions.

        m = Morphology(image_size=64); m.feed('real', x); m.feed('fake', G(z)); m.result()

    A stage below 16 x 16 has nothing to label: feed() does nothing and result() says so."""
    STATISTICS = MORPH_STATISTICS

    def _statistics(self, x):
        return arbor_statistics(x, self.otsu_class, self.min_size)

    def _inactive_note(self):
        return f"{self.image_size} x {self.image_size} images are below {MORPH_MIN} x {MORPH_MIN}: nothing to label"

    def _rows(self, s):
        """what feed() keeps of one minibatch's statistics: a row per statistic, then `scored`"""
        return torch.stack([s[name] for name in self.STATISTICS] + [s["scored"].to(torch.float64)])

    def __init__(self, image_size, n_colors=1, otsu_class=1, min_size=1, device="cuda"):
        if n_colors not in (1, 3):
            raise ValueError(f"n_colors={n_colors}: 1 or 3")
        if image_size < 1 or image_size & (image_size - 1):
            raise ValueError(f"image_size={image_size} must be a power of two")
        if image_size > MORPH_MAX:
            raise ValueError(f"image_size={image_size}: the kernels take up to {MORPH_MAX} x {MORPH_MAX}")
        if otsu_class not in (1, 2, 3):
            raise ValueError(f"otsu_class={otsu_class}: 1, 2 or 3")
        if isinstance(min_size, bool) or int(min_size) != min_size or min_size < 1:
            raise ValueError(f"min_size={min_size!r} must be an integer >= 1")
        self.image_size, self.n_colors, self.otsu_class, self.min_size = int(image_size), int(n_colors), int(otsu_class), int(min_size)
        self.device = torch.device(device)
        self.active = self.image_size >= MORPH_MIN
        self.count = {"real": 0, "fake": 0}
        self.values = {"real": [], "fake": []}        # per feed a (k + 1, b) fp64 tensor: the k statistics and `scored`

    def feed(self, which, images):
        if which not in self.count:
            raise ValueError(f"which={which!r}: 'real' or 'fake'")
        x = channels_last(images.to(self.device))
        if tuple(x.shape[1:]) != (self.image_size, self.image_size, self.n_colors):
            raise ValueError(f"images must be {self.image_size} pixels wide with {self.n_colors} colours, got {tuple(images.shape)}")
        if not self.active:
            return
        self.values[which].append(self._rows(self._statistics(x)))
        self.count[which] += x.shape[0]

    def result(self):
        """{'fill' | 'components' | 'largest_share' | 'dimension': {'real', 'real_sem', 'fake', 'fake_sem': mean and its standard
        error over the scored images of a side (None for one image), 'ks': the two-sample Kolmogorov-Smirnov distance of the
        per-image values}, 'images': n fed per side, 'skipped_real', 'skipped_fake': images not scored}; when a side has no scored
        image, or the stage is below 16 x 16: no statistic and a 'note'"""
        if not self.active:
            return {"images": 0, "skipped_real": 0, "skipped_fake": 0, "note": self._inactive_note()}
        n = self.count["real"]
        if n == 0 or n != self.count["fake"]:
            raise ValueError(f"{n} real and {self.count['fake']} generated images; feed both sets equally")
        side = {}
        for which in ("real", "fake"):
            v = torch.cat(self.values[which], dim=1).cpu()
            k = len(self.STATISTICS)
            side[which] = v[:k][:, v[k] > 0.5]
        out = {"images": n, "skipped_real": n - side["real"].shape[1], "skipped_fake": n - side["fake"].shape[1]}
        if side["real"].shape[1] == 0 or side["fake"].shape[1] == 0:
            out["note"] = "no scored image on the {} side: every image there lacks four grey levels, a noise floor or a kept pixel".format(
                "data" if side["real"].shape[1] == 0 else "generated")
            return out
        for i, name in enumerate(self.STATISTICS):
            row = {"ks": ks_distance(side["real"][i], side["fake"][i])}
            for which in ("real", "fake"):
                v = side[which][i]
                row[which] = float(v.mean())
                row[which + "_sem"] = float(v.std(unbiased=True)) / math.sqrt(v.numel()) if v.numel() > 1 else None
            out[name] = row
        return out

    def _profile(self, axis, bins, scale):
        """{axis: [i scale], 'real', 'fake': per side the mean over its scored images of the `bins` integer rows a subclass's _rows()
        appends below `scored` (exact int64 sums divided by their number)}, cut after the last bin at which either side is non-zero"""
        k = len(self.STATISTICS)
        mean = {}
        for which in ("real", "fake"):
            v = torch.cat(self.values[which], dim=1).cpu()
            c = v[k + 1:][:, v[k] > 0.5].to(torch.int64)
            mean[which] = [int(t) / float(c.shape[1]) for t in c.sum(dim=1)]
        n = max([i + 1 for i in range(bins) if mean["real"][i] or mean["fake"][i]], default=0)
        return {axis: [i * scale for i in range(n)], "real": mean["real"][:n], "fake": mean["fake"][:n]}


def evaluate_morphology(generator, dataset, n_images=8192, batch_size=64, seed=0, otsu_class=1, min_size=1, real_from=None,
                        return_metric=False):
    """The arbor statistics of `generator`'s samples against `dataset`'s images at the generator's current resolution, built like
    evaluate_spectrum: n_images reals through the data set's own augmentation chain (its indices cycled, its generator swapped for a
    private one seeded seed + 1 and its image size set for the duration, both restored afterwards), n_images fakes under no_grad from
    latents of the sampler's distribution drawn from a private generator seeded seed + 2; one minibatch of images per side alive at
    a time; torch's global and device generators are never consumed.
    real_from: a Morphology that an earlier call returned (return_metric=True: the call then returns (result, metric)) with the same
    settings -- its data side is taken over instead of being computed again, and `dataset` is not touched (it may be None)."""
    return _evaluate_two_sets(Morphology, generator, dataset, n_images, batch_size, seed, otsu_class, min_size, real_from, return_metric)


def _evaluate_two_sets(metric_class, generator, dataset, n_images, batch_size, seed, otsu_class, min_size, real_from, return_metric,
                       **options):
    """the body of evaluate_morphology, evaluate_skeleton, evaluate_sholl and evaluate_branches: metric_class is Morphology, Skeleton,
    Sholl or Branches; options: further settings of the metric's constructor, which real_from must match as well"""
    device = next(generator.parameters()).device
    size = int(generator.image_size)
    metric = metric_class(size, n_colors=int(getattr(generator, "N_colors", 1)), otsu_class=otsu_class, min_size=min_size, device=device,
                          **options)
    if not metric.active:
        return (metric.result(), metric) if return_metric else metric.result()
    if real_from is not None:
        if (real_from.image_size, real_from.n_colors, real_from.otsu_class, real_from.min_size, real_from.count["real"]) != \
                (metric.image_size, metric.n_colors, metric.otsu_class, metric.min_size, int(n_images)) or \
                any(getattr(real_from, name, None) != getattr(metric, name) for name in options):
            raise ValueError("real_from was fed with other settings")
        metric.count["real"], metric.values["real"] = real_from.count["real"], list(real_from.values["real"])
    n_images, batch_size = int(n_images), int(batch_size)
    if n_images < 1 or batch_size < 1:
        raise ValueError(f"n_images={n_images} and batch_size={batch_size} must be positive")
    _feed_two_sets(metric, generator, dataset if real_from is None else None, n_images, batch_size, seed)
    return (metric.result(), metric) if return_metric else metric.result()


def _format_arbor(result, title, statistics, width=14, profile=None):
    """the table eval.py prints for an arbor metric: one row per statistic -- data, generated (mean +- standard error) and the KS
    distance --, labels `width` wide; profile (axis, wording): then the mean profile of either side, one number per bin, and the
    wording formatted with the bins' step"""
    if statistics[0] not in result:
        return f"{title}: {result['note']}"
    pm = lambda v, e: f"{v:10.4f} +- {e:8.4f}" if e is not None else f"{v:10.4f}" + " " * 12   # noqa: E731
    rows = [f"{title} ({result['images']} images per side; not scored: {result['skipped_real']} of the data, "
            f"{result['skipped_fake']} generated)", f"{'':>{width}s} {'data':>22s} {'generated':>22s} {'KS':>7s}"]
    for name in statistics:
        r = result[name]
        rows.append(f"{name:>{width}s} {pm(r['real'], r['real_sem'])} {pm(r['fake'], r['fake_sem'])} {r['ks']:7.3f}")
    if profile is not None:
        axis, wording = profile
        p = result["profile"]
        step = p[axis][1] if len(p[axis]) > 1 else 0.0
        rows.append(f"{'profile data':>{width}s} " + " ".join(f"{v:.2f}" for v in p["real"]) + "   (" + wording.format(step) + ")")
        rows.append(f"{'generated':>{width}s} " + " ".join(f"{v:.2f}" for v in p["fake"]))
    return "\n".join(rows)


def format_morphology(result, title="Arbor morphology"):
    return _format_arbor(result, title, MORPH_STATISTICS)


# ---- arbor skeleton: thinning, tips, junctions and length (csrc/skeleton.hip; include/ngan.h, last section) ------------------------------
SKEL_MAX = 512                               # the largest image whose bit rows the thinning kernel holds in one workgroup's LDS
SKELETON_STATISTICS = ("length", "tips", "junctions", "width")
SKEL_STATS = ("pixels", "tips", "junctions", "isolated", "orth", "diag", "passes", "area")     # the columns of `stats`


def thin(mask, want_skeleton=True):
    """(skeleton, stats) of (B, R, R) uint8 masks (non-zero: foreground), R a power of two in 16 .. 512: the Guo-Hall thinning of every
    mask as (B, R, R) uint8 0 / 1 (None with want_skeleton=False; the stats are the same bits either way) and stats (B, 8) int32:
    {pixels, tips, junctions, isolated, orth, diag} of the skeleton, the sub-iterations run, the mask's area (include/ngan.h)"""
    mask = _square_bytes(mask, "mask")
    b, r, _ = mask.shape
    skeleton = torch.empty_like(mask) if want_skeleton else None
    stats = torch.empty(b, 8, device=mask.device, dtype=torch.int32)
    _C.call("ngan_skel_thin", mask, skeleton, stats, b, r)
    return skeleton, stats


def skeleton_counts(mask):
    """(B, 8) int32: {pixels, tips, junctions, isolated, orth, diag, 0, area} of (B, R, R) uint8 masks as they are, not thinned"""
    mask = _square_bytes(mask, "mask")
    b, r, _ = mask.shape
    stats = torch.empty(b, 8, device=mask.device, dtype=torch.int32)
    _C.call("ngan_skel_counts", mask, stats, b, r)
    return stats


def skeleton_statistics(images, otsu_class=1, min_size=1, threshold=None):
    """Per-image skeleton statistics of channels-last fp32 images (B, R, R, C) in [-1, 1], R up to 512, fp64 tensors on the device (no
    host read-back): the kept mask of `arbor_statistics` (same otsu_class, min_size, threshold) is thinned, and
        length      (orth + sqrt(2) diag) / R: skeleton length in image widths    tips        skeleton pixels with one neighbour run
        width       kept pixels / skeleton pixels: the mean thickness             junctions   skeleton pixels where three or more meet
        scored      as in arbor_statistics, and False when the skeleton is empty: the others are then not to be used"""
    r, ok, stats, kept = _kept_mask(images, otsu_class, min_size, threshold)
    _, sk = thin(kept, want_skeleton=False)
    s, k = sk.to(torch.float64), stats.to(torch.float64)
    return {"length": (s[:, 4] + math.sqrt(2.0) * s[:, 5]) / float(r), "tips": s[:, 1], "junctions": s[:, 2], "width": k[:, 3] / s[:, 0],
            "scored": ok & (stats[:, 3] > 0) & (sk[:, 0] > 0)}


class Skeleton(Morphology):
    """Collects the per-image skeleton statistics of real and generated images and compares their distributions, as Morphology does:

        m = Skeleton(image_size=64); m.feed('real', x); m.feed('fake', G(z)); m.result()

    A stage below 16 x 16 has nothing to thin and one above 512 x 512 does not fit the kernel: feed() does nothing and result() says so."""
    STATISTICS = SKELETON_STATISTICS

    def __init__(self, image_size, n_colors=1, otsu_class=1, min_size=1, device="cuda"):
        super().__init__(image_size, n_colors=n_colors, otsu_class=otsu_class, min_size=min_size, device=device)
        self.active = MORPH_MIN <= self.image_size <= SKEL_MAX

    def _statistics(self, x):
        return skeleton_statistics(x, self.otsu_class, self.min_size)

    def _inactive_note(self):
        if self.image_size > SKEL_MAX:
            return f"{self.image_size} x {self.image_size} images are above {SKEL_MAX} x {SKEL_MAX}: the thinning kernel does not take them"
        return f"{self.image_size} x {self.image_size} images are below {MORPH_MIN} x {MORPH_MIN}: nothing to thin"


def evaluate_skeleton(generator, dataset, n_images=8192, batch_size=64, seed=0, otsu_class=1, min_size=1, real_from=None,
                      return_metric=False):
    """The skeleton statistics of `generator`'s samples against `dataset`'s images at the generator's current resolution, with the
    contract of evaluate_morphology: private generators seeded seed + 1 (augmentation) and seed + 2 (latents), the data set's generator
    and image size restored afterwards, torch's global and device generators never consumed; real_from: a Skeleton that an earlier
    call returned (return_metric=True) with the same settings, whose data side is taken over."""
    return _evaluate_two_sets(Skeleton, generator, dataset, n_images, batch_size, seed, otsu_class, min_size, real_from, return_metric)


def format_skeleton(result, title="Arbor skeleton"):
    return _format_arbor(result, title, SKELETON_STATISTICS)


# ---- arbor geometry: distance transform, soma and Sholl profile (csrc/sholl.hip; include/ngan.h, last section) ---------------------------
SHOLL_BINS = 91                              # rings a Sholl histogram holds: k <= 90 for every size and every centre inside the image
SHOLL_STATISTICS = ("calibre", "soma", "sholl_peak", "sholl_radius", "reach")


def sholl_step(R):
    """the ring step in pixels of an R x R image: max(2, R / 64)"""
    return max(2, int(R) // 64)


def distance_transform(mask):
    """(dist2, soma) of (B, R, R) uint8 masks (non-zero: foreground), R a power of two in 16 .. 1024.  dist2 (B, R, R) int32: 0 on the
    background, on a foreground pixel the exact squared Euclidean distance to the nearest background pixel, the ring of pixels just
    outside the image included.  soma (B, 3) int32: {y, x, dist2} of the largest dist2 -- centre and squared radius of the largest
    inscribed disc --, the smallest index y * R + x among equals; {-1, -1, 0} for an empty mask (include/ngan.h)"""
    mask = _square_bytes(mask, "mask")
    b, r, _ = mask.shape
    dist2 = torch.empty(b, r, r, device=mask.device, dtype=torch.int32)
    soma = torch.empty(b, 3, device=mask.device, dtype=torch.int32)
    ws = torch.empty(max(16, _C.lib().ngan_geom_workspace_bytes(b, r)), device=mask.device, dtype=torch.uint8)
    _C.call("ngan_geom_edt", mask, dist2, soma, ws, b, r)
    return dist2, soma


def sholl_crossings(skeleton, dist2, centre):
    """(crossings, roots) of (B, R, R) uint8 skeletons (any mask), their masks' dist2 (B, R, R) int32 and centres (B, 3) int32 {y, x, .}
    (`distance_transform`'s soma as it is).  crossings (B, 91) int32: the edges of the skeleton graph -- the orth and diag pairs of
    `skeleton_counts` -- whose ends lie in different rings of width sholl_step(R) about the centre, counted in the outer ring's bin.
    roots (B) fp64: the sum of sqrt(dist2) over the skeleton's pixels, bit-reproducible.  An image whose centre is {-1, -1, .} gets
    zeros (include/ngan.h)"""
    skeleton = _square_bytes(skeleton, "skeleton")
    b, r, _ = skeleton.shape
    if not (isinstance(dist2, torch.Tensor) and dist2.dtype == torch.int32 and tuple(dist2.shape) == (b, r, r)):
        raise TypeError(f"dist2: expected an int32 tensor {(b, r, r)}")
    if not (isinstance(centre, torch.Tensor) and centre.dtype == torch.int32 and tuple(centre.shape) == (b, 3)):
        raise TypeError(f"centre: expected an int32 tensor {(b, 3)}")
    crossings = torch.empty(b, SHOLL_BINS, device=skeleton.device, dtype=torch.int32)
    roots = torch.empty(b, device=skeleton.device, dtype=torch.float64)
    _C.call("ngan_geom_sholl", skeleton, dist2.contiguous(), centre.contiguous(), crossings, roots, b, r)
    return crossings, roots


def sholl_statistics(images, otsu_class=1, min_size=1, threshold=None):
    """Per-image arbor geometry of channels-last fp32 images (B, R, R, C) in [-1, 1], R up to 512, fp64 tensors on the device (no host
    read-back): the kept mask of `arbor_statistics` (same otsu_class, min_size, threshold) is thinned and distance-transformed, and the
    skeleton's edges are counted where they cross circles about the soma, the centre of the largest inscribed disc:
        calibre       2 roots / n - 1 with n the skeleton pixels: the mean process width in pixels (a bar of odd width w scores w)
        soma          sqrt(soma dist2): the radius in pixels of the largest inscribed disc
        sholl_peak    the largest number of crossings of any ring       sholl_radius   the smallest such ring's radius, in image widths
        reach         the radius of the last ring with a crossing, in image widths (the enclosing radius); 0 without a crossing
        scored        as in skeleton_statistics: the others are not to be used where it is False
        crossings     (B, 91) int32, the Sholl histogram itself"""
    r, ok, stats, kept = _kept_mask(images, otsu_class, min_size, threshold)
    skeleton, sk = thin(kept)
    dist2, soma = distance_transform(kept)
    crossings, roots = sholl_crossings(skeleton, dist2, soma)
    scale = sholl_step(r) / float(r)
    c = crossings.to(torch.int64)
    peak = c.max(dim=1).values
    ring = torch.arange(SHOLL_BINS, device=c.device, dtype=torch.int64)
    first_peak = torch.where(c == peak[:, None], ring, torch.full_like(ring, SHOLL_BINS)).min(dim=1).values
    last = torch.where(c > 0, ring, torch.zeros_like(ring)).max(dim=1).values
    return {"calibre": 2.0 * roots / sk[:, 0].to(torch.float64) - 1.0, "soma": soma[:, 2].to(torch.float64).sqrt(),
            "sholl_peak": peak.to(torch.float64), "sholl_radius": torch.where(peak > 0, first_peak, torch.zeros_like(peak)).to(torch.float64) * scale,
            "reach": last.to(torch.float64) * scale, "scored": ok & (stats[:, 3] > 0) & (sk[:, 0] > 0), "crossings": crossings}


class Sholl(Skeleton):
    """Collects the per-image arbor geometry of real and generated images and compares their distributions, as Skeleton does, and keeps
    the Sholl histograms for the mean profile of each side:

        m = Sholl(image_size=64); m.feed('real', x); m.feed('fake', G(z)); m.result()

    It thins, so it is active for the stages the thinning kernel takes, 16 x 16 .. 512 x 512: otherwise feed() does nothing and result()
    says so."""
    STATISTICS = SHOLL_STATISTICS

    def _statistics(self, x):
        return sholl_statistics(x, self.otsu_class, self.min_size)

    def _rows(self, s):
        """the rows of Morphology, then the 91 crossings of every image (integers, exact in fp64)"""
        return torch.cat([super()._rows(s), s["crossings"].to(torch.float64).t()])

    def result(self):
        """what Skeleton.result() returns, with the five statistics of SHOLL_STATISTICS, and 'profile': {'radius': ring radii k s / R in
        image widths, 'real', 'fake': the mean crossings of that ring over the scored images of the side (exact int64 sums divided by
        their number)}, cut after the last ring at which either side has a crossing"""
        out = super().result()
        if self.STATISTICS[0] in out:
            out["profile"] = self._profile("radius", SHOLL_BINS, sholl_step(self.image_size) / float(self.image_size))
        return out


def evaluate_sholl(generator, dataset, n_images=8192, batch_size=64, seed=0, otsu_class=1, min_size=1, real_from=None, return_metric=False):
    """The arbor geometry of `generator`'s samples against `dataset`'s images at the generator's current resolution, with the contract
    of evaluate_skeleton: private generators seeded seed + 1 (augmentation) and seed + 2 (latents), the data set's generator and image
    size restored afterwards, torch's global and device generators never consumed; real_from: a Sholl that an earlier call returned
    (return_metric=True) with the same settings, whose data side is taken over."""
    return _evaluate_two_sets(Sholl, generator, dataset, n_images, batch_size, seed, otsu_class, min_size, real_from, return_metric)


def format_sholl(result, title="Arbor geometry"):
    """the table of _format_arbor, then the mean Sholl profile of either side, one number per ring"""
    return _format_arbor(result, title, SHOLL_STATISTICS, profile=("radius", "mean crossings per ring, rings {:.4f} image widths apart"))


# ---- arbor branches: nodes, spur pruning and branch lengths (csrc/branch.hip; include/ngan.h, last section) -------------------------------
BRANCH_BINS = 64                             # bins of a branch-length histogram, max(1, R / 128) pixels wide; the last one is open
BRANCH_STATISTICS = ("forks", "nodes", "terminals", "spurs", "terminal_length", "link_length", "longest")
BRANCH_STATS = ("pixels", "node_pixels", "nodes", "branches", "terminal", "links", "free", "spurs", "term_orth", "term_diag", "link_orth",
                "link_diag", "free_orth", "free_diag", "spur_orth", "spur_diag", "node_orth", "node_diag", "longest", "forks")


def default_spur(R):
    """the spur length in pixels that branch_statistics prunes below when none is given: max(2, R / 32)"""
    return max(2, int(R) // 32)


def _spur(spur):
    if isinstance(spur, bool) or not isinstance(spur, int) or spur < 1:
        raise ValueError(f"spur={spur!r} must be an integer >= 1")
    return spur


def branch_graph(skeleton, spur=1, want_labels=False):
    """(labels, stats, hist) of (B, R, R) uint8 skeletons (any mask; non-zero: set), R a power of two in 16 .. 512.  The set pixels are
    the vertices of a graph whose edges are the orth and diag pairs of `skeleton_counts`; pixels with three or more edges are node
    pixels, their components nodes, and the components of the other pixels branches (paths and cycles).  A branch with no attachment
    to a node is free, one with two a link, one with one a spur when it has fewer than `spur` pixels and a terminal branch otherwise; a
    node that keeps three or more attachments of branches that are no spurs is a fork (include/ngan.h).
    labels (B, R, R) int32 (None with want_labels=False; stats and hist are the same bits either way): -1 on the background, the
    smallest linear index of its branch on a branch pixel, -2 - the smallest linear index of its node on a node pixel.
    stats (B, 20) int32 in the order of BRANCH_STATS; hist (B, 64) int32: the floor lengths of the terminal and link branches"""
    skeleton = _square_bytes(skeleton, "skeleton")
    spur = _spur(spur)
    b, r, _ = skeleton.shape
    if not (MORPH_MIN <= r <= SKEL_MAX and r & (r - 1) == 0):
        raise ValueError(f"R={r}: a power of two in {MORPH_MIN} .. {SKEL_MAX}")
    dev = skeleton.device
    labels = torch.empty(b, r, r, device=dev, dtype=torch.int32) if want_labels else None
    stats = torch.empty(b, len(BRANCH_STATS), device=dev, dtype=torch.int32)
    hist = torch.empty(b, BRANCH_BINS, device=dev, dtype=torch.int32)
    ws = torch.empty(max(16, _C.lib().ngan_branch_workspace_bytes(b, r)), device=dev, dtype=torch.uint8)
    _C.call("ngan_branch_graph", skeleton, labels, stats, hist, ws, b, r, spur)
    return labels, stats, hist


def branch_statistics(images, otsu_class=1, min_size=1, threshold=None, spur=None):
    """Per-image branch statistics of channels-last fp32 images (B, R, R, C) in [-1, 1], R up to 512, fp64 tensors on the device (no host
    read-back): the kept mask of `arbor_statistics` (same otsu_class, min_size, threshold) is thinned and its skeleton cut into nodes
    and branches; terminal branches below `spur` pixels (None: default_spur(R)) are pruned as thinning spurs, in one round.
        forks             nodes that keep three or more branches          nodes        branch points, pruned or not
        terminals         terminal branches that are no spurs             spurs        the pruned ones
        terminal_length   (term_orth + sqrt(2) term_diag) / max(1, terminals) / R: the mean terminal branch in image widths; 0 without one
        link_length       the same over the branches between two nodes    longest      the longest branch that is no spur, / R
        scored            as in skeleton_statistics: the others are not to be used where it is False
        hist              (B, 64) int32, the branch-length histogram itself"""
    spur = None if spur is None else _spur(spur)
    r, ok, stats, kept = _kept_mask(images, otsu_class, min_size, threshold)
    skeleton, sk = thin(kept)
    _, st, hist = branch_graph(skeleton, default_spur(r) if spur is None else spur)
    s = st.to(torch.float64)
    root2 = math.sqrt(2.0)
    return {"forks": s[:, 19], "nodes": s[:, 2], "terminals": s[:, 4], "spurs": s[:, 7],
            "terminal_length": (s[:, 8] + root2 * s[:, 9]) / s[:, 4].clamp(min=1.0) / float(r),
            "link_length": (s[:, 10] + root2 * s[:, 11]) / s[:, 5].clamp(min=1.0) / float(r), "longest": s[:, 18] / float(r),
            "scored": ok & (stats[:, 3] > 0) & (sk[:, 0] > 0), "hist": hist}


class Branches(Skeleton):
    """Collects the per-image branch statistics of real and generated images and compares their distributions, as Skeleton does, and
    keeps the branch-length histograms for the mean profile of each side:

        m = Branches(image_size=64); m.feed('real', x); m.feed('fake', G(z)); m.result()

    spur: terminal branches below that many pixels are pruned (None: default_spur(image_size)).  It thins, so it is active for the
    stages the thinning kernel takes, 16 x 16 .. 512 x 512: otherwise feed() does nothing and result() says so."""
    STATISTICS = BRANCH_STATISTICS

    def __init__(self, image_size, n_colors=1, otsu_class=1, min_size=1, device="cuda", spur=None):
        super().__init__(image_size, n_colors=n_colors, otsu_class=otsu_class, min_size=min_size, device=device)
        self.spur = default_spur(self.image_size) if spur is None else _spur(spur)

    def _statistics(self, x):
        return branch_statistics(x, self.otsu_class, self.min_size, spur=self.spur)

    def _rows(self, s):
        """the rows of Morphology, then the 64 bins of every image (integers, exact in fp64)"""
        return torch.cat([super()._rows(s), s["hist"].to(torch.float64).t()])

    def result(self):
        """what Skeleton.result() returns, with the seven statistics of BRANCH_STATISTICS, and 'profile': {'length': the bins' lower
        edges k max(1, R / 128) / R in image widths, 'real', 'fake': the mean number of terminal and link branches of that length over
        the scored images of the side (exact int64 sums divided by their number)}, cut after the last bin that either side fills"""
        out = super().result()
        if self.STATISTICS[0] in out:
            out["profile"] = self._profile("length", BRANCH_BINS, max(1, self.image_size // 128) / float(self.image_size))
        return out


def evaluate_branches(generator, dataset, n_images=8192, batch_size=64, seed=0, otsu_class=1, min_size=1, real_from=None,
                      return_metric=False, spur=None):
    """The branch statistics of `generator`'s samples against `dataset`'s images at the generator's current resolution, with the contract
    of evaluate_skeleton: private generators seeded seed + 1 (augmentation) and seed + 2 (latents), the data set's generator and image
    size restored afterwards, torch's global and device generators never consumed; real_from: a Branches that an earlier call returned
    (return_metric=True) with the same settings, `spur` included, whose data side is taken over."""
    return _evaluate_two_sets(Branches, generator, dataset, n_images, batch_size, seed, otsu_class, min_size, real_from, return_metric,
                              spur=spur)


def format_branches(result, title="Arbor branches"):
    """the table of _format_arbor, labels 16 wide, then the mean branch-length histogram of either side, one number per bin"""
    return _format_arbor(result, title, BRANCH_STATISTICS, width=16, profile=("length", "mean branches per bin, bins {:.4f} image widths wide"))


# ---- arbor trees: skeletons rooted at the soma, and SWC files (csrc/tree.hip; include/ngtree.h) ------------------------------------------
TREE_STATISTICS = ("trees", "cycles", "tips", "forks", "path_max", "path_mean", "contraction", "max_order")
TREE_STATS = ("pixels", "trees", "orth", "diag", "cycles", "leaves", "tips", "forks", "path_max", "max_order", "main_root", "main_pixels")
TREE_ORTH = 408                              # the cost of an orth edge (a diag edge costs 577): a path length in pixels is cost / 408


def _trace(skeleton, centre, want_order):
    """arbor_tree's dictionary and the workspace of the call (tools/tree_time.py reads the sweep counts there)"""
    skeleton = _square_bytes(skeleton, "skeleton")
    b, r, _ = skeleton.shape
    if not (MORPH_MIN <= r <= SKEL_MAX and r & (r - 1) == 0):
        raise ValueError(f"R={r}: a power of two in {MORPH_MIN} .. {SKEL_MAX}")
    if not (isinstance(centre, torch.Tensor) and centre.dtype == torch.int32 and tuple(centre.shape) == (b, 3)):
        raise TypeError(f"centre: expected an int32 tensor {(b, 3)}")
    dev = skeleton.device
    plane = lambda: torch.empty(b, r, r, device=dev, dtype=torch.int32)   # noqa: E731
    out = {"cost": plane(), "parent": plane(), "order": plane() if want_order else None,
           "stats": torch.empty(b, len(TREE_STATS), device=dev, dtype=torch.int32), "sums": torch.empty(b, 2, device=dev, dtype=torch.float64)}
    ws = torch.empty(max(16, _C.lib().ngtree_workspace_bytes(b, r)), device=dev, dtype=torch.uint8)
    _C.call("ngtree_trace", skeleton, centre.contiguous(), out["cost"], out["parent"], out["order"], out["stats"], out["sums"], ws, b, r)
    return out, ws


def arbor_tree(skeleton, centre, want_order=True):
    """{cost, parent, order, stats, sums} of (B, R, R) uint8 skeletons (any mask; non-zero: set), R a power of two in 16 .. 512, and
    centres (B, 3) int32 {y, x, .} (`distance_transform`'s soma as it is).  The set pixels are the vertices of the graph of
    `branch_graph`; an orth edge costs 408 and a diag edge 577.  In every component the pixel nearest the centre (the smallest index
    among equals) is a root, and the component of the nearest root of all is the main tree (include/ngtree.h).
    cost (B, R, R) int32: -1 on the background, else the cost of the cheapest path from the component's root (pixels: cost / 408).
    parent (B, R, R) int32: -2 on the background, -1 on a root, else the neighbour on a cheapest path, the smallest index among equals.
    order (B, R, R) int32 (None with want_order=False; the others are the same bits either way): -1 on the background, 0 on a root,
    else order[parent] + (parent has two or more children), the centrifugal branch order.
    stats (B, 12) int32 in the order of TREE_STATS; sums (B, 2) fp64: {the summed cost of the tips, the sum over the tips with a
    cost of their Euclidean distance from the root over their path length}.  An image whose centre is {-1, -1, .} has no root: the
    background values everywhere, zeros in stats but main_root = -1, zeros in sums"""
    return _trace(skeleton, centre, want_order)[0]


def tree_statistics(images, otsu_class=1, min_size=1, threshold=None):
    """Per-image tree statistics of channels-last fp32 images (B, R, R, C) in [-1, 1], R up to 512, fp64 tensors on the device (no host
    read-back): the kept mask of `arbor_statistics` (same otsu_class, min_size, threshold) is thinned and distance-transformed, and the
    skeleton is traced outwards from the soma, the centre of the largest inscribed disc:
        trees         components of the skeleton                      cycles       its cycle rank, edges - pixels + trees: 0 for a forest
        tips          pixels where a path from a root ends            forks        pixels where one splits
        path_max      the longest path from a root, in image widths   path_mean    the mean over the tips of their path lengths
        contraction   the mean over the tips of the Euclidean distance from the root over the path length (1: straight)
        max_order     the largest centrifugal branch order
        scored        as in skeleton_statistics: the others are not to be used where it is False
    The two means divide by max(1, tips); an isolated pixel is a tip with path 0 and contraction 0."""
    r, ok, stats, kept = _kept_mask(images, otsu_class, min_size, threshold)
    skeleton, sk = thin(kept)
    _, soma = distance_transform(kept)
    t = arbor_tree(skeleton, soma, want_order=False)
    s = t["stats"].to(torch.float64)
    tips = s[:, 6].clamp(min=1.0)
    return {"trees": s[:, 1], "cycles": s[:, 4], "tips": s[:, 6], "forks": s[:, 7], "path_max": s[:, 8] / float(TREE_ORTH) / float(r),
            "path_mean": t["sums"][:, 0] / tips / float(TREE_ORTH) / float(r), "contraction": t["sums"][:, 1] / tips, "max_order": s[:, 9],
            "scored": ok & (stats[:, 3] > 0) & (sk[:, 0] > 0)}


class Tree(Skeleton):
    """Collects the per-image tree statistics of real and generated images and compares their distributions, as Skeleton does:

        m = Tree(image_size=64); m.feed('real', x); m.feed('fake', G(z)); m.result()

    It thins, so it is active for the stages the thinning kernel takes, 16 x 16 .. 512 x 512: otherwise feed() does nothing and result()
    says so."""
    STATISTICS = TREE_STATISTICS

    def _statistics(self, x):
        return tree_statistics(x, self.otsu_class, self.min_size)


def evaluate_tree(generator, dataset, n_images=8192, batch_size=64, seed=0, otsu_class=1, min_size=1, real_from=None, return_metric=False):
    """The tree statistics of `generator`'s samples against `dataset`'s images at the generator's current resolution, with the contract
    of evaluate_skeleton: private generators seeded seed + 1 (augmentation) and seed + 2 (latents), the data set's generator and image
    size restored afterwards, torch's global and device generators never consumed; real_from: a Tree that an earlier call returned
    (return_metric=True) with the same settings, whose data side is taken over."""
    return _evaluate_two_sets(Tree, generator, dataset, n_images, batch_size, seed, otsu_class, min_size, real_from, return_metric)


def format_tree(result, title="Arbor trees"):
    return _format_arbor(result, title, TREE_STATISTICS)


def swc_nodes(skeleton, dist2, soma, tree, fragments=True):
    """The nodes of the SWC file of ONE traced skeleton, as host arrays {id, type, x, y, z, radius, parent} (int64 but x, y, z, radius:
    fp64): skeleton (R, R), dist2 (R, R) and soma (3) of its mask, tree: arbor_tree's cost and parent of that image, (R, R) each (tensors
    or arrays).  Node 1 is the soma centre: type 1, radius sqrt(soma dist2), parent -1.  The main tree's root is its child, or node 1
    itself where the two coincide; every other node is type 3 with x the column, y the row, z 0 and radius sqrt(dist2) in pixels, its
    parent the node of its parent pixel.  The main tree comes first, ordered by (cost, index), so a parent always precedes its
    children; the fragments follow in the order of their roots' indices, each ordered likewise, their roots with parent -1
    (fragments=False: the main tree alone).  No node without a soma ({-1, -1, .}).  Plain host code: this is no hot path, and the
    pixel-level tree is neither resampled nor smoothed."""
    import numpy as np
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)   # noqa: E731
    sk, d2, cost, parent = (host(a) for a in (skeleton, dist2, tree["cost"], tree["parent"]))
    sy, sx, sd = (int(v) for v in host(soma).reshape(-1)[:3])
    r = sk.shape[-1]
    sk, d2, cost, parent = sk.reshape(-1) != 0, d2.reshape(-1), cost.reshape(-1).astype(np.int64), parent.reshape(-1).astype(np.int64)
    empty = {"id": np.zeros(0, np.int64), "type": np.zeros(0, np.int64), "x": np.zeros(0), "y": np.zeros(0), "z": np.zeros(0),
             "radius": np.zeros(0), "parent": np.zeros(0, np.int64)}
    if sy < 0:
        return empty
    pixels = np.flatnonzero(sk & (cost >= 0))
    # every pixel's root: follow the parents; costs fall along them, so pixels taken in ascending cost find their parent's root done
    pixels = pixels[np.lexsort((pixels, cost[pixels]))]
    root = np.full(sk.size, -1, np.int64)
    for p in pixels:
        root[p] = p if parent[p] < 0 else root[parent[p]]
    roots = pixels[parent[pixels] < 0]
    if roots.size:
        key = (roots // r - sy) ** 2 + (roots % r - sx) ** 2
        main = int(roots[np.lexsort((roots, key))[0]])
    else:
        main = -1
    soma_is_root = main == sy * r + sx
    mine = pixels[root[pixels] == main]                                  # (already in (cost, index) order)
    rest = pixels[root[pixels] != main] if fragments else pixels[:0]
    rest = rest[np.lexsort((rest, cost[rest], root[rest]))]
    order = np.concatenate([mine[1:] if soma_is_root else mine, rest])
    node_of = np.full(sk.size, -1, np.int64)
    if soma_is_root:
        node_of[main] = 1
    node_of[order] = np.arange(2, 2 + order.size)
    up = np.where(parent[order] >= 0, node_of[np.maximum(parent[order], 0)], np.where(order == main, 1, -1))
    one = np.ones(1, np.int64)
    return {"id": np.arange(1, 2 + order.size), "type": np.concatenate([one, np.full(order.size, 3, np.int64)]),
            "x": np.concatenate([[float(sx)], (order % r).astype(np.float64)]), "y": np.concatenate([[float(sy)], (order // r).astype(np.float64)]),
            "z": np.zeros(1 + order.size), "radius": np.sqrt(np.concatenate([[float(sd)], d2[order].astype(np.float64)])),
            "parent": np.concatenate([-one, up])}


def write_swc(path, nodes, comments=()):
    """writes swc_nodes' arrays as an SWC file: `#` comment lines first, then one line per node, `id type x y z radius parent`"""
    with open(path, "w") as f:
        for line in comments:
            f.write("# " + str(line).replace("\n", " ") + "\n")
        f.write("# id type x y z radius parent\n")
        for i in range(len(nodes["id"])):
            f.write("{:d} {:d} {:.1f} {:.1f} {:.1f} {!r} {:d}\n".format(int(nodes["id"][i]), int(nodes["type"][i]), float(nodes["x"][i]),
                                                                   float(nodes["y"][i]), float(nodes["z"][i]), float(nodes["radius"][i]),
                                                                   int(nodes["parent"][i])))


ARBOR_CSV = ("file",) + TREE_STATISTICS + ("length", "soma", "scored")


def export_arbors(images, directory, prefix, otsu_class=1, min_size=1, threshold=None, fragments=True, first=0):
    """Writes, for image i of `images` ((B, R, R, C) or (B, C, R, R) fp32 in [-1, 1], R up to 512), <prefix>_<first + i>.swc -- its
    skeleton traced from the soma (swc_nodes; fragments=False: the main tree alone) --, <prefix>_<first + i>.png -- the 8-bit image as
    the metrics see it --, and one row of <directory>/arbors.csv (appended; the header when the file is new): the file name, the
    tree statistics, the skeleton's `length` and the soma radius in pixels, and `scored`.  Returns the rows as dictionaries."""
    import csv
    import os
    from PIL import Image
    x = channels_last(images)
    levels, _ = morph_levels(x)
    r, ok, stats, kept = _kept_mask(x, otsu_class, min_size, threshold)
    skeleton, sk = thin(kept)
    dist2, soma = distance_transform(kept)
    tree = arbor_tree(skeleton, soma, want_order=False)
    st = tree_statistics(x, otsu_class, min_size, threshold)
    length = (sk[:, 4].to(torch.float64) + math.sqrt(2.0) * sk[:, 5].to(torch.float64)) / float(r)
    os.makedirs(directory, exist_ok=True)
    table = os.path.join(directory, "arbors.csv")
    new = not os.path.exists(table)
    host = {k: v.cpu() for k, v in dict(tree, skeleton=skeleton, dist2=dist2, soma=soma, levels=levels, length=length, **st).items()
            if v is not None}
    rows = []
    with open(table, "a", newline="") as f:
        out = csv.writer(f)
        if new:
            out.writerow(ARBOR_CSV)
        for i in range(x.shape[0]):
            name = f"{prefix}_{first + i:04d}"
            one = {"cost": host["cost"][i], "parent": host["parent"][i]}
            nodes = swc_nodes(host["skeleton"][i], host["dist2"][i], host["soma"][i], one, fragments=fragments)
            s = dict(zip(TREE_STATS, host["stats"][i].tolist()))
            write_swc(os.path.join(directory, name + ".swc"), nodes, comments=(
                f"{name}: {r} x {r} pixels, threshold class {otsu_class}, components below {min_size} pixels dropped",
                "skeleton (Guo-Hall thinning) traced from the soma, the centre of the largest inscribed disc; pixel units, not resampled",
                f"trees {s['trees']} cycles {s['cycles']} tips {s['tips']} forks {s['forks']} main_pixels {s['main_pixels']}"
                + ("" if fragments else " (main tree alone)")))
            Image.fromarray(host["levels"][i].numpy()).save(os.path.join(directory, name + ".png"))
            row = dict({"file": name}, **{k: float(host[k][i]) for k in TREE_STATISTICS}, length=float(host["length"][i]),
                       soma=math.sqrt(float(host["soma"][i, 2])), scored=int(bool(host["scored"][i])))
            out.writerow([row[k] for k in ARBOR_CSV])
            rows.append(row)
    return rows


def format_table(result, title="SWD x 1e3"):
    if "scales" in result:
        return format_msssim(result) if title == "SWD x 1e3" else format_msssim(result, title)
    if not result["levels"]:
        return f"{title}: {result['note']}"
    head = " ".join(f"{r:>9d}" for r in result["levels"]) + "      mean"
    row = " ".join(f"{v:9.3f}" for v in result["swd"]) + f" {result['mean']:9.3f}"
    return f"{title}\n{head}\n{row}"
