"""Sample grid from a checkpoint: the counterpart of the reference's eval.py (eval.py:8-26).

    python neuron-gan_amd/eval.py -n 16 -weights GenDisc_0010.pth -output samples.png [--ema]

Same flags, meaning and defaults: -weights is a file in config.weights_dir, -output a file in config.images_dir (an absolute path is
taken as it is).  Added: --ema samples from the averaged generator the checkpoint carries ('Generator_ema_state', written by a run
with --ema_beta; KeyError if it holds none).  --swd [N] prints, instead of writing a grid, the sliced Wasserstein distance (metrics.py)
of the checkpoint's generator per pyramid level against N images (default 8192) of the data set that --dataset_dir (a folder, as
train.py reads it; default config.dataset_dir) or --images (a .pt / .npy file of (N, C, R, R) images in [-1, 1]) names; with --ema
the table of the averaged generator follows.  --msssim [N] prints the mean MS-SSIM (metrics.py) over N pairs of samples (default
10000) -- a collapsed generator scores near 1 -- and, when --dataset_dir or --images names a data set (or config.dataset_dir exists),
the same statistic over N pairs of its augmented images to read it against; it combines with --swd and --ema.  --spectrum [N] prints
the radial power spectrum (metrics.py) of N samples (default 8192) against N images of the data set, named as for --swd, at the octave
edges, with the mean distance in dB and the top octave's signed deficit; it combines with --swd, --msssim and --ema.  --morph [N] prints
the arbor morphology (metrics.py) of N samples (default 8192) against N images of the data set, named as for --swd: components,
largest component's share, fill and box-counting dimension with the Kolmogorov-Smirnov distance of each; components below
--morph_min_size pixels are dropped; it combines with --swd, --msssim, --spectrum, --ema and --images.  --skeleton [N] prints, after
the morphology table when both are asked for, the arbor skeleton (metrics.py) of N samples (default 8192) against N images of the
data set: skeleton length in image widths, tips, junctions and mean process width with the Kolmogorov-Smirnov distance of each;
components below --skeleton_min_size pixels are not thinned; it combines with every switch above.  --sholl [N] prints, after the skeleton
table when both are asked for, the arbor geometry (metrics.py) of N samples (default 8192) against N images of the data set: mean
process calibre and soma radius in pixels, the peak of the Sholl histogram about the soma and its radius, and the enclosing radius, in
image widths, with the Kolmogorov-Smirnov distance of each, then the mean Sholl profile of either side; components below
--sholl_min_size pixels are not measured; it combines with every switch above.  --branches [N] prints, after the geometry table when
both are asked for, the arbor branches (metrics.py) of N samples (default 8192) against N images of the data set: forks (branch points
that keep three branches after spur pruning), nodes, terminal branches, spurs, the mean terminal and link branch and the longest branch
in image widths, with the Kolmogorov-Smirnov distance of each, then the mean branch-length histogram of either side; terminal branches
below --branch_spur pixels count as spurs (0: max(2, image size / 32)), components below --branch_min_size pixels are not measured; it
combines with every switch above.

    python neuron-gan_amd/eval.py -weights GenDisc_0010.pth --swd 8192 --dataset_dir data/science_2022 [--ema]
    python neuron-gan_amd/eval.py -weights GenDisc_0010.pth --msssim 10000 --dataset_dir data/science_2022 [--ema]
    python neuron-gan_amd/eval.py -weights GenDisc_0010.pth --spectrum 8192 --dataset_dir data/science_2022 [--ema]
    python neuron-gan_amd/eval.py -weights GenDisc_0010.pth --morph 8192 --dataset_dir data/science_2022 [--ema]
    python neuron-gan_amd/eval.py -weights GenDisc_0010.pth --skeleton 8192 --dataset_dir data/science_2022 [--ema]
    python neuron-gan_amd/eval.py -weights GenDisc_0010.pth --sholl 8192 --dataset_dir data/science_2022 [--ema]
    python neuron-gan_amd/eval.py -weights GenDisc_0010.pth --branches 8192 --dataset_dir data/science_2022 [--ema]

The generator runs on the HIP kernels, so this needs a GPU, like train.py."""
import argparse
import os
import sys


def build_arg_parser():
    p = argparse.ArgumentParser()
    p.add_argument('-n', type=int, default=16, help='Number of samples created')
    p.add_argument('-output', type=str, default='samples_default.png', help='Filename of the output image file stored in ./samples')
    p.add_argument('-weights', type=str, default='gen_dis_default.pth', help='Filename of the weights stored in ./weights')
    # addition of this implementation
    p.add_argument('--ema', action='store_true', default=False, help='sample from the averaged generator of the checkpoint')
    p.add_argument('--swd', type=int, nargs='?', const=8192, default=None, metavar='N',
                   help='print the sliced Wasserstein distance per pyramid level against N images of the data set (default 8192)')
    p.add_argument('--swd_seed', type=int, default=0, help='seed of the SWD patch corners, directions, latents and augmentations')
    p.add_argument('--msssim', type=int, nargs='?', const=10000, default=None, metavar='N',
                   help='print the mean MS-SSIM over N pairs of samples, and of the data set when one is named (default 10000)')
    p.add_argument('--msssim_seed', type=int, default=0, help='seed of the MS-SSIM latents and augmentations')
    p.add_argument('--spectrum', type=int, nargs='?', const=8192, default=None, metavar='N',
                   help='print the radial power spectrum of N samples against N images of the data set (default 8192)')
    p.add_argument('--spectrum_seed', type=int, default=0, help='seed of the spectrum latents and augmentations')
    p.add_argument('--morph', type=int, nargs='?', const=8192, default=None, metavar='N',
                   help='print the arbor morphology of N samples against N images of the data set (default 8192)')
    p.add_argument('--morph_seed', type=int, default=0, help='seed of the morphology latents and augmentations')
    p.add_argument('--morph_min_size', type=int, default=1, help='components below this many pixels are dropped (1 drops none)')
    p.add_argument('--skeleton', type=int, nargs='?', const=8192, default=None, metavar='N',
                   help='print the arbor skeleton of N samples against N images of the data set (default 8192)')
    p.add_argument('--skeleton_seed', type=int, default=0, help='seed of the skeleton latents and augmentations')
    p.add_argument('--skeleton_min_size', type=int, default=1, help='components below this many pixels are not thinned (1 drops none)')
    p.add_argument('--sholl', type=int, nargs='?', const=8192, default=None, metavar='N',
                   help='print the arbor geometry (calibre, soma, Sholl profile) of N samples against N images of the data set (default 8192)')
    p.add_argument('--sholl_seed', type=int, default=0, help='seed of the arbor-geometry latents and augmentations')
    p.add_argument('--sholl_min_size', type=int, default=1, help='components below this many pixels are not measured (1 drops none)')
    p.add_argument('--branches', type=int, nargs='?', const=8192, default=None, metavar='N',
                   help='print the arbor branches (forks, spurs, branch lengths) of N samples against N images of the data set (default 8192)')
    p.add_argument('--branch_seed', type=int, default=0, help='seed of the arbor-branch latents and augmentations')
    p.add_argument('--branch_min_size', type=int, default=1, help='components below this many pixels are not measured (1 drops none)')
    p.add_argument('--branch_spur', type=int, default=0, help='terminal branches below this many pixels are pruned as thinning spurs '
                                                              '(0: max(2, image size / 32))')
    p.add_argument('--dataset_dir', type=str, default='', help='folder of training images (default: config.dataset_dir)')
    p.add_argument('--images', type=str, default='', help='.pt / .npy file with the images (N, C, R, R) in [-1, 1]')
    return p


def load_dataset(options, config, device):
    """the data set `--swd` / `--msssim` / `--spectrum` / `--morph` / `--skeleton` / `--sholl` / `--branches` score against, read the way train.py reads it"""
    import numpy as np
    import torch
    from .data import NeuronDataset
    from .train import TensorImageDataset
    if options.images:
        data = torch.load(options.images) if options.images.endswith('.pt') else torch.from_numpy(np.load(options.images))
        data = data.float()
        if data.dim() == 4 and data.shape[1] == 1:
            return NeuronDataset((data + 1.0) * 0.5, augmentations=True, im_translation=float(config.translation), device=device,
                                 seed=options.swd_seed)
        return TensorImageDataset(data.to(device))
    directory = os.path.abspath(options.dataset_dir or config.dataset_dir)
    if not os.path.exists(directory):
        raise ValueError('The dataset path {} does not exist.'.format(directory))
    return NeuronDataset.from_directory(directory, augmentations=True, im_translation=float(config.translation), device=device,
                                        seed=options.swd_seed, fill_seed=options.swd_seed)


def main(argv=None):
    import torch
    from .configs import config
    from .models import Generator_PG
    from .utils import plot_gen_samples
    options = build_arg_parser().parse_args(list(sys.argv[1:] if argv is None else argv))
    weights = os.path.join(config.weights_dir, options.weights)
    output = os.path.join(config.images_dir, options.output)
    if not os.path.exists(weights):
        raise FileExistsError(f'{weights} does not exist.')
    if not torch.cuda.is_available():
        raise RuntimeError("the HIP path needs a GPU (there is no CPU fallback)")
    device = torch.device('cuda')
    if options.msssim is not None and options.msssim < 1:
        raise ValueError('--msssim {}: at least one pair'.format(options.msssim))
    if options.spectrum is not None and options.spectrum < 1:
        raise ValueError('--spectrum {}: at least one image'.format(options.spectrum))
    if options.morph is not None and (options.morph < 1 or options.morph_min_size < 1):
        raise ValueError('--morph {} --morph_min_size {}: at least one image and one pixel'.format(options.morph, options.morph_min_size))
    if options.skeleton is not None and (options.skeleton < 1 or options.skeleton_min_size < 1):
        raise ValueError('--skeleton {} --skeleton_min_size {}: at least one image and one pixel'.format(options.skeleton,
                                                                                                        options.skeleton_min_size))
    if options.sholl is not None and (options.sholl < 1 or options.sholl_min_size < 1):
        raise ValueError('--sholl {} --sholl_min_size {}: at least one image and one pixel'.format(options.sholl, options.sholl_min_size))
    if options.branches is not None and (options.branches < 1 or options.branch_min_size < 1 or options.branch_spur < 0):
        raise ValueError('--branches {} --branch_min_size {} --branch_spur {}: at least one image and one pixel, and no negative spur'.format(
            options.branches, options.branch_min_size, options.branch_spur))
    if options.swd is not None:
        from .metrics import evaluate_swd, format_table
        if options.swd < 1:
            raise ValueError('--swd {}: at least one image'.format(options.swd))
        dataset = load_dataset(options, config, device)
        for use_ema in ((False, True) if options.ema else (False,)):
            G = Generator_PG.from_state_dict(weights, device=device, use_ema=use_ema, verbose=False).to(device)
            res = evaluate_swd(G, dataset, n_images=options.swd, batch_size=min(options.swd, 32), seed=options.swd_seed)
            print(format_table(res, 'SWD x 1e3, {} generator of {} against {} images'.format(
                'averaged' if use_ema else 'training', options.weights, options.swd)))
        if options.msssim is None and options.spectrum is None and options.morph is None and options.skeleton is None and options.sholl is None and options.branches is None:
            return 0
    if options.msssim is not None:
        from .metrics import evaluate_msssim, format_msssim
        named = options.images or options.dataset_dir or os.path.exists(config.dataset_dir)
        dataset = load_dataset(options, config, device) if named else None      # no data set: the generated side alone
        for use_ema in ((False, True) if options.ema else (False,)):
            G = Generator_PG.from_state_dict(weights, device=device, use_ema=use_ema, verbose=False).to(device)
            res = evaluate_msssim(G, dataset, n_pairs=options.msssim, batch_size=min(options.msssim, 32), seed=options.msssim_seed)
            print(format_msssim(res, 'MS-SSIM between pairs, {} generator of {}'.format('averaged' if use_ema else 'training',
                                                                                       options.weights)))
        if options.spectrum is None and options.morph is None and options.skeleton is None and options.sholl is None and options.branches is None:
            return 0
    if options.spectrum is not None:
        from .metrics import evaluate_spectrum, format_spectrum
        dataset = load_dataset(options, config, device)
        for use_ema in ((False, True) if options.ema else (False,)):
            G = Generator_PG.from_state_dict(weights, device=device, use_ema=use_ema, verbose=False).to(device)
            res = evaluate_spectrum(G, dataset, n_images=options.spectrum, batch_size=min(options.spectrum, 32),
                                    seed=options.spectrum_seed)
            print(format_spectrum(res, 'Radial power spectrum, {} generator of {}'.format('averaged' if use_ema else 'training',
                                                                                          options.weights)))
        if options.morph is None and options.skeleton is None and options.sholl is None and options.branches is None:
            return 0
    if options.morph is not None:
        from .metrics import evaluate_morphology, format_morphology
        dataset = load_dataset(options, config, device)
        for use_ema in ((False, True) if options.ema else (False,)):
            G = Generator_PG.from_state_dict(weights, device=device, use_ema=use_ema, verbose=False).to(device)
            res = evaluate_morphology(G, dataset, n_images=options.morph, batch_size=min(options.morph, 32), seed=options.morph_seed,
                                      min_size=options.morph_min_size)
            print(format_morphology(res, 'Arbor morphology, {} generator of {}'.format('averaged' if use_ema else 'training',
                                                                                     options.weights)))
        if options.skeleton is None and options.sholl is None and options.branches is None:
            return 0
    if options.skeleton is not None:
        from .metrics import evaluate_skeleton, format_skeleton
        dataset = load_dataset(options, config, device)
        for use_ema in ((False, True) if options.ema else (False,)):
            G = Generator_PG.from_state_dict(weights, device=device, use_ema=use_ema, verbose=False).to(device)
            res = evaluate_skeleton(G, dataset, n_images=options.skeleton, batch_size=min(options.skeleton, 32), seed=options.skeleton_seed,
                                    min_size=options.skeleton_min_size)
            print(format_skeleton(res, 'Arbor skeleton, {} generator of {}'.format('averaged' if use_ema else 'training',
                                                                                 options.weights)))
        if options.sholl is None and options.branches is None:
            return 0
    if options.sholl is not None:
        from .metrics import evaluate_sholl, format_sholl
        dataset = load_dataset(options, config, device)
        for use_ema in ((False, True) if options.ema else (False,)):
            G = Generator_PG.from_state_dict(weights, device=device, use_ema=use_ema, verbose=False).to(device)
            res = evaluate_sholl(G, dataset, n_images=options.sholl, batch_size=min(options.sholl, 32), seed=options.sholl_seed,
                                 min_size=options.sholl_min_size)
            print(format_sholl(res, 'Arbor geometry, {} generator of {}'.format('averaged' if use_ema else 'training', options.weights)))
        if options.branches is None:
            return 0
    if options.branches is not None:
        from .metrics import evaluate_branches, format_branches
        dataset = load_dataset(options, config, device)
        for use_ema in ((False, True) if options.ema else (False,)):
            G = Generator_PG.from_state_dict(weights, device=device, use_ema=use_ema, verbose=False).to(device)
            res = evaluate_branches(G, dataset, n_images=options.branches, batch_size=min(options.branches, 32), seed=options.branch_seed,
                                    min_size=options.branch_min_size, spur=options.branch_spur or None)
            print(format_branches(res, 'Arbor branches, {} generator of {}'.format('averaged' if use_ema else 'training', options.weights)))
        return 0
    G = Generator_PG.from_state_dict(weights, device=device, use_ema=options.ema).to(device)
    plot_gen_samples(G, N_images=options.n, filename=output)
    return 0


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import launch                      # standard library only; loads this directory as the package `neuron_gan_amd`
    sys.exit(launch.load_package().eval.main())
