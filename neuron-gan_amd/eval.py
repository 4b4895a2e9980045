"""Sample grid from a checkpoint: the counterpart of the reference's eval.py (eval.py:8-26).

    python neuron-gan_amd/eval.py -n 16 -weights GenDisc_0010.pth -output samples.png [--ema]
    python neuron-gan_amd/eval.py -weights GenDisc_0010.pth --swd 8192 --sholl --dataset_dir data/science_2022 [--ema]

Same flags, meaning and defaults: -weights is a file in config.weights_dir, -output a file in config.images_dir (an absolute path is
taken as it is).  Added: --ema samples from the averaged generator the checkpoint carries ('Generator_ema_state', written by a run
with --ema_beta; KeyError if it holds none).  One switch per row of metric_table.METRICS -- --swd, --msssim, --spectrum, --morph,
--skeleton, --sholl, --branches, each with an optional N (default 8192; --msssim: 10000 pairs) -- prints, instead of writing a grid, that
metric's table (metrics.py) of the checkpoint's generator over N samples against N images of the data set that --dataset_dir (a folder,
as train.py reads it; default config.dataset_dir) or --images (a .pt / .npy file of (N, C, R, R) images in [-1, 1]) names; with --ema the
table of the averaged generator follows.  The switches combine; the tables come in the order above.  Each metric has its --<name>_seed.
--msssim also scores without a data set, the generated pairs alone (a collapsed generator scores near 1).  The four arbor metrics drop
components below --<name>_min_size pixels; --branches counts terminal branches below --branch_spur pixels as spurs (0: max(2, image
size / 32)).  --tree [N] (with --tree_seed, --tree_min_size) prints the table of the rooted skeletons after those, in the same way.
--swc DIR exports --swc_count (default 64) samples of the generator, traced from the soma, as SWC files with a PNG each and a table
arbors.csv (metrics.export_arbors): of the averaged generator too with --ema, and of the data set when --dataset_dir or --images is
given; --swc_seed seeds them, --swc_main_only leaves the fragments out, --tree_min_size drops small components.

The generator runs on the HIP kernels, so this needs a GPU, like train.py."""
import argparse
import os
import sys


def build_arg_parser():
    from .metric_table import METRICS, settings
    p = argparse.ArgumentParser()
    p.add_argument('-n', type=int, default=16, help='Number of samples created')
    p.add_argument('-output', type=str, default='samples_default.png', help='Filename of the output image file stored in ./samples')
    p.add_argument('-weights', type=str, default='gen_dis_default.pth', help='Filename of the weights stored in ./weights')
    # addition of this implementation
    p.add_argument('--ema', action='store_true', default=False, help='sample from the averaged generator of the checkpoint')
    for m in METRICS:
        p.add_argument('--' + m.switch, type=int, nargs='?', const=m.count_default, default=None, metavar='N',
                       help='print the table "{}" over N {} per side (default {})'.format(m.title, m.count, m.count_default))
        for name, _, default, text in settings(m)[2:]:
            p.add_argument('--' + name, type=int, default=default, help=text)
    # the arbor trees are no row of the table (scoring checkpoints with them during training is not wired up): their switches stand here
    p.add_argument('--tree', type=int, nargs='?', const=8192, default=None, metavar='N',
                   help='print the table "Arbor trees" over N images per side (default 8192)')
    p.add_argument('--tree_seed', type=int, default=0, help='seed of the latents, augmentations and other draws: Arbor trees')
    p.add_argument('--tree_min_size', type=int, default=1, help='components below this many pixels are dropped (1 drops none)')
    p.add_argument('--swc', type=str, default='', metavar='DIR',
                   help='export traced samples into DIR: one .swc and one .png per image and a row of DIR/arbors.csv')
    p.add_argument('--swc_count', type=int, default=64, help='samples to export per set')
    p.add_argument('--swc_seed', type=int, default=0, help='seed of the latents and augmentations of the exported samples')
    p.add_argument('--swc_main_only', action='store_true', default=False, help='write the main tree alone, without the fragments')
    p.add_argument('--dataset_dir', type=str, default='', help='folder of training images (default: config.dataset_dir)')
    p.add_argument('--images', type=str, default='', help='.pt / .npy file with the images (N, C, R, R) in [-1, 1]')
    return p


def load_dataset(options, config, device):
    """the data set the metric switches score against, read the way train.py reads it"""
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


def export_swc(options, config, weights, device):
    """--swc: --swc_count samples of the checkpoint's generator (prefix `generated`), of the averaged one too with --ema (`averaged`),
    and, when --dataset_dir or --images names a data set, as many of its images through its augmentation chain (`data`), each as an
    SWC file, a PNG and a row of arbors.csv in the directory; latents and augmentations from private generators"""
    import torch
    from . import metrics
    from .models import Generator_PG
    n = options.swc_count
    if n < 1 or options.swc_seed < 0 or options.tree_min_size < 1:
        raise ValueError('--swc_count {} --swc_seed {} --tree_min_size {}: the lowest legal values are 1, 0, 1'.format(
            n, options.swc_seed, options.tree_min_size))
    directory = os.path.abspath(options.swc)
    kw = dict(min_size=options.tree_min_size, fragments=not options.swc_main_only)
    size = None
    for use_ema in ((False, True) if options.ema else (False,)):
        G = Generator_PG.from_state_dict(weights, device=device, use_ema=use_ema, verbose=False).to(device)
        size = int(G.image_size)
        lat = torch.Generator(device='cpu').manual_seed(options.swc_seed + 2)
        for i in range(0, n, 32):
            with torch.no_grad():
                fakes = G(metrics._latents(G, min(32, n - i), lat, device)).detach()
            metrics.export_arbors(fakes, directory, 'averaged' if use_ema else 'generated', first=i, **kw)
    if options.images or options.dataset_dir:
        dataset = load_dataset(options, config, device)
        with metrics._private_stream(dataset, size, options.swc_seed):
            for i in range(0, n, 32):
                idx = [(i + j) % len(dataset) for j in range(min(32, n - i))]
                metrics.export_arbors(metrics._real_batch(dataset, idx, device), directory, 'data', first=i, **kw)
    print('{} traced samples per set written to {}'.format(n, directory))


def main(argv=None):
    import torch
    from . import metrics
    from .configs import config
    from .metric_table import METRICS, settings
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
    asked = [(m, getattr(options, m.switch)) for m in METRICS if getattr(options, m.switch) is not None]
    for m, n in asked:
        given = [('--' + m.switch, n, 1)] + [('--' + name, getattr(options, name), lowest) for name, lowest, _, _ in settings(m)[3:]]
        if any(value < lowest for _, value, lowest in given):
            raise ValueError(' '.join('{} {}'.format(flag, value) for flag, value, _ in given) + ': the lowest legal values are ' +
                             ', '.join(str(lowest) for _, _, lowest in given))
    for m, n in asked:
        named = m.needs_data or options.images or options.dataset_dir or os.path.exists(config.dataset_dir)
        dataset = load_dataset(options, config, device) if named else None      # no data set: the generated side alone
        kw = {'n_' + m.count: n, 'batch_size': min(n, 32), 'seed': getattr(options, m.prefix + '_seed')}
        for name, _, _, at_zero, _ in m.options:
            value = getattr(options, m.prefix + '_' + name)
            kw[name] = value if at_zero is None else value or None             # (0: the metric's own default)
        for use_ema in ((False, True) if options.ema else (False,)):
            G = Generator_PG.from_state_dict(weights, device=device, use_ema=use_ema, verbose=False).to(device)
            res = getattr(metrics, m.evaluate)(G, dataset, **kw)
            # the objective the checkpoint was trained with goes into the title, unless it is the reference's (a file without the key)
            objective = getattr(G, 'trained_objective', 'wasserstein')
            print(getattr(metrics, m.format)(res, '{}, {} generator of {}{}{}'.format(
                m.title, 'averaged' if use_ema else 'training', options.weights, m.title_tail.format(n=n),
                '' if objective == 'wasserstein' else ', {} objective'.format(objective))))
    done = bool(asked)
    if options.tree is not None:
        if options.tree < 1 or options.tree_min_size < 1 or options.tree_seed < 0:
            raise ValueError('--tree {} --tree_seed {} --tree_min_size {}: the lowest legal values are 1, 0, 1'.format(
                options.tree, options.tree_seed, options.tree_min_size))
        dataset = load_dataset(options, config, device)
        for use_ema in ((False, True) if options.ema else (False,)):
            G = Generator_PG.from_state_dict(weights, device=device, use_ema=use_ema, verbose=False).to(device)
            res = metrics.evaluate_tree(G, dataset, n_images=options.tree, batch_size=min(options.tree, 32), seed=options.tree_seed,
                                        min_size=options.tree_min_size)
            objective = getattr(G, 'trained_objective', 'wasserstein')
            print(metrics.format_tree(res, 'Arbor trees, {} generator of {}{}'.format(
                'averaged' if use_ema else 'training', options.weights,
                '' if objective == 'wasserstein' else ', {} objective'.format(objective))))
        done = True
    if options.swc:
        export_swc(options, config, weights, device)
        done = True
    if done:
        return 0
    G = Generator_PG.from_state_dict(weights, device=device, use_ema=options.ema).to(device)
    plot_gen_samples(G, N_images=options.n, filename=output)
    return 0


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import launch                      # standard library only; loads this directory as the package `neuron_gan_amd`
    sys.exit(launch.load_package().eval.main())
