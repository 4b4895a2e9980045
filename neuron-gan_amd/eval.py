"""Sample grid from a checkpoint: the counterpart of the reference's eval.py (eval.py:8-26).

    python neuron-gan_amd/eval.py -n 16 -weights GenDisc_0010.pth -output samples.png [--ema]

Same flags, meaning and defaults: -weights is a file in config.weights_dir, -output a file in config.images_dir (an absolute path is
taken as it is).  Added: --ema samples from the averaged generator the checkpoint carries ('Generator_ema_state', written by a run
with --ema_beta; KeyError if it holds none).  The generator runs on the HIP kernels, so this needs a GPU, like train.py."""
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
    return p


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
    G = Generator_PG.from_state_dict(weights, device=device, use_ema=options.ema).to(device)
    plot_gen_samples(G, N_images=options.n, filename=output)
    return 0


if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import launch                      # standard library only; loads this directory as the package `neuron_gan_amd`
    sys.exit(launch.load_package().eval.main())
