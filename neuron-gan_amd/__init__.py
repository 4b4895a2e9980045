"""neuron-gan_amd: MI355X-native PGGAN / WGAN-GP training step behind the neuron-gan API.

The directory name carries a hyphen, so it is loaded under the module name `neuron_gan_amd`
(see `__graft_entry__.load_package`).  Layout:
    csrc/              hand-written gfx950 kernels + the C ABI of include/ngan.h  -> libngan_hip.so
    _C.py              ctypes binding (fails loudly if the library is missing; no CPU fallback)
    ops.py             differentiable operators closed under double-backward
    wgan_ops.py        first-order operators of the WGAN nets (stride-2 convolutions, BatchNorm-on-load)
    models.py          Generator_PG / Discriminator_PG (and Generator_wgan / Discriminator_wgan) with the reference's surface and state_dict keys
    loss_functions.py  D_W_loss / G_W_loss / D_grad_pen_loss
    utils.py           sample_latent_vec, the Checkpointer, sample grids
    metric_table.py    the checkpoint metrics as one table: configuration names, flags, checkpoint keys, functions, titles
    scoring.py         scoring a checkpoint during training: one routine over that table (`score`, `score_due`, `score_<metric>`)
    configs/config.py  module-as-singleton configuration
    train.py           the G/D step driver (flat parameters, fused Adam, data-parallel gradient exchange), epoch driver, CLI
    eval.py            sample grid from a checkpoint (the reference's eval.py), optionally from the averaged generator
    launch.py          sharding rule of a data-parallel run and the `--gpus N` rank launcher (standard library only)
    data.py            device-resident dataset with the reference's augmentation chain as one launch per batch
    metrics.py         sample quality: sliced Wasserstein distance on Laplacian-pyramid patches (csrc/swd.hip), `evaluate_swd`;
                       sample diversity: MS-SSIM between pairs of samples (csrc/msssim.hip), `evaluate_msssim`;
                       spectral fidelity: radial power spectrum of samples against the data (csrc/spectrum.hip), `evaluate_spectrum`;
                       arbor morphology: connected components and box-counting dimension of the thresholded image (csrc/morph.hip),
                       `evaluate_morphology`;
                       arbor skeleton: thinning, tips, junctions, length and width of the same mask (csrc/skeleton.hip),
                       `evaluate_skeleton`;
                       arbor geometry: exact distance transform, soma and Sholl profile of the same mask (csrc/sholl.hip),
                       `evaluate_sholl`;
                       arbor branches: nodes, spur pruning and branch lengths of the same skeleton (csrc/branch.hip),
                       `evaluate_branches`
    workmodel.py       algorithmic FLOP / byte model of an iteration (what bench.py's roofline figures divide by)
"""
from . import _C, launch, ops, wgan_ops, utils, models, loss_functions, train, data, workmodel, metrics, eval  # noqa: F401, A004
from .configs import config  # noqa: F401

__version__ = "0.1.0"
