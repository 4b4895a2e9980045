"""Module-as-singleton configuration with the reference's variable names and validation rules.

Mirrors /root/reference/configs/config.py: the module's globals ARE the configuration (config.py:8-63), a user
file can overlay them (`import_configs`, config.py:208-263), unknown names are rejected (config.py:242-243) and
`validate_configs` applies the same PGGAN checks and derives `transit_sch` from `transit_period`
(config.py:165-200).  Differences, all outside the training-step hot path: no interactive prompts (a clash
raises instead of asking, config.py:137-146) and directories are only created when `create_dirs=True`.
"""
import importlib.util
import os
import sys
import uuid
from types import FunctionType, ModuleType

import numpy as np
import torch

from ..metric_table import METRICS, settings

_HERE = os.path.dirname(os.path.abspath(__file__))

_DEFAULTS = dict(
    # directories
    root_dir=os.path.abspath(os.path.join(_HERE, os.pardir)), configs_dir=_HERE,
    # WGAN
    wgan=False, n_critic=1, adapt_critic=False, weights_init='', unroll_steps=0,
    # PGGAN
    pggan=True, grad_pen_lambda=10, transit_sch=[25000, 50000, 75000, 100000, 125000], transit_period=None,
    alpha_step=0.0001,
    # training
    ID=uuid.uuid4().hex[:4], RMSprop=False, learning_rate=0.0001, batch_size=8, N_epochs=150000, N_epochs_session=None,
    beta1=0.5, sim_loss_lambda=0.0, sim_loss_lambda_decay_rate=0.0, drift_epsilon=0.001, resume=False, N_workers=2,
    seed=1, checkpointing_period=100, device='default', pin_memory=False, ema_beta=0.0,
    # the checkpoint metrics: <prefix>_period, _images (or _pairs), _seed and the metric's own options, row by row
    **{name: default for m in METRICS for name, _, default, _ in settings(m)},
    diffaug='', diffaug_p=1.0, diffaug_seed=0, lsgan=False, mbstd_group=0, grad_pen_mode='gp', grad_pen_interval=1,
    spec_loss_lambda=0.0, spec_loss_floor=1e-3, spec_loss_images=256, spec_loss_seed=0, sim_loss_on='real', sim_loss_center=False,
    ada_target=0.0, ada_interval=4, ada_kimg=500.0, ada_p_init=0.0,
    # dataset
    dataset_name='science_2022', translation=0.05, image_preprocessing='cpu',
    # architecture
    latent_dim=512, image_size=512, N_colors=1, LeakyReLU_leak=0.2,
    N_gen_features=[128, 64, 32, 32, 16, 16], N_dis_features=[16, 16, 32, 32, 64, 128],
)
_DEFAULTS.update(
    data_dir=os.path.join(_DEFAULTS['root_dir'], 'data'), images_dir=os.path.join(_DEFAULTS['root_dir'], 'images'),
    weights_dir=os.path.join(_DEFAULTS['root_dir'], 'weights'), plots_dir=os.path.join(_DEFAULTS['root_dir'], 'plots'),
    logs_dir=os.path.join(_DEFAULTS['root_dir'], 'logs'))
_DEFAULTS.update(dataset_dir=os.path.join(_DEFAULTS['data_dir'], _DEFAULTS['dataset_name']),
                 samples_sub_dir=os.path.join(_DEFAULTS['images_dir'], _DEFAULTS['ID']))

globals().update(_DEFAULTS)
configs_name = dict(_DEFAULTS)  # the set of legal configuration names (reference: config.py:81)

# widths keyed by training ID (reference config.py:84-105)
_ID_WIDTHS = {
    ('0004', '0005'): ([1024, 512, 256, 128, 64, 32, 16, 8], [16, 32, 64, 128, 128, 128, 128]),
    ('0006',): ([512, 256, 128, 64, 32, 16, 8, 8], [64, 128, 256, 256, 256, 128, 64]),
    ('0007',): ([512, 256, 128, 64, 32, 16], [16, 32, 64, 128, 256, 512]),
    ('0008',): ([512, 256, 128, 64], [64, 128, 256, 512]),
    ('0009',): ([32, 32, 32, 32, 16, 16], [16, 16, 32, 32, 32, 32]),
    ('0010', '0011', '0012'): ([128, 64, 32, 32, 16, 16], [16, 16, 32, 32, 64, 128]),
}


def define_ID_dependent_configs():
    g = globals()
    assert g['ID'] != '', 'ID is not defined.'
    for ids, (gen, dis) in _ID_WIDTHS.items():
        if g['ID'] in ids:
            g['N_gen_features'], g['N_dis_features'] = list(gen), list(dis)
    g['samples_sub_dir'] = os.path.join(g['images_dir'], '{}'.format(g['ID']))


def print_configs():
    print('Configurations:')
    for name in configs_name:
        print(f'{name}:', globals()[name])


def validate_configs(create_dirs=False):
    g = globals()
    for d in ('dataset_dir', 'images_dir', 'samples_sub_dir', 'weights_dir', 'plots_dir'):
        g[d] = os.path.abspath(g[d])
    if create_dirs:
        for d in ('images_dir', 'weights_dir', 'plots_dir', 'logs_dir', 'samples_sub_dir'):
            os.makedirs(g[d], exist_ok=True)
    if g['device'] == 'default':
        g['device'] = 'cuda' if torch.cuda.is_available() else 'cpu'

    image_size_log = np.round(np.log2(g['image_size']))
    assert g['image_size'] == 2 ** image_size_log, 'Image size must be a power of 2.'
    assert g['device'] in ['cpu', 'cuda', 'mps'], f"device:{g['device']} is not supported."
    assert g['ID'] != '', 'The training ID is undefined.'
    # the averaged generator (an addition of this implementation): 0 is off, otherwise the decay
    if not (isinstance(g['ema_beta'], (int, float)) and 0 <= g['ema_beta'] < 1):
        raise ValueError(f"ema_beta={g['ema_beta']!r} must lie in [0, 1)")
    # the metrics scored at checkpoints (additions of this implementation, one row of metric_table.METRICS each): <prefix>_period 0 is
    # off, otherwise every checkpoint whose epoch is a multiple of it is scored on <prefix>_images images (msssim_pairs pairs) per side,
    # drawn with <prefix>_seed; the arbor metrics drop components below <prefix>_min_size pixels (1 drops none) and branch_spur prunes
    # terminal branches below that many pixels as thinning spurs, 0: max(2, image size / 32)
    for m in METRICS:
        for name, lowest, _, _ in settings(m):
            if not (isinstance(g[name], int) and not isinstance(g[name], bool) and g[name] >= lowest):
                raise ValueError(f"{name}={g[name]!r} must be an integer >= {lowest}")
    # differentiable augmentation of the critic's inputs (an addition of this implementation): diffaug '' is off, otherwise a comma
    # list of groups, each applied to each sample with probability diffaug_p; diffaug_seed seeds the parameters' private stream
    groups = [s.strip() for s in g['diffaug'].split(',')] if isinstance(g['diffaug'], str) else None
    if groups is None or any(s not in ('', 'color', 'translation', 'cutout', 'blit', 'geometry') for s in groups):
        raise ValueError(f"diffaug={g['diffaug']!r} must be a comma list from color, translation, cutout, blit, geometry (empty: off)")
    if isinstance(g['diffaug_p'], bool) or not (isinstance(g['diffaug_p'], (int, float)) and 0 <= g['diffaug_p'] <= 1):
        raise ValueError(f"diffaug_p={g['diffaug_p']!r} must lie in [0, 1]")
    if not (isinstance(g['diffaug_seed'], int) and not isinstance(g['diffaug_seed'], bool) and g['diffaug_seed'] >= 0):
        raise ValueError(f"diffaug_seed={g['diffaug_seed']!r} must be an integer >= 0")
    if any(groups) and g['wgan'] and not g['pggan']:
        raise ValueError(f"diffaug={g['diffaug']!r} is not available for the WGAN nets (wgan=True, pggan=False)")
    # adaptive augmentation probability (an addition of this implementation; Karras et al. 2020): ada_target 0 is off, otherwise the
    # value r_t = E[sign(D(real) - t)] is held at (0.6 recommended) by moving the probability of the diffaug groups, every
    # ada_interval-th iteration, at a rate of 0 -> 1 over 1000 ada_kimg real images, from ada_p_init; diffaug_p is then the upper clamp
    real = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and np.isfinite(v)      # noqa: E731
    if not (real(g['ada_target']) and 0 <= g['ada_target'] < 1):
        raise ValueError(f"ada_target={g['ada_target']!r} must be 0 (off) or lie in (0, 1)")
    if isinstance(g['ada_interval'], bool) or not (isinstance(g['ada_interval'], int) and g['ada_interval'] >= 1):
        raise ValueError(f"ada_interval={g['ada_interval']!r} must be an integer >= 1")
    if not (real(g['ada_kimg']) and g['ada_kimg'] > 0):
        raise ValueError(f"ada_kimg={g['ada_kimg']!r} must be a finite number > 0")
    if not (real(g['ada_p_init']) and 0 <= g['ada_p_init'] <= g['diffaug_p']):
        raise ValueError(f"ada_p_init={g['ada_p_init']!r} must lie in [0, diffaug_p = {g['diffaug_p']!r}]")
    if g['ada_target'] and not any(groups):
        raise ValueError(f"ada_target={g['ada_target']!r} adapts the probability of a diffaug policy, and none is named (diffaug='')")
    if g['ada_target'] and g['wgan'] and not g['pggan']:
        raise ValueError("ada_target > 0 is not available for the WGAN nets (wgan=True, pggan=False)")
    # the least-squares objective (an addition of this implementation: the reference ships its two losses and never calls them)
    if not isinstance(g['lsgan'], bool):
        raise ValueError(f"lsgan={g['lsgan']!r} must be True or False")
    if g['lsgan'] and g['wgan']:
        raise ValueError("lsgan=True is not available for the WGAN nets (wgan=True)")
    # the PG critic's minibatch standard-deviation channel (an addition of this implementation; Karras et al. 2018, section 3, use 4)
    if isinstance(g['mbstd_group'], bool) or not (isinstance(g['mbstd_group'], int) and g['mbstd_group'] >= 0):
        raise ValueError(f"mbstd_group={g['mbstd_group']!r} must be an integer >= 0 (0: off)")
    if g['mbstd_group'] and g['wgan']:
        raise ValueError("mbstd_group > 0 is not available for the WGAN nets (wgan=True)")
    # the penalty's form and lazy regularisation (additions of this implementation): 'gp' is the reference's two-sided penalty, 'lp' the
    # one-sided form, 'r1' the zero-centred one on the real images; the penalty runs every grad_pen_interval-th iteration with that many
    # times the weight
    if g['grad_pen_mode'] not in ('gp', 'lp', 'r1'):
        raise ValueError(f"grad_pen_mode={g['grad_pen_mode']!r} must be one of 'gp', 'lp', 'r1'")
    if isinstance(g['grad_pen_interval'], bool) or not (isinstance(g['grad_pen_interval'], int) and g['grad_pen_interval'] >= 1):
        raise ValueError(f"grad_pen_interval={g['grad_pen_interval']!r} must be an integer >= 1")
    if (g['grad_pen_mode'] != 'gp' or g['grad_pen_interval'] != 1) and g['wgan']:
        raise ValueError("grad_pen_mode / grad_pen_interval other than 'gp' / 1 are not available for the WGAN nets (wgan=True)")
    # spectral regularisation of the generator (an addition of this implementation; Durall et al. 2020): spec_loss_lambda 0 is off,
    # otherwise the weight of the term; spec_loss_floor the floor on the ratio of the spectra; the data's mean radial spectrum is taken
    # over spec_loss_images images per stage, drawn with spec_loss_seed
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and np.isfinite(v)      # noqa: E731
    if not (number(g['spec_loss_lambda']) and g['spec_loss_lambda'] >= 0):
        raise ValueError(f"spec_loss_lambda={g['spec_loss_lambda']!r} must be a finite number >= 0 (0: off)")
    if not (number(g['spec_loss_floor']) and g['spec_loss_floor'] > 0):
        raise ValueError(f"spec_loss_floor={g['spec_loss_floor']!r} must be a finite number > 0")
    if isinstance(g['spec_loss_images'], bool) or not (isinstance(g['spec_loss_images'], int) and g['spec_loss_images'] >= 1):
        raise ValueError(f"spec_loss_images={g['spec_loss_images']!r} must be an integer >= 1")
    if isinstance(g['spec_loss_seed'], bool) or not (isinstance(g['spec_loss_seed'], int) and g['spec_loss_seed'] >= 0):
        raise ValueError(f"spec_loss_seed={g['spec_loss_seed']!r} must be an integer >= 0")
    if g['spec_loss_lambda'] and g['wgan']:
        raise ValueError("spec_loss_lambda > 0 is not available for the WGAN nets (wgan=True)")
    # the similarity loss (sim_loss_lambda, the reference's switch): sim_loss_on 'real' is the reference's path -- the term is taken on
    # the real batch and only monitored; 'generated' takes it on the generator's images, where it trains the generator (an addition of
    # this implementation).  sim_loss_center: cosines of the images less their own means.  'generated' with sim_loss_lambda = 0 is
    # accepted and inert
    if g['sim_loss_on'] not in ('real', 'generated'):
        raise ValueError(f"sim_loss_on={g['sim_loss_on']!r} must be 'real' or 'generated'")
    if not isinstance(g['sim_loss_center'], bool):
        raise ValueError(f"sim_loss_center={g['sim_loss_center']!r} must be a bool")
    if g['sim_loss_on'] == 'generated' and g['wgan']:
        raise ValueError("sim_loss_on='generated' is not available for the WGAN nets (wgan=True)")
    if g['pggan']:
        err_msg = 'The number of layers in the generator and discriminator must match.'
        assert len(g['N_gen_features']) == len(g['N_dis_features']), err_msg
        N_upsamples = len(g['N_gen_features']) - 1
        assert g['image_size'] // (2 ** N_upsamples) >= 4, 'The initial image size must be >= 4. Reduce the number of layers'
        if g['transit_period'] is not None:
            g['transit_sch'] = [i * g['transit_period'] for i in range(1, N_upsamples + 1)]
        err_msg = 'The number of transitions ({}) does not match the number of convolution layers ({})'.format(
            len(g['transit_sch']), N_upsamples)
        assert N_upsamples == len(g['transit_sch']), err_msg
        assert g['N_epochs'] > g['transit_sch'][-1], 'The number of epochs must be greater than the last resolution transition'
        N_transition_epochs = np.ceil(1 / g['alpha_step'])
        err_msg = 'The transitions must be separated by at least {} epochs'.format(N_transition_epochs)
        assert np.all(np.diff(g['transit_sch']) > N_transition_epochs), err_msg


def set_configs(**overrides):
    """Programmatic overlay (what train.py does with CLI flags, train.py:101-104)."""
    for name, val in overrides.items():
        if name not in configs_name:
            raise ValueError(f"The overwritten config '{name}' is not defined.")
        globals()[name] = val
    define_ID_dependent_configs()


def import_configs(filename, overwritten_configs=None, create_dirs=False):
    overwritten_configs = dict(overwritten_configs or {})
    for name in overwritten_configs:
        if name not in configs_name:
            raise ValueError(f"The overwritten config '{name}' is not defined.")
    base, ext = os.path.splitext(filename)
    if ext == '':
        filename += '.py'
    elif ext != '.py':
        raise ValueError('Filename must be a .py file')
    path = filename if os.path.isabs(filename) else os.path.join(globals()['configs_dir'], filename)
    assert os.path.exists(path), f"The configuration file {filename} does not exist in {globals()['configs_dir']}"
    spec = importlib.util.spec_from_file_location('user.config', path)
    user = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(user)
    values = {}
    for name, val in vars(user).items():
        if isinstance(val, (ModuleType, FunctionType)) or name.startswith('__'):
            continue
        if name not in configs_name:
            raise ValueError(f"The imported config '{name}' is not defined.")
        values[name] = val
    values.update(overwritten_configs)
    globals().update(values)
    define_ID_dependent_configs()
    validate_configs(create_dirs=create_dirs)


define_ID_dependent_configs()
