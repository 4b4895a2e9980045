"""Training utilities on the hot path: the latent sampler (reference utils.py:54-92)."""
import torch

from .metric_table import METRICS

Latent_vecs_memo = {}


def sample_latent_vec(size: tuple, seed=None, mode='randn', device=torch.device('cpu')):
    """Latents are drawn on the CPU generator and moved afterwards, exactly like the reference (utils.py:69-91):
    'randn' = normal draws clamped to [-5, 5] and projected on the unit sphere; 'rand' = uniform in [-1, 1).
    With a seed, the global RNG state is saved/restored around the draw and the result is memoised."""
    device = torch.device(device)
    key = None
    if seed is not None:
        key = (size, mode, seed)
        if key in Latent_vecs_memo:
            return Latent_vecs_memo[key].to(device)
        rng_state = torch.get_rng_state()
        torch.manual_seed(seed)
    if mode == 'rand':
        z = 2 * torch.rand(*size, device='cpu') - 1
    elif mode == 'randn':
        z = torch.randn(*size, device='cpu').clamp(-5, 5)
        z = z / z.norm(p=2, dim=1, keepdim=True)
    else:
        raise ValueError('{} is not supported'.format(mode))
    if seed is not None:
        torch.set_rng_state(rng_state)
        Latent_vecs_memo[key] = z
    if device.type != 'cpu':
        z = z.to(device)
    return z


def sample_latent_vec_device(size: tuple, device, generator=None):
    """Same distribution drawn directly on the GPU (graph-capturable): used by the benchmark / fast training loop,
    where reproducing the CPU RNG stream is not required."""
    from . import ops
    z = torch.randn(*size, device=device, generator=generator)
    return ops.latent_normalize_(z, 5.0)          # clamp(-5, 5) and the projection on the unit sphere in one launch


# ---------------------------------------------------------------------------------------------------------------------
# Checkpoints: same dictionary layout as the reference's Checkpointer (utils.py:142-223), so files written
# by either side load in the other.  One optional extra key, 'optimizer_state', carries the fused Adam's moments and
# per-tensor step counts (the reference does not save optimiser state at all).  A trainer that keeps an averaged generator
# (train.py, `ema_beta`) adds 'Generator_ema_state': the averaged weights under the keys of 'Generator_state', tensors only.  The
# A PGGANTrainer writes 'objective' ("wasserstein" or "lsgan", train.py `objective=`) beside it; a file without the key is Wasserstein.  It
# also writes 'grad_pen_mode', 'grad_pen_interval' and 'grad_pen_iteration' (PENALTY_KEYS; a file without them is 'gp' / 1 / 0), and
# 'spec_loss_lambda' and 'spec_loss_floor' (SPECTRAL_KEYS; a file without them is 0 / 1e-3; resuming under other values is logged), and
# 'sim_loss_on' and 'sim_loss_center' (SIMILARITY_KEYS; a file without them is 'real' / False; likewise logged).  A
# critic built with mbstd_group > 0 lists 'mbstd_group' in 'Discriminator_attrs' and holds 'layers.<k>.weight_std' in its state; a file
# without the attribute holds the reference's critic.  The
# reference's loaders read the keys they know and ignore the rest (utils.py:185-199 index five series keys and the two attribute
# dictionaries, models.py the state dictionaries).  A run that scores its checkpoints (train.py, `<prefix>_period`) adds one key per row
# of metric_table.METRICS that scored, 'SWD' .. 'BRANCH': a list with one entry {epoch, image_size, ...} per scored checkpoint, whose
# fields scoring.py lists per metric -- plain Python numbers, lists and dictionaries, which the weights-only unpickler accepts as it is.
# ---------------------------------------------------------------------------------------------------------------------
import os  # noqa: E402

import numpy as np  # noqa: E402


def get_saved_attrs(model):
    """{name: value} of the attributes a net lists in `saved_attrs` (reference utils.py:124-129)."""
    return {a: getattr(model, a) for a in getattr(model, 'saved_attrs', [])}


def set_saved_attrs(model, saved_attrs_dict):
    for name, value in saved_attrs_dict.items():
        if not hasattr(model, name):
            raise ValueError('{} is not an attribute of {}', name, model)
        if name == 'alpha' and hasattr(model, '_set_alpha'):
            model._set_alpha(float(value))      # keeps the host mirror of the fade-in coefficient in step
        else:
            setattr(model, name, value)
    return saved_attrs_dict


def _numpy_allow_list():
    """What a reference checkpoint needs beyond tensors and plain containers: numpy arrays of plain numeric dtypes (the four loss
    series, utils.py:160-169).  Array reconstruction from a raw buffer executes nothing from the file."""
    core = getattr(np, "_core", None) or np.core
    return [np.ndarray, np.dtype, core.multiarray._reconstruct] + \
           [type(np.dtype(t)) for t in (np.float64, np.float32, np.float16, np.int64, np.int32, np.int16, np.int8, np.uint8, np.bool_)]


def load_checkpoint_dict(filename, device=torch.device('cpu')):
    """torch.load with the weights-only unpickler: checkpoint files come from users and from the reference's download link
    (gen_dis_default.pth, setup.py:79), so nothing in them may execute.  The reference's own `torch.load` (utils.py:185,
    models.py:397) is the full unpickler; the only non-tensor payload its checkpoints hold are numpy loss series, which are
    allow-listed explicitly.  A file that needs anything else is refused with torch's error."""
    with torch.serialization.safe_globals(_numpy_allow_list()):
        return torch.load(filename, map_location=device, weights_only=True)


EMA_KEY = 'Generator_ema_state'
OBJECTIVE_KEY = 'objective'      # of the trainer that wrote the file; a file without it was trained with the Wasserstein objective
# of a PGGANTrainer's penalty (train.py `grad_pen_mode=`, `grad_pen_interval=`) and its count of iterations; the values of a file without
# the keys
PENALTY_KEYS = {'grad_pen_mode': 'gp', 'grad_pen_interval': 1, 'grad_pen_iteration': 0}
# of a PGGANTrainer's spectral regularisation of the generator (train.py `spec_loss_lambda=`, `spec_loss_floor=`); the values of a file
# without the keys.  Weights like grad_pen_lambda: a run may be resumed under other values, which is logged
SPECTRAL_KEYS = {'spec_loss_lambda': 0.0, 'spec_loss_floor': 1e-3}
# of a PGGANTrainer's similarity term (train.py `sim_loss_on=`, `sim_loss_center=`); the values of a file without the keys.  Resuming
# under other values is allowed and logged, as for the spectral keys
SIMILARITY_KEYS = {'sim_loss_on': 'real', 'sim_loss_center': False}
# of a PGGANTrainer's adaptive augmentation probability (train.py `ada_target=` ...): the settings, the host count of iterations, the
# device counters {pos, neg, n, updates} and {p, last_r}; a file without the keys was trained with it off.  Written only by a trainer
# with ada_target > 0.  Resuming under another target, interval or kimg is allowed and logged; p carries over, clamped to the new
# diffaug_p.  ADA_SERIES_KEY: (epoch, p, r_t) per monitored epoch
ADA_KEYS = ('ada_target', 'ada_interval', 'ada_kimg', 'ada_iteration', 'ada_counters', 'ada_p')
ADA_SERIES_KEY = 'ADA'
SWD_KEY, MSSSIM_KEY, SPECTRUM_KEY, MORPH_KEY, SKELETON_KEY, SHOLL_KEY, BRANCH_KEY = (m.key for m in METRICS)


class Checkpointer:
    def __init__(self, Generator_net, Discriminator_net, lr: float, filename: str, N_epochs=100, verbose=True,
                 device=torch.device('cpu'), extra_checkpoint_period=50e3, trainer=None):
        self.Generator_net = Generator_net
        self.Discriminator_net = Discriminator_net
        self.lr = lr
        self.filename = filename
        self.epoch = 0
        self.Loss_real = np.zeros(N_epochs)
        self.Loss_fake = np.zeros(N_epochs)
        self.Loss_G = np.zeros(N_epochs)
        self.Loss_D = np.zeros(N_epochs)
        self.verbose = verbose
        self.device = device
        self.extra_checkpoint_period = extra_checkpoint_period
        self.trainer = trainer      # optional PGGANTrainer: adds / restores 'optimizer_state' (and 'Generator_ema_state')
        for m in METRICS:           # self.SWD .. self.BRANCH: one entry per scored checkpoint (train.py, `<prefix>_period`), saved only
            setattr(self, m.key, [])    # when the list holds any
        self.ADA = []               # (epoch, p, r_t) per monitored epoch of a trainer with ada_target > 0 (train.pggan_train), saved likewise

    def save_state(self, epoch):
        self.epoch = epoch
        cpu = lambda sd: {k: v.detach().to('cpu').clone() for k, v in sd.items()}
        checkpoint_dict = {'epoch': self.epoch,
                           'Generator_state': cpu(self.Generator_net.state_dict()),
                           'Generator_attrs': {k: (v.detach().cpu() if torch.is_tensor(v) else v)
                                               for k, v in get_saved_attrs(self.Generator_net).items()},
                           'Discriminator_state': cpu(self.Discriminator_net.state_dict()),
                           'Discriminator_attrs': {k: (v.detach().cpu() if torch.is_tensor(v) else v)
                                                   for k, v in get_saved_attrs(self.Discriminator_net).items()},
                           'lr': self.lr,
                           'Loss_real': self.Loss_real[:epoch], 'Loss_fake': self.Loss_fake[:epoch],
                           'Loss_G': self.Loss_G[:epoch], 'Loss_D': self.Loss_D[:epoch]}
        if self.trainer is not None:
            checkpoint_dict['optimizer_state'] = self.trainer.optimizer_state()
            if getattr(self.trainer, 'ema_enabled', False):
                checkpoint_dict[EMA_KEY] = cpu(self.trainer.ema_state())
            if hasattr(self.trainer, 'objective'):
                checkpoint_dict[OBJECTIVE_KEY] = self.trainer.objective
            if hasattr(self.trainer, 'grad_pen_mode'):
                for key, default in PENALTY_KEYS.items():
                    checkpoint_dict[key] = type(default)(getattr(self.trainer, key))
            if hasattr(self.trainer, 'spec_loss_lambda'):
                for key in SPECTRAL_KEYS:
                    checkpoint_dict[key] = float(getattr(self.trainer, key))
            if hasattr(self.trainer, 'sim_loss_on'):
                for key, default in SIMILARITY_KEYS.items():
                    checkpoint_dict[key] = type(default)(getattr(self.trainer, key))
            if getattr(self.trainer, 'ada_enabled', False):
                checkpoint_dict.update(self.trainer.ada_state())
        if self.ADA:
            checkpoint_dict[ADA_SERIES_KEY] = [tuple(entry) for entry in self.ADA]
        for m in METRICS:
            if getattr(self, m.key):
                checkpoint_dict[m.key] = [dict(entry) for entry in getattr(self, m.key)]
        torch.save(checkpoint_dict, self.filename)
        if epoch % self.extra_checkpoint_period == 0:
            base, ext = os.path.splitext(self.filename)
            torch.save(checkpoint_dict, base + '_{:d}k'.format(int(epoch / 1000)) + ext)
        if self.verbose:
            print('Training state at epoch {} saved in {}.'.format(self.epoch, self.filename))

    def load_state(self, filename=None):
        """filename None: resume everything from self.filename; otherwise load only the networks from `filename`.
        (The reference reads the networks from self.filename in both cases, utils.py:213-215 -- a slip that this
        implementation does not reproduce.)"""
        source = self.filename if filename is None else filename
        checkpoint_dict = load_checkpoint_dict(source, self.device)
        if filename is None and hasattr(self.trainer, 'objective'):
            saved = checkpoint_dict.get(OBJECTIVE_KEY, 'wasserstein')
            if saved != self.trainer.objective:
                raise ValueError('{} was trained with the {} objective and cannot be resumed with the {} objective'.format(
                    source, saved, self.trainer.objective))
        if filename is None and hasattr(self.trainer, 'grad_pen_mode'):
            saved = tuple(checkpoint_dict.get(k, PENALTY_KEYS[k]) for k in ('grad_pen_mode', 'grad_pen_interval'))
            own = (self.trainer.grad_pen_mode, self.trainer.grad_pen_interval)
            if saved != own:
                raise ValueError('{} was trained with grad_pen_mode={}, grad_pen_interval={} and cannot be resumed with grad_pen_mode={}, '
                                 'grad_pen_interval={}'.format(source, saved[0], saved[1], own[0], own[1]))
        if filename is None and hasattr(self.trainer, 'spec_loss_lambda'):
            saved = tuple(float(checkpoint_dict.get(k, d)) for k, d in SPECTRAL_KEYS.items())
            own = (float(self.trainer.spec_loss_lambda), float(self.trainer.spec_loss_floor))
            if saved != own:
                print('{} was trained with spec_loss_lambda={:g}, spec_loss_floor={:g}; the run goes on with spec_loss_lambda={:g}, '
                      'spec_loss_floor={:g}'.format(source, saved[0], saved[1], own[0], own[1]))
        if filename is None and hasattr(self.trainer, 'sim_loss_on'):
            saved = tuple(type(d)(checkpoint_dict.get(k, d)) for k, d in SIMILARITY_KEYS.items())
            own = (self.trainer.sim_loss_on, bool(self.trainer.sim_loss_center))
            if saved != own:
                print('{} was trained with sim_loss_on={}, sim_loss_center={}; the run goes on with sim_loss_on={}, '
                      'sim_loss_center={}'.format(source, saved[0], saved[1], own[0], own[1]))
        # the critic's minibatch standard-deviation group (models.Discriminator_PG(mbstd_group=); a file without the key is 0, off) changes
        # the head's parameters and its equalised-LR constant: the file's weights mean something else under another value
        saved_group = int(checkpoint_dict.get('Discriminator_attrs', {}).get('mbstd_group', 0))
        own_group = int(getattr(self.Discriminator_net, 'mbstd_group', 0))
        if saved_group != own_group:
            raise ValueError('{} was trained with mbstd_group={} and cannot be loaded into a critic with mbstd_group={}'.format(
                source, saved_group, own_group))
        if filename is None:
            self.epoch = checkpoint_dict['epoch']
            self.Loss_real[:self.epoch] = checkpoint_dict['Loss_real']
            self.Loss_fake[:self.epoch] = checkpoint_dict['Loss_fake']
            self.Loss_G[:self.epoch] = checkpoint_dict['Loss_G']
            self.Loss_D[:self.epoch] = checkpoint_dict['Loss_D']
            for m in METRICS:           # a resumed run continues the lists
                setattr(self, m.key, [dict(entry) for entry in checkpoint_dict.get(m.key, [])])
            self.ADA = [tuple(entry) for entry in checkpoint_dict.get(ADA_SERIES_KEY, [])]
        if 'Generator_attrs' in checkpoint_dict and 'Discriminator_attrs' in checkpoint_dict:
            # (the WGAN nets list no saved_attrs: the reference fails there, utils.py:194-198; here they count as empty)
            gen_attrs = {k: v for k, v in checkpoint_dict['Generator_attrs'].items() if k in getattr(self.Generator_net, 'saved_attrs', [])}
            dis_attrs = {k: v for k, v in checkpoint_dict['Discriminator_attrs'].items()
                         if k in getattr(self.Discriminator_net, 'saved_attrs', [])}
            if hasattr(self.Generator_net, 'set_resolution'):
                res, alpha = gen_attrs['image_size'], float(gen_attrs['alpha'])
                if self.Generator_net.image_size != res:
                    self.Generator_net.set_resolution(res, alpha)
                    self.Discriminator_net.set_resolution(res, alpha)
            set_saved_attrs(self.Generator_net, gen_attrs)
            set_saved_attrs(self.Discriminator_net, dis_attrs)
        if hasattr(type(self.Generator_net), 'from_state_dict'):
            gen_state = type(self.Generator_net).from_state_dict(source, verbose=False).state_dict()
            dis_state = type(self.Discriminator_net).from_state_dict(source, verbose=False).state_dict()
        else:       # fixed-architecture nets (WGAN): the saved state dicts, BatchNorm buffers included
            gen_state, dis_state = checkpoint_dict['Generator_state'], checkpoint_dict['Discriminator_state']
        self.Generator_net.load_state_dict(gen_state, strict=False)
        self.Discriminator_net.load_state_dict(dis_state, strict=False)
        if self.trainer is not None:
            self.trainer.refresh_stage()
            if filename is None and 'optimizer_state' in checkpoint_dict:
                saved_kind = checkpoint_dict['optimizer_state'].get('kind', 'adam')     # (checkpoints without a kind are Adam's)
                if saved_kind == self.trainer.optimizer_kind:
                    self.trainer.load_optimizer_state(checkpoint_dict['optimizer_state'])
                else:
                    # the reference never restores an optimiser (utils.py:213-215): start this one fresh, as it would
                    self.trainer.reset_optimizer_state()
                    print('{} holds {} state; the {} optimiser starts fresh'.format(source, saved_kind, self.trainer.optimizer_kind))
            if filename is None and hasattr(self.trainer, 'grad_pen_mode'):
                # a resumed run continues the lazy-regularisation schedule where it stopped (a weights-only load restarts it)
                self.trainer.grad_pen_iteration = int(checkpoint_dict.get('grad_pen_iteration', PENALTY_KEYS['grad_pen_iteration']))
            if filename is None and getattr(self.trainer, 'ada_enabled', False):
                # a resumed run counts, draws and updates where it stopped; a file without the keys was trained with it off
                if 'ada_target' in checkpoint_dict:
                    saved = tuple(checkpoint_dict[k] for k in ADA_KEYS[:3])
                    own = tuple(self.trainer.ada_state()[k] for k in ADA_KEYS[:3])
                    if saved != own:
                        print('{} was trained with ada_target={:g}, ada_interval={}, ada_kimg={:g}; the run goes on with ada_target={:g}, '
                              'ada_interval={}, ada_kimg={:g}'.format(source, *saved, *own))
                    self.trainer.load_ada_state(checkpoint_dict)
                else:
                    print('{} holds no adaptive augmentation state; p starts from ada_p_init'.format(source))
            elif filename is None and 'ada_target' in checkpoint_dict:
                print('{} was trained with ada_target={:g}; the run goes on with a fixed augmentation probability'.format(
                    source, checkpoint_dict['ada_target']))
            if getattr(self.trainer, 'ema_enabled', False):
                self.trainer.load_ema_state(checkpoint_dict.get(EMA_KEY, {}))
                if EMA_KEY not in checkpoint_dict:
                    print('{} holds no {}; the averaged generator starts from the loaded weights'.format(source, EMA_KEY))
        if self.verbose:
            print(('Loaded training state from {}' if filename is None else 'Loaded weights from {}').format(source))


# ---------------------------------------------------------------------------------------------------------------------
# Sampling: reference utils.py:346-355 (gen_samples), 568-610 (plot_gen_samples)
# ---------------------------------------------------------------------------------------------------------------------
def gen_samples(Generator, N_images=16, seed=None):
    device = next(Generator.parameters()).device
    z_latent = sample_latent_vec((N_images, Generator.latent_dim), seed=seed, device=device)
    with torch.no_grad():
        images = Generator(z_latent).detach()
    return images, z_latent


def make_image_grid(images: torch.Tensor, nrow: int, normalize=True, padding=2) -> torch.Tensor:
    """(N, C, H, W) -> (C, H', W') grid, the subset of torchvision.utils.make_grid the reference uses (utils.py:21, 608)."""
    images = images.detach().float().cpu()
    if normalize:
        lo, hi = float(images.min()), float(images.max())
        images = (images - lo) / max(hi - lo, 1e-5)
    n, c, h, w = images.shape
    ncol = min(nrow, n)
    nrows = (n + ncol - 1) // ncol
    grid = torch.zeros(c, nrows * (h + padding) + padding, ncol * (w + padding) + padding)
    for i in range(n):
        r, col = divmod(i, ncol)
        grid[:, padding + r * (h + padding):padding + r * (h + padding) + h,
             padding + col * (w + padding):padding + col * (w + padding) + w] = images[i]
    return grid


def plot_gen_samples(Generator, eval_noise=None, N_images=16, seed=None, filename=None):
    """Generate a grid of samples: eval mode, seeded + memoised latents, low-resolution samples enlarged to the final size
    with nearest-neighbour interpolation (utils.py:598-601), written as a PNG when `filename` is given.  Returns the grid."""
    was_training = Generator.training
    Generator.train(False)
    if eval_noise is None:
        images, _ = gen_samples(Generator, N_images, seed=seed)
    else:
        with torch.no_grad():
            images = Generator(eval_noise).detach()
        N_images = images.size(0)
    Generator.train(was_training)
    images = images.cpu()
    size = getattr(Generator, 'image_size_max', images.size(-1))      # (fixed-size nets: the WGAN generator)
    if images.size(-1) != size:
        images = torch.nn.functional.interpolate(images, size=(size, size))
    grid = make_image_grid(images, nrow=int(np.round(np.sqrt(N_images))))
    if filename is not None:
        from PIL import Image
        arr = (grid.clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0).numpy()
        Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(filename)
    return grid


def Calculate_D_steps(Loss_real, Loss_fake, N_min, N_max, Period):
    """Number of critic steps for the next epoch (reference utils.py:105-120): the critic is trained less when the gap between
    the real and fake scores is large compared to the spread of the real score over the last `Period` epochs."""
    if Loss_real and Loss_fake:
        real_std = np.std(Loss_real[-Period:])
        diff = np.mean(np.abs(np.subtract(Loss_fake[-Period:], Loss_real[-Period:])))
        n_steps = np.round(real_std / diff * N_max)
        n_steps = np.min([n_steps, N_max])
        n_steps = np.max([n_steps, N_min])
        return int(n_steps)
    return N_max


def similarity_loss(images_batch, Z_batch, Lambda=1.0):
    """Reference loss_functions.py:185-205: squared difference between the pairwise cosine similarities of the latents and of the
    images.  The reference evaluates it on the REAL batch and the latents (train.py:380), so it carries no gradient to either net:
    it is a monitored number, computed here with a few tiny torch matmuls (B x B), off the hot path."""
    b = images_batch.size(0)
    im = images_batch.reshape(b, -1)
    z = Z_batch.reshape(b, -1)
    im = im / im.norm(2, dim=1, keepdim=True)
    z = z / z.norm(2, dim=1, keepdim=True)
    return Lambda * torch.pow(z @ z.t() - im @ im.t(), 2).sum() / (b * (b - 1))


def init_weights(m: torch.nn.Module):
    """The reference's init for the WGAN / DCGAN nets (utils.py:96-101), applied with `net.apply(init_weights)`: normal(0, 0.02)
    conv weights, normal(1, 0.02) BatchNorm weights, zero BatchNorm biases; exact type match, so Linear layers and conv biases keep
    torch's default init."""
    if type(m) in [torch.nn.Conv2d, torch.nn.ConvTranspose2d]:
        m.weight.data.normal_(0.0, 0.02)
    elif type(m) == torch.nn.BatchNorm2d:
        m.weight.data.normal_(1.0, 0.02)
        m.bias.data.fill_(0.0)
