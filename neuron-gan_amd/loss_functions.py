"""WGAN / WGAN-GP and LSGAN losses with the reference's interface (loss_functions.py:7-74, 77-143, 148-180), running on the HIP ops.

    D_W_loss(G, D, drift_epsilon)(real)      -> (loss, score_real, score_fake)
    G_W_loss(G, D)(real)                     -> (loss, z)
    D_grad_pen_loss(G, D, Lambda)(real)      -> loss   (create_graph double-backward through the critic)
    D_LS_loss(G, D, real)                    -> (loss, score_real, score_fake)   least squares, Mao et al. 2017; functions, as in the
    G_LS_loss(G, D, real)                    -> (loss, score_fake)               reference, which ships them and never calls them
    G_spectral_loss(images, target, Lambda)  -> loss   spectral regularisation of a generator's images (Durall et al. 2020); an addition
    G_similarity_loss(images, z, Lambda)     -> loss   the reference's similarity_loss on GENERATED images, differentiable; an addition

Latents come from `utils.sample_latent_vec` unless a tensor is passed through the optional `z=` / `epsilon=`
keywords (how the parity tests inject the reference's draws).  Every loss takes an optional `augment=` hook (`DiffAugmentHook`, an
addition of this implementation: differentiable augmentation of everything the critic sees); None is the reference's path.  The
generator losses a trainer holds (G_W_loss, G_LS_module) also take a `spectral=` hook (`SpectralHook`: the spectral regularisation of
G_spectral_loss on the generator's raw images) and then return the term as a third value, and a `similarity=` hook (`SimilarityHook`:
G_similarity_loss on the same images and the step's latents), whose term is returned last.  NaN handling: the reference dumps locals and
raises `ValueError` (loss_functions.py:35-41, 70-72); here the check is optional (`check_nan`) because
`torch.isnan(...)` in an `if` is a host sync on the GPU -- the training loop checks once per epoch instead.
"""
import torch
import torch.nn as nn

from . import ops
from .utils import sample_latent_vec


def _latents(net, batch, device, z):
    if z is not None:
        return z
    return sample_latent_vec((batch, net.latent_dim), device=device)


# What a shifted-out or cut pixel holds.  DiffAugment writes 0; here that is fatal: the critic's biases start at zero and each of its
# blocks ends in PixelNorm with eps 1e-8, so a pixel whose whole neighbourhood is exactly 0 has an all-zero feature vector, where
# PixelNorm's derivative is rsqrt(eps) = 1e4 -- per block.  On a six-block critic a 64 x 64 zero patch takes the input-gradient norm
# from 1e-2 to 1e9 and the gradient penalty overflows (tests/test_diffaug_cpu.py pins both figures on the CPU oracle).  -1 is the
# images' black, what the reference's own RandomAffine fill becomes after Renormalize (data/NeuronDataset.py:112-126).
DIFFAUG_FILL = -1.0


class DiffAugmentHook:
    """The `augment=` hook of the three losses: differentiable augmentation (ops.DiffAugment) of every image the
    critic sees, each kind of image with a parameter table of its own (int32 (rows, 8), `ops.diffaug_table` / `ops.diffaug_params`):
        real   the real images                        fake   the W-loss's generated images
        tilde  the penalty's generated images         gen    the generator step's images (the only differentiated use)
    The critic-step images carry no gradient and are augmented without an autograd node; the penalty interpolates between images
    that are already augmented, so its double-backward graph is the un-augmented one.  colour=False: no table opens the colour
    group (b = 0, c = 1 everywhere), which saves the sum pass of every call.  fill: what shifted-out and cut pixels hold
    (`DIFFAUG_FILL`).  geo_real / geo_fake / geo_tilde / geo_gen: affine tables of the geometric groups (fp32 (rows, 8),
    `ops.diffgeo_table` / `ops.diffgeo_params`), one per kind of image likewise; where one is given the bilinear resampling
    (ops.DiffGeometry) runs first, and where the matching table of the older groups is None their launches are not issued."""

    def __init__(self, real=None, fake=None, tilde=None, gen=None, colour=True, fill=DIFFAUG_FILL, *, geo_real=None, geo_fake=None,
                 geo_tilde=None, geo_gen=None):
        self.real, self.fake, self.tilde, self.gen, self.colour, self.fill = real, fake, tilde, gen, bool(colour), float(fill)
        self.geo_real, self.geo_fake, self.geo_tilde, self.geo_gen = geo_real, geo_fake, geo_tilde, geo_gen

    def transform(self, x, table, geo, out=None):
        """T(x) without an autograd node: the resampling (where `geo` is given) first, then the colour / translation / cutout
        launches (where `table` is given); the last launch issued writes `out`"""
        if geo is not None:
            if table is None:
                return ops.diffgeo(x, geo, out=out, fill=self.fill)
            x = ops.diffgeo(x, geo, fill=self.fill)
        elif table is None:
            raise ValueError("DiffAugmentHook: this kind of image has neither a parameter table nor an affine table")
        return ops.diffaug(x, table, self.colour, out=out, fill=self.fill)

    def critic_batch(self, real, fake):
        """[T(real) | T(fake)], the W-loss's one critic batch: both halves are written straight into it"""
        b = real.size(0)
        out = torch.empty((b + fake.size(0),) + tuple(real.shape[1:]), device=real.device, dtype=real.dtype)
        self.transform(real, self.real, self.geo_real, out=out[:b])
        self.transform(fake, self.fake, self.geo_fake, out=out[b:])
        return out

    def penalty_pair(self, real, x_tilde):
        return self.transform(real, self.real, self.geo_real), self.transform(x_tilde, self.tilde, self.geo_tilde)

    def real_only(self, real):
        """T(real) alone: what the zero-centred penalty (D_grad_pen_loss, mode "r1") differentiates at -- the reals as the critic sees them"""
        return self.transform(real, self.real, self.geo_real)

    def generated(self, fake):
        if self.geo_gen is not None:
            fake = ops.DiffGeometry.apply(fake, self.geo_gen, self.fill)
        return fake if self.gen is None else ops.DiffAugment.apply(fake, self.gen, self.colour, self.fill)


def G_spectral_loss(images, target, Lambda=1.0, floor=1e-3, global_batch=None):
    """Spectral regularisation of a generator (Durall et al. 2020): Lambda / global_batch * sum_b l[b] with
    l[b] = mean_{k=1..R/2} ln((S[b][k] / target[k] + floor) / (1 + floor))^2, S the Hann-windowed radial power spectrum of image b
    (metrics.radial_spectrum, the same bits) and target the data's mean radial spectrum at this size (metrics.spectral_target), fp64
    (R/2 + 1,).  images: (B, 1, R, R) fp32 on the GPU, R a power of two in 16 .. 1024.  The loss is per sample, so an image's value
    does not depend on the rest of the batch; global_batch (default B) is the divisor of a batch shared between ranks.  An fp32 scalar,
    differentiable once in the images (ops.SpectralLoss: the adjoint transform on HIP)."""
    target = torch.as_tensor(target, dtype=torch.float64, device=images.device)
    b = images.shape[0] if global_batch is None else int(global_batch)
    return ops.SpectralLoss.apply(images, target, float(Lambda) / b, float(floor))[1]


class SpectralHook:
    """The `spectral=` hook of the generator losses: taps the generator's raw images -- before any DiffAugment transform: the data's
    spectrum is that of un-augmented samples -- and holds the term.  target: fp64 (R/2 + 1,) on the device; scale: Lambda / batch."""

    def __init__(self, target, scale, floor=1e-3):
        self.target, self.scale, self.floor = target, float(scale), float(floor)

    def tap(self, images):
        """(images passed through, the term): the gradient of what follows arrives at the pass-through and is added on the adjoint's
        store"""
        images, term, _ = ops.SpectralLoss.apply(images, self.target, self.scale, self.floor)
        return images, term


def G_similarity_loss(images, z, Lambda=1.0, center=False):
    """The reference's similarity_loss (loss_functions.py:183-205) on a generator's images, so that it trains the generator as its
    comment intends (the reference's loop hands it the real batch, train.py:379-381, where it reaches neither network):
    Lambda / (B (B - 1)) * sum_{i != j} (T_ij - S_ij)^2 with S the pairwise cosines of the flattened images and T those of the latents
    (include/nganx.h).  center: the cosines are those of the images less their own means -- on micrographs the
    raw ones sit at 0.9 because the black background dominates; the latents are never centred.  images: (B, ...) fp32 on the GPU,
    2 .. 64 rows of a multiple of 4 values; z: (B, latent_dim) fp32.  Lambda: a float, or an fp32 scalar on the device (read by the
    kernel at launch time: a captured graph follows it).  No epsilon: an image of zero (centred) norm gives NaN, as the reference's
    division does.  B = 1 has no pair and gives the zero scalar.  An fp32 scalar, differentiable once in the images
    (ops.SimilarityLoss); no gradient flows to z or Lambda."""
    lam = Lambda if isinstance(Lambda, torch.Tensor) else torch.full((), float(Lambda), device=images.device, dtype=torch.float32)
    return ops.SimilarityLoss.apply(images, z, lam, bool(center))[1]


class SimilarityHook:
    """The `similarity=` hook of the generator losses: taps the generator's raw images -- before the spectral tap and before any
    DiffAugment transform -- together with the latents they were generated from, and holds the term.  lam: the fp32 device scalar the
    head launch reads; center: G_similarity_loss's."""

    def __init__(self, lam, center=False):
        self.lam, self.center = lam, bool(center)

    def tap(self, images, z):
        """(images passed through, the term): the gradient of what follows arrives at the pass-through and is added on the mix
        launch's store"""
        images, term, _ = ops.SimilarityLoss.apply(images, z, self.lam, self.center)
        return images, term


def _hook_returns(head, spectral, similarity, spec_term, sim_term):
    """head, then the spectral term (with that hook), then the similarity term (with that hook)"""
    return head + (() if spectral is None else (spec_term,)) + (() if similarity is None else (sim_term,))


class D_W_loss(nn.Module):
    def __init__(self, generator_net, discriminator_net, drift_epsilon=0.0, check_nan=True):
        super().__init__()
        self.generator_net = generator_net
        self.discriminator_net = discriminator_net
        self.drift_epsilon = drift_epsilon
        self.check_nan = check_nan

    def forward(self, real_images, z=None, fake_images=None, augment=None, score_tap=None):
        """score_tap(scores, n_real): optional observer of the pass's per-sample scores [real | fake] before the head reduces them (the
        trainer's adaptive augmentation counts them); it carries no gradient and changes nothing"""
        batch_size, device = real_images.size(0), real_images.device
        if fake_images is None:
            z = _latents(self.generator_net, batch_size, device, z)
            with torch.no_grad():
                fake_images = self.generator_net(z)
        # D(real) and D(fake) share the weights and no op couples samples, so they run as ONE critic pass over the
        # concatenated batch (the reference makes two calls, loss_functions.py:21, 29; per-sample results are identical).  The one op
        # that does couple samples, the opt-in minibatch standard deviation, is told that the batch holds two calls (mbstd_segments)
        with ops.first_order_only(), ops.mbstd_segments(2):      # differentiated once (train.py:365): fused PixelNorm-backward epilogues apply
            both = torch.cat([real_images, fake_images], dim=0) if augment is None else augment.critic_batch(real_images, fake_images)
            scores = self.discriminator_net(both)
        if score_tap is not None:
            score_tap(scores, batch_size)
        # -mean(real) + mean(fake) + drift * mean(real^2) (loss_functions.py:22, 29, 33, 45) as one launch each way
        D_loss, score_real, score_fake = ops.WLossHead.apply(scores, batch_size, float(self.drift_epsilon) if self.drift_epsilon > 0 else 0.0)
        if self.check_nan:
            if torch.isnan(score_real):
                raise ValueError('Real loss is nan.')
            if torch.isnan(score_fake):
                raise ValueError('Fake loss is nan.')
        return D_loss, score_real, score_fake


class G_W_loss(nn.Module):
    def __init__(self, generator_net, discriminator_net, check_nan=True):
        super().__init__()
        self.generator_net = generator_net
        self.discriminator_net = discriminator_net
        self.check_nan = check_nan

    def forward(self, real_images_batch, z=None, augment=None, spectral=None, similarity=None):
        """spectral (a SpectralHook): the return value gains the spectral term, (loss, z, term); None is the reference's path.
        similarity (a SimilarityHook): the return value gains that term, last; it taps the raw images first."""
        batch_size, device = real_images_batch.size(0), real_images_batch.device
        z_latent = _latents(self.generator_net, batch_size, device, z)
        fake_images = self.generator_net(z_latent)
        term = sim_term = None
        if similarity is not None:
            fake_images, sim_term = similarity.tap(fake_images, z_latent)
        if spectral is not None:
            fake_images, term = spectral.tap(fake_images)
        if augment is not None:
            fake_images = augment.generated(fake_images)      # D(T(G(z))): the generator is trained through the transform
        with ops.first_order_only():      # differentiated once (train.py:384)
            G_loss = ops.WLossHead.apply(self.discriminator_net(fake_images), batch_size, 0.0)[0]       # -mean(D(G(z)))
        if self.check_nan and torch.isnan(G_loss):
            raise ValueError('Generator loss is nan.')
        return _hook_returns((G_loss, z_latent), spectral, similarity, term, sim_term)


# The reference's coding of the least-squares targets (loss_functions.py:99, 133): the critic pulls real scores to 1 and generated ones to
# 0, the generator pulls its scores to 1.  The kernels take the targets as arguments; the public functions expose this coding only.
LS_TARGET_REAL, LS_TARGET_FAKE, LS_TARGET_GEN = 1.0, 0.0, 1.0


def D_LS_loss(generator_net, discriminator_net, real_images_batch, Lambda=None, *, z=None, fake_images=None, augment=None, check_nan=True):
    """mean((D(x) - 1)^2) + mean(D(G(z))^2) (loss_functions.py:79-112) -> (D_loss, Score_real_avg, Score_fake_avg).  `Lambda` is the
    reference's unused argument.  One critic pass over [real | fake], differentiated once, and one launch for the scalar chain each way,
    as D_W_loss.forward; the drift term does not enter, as in the reference's function.  z= / fake_images= / augment= / check_nan=:
    the keyword extras of the W losses (module docstring)."""
    return _d_ls_loss(generator_net, discriminator_net, real_images_batch, z, fake_images, augment, check_nan, None)


def _d_ls_loss(generator_net, discriminator_net, real_images_batch, z, fake_images, augment, check_nan, score_tap):
    """D_LS_loss's body; score_tap as D_W_loss.forward's (D_LS_module passes it on)"""
    batch_size, device = real_images_batch.size(0), real_images_batch.device
    if fake_images is None:
        z = _latents(generator_net, batch_size, device, z)
        with torch.no_grad():
            fake_images = generator_net(z)
    with ops.first_order_only(), ops.mbstd_segments(2):
        both = torch.cat([real_images_batch, fake_images], dim=0) if augment is None else augment.critic_batch(real_images_batch, fake_images)
        scores = discriminator_net(both)
    if score_tap is not None:
        score_tap(scores, batch_size)
    D_loss, Score_real_avg, Score_fake_avg = ops.LSLossHead.apply(scores, batch_size, LS_TARGET_REAL, LS_TARGET_FAKE)
    if check_nan:
        if torch.isnan(Score_real_avg):
            raise ValueError('Real loss is nan.')
        if torch.isnan(Score_fake_avg):
            raise ValueError('Fake loss is nan.')
        if torch.isnan(D_loss):
            raise ValueError('D loss is nan.')
    return D_loss, Score_real_avg, Score_fake_avg


def G_LS_loss(generator_net, discriminator_net, real_images_batch, Lambda=None, *, z=None, augment=None, check_nan=True):
    """mean((D(G(z)) - 1)^2) (loss_functions.py:117-143) -> (G_loss, Score_fake_avg).  One deliberate departure: the reference detaches
    the generated images (loss_functions.py:125), so its generator would receive no gradient at all and could not be trained with
    this loss; here the value is the same and the gradient flows into the generator (through `augment`'s transform when given).
    (The signature is the reference's plus the W losses' keyword extras; the `spectral=` hook is G_LS_module's.)"""
    return _g_ls_loss(generator_net, discriminator_net, real_images_batch, z, augment, check_nan, None)[:2]


def _g_ls_loss(generator_net, discriminator_net, real_images_batch, z, augment, check_nan, spectral, similarity=None):
    """G_LS_loss's body; spectral (a SpectralHook): the return value gains the spectral term, (G_loss, Score_fake_avg, term);
    similarity (a SimilarityHook): it gains that term, last"""
    batch_size, device = real_images_batch.size(0), real_images_batch.device
    z = _latents(generator_net, batch_size, device, z)
    fake_images = generator_net(z)
    term = sim_term = None
    if similarity is not None:
        fake_images, sim_term = similarity.tap(fake_images, z)
    if spectral is not None:
        fake_images, term = spectral.tap(fake_images)
    if augment is not None:
        fake_images = augment.generated(fake_images)
    with ops.first_order_only():
        G_loss, Score_fake_avg, _ = ops.LSLossHead.apply(discriminator_net(fake_images), batch_size, LS_TARGET_GEN, LS_TARGET_FAKE)
    if check_nan:
        if torch.isnan(Score_fake_avg):
            raise ValueError('Fake loss is nan.')
        if torch.isnan(G_loss):
            raise ValueError('D loss is nan.')
    return _hook_returns((G_loss, Score_fake_avg), spectral, similarity, term, sim_term)


class D_LS_module(nn.Module):
    """D_LS_loss with D_W_loss's call shape: what a trainer with objective="lsgan" holds as `d_loss`"""

    def __init__(self, generator_net, discriminator_net, check_nan=True):
        super().__init__()
        self.generator_net, self.discriminator_net, self.check_nan = generator_net, discriminator_net, check_nan

    def forward(self, real_images, z=None, fake_images=None, augment=None, score_tap=None):
        return _d_ls_loss(self.generator_net, self.discriminator_net, real_images, z, fake_images, augment, self.check_nan, score_tap)


class G_LS_module(nn.Module):
    """G_LS_loss with G_W_loss's call shape and return value, (loss, z): what a trainer with objective="lsgan" holds as `g_loss`"""

    def __init__(self, generator_net, discriminator_net, check_nan=True):
        super().__init__()
        self.generator_net, self.discriminator_net, self.check_nan = generator_net, discriminator_net, check_nan

    def forward(self, real_images_batch, z=None, augment=None, spectral=None, similarity=None):
        """spectral (a SpectralHook): the return value gains the spectral term, (loss, z, term); similarity (a SimilarityHook): it
        gains that term, last"""
        z_latent = _latents(self.generator_net, real_images_batch.size(0), real_images_batch.device, z)
        out = _g_ls_loss(self.generator_net, self.discriminator_net, real_images_batch, z_latent, augment, self.check_nan, spectral,
                         similarity)
        return (out[0], z_latent) + tuple(out[2:])


PENALTY_MODES = ("gp", "lp", "r1")      # D_grad_pen_loss(mode=)


class D_grad_pen_loss(nn.Module):
    """mode "gp": the reference's two-sided penalty Lambda * mean((||grad D(x_hat)|| - 1)^2) on interpolates (loss_functions.py:148-180).
    "lp": the one-sided form on the same interpolates, Lambda * mean(max(0, ||grad D(x_hat)|| - 1)^2) (WGAN-LP, Petzka et al. 2018).
    "r1": (Lambda / 2) * mean(||grad D(x)||^2) at the real images alone (Mescheder et al. 2018) -- no latent, no generator pass, no
    epsilon and no interpolate: `z`, `x_tilde` and `epsilon` are accepted and ignored; with an `augment` hook the gradient is taken at
    the augmented reals, the ones the critic's loss sees (`real_only`)."""

    def __init__(self, generator_net, discriminator_net, Lambda, mode="gp"):
        super().__init__()
        if mode not in PENALTY_MODES:
            raise ValueError(f"mode must be one of {list(PENALTY_MODES)}, got {mode!r}")
        self.generator_net = generator_net
        self.discriminator_net = discriminator_net
        self.Lambda = Lambda
        self.mode = mode
        self.last_grad_norms = None  # per-sample |grad D| of the last call (monitoring / parity tests)
        self._ones_cache = None

    def _ones(self, like):
        if self._ones_cache is None or self._ones_cache.shape != like.shape or self._ones_cache.device != like.device:
            self._ones_cache = torch.ones_like(like)
        return self._ones_cache

    def forward(self, real_images, z=None, epsilon=None, x_tilde=None, augment=None):
        if not self.Lambda > 0:
            # the reference returns the integer CPU scalar torch.tensor(0) here (loss_functions.py:179), which only survives being
            # stacked / accumulated with device tensors by accident; same value, on the images' device
            return torch.zeros((), device=real_images.device)
        if self.mode == "r1":
            return self._forward_r1(real_images, augment)
        batch_size, device = real_images.size(0), real_images.device
        if x_tilde is None:
            z_latent = _latents(self.generator_net, batch_size, device, z)
            with torch.no_grad():
                x_tilde = self.generator_net(z_latent)
        if epsilon is None:
            epsilon = torch.rand((batch_size, 1, 1, 1), device=device)
        if augment is not None:
            real_images, x_tilde = augment.penalty_pair(real_images, x_tilde)
        x_hat = ops.xhat(real_images, x_tilde, epsilon)
        x_hat.requires_grad_()
        output = self.discriminator_net(x_hat)
        # d(sum of the scores)/d(x_hat) (loss_functions.py:175): grad_outputs = ones instead of a sum node
        # (inputs_only: x_hat is the only input asked for, so the critic's weight gradients of this pass would be thrown away)
        with ops.inputs_only():
            Disc_grad = torch.autograd.grad(outputs=output, inputs=x_hat, grad_outputs=self._ones(output), create_graph=True)[0]
        if self.mode == "lp":
            penalty, norms = ops.PenaltyHead.apply(Disc_grad, float(self.Lambda), ops.PENALTY_ONE_SIDED)
        else:
            penalty, norms = ops.GradPenaltyHead.apply(Disc_grad, float(self.Lambda))
        self.last_grad_norms = norms.detach()
        return penalty

    def _forward_r1(self, real_images, augment):
        # a critic pass of its own over the reals (the critic's loss shares no graph node with it: the trainer runs the two backwards one
        # after the other).  Without a hook a detached alias is the leaf, so the caller's tensor keeps its requires_grad as it was; the
        # hook's output is a fresh tensor (a view of the step's buffer in the trainer's hook: the alias keeps the buffer untouched)
        x = real_images if augment is None else augment.real_only(real_images)
        x = x.detach().requires_grad_()
        output = self.discriminator_net(x)
        with ops.inputs_only():
            Disc_grad = torch.autograd.grad(outputs=output, inputs=x, grad_outputs=self._ones(output), create_graph=True)[0]
        penalty, norms = ops.PenaltyHead.apply(Disc_grad, float(self.Lambda), ops.PENALTY_ZERO_CENTRED)
        self.last_grad_norms = norms.detach()
        return penalty
