"""Synchronised BatchNorm for the data-parallel WGAN trainer, host side: the opt-in flag, the refusals that stay, and the C entry points'
argument checks (no GPU: every check runs before anything is launched)."""
import ctypes
import os

import pytest
import torch

import __graft_entry__ as graft

pkg = graft.load_package()
from neuron_gan_amd import models, ops, train, utils  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(pkg._C.LIB_PATH):
        graft.build()
    return pkg._C.lib()


def nets():
    torch.manual_seed(1)
    G = models.Generator_wgan([16, 8], latent_dim=8, image_size=16, N_colors=1)
    D = models.Discriminator_wgan([8, 16], image_size=16, N_colors=1)
    G.apply(utils.init_weights)
    D.apply(utils.init_weights)
    return G, D


def two_ranks(monkeypatch):
    monkeypatch.setattr(train.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(train.dist, "get_world_size", lambda group=None: 2)


def test_world_two_without_the_flag_still_refused(monkeypatch):
    two_ranks(monkeypatch)
    G, D = nets()
    with pytest.raises(NotImplementedError, match="one GPU"):
        train.WGANTrainer(G, D)
    with pytest.raises(NotImplementedError, match="sync_batchnorm"):
        train.WGANTrainer(G, D, sync_batchnorm=False)


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_world_two_with_the_flag_constructs_and_refuses_capture(monkeypatch, kind):
    two_ranks(monkeypatch)
    G, D = nets()
    tr = train.WGANTrainer(G, D, optimizer=kind, sync_batchnorm=True, device_latents=True)
    assert tr.world == 2 and tr.sync_batchnorm
    for opt in (tr.opt_d, tr.opt_g):
        assert opt.hyper_host[opt.GRAD_SCALE] == 0.5
    assert isinstance(tr.opt_d, (train.ClippedFusedAdam, train.ClippedFusedRMSprop))
    real = torch.zeros(2, 1, 16, 16)          # a CPU tensor: any CUDA work before the refusal would fail differently
    with pytest.raises(NotImplementedError, match="eager"):
        tr.capture(real)
    assert not tr.has_graph(real.shape)


def test_flag_without_a_process_group_raises():
    assert not (torch.distributed.is_available() and torch.distributed.is_initialized())
    G, D = nets()
    with pytest.raises(ValueError, match="process group"):
        train.WGANTrainer(G, D, sync_batchnorm=True)
    tr = train.WGANTrainer(G, D)              # the default keeps the one-GPU trainer
    assert tr.world == 1 and not tr.sync_batchnorm


def test_bf16_with_the_flag_still_refused(monkeypatch):
    two_ranks(monkeypatch)
    G, D = nets()
    prev = ops.get_conv_precision()
    try:
        ops.set_conv_precision("bf16")
        with pytest.raises(NotImplementedError, match="fp32"):
            train.WGANTrainer(G, D, sync_batchnorm=True)
    finally:
        ops.set_conv_precision(prev)


def test_sync_entry_points_validate_on_the_host(lib):
    one = ctypes.c_void_p(16)        # any non-null address: the checks come before any launch
    # null pointers
    assert lib.ngan_bn_moments(None, 64, 8, one, one, None) < 0
    assert b"null" in lib.ngan_last_error()
    assert lib.ngan_bn_merge_fold(None, 2, 8, one, one, one, one, one, one, None, None, None, 0.1, 1e-5, one, None) < 0
    assert b"null" in lib.ngan_last_error()
    assert lib.ngan_bn_merge_fold(one, 2, 8, one, one, one, one, one, one, None, None, None, 0.1, 1e-5, None, None) < 0
    assert b"null" in lib.ngan_last_error()
    assert lib.ngan_bn_act_bwd_partial(one, None, one, one, one, one, 1, 0.2, 64, 8, one, one, None) < 0
    assert b"null" in lib.ngan_last_error()
    assert lib.ngan_bn_act_bwd_merged(one, one, one, one, one, one, one, 1, 0.2, 64, 8, None, 2, 0, one, one, None, None, one, None) < 0
    assert b"null" in lib.ngan_last_error()
    # the moments' workspace holds doubles
    assert lib.ngan_bn_moments(one, 64, 8, one, ctypes.c_void_p(20), None) < 0
    assert b"8-byte aligned" in lib.ngan_last_error()
    # running mean without running variance
    assert lib.ngan_bn_merge_fold(one, 2, 8, one, one, one, one, one, one, one, None, None, 0.1, 1e-5, one, None) < 0
    assert b"go together" in lib.ngan_last_error()
    # world < 1
    assert lib.ngan_bn_merge_fold(one, 0, 8, one, one, one, one, one, one, None, None, None, 0.1, 1e-5, one, None) < 0
    assert b"world=0" in lib.ngan_last_error()
    assert lib.ngan_bn_act_bwd_merged(one, one, one, one, one, one, one, 1, 0.2, 64, 8, one, 0, 0, one, one, None, None, one, None) < 0
    assert b"world=0" in lib.ngan_last_error()
    # a rank outside the gathered records
    assert lib.ngan_bn_act_bwd_merged(one, one, one, one, one, one, one, 1, 0.2, 64, 8, one, 2, 2, one, one, None, None, one, None) < 0
    assert b"rank=2" in lib.ngan_last_error()
    # C <= 0, and an empty pixel range
    assert lib.ngan_bn_moments(one, 64, 0, one, one, None) < 0
    assert b"C=0" in lib.ngan_last_error()
    assert lib.ngan_bn_moments(one, 0, 8, one, one, None) < 0
    assert b"npix=0" in lib.ngan_last_error()
    assert lib.ngan_bn_merge_fold(one, 2, -1, one, one, one, one, one, one, None, None, None, 0.1, 1e-5, one, None) < 0
    assert b"C=-1" in lib.ngan_last_error()
    assert lib.ngan_bn_act_bwd_partial(one, one, one, one, one, one, 1, 0.2, 64, 0, one, one, None) < 0
    assert b"C=0" in lib.ngan_last_error()
    assert lib.ngan_bn_act_bwd_merged(one, one, one, one, one, one, one, 1, 0.2, 64, 0, one, 2, 0, one, one, None, None, one, None) < 0
    assert b"C=0" in lib.ngan_last_error()
