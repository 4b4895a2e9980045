"""WGAN path, host side: construction and init against the reference's classes, the config / CLI mapping, checkpoints."""
import importlib.util
import os
import sys

import pytest
import torch

import __graft_entry__ as graft

pkg = graft.load_package()
from neuron_gan_amd import models, ops, train, utils  # noqa: E402

REF = "/root/reference"


def _ref_models():
    path = os.path.join(REF, "models.py")
    if not os.path.exists(path):
        pytest.skip("reference sources absent")
    sys.path.insert(0, REF)
    try:
        spec = importlib.util.spec_from_file_location("_ref_models_wgan", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    finally:
        sys.path.remove(REF)


def _ref_init(m):
    if type(m) in [torch.nn.Conv2d, torch.nn.ConvTranspose2d]:
        m.weight.data.normal_(0.0, 0.02)
    elif type(m) == torch.nn.BatchNorm2d:
        m.weight.data.normal_(1.0, 0.02)
        m.bias.data.fill_(0.0)


def build(mod, gw, dw, latent, size, colors, init):
    torch.manual_seed(1)
    G = mod.Generator_wgan(gw, latent_dim=latent, image_size=size, N_colors=colors)
    D = mod.Discriminator_wgan(dw, image_size=size, N_colors=colors)
    G.apply(init)
    D.apply(init)
    return G, D


def test_exports():
    assert "Generator_wgan" in models.__all__ and "Discriminator_wgan" in models.__all__
    assert callable(utils.init_weights)


@pytest.mark.parametrize("shape", [([32, 16, 8], [8, 16, 32], 16, 64, 1), ([128, 64, 32, 32, 16, 16], [16, 16, 32, 32, 64, 128], 512, 512, 1),
                                   ([16, 8], [8, 16], 32, 32, 3)])
def test_construction_and_init_match_reference(shape):
    ref = _ref_models()
    G, D = build(models, *shape, utils.init_weights)
    Gr, Dr = build(ref, *shape, _ref_init)
    for a, b in ((G, Gr), (D, Dr)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), k


def test_init_weights_reference_semantics():
    torch.manual_seed(0)
    G, D = build(models, [16, 8], [8, 16], 8, 16, 1, utils.init_weights)
    for m in list(G.modules()) + list(D.modules()):
        if type(m) == torch.nn.BatchNorm2d:
            assert torch.all(m.bias == 0)
            assert float((m.weight.detach() - 1).abs().max()) < 0.2
        if type(m) in (torch.nn.Conv2d, torch.nn.ConvTranspose2d):
            assert float(m.weight.std()) < 0.05


def _cfg(**kw):
    from types import SimpleNamespace
    base = dict(wgan=True, pggan=False, RMSprop=False, learning_rate=1e-4, beta1=0.5, drift_epsilon=0.001, n_critic=5,
                grad_pen_lambda=10, alpha_step=1e-4)
    base.update(kw)
    return SimpleNamespace(**base)


def test_make_trainer_dispatch():
    G, D = build(models, [16, 8], [8, 16], 8, 16, 1, utils.init_weights)
    tr = train.make_trainer(_cfg(RMSprop=True), G, D)
    assert isinstance(tr, train.WGANTrainer)
    assert isinstance(tr.opt_d, train.ClippedFusedRMSprop) and isinstance(tr.opt_g, train.FusedRMSprop)
    assert tr.opt_d.clip == 0.01 and tr.n_critic == 5
    G, D = build(models, [16, 8], [8, 16], 8, 16, 1, utils.init_weights)
    tr = train.make_trainer(_cfg(), G, D)
    assert isinstance(tr.opt_d, train.ClippedFusedAdam) and tr.optimizer_kind == "adam"
    with pytest.raises(ValueError, match="pggan"):
        train.make_trainer(_cfg(pggan=True), G, D)


def test_low_precision_and_world_refused(monkeypatch):
    G, D = build(models, [16, 8], [8, 16], 8, 16, 1, utils.init_weights)
    prev = ops.get_conv_precision()
    try:
        ops.set_conv_precision("bf16")
        with pytest.raises(NotImplementedError, match="fp32"):
            train.WGANTrainer(G, D)
    finally:
        ops.set_conv_precision(prev)
    monkeypatch.setattr(train.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(train.dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError, match="one GPU"):
        train.WGANTrainer(G, D)


def test_checkpoint_round_trip(tmp_path):
    G, D = build(models, [16, 8], [8, 16], 8, 16, 1, utils.init_weights)
    tr = train.WGANTrainer(G, D, optimizer="rmsprop")
    with torch.no_grad():
        for m in G.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.add_(0.5)
                m.num_batches_tracked.add_(3)
        for p, o in zip(tr.flat_d.params, tr.flat_d.offsets):
            tr.flat_d.square_avg[o:o + p.numel()].fill_(0.25)
    fn = str(tmp_path / "ck.pth")
    utils.Checkpointer(G, D, 1e-4, fn, N_epochs=4, trainer=tr).save_state(2)
    G2, D2 = build(models, [16, 8], [8, 16], 8, 16, 1, lambda m: None)
    tr2 = train.WGANTrainer(G2, D2, optimizer="rmsprop")
    ck = utils.Checkpointer(G2, D2, 1e-4, fn, N_epochs=4, trainer=tr2, verbose=False)
    ck.load_state()
    assert ck.epoch == 2
    for a, b in ((G, G2), (D, D2)):
        sa, sb = a.state_dict(), b.state_dict()
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(tr2.flat_d.square_avg, tr.flat_d.square_avg)
    assert tr2.flat_g.flat.data_ptr() == G2.layers[0].weight.data_ptr()    # still the flat buffer's views


# ---- fixtures (tools/make_golden_wgan.py) ---------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _tool():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_make_golden_wgan", os.path.join(root, "tools", "make_golden_wgan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_wgan_small_regenerates_bit_identically(tmp_path):
    if not os.path.exists(os.path.join(REF, "models.py")):
        pytest.skip("reference sources absent")
    tool = _tool()
    threads = torch.get_num_threads()
    try:
        tool.small(_ref_models(), out_dir=str(tmp_path))
    finally:
        torch.set_num_threads(threads)
    import numpy as np
    new, old = np.load(str(tmp_path / "wgan_small.npz")), np.load(os.path.join(GOLDEN, "wgan_small.npz"))
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert np.array_equal(new[k], old[k]), k


@pytest.mark.parametrize("name", ["wgan_small.npz", "wgan_full.npz"])
def test_fixtures_exist_and_are_small(name):
    path = os.path.join(GOLDEN, name)
    assert os.path.exists(path)
    assert os.path.getsize(path) < 1 << 20


def test_construction_and_init_match_wgan_small_fixture():
    import numpy as np
    fx = np.load(os.path.join(GOLDEN, "wgan_small.npz"))
    cfg = _tool().SMALL
    G, D = build(models, cfg["gw"], cfg["dw"], cfg["latent"], cfg["size"], cfg["colors"], utils.init_weights)
    for tag, net in (("init_G", G), ("init_D", D)):
        sd = net.state_dict()
        keys = [k[len(tag) + 1:] for k in fx.files if k.startswith(tag + ".")]
        assert sorted(keys) == sorted(sd)
        for k in keys:
            ref = fx[f"{tag}.{k}"]
            assert tuple(sd[k].shape) == ref.shape and np.array_equal(sd[k].numpy(), ref), k


def test_wgan_critic_steps_over_the_series():
    # one epoch: no spread yet -> the maximum; identical series: the ratio is undefined -> the maximum (the reference's
    # Calculate_D_steps would take int(NaN) there)
    assert train.wgan_critic_steps([1.0], [0.5], 5) == 5
    assert train.wgan_critic_steps([1.0, 1.0, 1.0], [1.0, 1.0, 1.0], 5) == 5
    # large gap against a small spread: the critic trains less (down to 1)
    assert train.wgan_critic_steps([1.0, 1.01, 0.99], [5.0, 5.0, 5.0], 5) == 1
    # spread comparable to the gap: in between, from the reference's formula
    assert train.wgan_critic_steps([0.0, 1.0, 0.0, 1.0], [0.5, 1.5, 0.5, 1.5], 5) == 5
    n = train.wgan_critic_steps([0.0, 1.0, 0.0, 1.0], [2.0, 3.0, 2.0, 3.0], 5)
    assert n == int(round(0.5 / 2.0 * 5))
