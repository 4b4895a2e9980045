"""The minibatch standard-deviation layer on the CPU: the closed forms the kernels implement against torch.autograd on the plain-torch
concat formulation in fp64, the field form against the convolution on the concatenated tensor, the group-size rule, the critic's
parameters under a seed, and the checkpoint's `mbstd_group` (tests/mbstd_cases.py holds the restatements)."""
import types

import numpy as np
import pytest
import torch

import mbstd_cases as M

CASES = [(4, 1, 4, 3, 4), (8, 1, 4, 2, 8), (6, 1, 4, 2, 4), (5, 1, 4, 1, 4), (8, 2, 4, 3, 4), (8, 1, 8, 2, 4)]


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), requires_grad=grad)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_closed_forms_equal_autograd_at_both_orders(case):
    _, seg, grp, _, _ = case
    for family in M.families_of(case):
        d = M.inputs(family, case)
        x, gs, h = t64(d["x"], True), t64(d["gs"], True), t64(d["h"])
        s = M.mbstd_torch(x, seg, grp)
        ref = M.mbstd_fwd_ref(d["x"], seg, grp)["s"][0]
        assert np.abs(s.detach().numpy() - ref).max() <= 1e-15 * np.abs(ref).max()
        (gx,) = torch.autograd.grad(s, x, gs, create_graph=True)
        want = M.mbstd_bwd_ref(d["gs"], d["x"], seg, grp)["gx"][0]
        assert np.abs(gx.detach().numpy() - want).max() <= 1e-13 * max(np.abs(want).max(), 1e-300), (family, "gx")
        dgs, dx = torch.autograd.grad((gx * h).sum(), (gs, x))
        want = M.mbstd_bwdbwd_ref(d["h"], d["gs"], d["x"], seg, grp)
        for got, key in ((dgs, "dgs"), (dx, "dx")):
            w = want[key][0]
            assert np.abs(got.numpy() - w).max() <= 1e-12 * max(np.abs(w).max(), 1e-300), (family, key)
        if M.group_size(case[0] // seg, grp) == 1:           # the statistic is the constant sqrt(eps) and its gradient is zero
            assert np.allclose(ref, 1e-4, rtol=1e-12) and not gx.detach().numpy().any()


@pytest.mark.parametrize("hh", [1, 2, 3, 4])
def test_field_form_equals_the_concat_conv(hh):
    b, ch = 3, 4
    d = M.draws(M.seed_of(5, hh), x=(b, ch, hh, hh), s=(b,), w=(ch, ch, 3, 3), w_std=(ch, 1, 3, 3), g=(b, hh, hh, ch))
    scale = 0.37
    x, s, w, w_std = t64(d["x"]), t64(d["s"], True), t64(d["w"]), t64(d["w_std"], True)
    whole = M.concat_conv_field(x, s, w, w_std, scale)                              # NCHW
    conv = torch.nn.functional.conv2d(scale * x, w, None, padding=1).permute(0, 2, 3, 1).detach().numpy()
    got = M.stdfield_add_ref(conv, d["s"], d["w_std"], scale)["out"][0]
    assert np.abs(got - whole.permute(0, 2, 3, 1).detach().numpy()).max() < 1e-14
    g = t64(d["g"])
    gs, gw = torch.autograd.grad((whole.permute(0, 2, 3, 1) * g).sum(), (s, w_std))
    assert np.abs(M.stdfield_ds_ref(d["g"], d["w_std"], scale)["gs"][0] - gs.numpy()).max() < 1e-14
    assert np.abs(M.stdfield_dw_ref(d["g"], d["s"], scale)["gw"][0] - gw.numpy()).max() < 1e-14


def test_group_size_rule(ngan):
    size = ngan.ops.mbstd_group_size
    assert [size(b, 4) for b in (4, 8, 6, 5, 1, 16, 2)] == [4, 4, 3, 1, 1, 4, 2]
    assert all(size(b, g) == M.group_size(b, g) for b in range(1, 33) for g in range(1, 10))
    for bad in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ValueError):
            size(*bad)


def test_the_concat_critic_reduces_to_the_oracle_when_the_extra_weights_vanish():
    """mbstd_discriminator_forward is the oracle's critic plus the extra channel: with weight_std = 0 and the head's weights rescaled to
    the oracle's constant it gives the oracle's scores"""
    O = M.O
    torch.manual_seed(0)
    from __graft_entry__ import load_package
    D = load_package().models.Discriminator_PG([8, 8], image_size_init=4, mbstd_group=4)
    D.set_resolution(8, 0.5)
    p = {k: v.detach().double() for k, v in D.state_dict().items()}
    spec = O.NetSpec(image_size_init=4, slope=0.2, alpha=0.5)
    x = torch.randn(4, 1, 8, 8, dtype=torch.float64)
    q = dict(p)
    q["layers.0.weight_std"] = torch.zeros_like(p["layers.0.weight_std"])
    q["layers.0.weight"] = p["layers.0.weight"] * (O.weight_scale(8 * 9, 0.2) / O.weight_scale(9 * 9, 0.2))
    plain = {k: v for k, v in p.items() if k != "layers.0.weight_std"}
    assert torch.allclose(M.mbstd_discriminator_forward(q, x, spec, 4), O.discriminator_forward(plain, x, spec), rtol=1e-12, atol=1e-14)
    assert not torch.allclose(M.mbstd_discriminator_forward(p, x, spec, 4), M.mbstd_discriminator_forward(q, x, spec, 4))


def test_critic_parameters_under_a_seed(ngan):
    Dn = ngan.models.Discriminator_PG
    widths = [8, 16]
    torch.manual_seed(11)
    default = Dn(widths, image_size_init=4)
    torch.manual_seed(11)
    off = Dn(widths, image_size_init=4, mbstd_group=0)
    torch.manual_seed(11)
    on = Dn(widths, image_size_init=4, mbstd_group=4)
    sd, so, sn = default.state_dict(), off.state_dict(), on.state_dict()
    assert list(so) == list(sd) and all(torch.equal(so[k], sd[k]) for k in sd)
    assert off.saved_attrs == default.saved_attrs and off.mbstd_group == 0 and "mbstd_group" not in off.saved_attrs
    assert [s[0] for s in ngan.models._plan(off.layers)] == [s[0] for s in ngan.models._plan(default.layers)]
    assert set(sn) == set(sd) | {"layers.0.weight_std"} and all(torch.equal(sn[k], sd[k]) for k in sd)
    w_std = sn["layers.0.weight_std"]
    assert tuple(w_std.shape) == (16, 1, 3, 3) and tuple(sn["layers.0.weight"].shape) == (16, 16, 3, 3)
    gain = np.sqrt(2.0 / (1.0 + 0.2 ** 2))
    assert on.layers[0].scale_value == pytest.approx(gain / np.sqrt(17 * 9), rel=1e-12)
    assert default.layers[0].scale_value == pytest.approx(gain / np.sqrt(16 * 9), rel=1e-12)
    assert float(on.layers[0].weight_scale) == pytest.approx(on.layers[0].scale_value, rel=1e-6)
    # drawn last, by the He rule of a (C, C + 1, 3, 3) weight: the next draw of the default critic's stream, scaled
    torch.manual_seed(11)
    Dn(widths, image_size_init=4)
    assert torch.equal(w_std, torch.empty(16, 1, 3, 3).normal_(0.0, gain / np.sqrt(17 * 9)))
    assert "mbstd_group" in on.saved_attrs and on.mbstd_group == 4
    assert [s[0] for s in ngan.models._plan(on.layers)][0] == "mbstd_head" and [s[0] for s in ngan.models._plan(off.layers)][0] == "conv_lrelu_pn"
    # the parameter is tagged for the fused optimiser and travels in the flat gradient buffer, through growth
    assert on.layers[0].weight_std._ngan_name == "layers.0.weight_std"
    on.set_resolution(8, 1.0)
    assert "layers.1.weight_std" in on.state_dict() and on.layers[1].weight_std._ngan_name == "layers.0.weight_std"
    flat = ngan.train.FlatParams(on)
    assert "layers.0.weight_std" in flat.names and on.layers[1].weight_std.grad is not None
    assert any(p is on.layers[1].weight_std for p in ngan.train.active_parameters(on))
    with pytest.raises(ValueError):
        Dn(widths, mbstd_group=-1)


def nets(ngan, group, seed=1):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([16, 8], image_size_init=4, latent_dim=16)
    D = ngan.models.Discriminator_PG([8, 16], image_size_init=4, mbstd_group=group)
    return G, D


def test_checkpoint_round_trips_the_group(ngan, tmp_path):
    utils, train = ngan.utils, ngan.train
    files = {}
    for group in (0, 4):
        G, D = nets(ngan, group)
        G.set_resolution(8, 1.0)
        D.set_resolution(8, 1.0)
        files[group] = str(tmp_path / f"GenDisc_{group}.pth")
        utils.Checkpointer(G, D, 1e-4, files[group], N_epochs=10, verbose=False, trainer=train.PGGANTrainer(G, D)).save_state(2)
        attrs = utils.load_checkpoint_dict(files[group])["Discriminator_attrs"]
        assert attrs.get("mbstd_group", 0) == group and ("mbstd_group" in attrs) == (group > 0)
        back = ngan.models.Discriminator_PG.from_state_dict(files[group], verbose=False)
        assert back.mbstd_group == group and list(back.state_dict()) == list(D.state_dict())
        assert all(torch.equal(back.state_dict()[k], v.cpu()) for k, v in D.state_dict().items())
        assert (back.layers[1].scale_value == D.layers[1].scale_value)
    for saved, group, ok in ((0, 0, True), (4, 4, True), (4, 0, False), (0, 4, False)):
        G, D = nets(ngan, group, seed=2)
        ck = utils.Checkpointer(G, D, 1e-4, files[saved], N_epochs=10, verbose=False, trainer=train.PGGANTrainer(G, D))
        if ok:
            ck.load_state()
            assert ck.epoch == 2 and D.image_size == 8
            want = utils.load_checkpoint_dict(files[saved])["Discriminator_state"]
            assert all(torch.equal(D.state_dict()[k], want[k]) for k in want) and set(want) == set(D.state_dict())
        else:
            with pytest.raises(ValueError, match="mbstd_group") as e:
                ck.load_state()
            assert "mbstd_group=0" in str(e.value) and "mbstd_group=4" in str(e.value) and ck.epoch == 0


def test_command_line_and_configuration(ngan, monkeypatch):
    train = ngan.train
    from neuron_gan_amd.configs import config as cfg
    assert cfg.configs_name["mbstd_group"] == 0
    argv = ["--pggan", "--mbstd_group", "4"]
    assert train.cli_overrides(argv, train.build_arg_parser().parse_args(argv), cfg.configs_name)["mbstd_group"] == 4
    assert "mbstd_group" not in train.cli_overrides([], train.build_arg_parser().parse_args([]), cfg.configs_name)
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    try:
        for bad in (-1, True, 2.0, "4"):
            with pytest.raises(ValueError, match="mbstd_group"):
                cfg.set_configs(mbstd_group=bad)
                cfg.validate_configs(create_dirs=False)
        with pytest.raises(ValueError, match="mbstd_group"):
            cfg.set_configs(mbstd_group=4, wgan=True, pggan=False)
            cfg.validate_configs(create_dirs=False)
    finally:
        cfg.set_configs(**saved)
    base = dict(wgan=True, pggan=False, RMSprop=False, learning_rate=1e-4, grad_pen_lambda=0.0, drift_epsilon=0.001, n_critic=1,
                alpha_step=0.05, beta1=0.5)
    with pytest.raises(ValueError, match="mbstd_group"):
        train.make_trainer(types.SimpleNamespace(**base, mbstd_group=4), None, None)
    # the bf16 storage mode is refused by name
    G, D = nets(ngan, 4)
    ngan.ops.set_conv_precision("bf16")
    try:
        with pytest.raises(NotImplementedError, match="bf16"):
            train.PGGANTrainer(G, D)
    finally:
        ngan.ops.set_conv_precision("f32")
