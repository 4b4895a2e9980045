"""CPU checks of the RMSprop optimiser (the reference's RMSprop switch, train.py:220-225): trainer construction and state layout on
CPU nets, the configuration -> trainer mapping of the command-line driver, and host-side argument validation of the two new C-ABI
entry points.  No kernel is launched here; the arithmetic is tested on the GPU (test_gpu_rmsprop.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope="session")
def built(ngan):
    if not os.path.exists(ngan._C.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ngan


def small_nets(ngan):
    torch.manual_seed(5)
    G = ngan.models.Generator_PG([32, 16, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 16, 32], image_size_init=4)
    return G, D


def test_rmsprop_trainer_builds_fused_rmsprop_without_a_first_moment(ngan):
    G, D = small_nets(ngan)
    lr = 3e-4
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=lr, optimizer="rmsprop")
    assert tr.optimizer_kind == "rmsprop"
    for opt, flat in ((tr.opt_g, tr.flat_g), (tr.opt_d, tr.flat_d)):
        assert type(opt) is ngan.train.FusedRMSprop and opt.flat is flat
        # {lr, alpha, eps, grad_scale, 1 - alpha}, 1 - alpha formed in double as torch's `value=1 - alpha`
        assert opt.hyper_host == [lr, 0.99, 1e-8, 1.0, 1.0 - 0.99]
        assert opt.hyper.tolist() == torch.tensor([lr, 0.99, 1e-8, 1.0, 1.0 - 0.99], dtype=torch.float32).tolist()
        assert opt.param_groups[0]["lr"] == lr
        assert flat.exp_avg is None and flat.exp_avg_sq is None                  # no Adam buffers are allocated
        assert flat.square_avg.shape == flat.flat.shape and float(flat.square_avg.abs().sum()) == 0.0
    st = tr.optimizer_state()
    assert st["kind"] == "rmsprop"
    for tag, net in (("G", G), ("D", D)):
        names = [n for n, _ in net.named_parameters()]
        assert st[tag]["names"] == names and st[tag]["lr"] == lr
        assert set(st[tag]["square_avg"]) == set(names) and "exp_avg" not in st[tag] and "exp_avg_sq" not in st[tag]
        for n, p in net.named_parameters():
            assert st[tag]["square_avg"][n].shape == p.shape
    opt = tr.opt_d
    opt.set_grad_scale(0.5)
    assert opt.hyper_host[3] == 0.5 and opt.hyper.tolist()[3] == 0.5
    opt.set_lr(1e-5)
    assert opt.hyper.tolist()[0] == np.float32(1e-5)
    # torch's defaults can be changed as in optim.RMSprop(alpha=, eps=)
    G, D = small_nets(ngan)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=lr, optimizer="rmsprop", rmsprop_alpha=0.9, rmsprop_eps=1e-6)
    assert tr.opt_g.hyper_host == [lr, 0.9, 1e-6, 1.0, 1.0 - 0.9]


def test_default_trainer_is_still_adam(ngan):
    G, D = small_nets(ngan)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=1e-4, beta1=0.3)
    assert tr.optimizer_kind == "adam" and type(tr.opt_g) is ngan.train.FusedAdam and type(tr.opt_d) is ngan.train.FusedAdam
    assert tr.opt_g.hyper_host[:5] == [1e-4, 0.3, 0.999, 1e-8, 1.0]
    assert tr.flat_g.exp_avg is not None and tr.flat_g.exp_avg_sq is not None and tr.flat_g.square_avg is None
    st = tr.optimizer_state()
    assert st["kind"] == "adam" and "square_avg" not in st["G"] and set(st["G"]["exp_avg"]) == set(st["G"]["names"])


def test_unknown_optimizer_is_refused(ngan):
    G, D = small_nets(ngan)
    with pytest.raises(ValueError, match="optimizer"):
        ngan.train.PGGANTrainer(G, D, optimizer="sgd")


def test_adam_state_does_not_load_into_a_rmsprop_trainer(ngan):
    G, D = small_nets(ngan)
    adam_state = ngan.train.PGGANTrainer(G, D).optimizer_state()
    legacy = {k: v for k, v in adam_state.items() if k != "kind"}           # checkpoints written before the kind existed
    G, D = small_nets(ngan)
    tr = ngan.train.PGGANTrainer(G, D, optimizer="rmsprop")
    for st in (adam_state, legacy):
        with pytest.raises(ValueError, match="adam"):
            tr.load_optimizer_state(st)
    # and the other way round
    G, D = small_nets(ngan)
    with pytest.raises(ValueError, match="rmsprop"):
        ngan.train.PGGANTrainer(G, D).load_optimizer_state(tr.optimizer_state())


def test_rmsprop_state_round_trips(ngan):
    G, D = small_nets(ngan)
    tr = ngan.train.PGGANTrainer(G, D, optimizer="rmsprop")
    torch.manual_seed(1)
    tr.flat_g.square_avg.copy_(torch.rand_like(tr.flat_g.square_avg))
    tr.flat_g.seg_step.copy_(torch.arange(len(tr.flat_g.params), dtype=torch.float32))
    tr.opt_g.set_lr(7e-5)
    st = tr.optimizer_state()
    G2, D2 = small_nets(ngan)
    tr2 = ngan.train.PGGANTrainer(G2, D2, optimizer="rmsprop")
    tr2.load_optimizer_state(st)
    for p, o in zip(tr.flat_g.params, tr.flat_g.offsets):
        assert torch.equal(tr.flat_g.square_avg[o:o + p.numel()], tr2.flat_g.square_avg[o:o + p.numel()])
    assert torch.equal(tr.flat_g.seg_step, tr2.flat_g.seg_step) and tr2.opt_g.param_groups[0]["lr"] == 7e-5
    tr2.reset_optimizer_state()
    assert float(tr2.flat_g.square_avg.abs().sum()) == 0.0 and float(tr2.flat_g.seg_step.sum()) == 0.0


@pytest.fixture
def config(ngan):
    cfg = ngan.config
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    yield cfg
    for k, v in saved.items():
        setattr(cfg, k, v)


def test_make_trainer_maps_the_rmsprop_switch(ngan, config):
    config.set_configs(RMSprop=True, learning_rate=2e-4, beta1=0.3)
    G, D = small_nets(ngan)
    tr = ngan.train.make_trainer(config, G, D)
    assert tr.optimizer_kind == "rmsprop" and type(tr.opt_g) is ngan.train.FusedRMSprop
    assert tr.opt_g.hyper_host == [2e-4, 0.99, 1e-8, 1.0, 1.0 - 0.99] and tr.opt_d.param_groups[0]["lr"] == 2e-4
    assert tr.device_latents
    config.set_configs(RMSprop=False)
    G, D = small_nets(ngan)
    tr = ngan.train.make_trainer(config, G, D)
    assert tr.optimizer_kind == "adam" and type(tr.opt_d) is ngan.train.FusedAdam
    assert tr.opt_d.hyper_host[:4] == [2e-4, 0.3, 0.999, 1e-8]


def test_command_line_and_config_file_reach_make_trainer(ngan, config, tmp_path):
    train = ngan.train
    argv = ["--RMSprop", "--learning_rate", "0.0003"]
    options = train.build_arg_parser().parse_args(argv)
    overrides = train.cli_overrides(argv, options, config.configs_name)
    assert overrides == {"RMSprop": True, "learning_rate": 3e-4}
    config.set_configs(**overrides)
    assert train.make_trainer(config, *small_nets(ngan)).optimizer_kind == "rmsprop"
    # a flag that is not on the command line does not override: its argparse default (False) must not switch RMSprop off
    options = train.build_arg_parser().parse_args([])
    assert "RMSprop" not in train.cli_overrides([], options, config.configs_name)
    user = tmp_path / "rms_config.py"
    user.write_text("ID = '0042'\nRMSprop = True\n")
    config.set_configs(RMSprop=False)
    config.import_configs(str(user), train.cli_overrides([], options, config.configs_name))
    assert config.RMSprop is True and train.make_trainer(config, *small_nets(ngan)).optimizer_kind == "rmsprop"


def test_rmsprop_entry_points_validate_on_the_host(built):
    lib = built._C.lib()
    one = ctypes.c_void_p(16)        # any non-null address: every check comes before a launch
    assert lib.ngan_rmsprop_step(None, None, None, None, None, None, None, 1, None, None, 1, None, 5, None) < 0
    assert b"null" in lib.ngan_last_error()
    assert lib.ngan_rmsprop_step(one, one, one, one, one, one, one, 1, one, one, 1, one, 9, None) < 0      # Adam's hyper layout
    assert b"hyper holds 9 floats" in lib.ngan_last_error()
    assert lib.ngan_rmsprop_step(one, one, one, one, one, one, one, 0, one, one, 1, one, 5, None) < 0
    assert b"n_seg=0" in lib.ngan_last_error()
    for name in ("ngan_linear_wgrad_rmsprop", "ngan_bf16_linear_wgrad_rmsprop"):
        fn = getattr(lib, name)
        assert fn(None, None, None, None, None, 5, 16, 512, 256, 128, 1.0, None) < 0
        assert b"null" in lib.ngan_last_error()
        assert fn(one, one, one, one, one, 9, 16, 512, 256, 128, 1.0, None) < 0
        assert b"hyper holds 9 floats" in lib.ngan_last_error()
        assert fn(one, one, one, one, one, 5, 16, 520, 256, 128, 1.0, None) < 0                      # K a multiple of 16, <= 512
        assert b"K=520" in lib.ngan_last_error()
        assert fn(one, one, one, one, one, 5, 16, 1024, 256, 128, 1.0, None) < 0
        assert fn(one, one, one, one, one, 5, 0, 512, 256, 128, 1.0, None) < 0
    assert built._C.SIGNATURES["ngan_bf16_linear_wgrad_rmsprop"] == built._C.SIGNATURES["ngan_linear_wgrad_rmsprop"]
