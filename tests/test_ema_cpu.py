"""The averaged generator (ema_beta) without a GPU: host-side validation of the new entry points, the configuration name and flag,
the checkpoint key and its loaders, the eval tool's command line.  The arithmetic is tested on the GPU (test_gpu_ema.py)."""
import ctypes
import os

import pytest
import torch

EMA_KEY = "Generator_ema_state"


def test_new_entry_points_validate_on_the_host(ngan):
    """null pointers, a wrong n_hyper and K = 520 are refused with a negative status before any launch"""
    lib = ngan._C.lib()
    one = ctypes.c_void_p(16)            # any non-null address: every check below comes before the launch
    N = None
    # null pointers (the average and its weight among them)
    assert lib.ngan_adam_step_ema(N, N, N, N, N, N, N, N, 1, N, N, 1, N, 9, N, N, None) < 0
    assert b"null" in lib.ngan_last_error()
    assert lib.ngan_adam_step_ema(one, one, one, one, one, one, one, one, 1, one, one, 1, one, 9, None, one, None) < 0
    assert lib.ngan_adam_step_ema(one, one, one, one, one, one, one, one, 1, one, one, 1, one, 9, one, None, None) < 0
    assert lib.ngan_rmsprop_step_ema(one, one, one, one, one, one, one, 1, one, one, 1, one, 5, None, one, None) < 0
    assert lib.ngan_rmsprop_step_ema(one, one, one, one, one, one, one, 1, one, one, 1, one, 5, one, None, None) < 0
    assert lib.ngan_ema_step(one, None, one, one, one, one, one, 1, one, None) < 0
    assert lib.ngan_ema_step(one, one, one, one, one, one, one, 1, None, None) < 0
    assert b"null" in lib.ngan_last_error()
    assert lib.ngan_ema_step(one, one, one, one, one, one, one, 0, one, None) < 0
    for name in ("ngan_linear_wgrad_adam_ema", "ngan_bf16_linear_wgrad_adam_ema"):
        fn = getattr(lib, name)
        assert fn(one, one, one, one, one, one, one, 9, 16, 512, 256, 128, 1.0, None, one, None) < 0
        assert fn(one, one, one, one, one, one, one, 9, 16, 512, 256, 128, 1.0, one, None, None) < 0
        assert b"null" in lib.ngan_last_error()
        assert fn(one, one, one, one, one, one, one, 5, 16, 512, 256, 128, 1.0, one, one, None) == -1
        assert b"hyper holds 5 floats" in lib.ngan_last_error()
        assert fn(one, one, one, one, one, one, one, 9, 16, 520, 256, 128, 1.0, one, one, None) < 0
        assert b"K=520" in lib.ngan_last_error()
    for name in ("ngan_linear_wgrad_rmsprop_ema", "ngan_bf16_linear_wgrad_rmsprop_ema"):
        fn = getattr(lib, name)
        assert fn(one, one, one, one, one, 5, 16, 512, 256, 128, 1.0, None, one, None) < 0
        assert fn(one, one, one, one, one, 5, 16, 512, 256, 128, 1.0, one, None, None) < 0
        assert b"null" in lib.ngan_last_error()
        assert fn(one, one, one, one, one, 9, 16, 512, 256, 128, 1.0, one, one, None) == -1
        assert b"hyper holds 9 floats" in lib.ngan_last_error()
        assert fn(one, one, one, one, one, 5, 16, 520, 256, 128, 1.0, one, one, None) < 0
        assert b"K=520" in lib.ngan_last_error()
    # wrong hyper counts of the flat forms
    assert lib.ngan_adam_step_ema(one, one, one, one, one, one, one, one, 1, one, one, 1, one, 5, one, one, None) == -1
    assert b"hyper holds 5 floats" in lib.ngan_last_error()
    assert lib.ngan_rmsprop_step_ema(one, one, one, one, one, one, one, 1, one, one, 1, one, 9, one, one, None) == -1
    assert b"hyper holds 9 floats" in lib.ngan_last_error()


def test_ema_beta_is_a_configuration_name_and_a_flag(ngan):
    cfg, train = ngan.config, ngan.train
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    try:
        assert "ema_beta" in cfg.configs_name and cfg.configs_name["ema_beta"] == 0.0
        argv = ["--ema_beta", "0.999"]
        options = train.build_arg_parser().parse_args(argv)
        over = train.cli_overrides(argv, options, cfg.configs_name)
        assert over == {"ema_beta": 0.999}
        assert "ema_beta" not in train.cli_overrides([], train.build_arg_parser().parse_args([]), cfg.configs_name)
        cfg.set_configs(**over)
        cfg.validate_configs()
        assert cfg.ema_beta == 0.999
        for bad in (1.5, 1.0, -0.1):
            cfg.set_configs(ema_beta=bad)
            with pytest.raises(ValueError, match="ema_beta"):
                cfg.validate_configs()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)


def test_trainer_argument_is_validated(ngan):
    mk = lambda: (ngan.models.Generator_PG([16, 16], image_size_init=4, latent_dim=32),
                  ngan.models.Discriminator_PG([16, 16], image_size_init=4))
    for off in (0, 0.0, None):
        tr = ngan.train.PGGANTrainer(*mk(), ema_beta=off)
        assert not tr.ema_enabled and tr.flat_g.ema is None and tr.opt_g.ema_w is None
        with pytest.raises(RuntimeError):
            tr.ema_state()
    for bad in (1.0, 1.5, -0.5):
        with pytest.raises(ValueError, match="ema_beta"):
            ngan.train.PGGANTrainer(*mk(), ema_beta=bad)
    tr = ngan.train.PGGANTrainer(*mk(), ema_beta=0.999)
    assert tr.ema_enabled and tr.flat_d.ema is None and tr.opt_d.ema_w is None          # only the generator is averaged
    assert torch.equal(tr.flat_g.ema, tr.flat_g.flat) and tr.flat_g.ema.data_ptr() != tr.flat_g.flat.data_ptr()
    # w = fp32(1 - beta), rounded from the double
    assert float(tr.opt_g.ema_w) == float(torch.tensor(1.0 - 0.999, dtype=torch.float32))
    tr.set_ema_beta(0.5)
    assert float(tr.opt_g.ema_w) == 0.5
    with pytest.raises(ValueError):
        tr.set_ema_beta(1.0)
    assert any(t is tr.flat_g.ema for t in tr._training_state())
    assert set(tr.ema_state()) == set(tr.G.state_dict())


def nets(ngan, seed):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([16, 16, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 16, 16], image_size_init=4)
    G.set_resolution(8, 0.5)
    D.set_resolution(8, 0.5)
    return G, D


def test_checkpoint_key_round_trip(ngan, tmp_path, capsys):
    utils, train = ngan.utils, ngan.train
    G, D = nets(ngan, 1)
    tr = train.PGGANTrainer(G, D, ema_beta=0.9)
    tr.flat_g.ema.add_(0.25)                                  # an average that differs from the weights
    f = str(tmp_path / "GenDisc_e.pth")
    utils.Checkpointer(G, D, 1e-4, f, N_epochs=10, verbose=False, trainer=tr).save_state(3)
    saved = utils.load_checkpoint_dict(f)                     # the weights-only unpickler accepts the key
    assert list(saved[EMA_KEY].keys()) == list(saved["Generator_state"].keys())
    for k, v in saved[EMA_KEY].items():
        assert torch.is_tensor(v) and torch.equal(v, saved["Generator_state"][k] + 0.25), k
    # resume restores it
    G2, D2 = nets(ngan, 2)
    tr2 = train.PGGANTrainer(G2, D2, ema_beta=0.9)
    capsys.readouterr()
    ck2 = utils.Checkpointer(G2, D2, 1e-4, f, N_epochs=10, verbose=False, trainer=tr2)
    ck2.load_state()
    assert capsys.readouterr().out == ""
    assert torch.equal(tr2.flat_g.flat, tr.flat_g.flat)
    want = tr.ema_state()                                     # (per tensor: the alignment gaps of the flat buffer hold nothing)
    assert all(torch.equal(v, want[k]) for k, v in tr2.ema_state().items()) and set(want) == set(tr2.ema_state())
    # a trainer that does not average writes no key, and its file loads as ever; an averaging trainer then starts from the weights
    G3, D3 = nets(ngan, 3)
    plain = train.PGGANTrainer(G3, D3)
    f3 = str(tmp_path / "GenDisc_p.pth")
    utils.Checkpointer(G3, D3, 1e-4, f3, N_epochs=10, verbose=False, trainer=plain).save_state(2)
    assert EMA_KEY not in utils.load_checkpoint_dict(f3)
    tr2.flat_g.ema.add_(1.0)
    utils.Checkpointer(G2, D2, 1e-4, f3, N_epochs=10, verbose=False, trainer=tr2).load_state()
    out = capsys.readouterr().out
    assert EMA_KEY in out and "starts from the loaded weights" in out and len(out.strip().splitlines()) == 1
    assert torch.equal(tr2.flat_g.flat, plain.flat_g.flat)
    assert all(torch.equal(v, G2.state_dict()[k]) for k, v in tr2.ema_state().items())
    # the averaged file read by a trainer that does not average: the key is ignored
    G4, D4 = nets(ngan, 4)
    utils.Checkpointer(G4, D4, 1e-4, f, N_epochs=10, verbose=False, trainer=train.PGGANTrainer(G4, D4)).load_state()
    assert all(torch.equal(a, b) for a, b in zip(G4.state_dict().values(), G.state_dict().values()))
    # from_state_dict picks the other tensors
    Gw = ngan.models.Generator_PG.from_state_dict(f, verbose=False)
    Ge = ngan.models.Generator_PG.from_state_dict(f, verbose=False, use_ema=True)
    assert Ge.image_size == 8 and abs(Ge.alpha_value() - 0.5) < 1e-7
    for (k, a), b in zip(Gw.state_dict().items(), Ge.state_dict().values()):
        assert torch.equal(a, saved["Generator_state"][k]) and torch.equal(b, saved[EMA_KEY][k])
    with pytest.raises(KeyError, match=EMA_KEY):
        ngan.models.Generator_PG.from_state_dict(f3, verbose=False, use_ema=True)


def test_load_ema_state_keeps_weights_for_missing_tensors(ngan):
    G, D = nets(ngan, 5)
    tr = ngan.train.PGGANTrainer(G, D, ema_beta=0.9)
    state = tr.ema_state()
    name = "layers.0.weight"
    tr.flat_g.ema.zero_()
    tr.load_ema_state({name: state[name] + 1.0, "ToIm.weight": torch.zeros(3)})      # one tensor, one of a wrong shape
    got = tr.ema_state()
    for k, v in got.items():
        assert torch.equal(v, state[k] + 1.0 if k == name else state[k]), k


def test_eval_parser_has_the_reference_flags(ngan):
    p = ngan.eval.build_arg_parser()
    d = p.parse_args([])
    assert (d.n, d.output, d.weights, d.ema) == (16, "samples_default.png", "gen_dis_default.pth", False)
    o = p.parse_args(["-n", "4", "-output", "a.png", "-weights", "w.pth", "--ema"])
    assert (o.n, o.output, o.weights, o.ema) == (4, "a.png", "w.pth", True)
    with pytest.raises(FileExistsError):          # (checked before the GPU is asked for)
        ngan.eval.main(["-weights", os.path.join(os.sep, "nonexistent", "w.pth")])
