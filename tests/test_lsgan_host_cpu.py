"""The least-squares objective, host side: the flag and the configuration name, the refusals, what make_trainer forwards, the loss
objects a trainer holds under either objective, the checkpoint key, and the host-side argument checks of the two entry points.  No
kernel is launched here; the arithmetic is tested on the GPU (tests/test_gpu_lsgan.py)."""
import ctypes
import os
import re
import types

import pytest
import torch


def test_flag_and_configuration_name(ngan):
    cfg, train = ngan.config, ngan.train
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    try:
        assert cfg.configs_name["lsgan"] is False
        options = train.build_arg_parser().parse_args(["--lsgan"])
        assert options.lsgan is True and train.build_arg_parser().parse_args([]).lsgan is False
        assert train.cli_overrides(["--lsgan"], options, cfg.configs_name) == {"lsgan": True}
        assert "lsgan" not in train.cli_overrides([], train.build_arg_parser().parse_args([]), cfg.configs_name)
        cfg.set_configs(lsgan=True)
        cfg.validate_configs()
        assert cfg.lsgan is True
        for bad in (1, 0, "yes", None, 1.0):
            cfg.set_configs(lsgan=bad)
            with pytest.raises(ValueError, match="lsgan"):
                cfg.validate_configs()
        # the WGAN nets: refused by the configuration and by make_trainer
        cfg.set_configs(lsgan=True, wgan=True, pggan=False)
        with pytest.raises(ValueError, match="lsgan"):
            cfg.validate_configs()
        with pytest.raises(ValueError, match="lsgan"):
            train.make_trainer(cfg, None, None)
        cfg.set_configs(lsgan=False)
        cfg.validate_configs()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)


def test_make_trainer_forwards_the_objective(ngan, monkeypatch):
    train = ngan.train
    seen = []
    monkeypatch.setattr(train, "PGGANTrainer", lambda G, D, **kw: seen.append(kw) or "pg")
    base = dict(wgan=False, pggan=True, RMSprop=False, learning_rate=1e-4, grad_pen_lambda=0.0, drift_epsilon=0.001, n_critic=1,
                alpha_step=0.05, beta1=0.5)
    assert train.make_trainer(types.SimpleNamespace(**base, lsgan=True), None, None) == "pg"
    assert train.make_trainer(types.SimpleNamespace(**base, lsgan=False), None, None) == "pg"
    assert train.make_trainer(types.SimpleNamespace(**base), None, None) == "pg"              # a configuration from before the name
    assert train.make_trainer(types.SimpleNamespace(**{**base, "RMSprop": True}, lsgan=True), None, None) == "pg"
    assert [kw.get("objective") for kw in seen] == ["lsgan", None, None, "lsgan"]            # the default is left to the trainer
    assert [kw["optimizer"] for kw in seen] == ["adam", "adam", "adam", "rmsprop"] and all(kw["grad_pen_lambda"] == 0.0 for kw in seen)


def nets(ngan, seed=1):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([16, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 16], image_size_init=4)
    return G, D


def test_trainer_holds_the_objective_as_its_loss_objects(ngan):
    train, LF = ngan.train, ngan.loss_functions
    assert train.OBJECTIVES == ("wasserstein", "lsgan")
    for kw in ({}, {"objective": "wasserstein"}):
        tr = train.PGGANTrainer(*nets(ngan), **kw)
        assert tr.objective == "wasserstein" and type(tr.d_loss) is LF.D_W_loss and type(tr.g_loss) is LF.G_W_loss
        assert tr.d_loss.drift_epsilon == 0.001
    tr = train.PGGANTrainer(*nets(ngan), objective="lsgan", grad_pen_lambda=0.0)
    assert tr.objective == "lsgan" and type(tr.d_loss) is LF.D_LS_module and type(tr.g_loss) is LF.G_LS_module
    assert type(tr.gp_loss) is LF.D_grad_pen_loss and tr.gp_loss.Lambda == 0.0                # the penalty object stays
    assert not hasattr(tr.d_loss, "drift_epsilon") and not tr.d_loss.check_nan and not tr.g_loss.check_nan
    for bad in ("ls", "hinge", "", None, "LSGAN"):
        with pytest.raises(ValueError, match="wasserstein.*lsgan"):
            train.PGGANTrainer(*nets(ngan), objective=bad)
    assert (LF.LS_TARGET_REAL, LF.LS_TARGET_FAKE, LF.LS_TARGET_GEN) == (1.0, 0.0, 1.0)        # the reference's coding
    # the reference's positional signatures, the W losses' extras keyword-only
    import inspect
    for fn, extras in ((LF.D_LS_loss, ["z", "fake_images", "augment", "check_nan"]), (LF.G_LS_loss, ["z", "augment", "check_nan"])):
        ps = inspect.signature(fn).parameters
        assert list(ps)[:4] == ["generator_net", "discriminator_net", "real_images_batch", "Lambda"] and ps["Lambda"].default is None
        assert [n for n, p in ps.items() if p.kind is p.KEYWORD_ONLY] == extras
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # a host tensor never falls back to eager PyTorch
        ngan.ops.LSLossHead.apply(torch.zeros(4), 2, 1.0, 0.0)


def test_checkpoint_carries_the_objective(ngan, tmp_path):
    utils, train = ngan.utils, ngan.train
    assert utils.OBJECTIVE_KEY == "objective"
    files = {}
    for objective in train.OBJECTIVES:
        G, D = nets(ngan)
        tr = train.PGGANTrainer(G, D, objective=objective)
        files[objective] = str(tmp_path / f"GenDisc_{objective}.pth")
        utils.Checkpointer(G, D, 1e-4, files[objective], N_epochs=10, verbose=False, trainer=tr).save_state(2)
        assert utils.load_checkpoint_dict(files[objective])[utils.OBJECTIVE_KEY] == objective    # the weights-only unpickler takes it
    # a file from before the key (or from the reference) is Wasserstein
    d = utils.load_checkpoint_dict(files["wasserstein"])
    del d[utils.OBJECTIVE_KEY]
    files["old"] = str(tmp_path / "GenDisc_old.pth")
    torch.save(d, files["old"])
    for saved, objective, ok in (("wasserstein", "wasserstein", True), ("lsgan", "lsgan", True), ("old", "wasserstein", True),
                                 ("lsgan", "wasserstein", False), ("wasserstein", "lsgan", False), ("old", "lsgan", False)):
        G, D = nets(ngan, 2)
        ck = utils.Checkpointer(G, D, 1e-4, files[saved], N_epochs=10, verbose=False, trainer=train.PGGANTrainer(G, D, objective=objective))
        if ok:
            ck.load_state()
            assert ck.epoch == 2
        else:
            with pytest.raises(ValueError, match="wasserstein.*lsgan|lsgan.*wasserstein") as e:
                ck.load_state()
            assert "wasserstein" in str(e.value) and "lsgan" in str(e.value) and ck.epoch == 0     # names both; nothing was loaded
    # weights alone (the --weights_init path) load across objectives, and a checkpointer without a trainer reads either file
    G, D = nets(ngan, 3)
    utils.Checkpointer(G, D, 1e-4, str(tmp_path / "x.pth"), N_epochs=10, verbose=False,
                       trainer=train.PGGANTrainer(G, D, objective="wasserstein")).load_state(files["lsgan"])
    utils.Checkpointer(G, D, 1e-4, files["lsgan"], N_epochs=10, verbose=False).load_state()
    load = ngan.models.Generator_PG.from_state_dict
    assert [load(files[k], verbose=False).trained_objective for k in ("lsgan", "wasserstein", "old")] == ["lsgan", "wasserstein", "wasserstein"]


def test_eval_prints_the_objective_with_its_tables(ngan, monkeypatch, tmp_path, capsys):
    """an LSGAN checkpoint's tables say so in their titles; a Wasserstein one's (and a file's without the key) read as ever"""
    from neuron_gan_amd.metric_table import METRICS
    m = next(m for m in METRICS if m.switch == "msssim")
    real = ngan.models.Generator_PG.from_state_dict

    def from_state_dict(filename, device=None, use_ema=False, verbose=True):
        G = real(filename, verbose=False, use_ema=use_ema)               # on the host
        G.to = lambda device: G
        return G
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(ngan.models.Generator_PG, "from_state_dict", from_state_dict)
    monkeypatch.setattr(ngan.eval, "load_dataset", lambda options, config, device: None)
    monkeypatch.setattr(ngan.metrics, m.evaluate, lambda G, dataset, **kw: None)
    monkeypatch.setattr(ngan.metrics, m.format, lambda res, title: title)
    out = {}
    for objective in ngan.train.OBJECTIVES:
        G, D = nets(ngan)
        f = str(tmp_path / f"GenDisc_{objective}.pth")
        ngan.utils.Checkpointer(G, D, 1e-4, f, N_epochs=10, verbose=False, trainer=ngan.train.PGGANTrainer(G, D, objective=objective)).save_state(1)
        capsys.readouterr()
        assert ngan.eval.main(["-weights", f, "--msssim", "4"]) == 0
        out[objective] = capsys.readouterr().out
    tail = m.title_tail.format(n=4)
    assert out["wasserstein"] == "{}, training generator of {}{}\n".format(m.title, str(tmp_path / "GenDisc_wasserstein.pth"), tail)
    assert out["lsgan"] == "{}, training generator of {}{}, lsgan objective\n".format(m.title, str(tmp_path / "GenDisc_lsgan.pth"), tail)


def test_entry_points_are_bound_and_validate_on_the_host(ngan):
    lib = ngan._C.lib()
    err = lib.ngan_last_error
    one = ctypes.c_void_p(64)            # any non-null address: every check below comes before the launch
    N = None
    # the extension section of the header (include/ngan_objectives.h, included by ngan.h), its ctypes table and the library agree
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "ngan.h")).read()
    declared = set(re.findall(r"\b(ngan_[a-z0-9_]+)\s*\(", open(os.path.join(root, "include", "ngan_objectives.h")).read()))
    assert '#include "ngan_objectives.h"' in main and declared == {"ngan_lsloss_head", "ngan_lsloss_head_bwd"}
    assert declared <= set(ngan._C.exported_symbols())
    raw = ctypes.CDLL(ngan._C.LIB_PATH)
    assert all(hasattr(raw, name) for name in declared)
    sig = ngan._C.SIGNATURES
    assert sig["ngan_lsloss_head"] == ngan._C.SIGNATURES["ngan_wloss_head"][:3] + [ctypes.c_float] + ngan._C.SIGNATURES["ngan_wloss_head"][3:]
    assert sig["ngan_lsloss_head_bwd"] == ngan._C.SIGNATURES["ngan_wloss_head_bwd"][:3] + [ctypes.c_float] + ngan._C.SIGNATURES["ngan_wloss_head_bwd"][3:]
    head, bwd = lib.ngan_lsloss_head, lib.ngan_lsloss_head_bwd
    for p in ((N, one, one, one), (one, N, one, one), (one, one, N, one), (one, one, one, N)):
        assert head(p[0], 4, 4, 1.0, 0.0, p[1], p[2], p[3], None) == -1 and b"lsloss_head" in err()
    for n_real, n_fake in ((0, 4), (-1, 4), (4, -1), (0, 0)):
        assert head(one, n_real, n_fake, 1.0, 0.0, one, one, one, None) == -1 and b"lsloss_head" in err()
        assert bwd(one, n_real, n_fake, 1.0, 0.0, one, one, one, one, None) == -1 and b"lsloss_head_bwd" in err()
    assert bwd(N, 4, 4, 1.0, 0.0, one, one, one, one, None) == -1 and bwd(one, 4, 4, 1.0, 0.0, one, one, one, N, None) == -1
