"""The penalty's forms and lazy regularisation, host side: the two entry points of include/ngan_penalty.h are bound and refuse bad
arguments before any launch, the configuration names and flags, the refusals for the WGAN nets, what make_trainer forwards, the
checkpoint keys and the due / not-due schedule.  No kernel is launched here; the arithmetic is tested on the GPU
(tests/test_gpu_penalty.py) and its bounds on the CPU (tests/test_penalty_bounds_cpu.py)."""
import ctypes
import os
import re
import types

import pytest
import torch


def nets(ngan, seed=1):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([16, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 16], image_size_init=4)
    return G, D


def test_entry_points_are_bound_and_validate_on_the_host(ngan):
    lib = ngan._C.lib()
    err = lib.ngan_last_error
    one = ctypes.c_void_p(64)            # any non-null, 16-byte aligned address: every check below comes before the launch
    odd = ctypes.c_void_p(68)            # 4-byte aligned only
    off = ctypes.c_void_p(66)            # not even that
    N = None
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    main = open(os.path.join(root, "include", "ngan.h")).read()
    declared = set(re.findall(r"\b(ngan_[a-z0-9_]+)\s*\(", open(os.path.join(root, "include", "ngan_penalty.h")).read()))
    assert '#include "ngan_penalty.h"' in main and declared == {"ngan_penalty_head", "ngan_penalty_bwd"}
    assert declared <= set(ngan._C.exported_symbols())
    raw = ctypes.CDLL(ngan._C.LIB_PATH)
    assert all(hasattr(raw, name) for name in declared)
    head, bwd = lib.ngan_penalty_head, lib.ngan_penalty_bwd
    for form in (1, 2):
        for p in ((N, one, one, one), (one, N, one, one), (one, one, N, one), (one, one, one, N)):
            assert head(p[0], 4, 8, form, 10.0, p[1], p[2], p[3], None) == -1 and b"penalty_head" in err()
            assert bwd(p[0], p[1], 4, 8, form, 10.0, p[2], p[3], None) == -1 and b"penalty_bwd" in err()
        for B, n in ((0, 8), (-1, 8), (4, 0), (4, -4)):
            assert head(one, B, n, form, 10.0, one, one, one, None) == -1 and b"penalty_head" in err()
            assert bwd(one, one, B, n, form, 10.0, one, one, None) == -1 and b"penalty_bwd" in err()
        # rows that do not start on 16-byte boundaries: the head refuses them by its shape status, as ngan_sample_l2norm does
        shape = lib.ngan_sample_l2norm(one, one, one, 2, 5, None)
        assert shape < 0 and shape != -1
        assert head(one, 2, 5, form, 10.0, one, one, one, None) == shape and b"16-byte" in err()
        assert head(odd, 2, 8, form, 10.0, one, one, one, None) == shape
        assert head(one, 2, 8, form, 10.0, one, off, one, None) == shape
        assert bwd(off, one, 2, 8, form, 10.0, one, one, None) == shape and bwd(one, one, 2, 8, form, 10.0, one, off, None) == shape
    for form in (0, 3, -1):
        assert head(one, 4, 8, form, 10.0, one, one, one, None) == -1 and b"unknown form" in err()
        assert bwd(one, one, 4, 8, form, 10.0, one, one, None) == -1 and b"unknown form" in err()
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # a host tensor never falls back to eager PyTorch
        ngan.ops.PenaltyHead.apply(torch.zeros(2, 8), 10.0, 2)
    assert (ngan.ops.PENALTY_ONE_SIDED, ngan.ops.PENALTY_ZERO_CENTRED) == (1, 2)


def test_configuration_names_flags_and_refusals(ngan):
    cfg, train = ngan.config, ngan.train
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    try:
        assert (cfg.configs_name["grad_pen_mode"], cfg.configs_name["grad_pen_interval"]) == ("gp", 1)
        parse = train.build_arg_parser().parse_args
        assert (parse([]).grad_pen_mode, parse([]).grad_pen_interval) == ("gp", 1)
        argv = ["--grad_pen_mode", "r1", "--grad_pen_interval", "4"]
        assert train.cli_overrides(argv, parse(argv), cfg.configs_name) == {"grad_pen_mode": "r1", "grad_pen_interval": 4}
        assert not {"grad_pen_mode", "grad_pen_interval"} & set(train.cli_overrides([], parse([]), cfg.configs_name))
        for mode in ("gp", "lp", "r1"):
            assert parse(["--grad_pen_mode", mode]).grad_pen_mode == mode
        with pytest.raises(SystemExit):
            parse(["--grad_pen_mode", "r2"])
        cfg.set_configs(grad_pen_mode="lp", grad_pen_interval=16)
        cfg.validate_configs()
        assert (cfg.grad_pen_mode, cfg.grad_pen_interval) == ("lp", 16)
        for bad in ("r2", "", None, 1, "GP"):
            cfg.set_configs(grad_pen_mode=bad, grad_pen_interval=1)
            with pytest.raises(ValueError, match="grad_pen_mode"):
                cfg.validate_configs()
        for bad in (0, -1, 2.0, "4", None, True):
            cfg.set_configs(grad_pen_mode="gp", grad_pen_interval=bad)
            with pytest.raises(ValueError, match="grad_pen_interval"):
                cfg.validate_configs()
        # the WGAN nets clip weights: refused by the configuration, by make_trainer and by the trainer
        for kw in (dict(grad_pen_mode="r1", grad_pen_interval=1), dict(grad_pen_mode="gp", grad_pen_interval=2)):
            cfg.set_configs(wgan=True, pggan=False, **kw)
            with pytest.raises(ValueError, match="grad_pen"):
                cfg.validate_configs()
            with pytest.raises(ValueError, match="grad_pen"):
                train.make_trainer(cfg, None, None)
            with pytest.raises(ValueError, match="grad_pen"):
                train.WGANTrainer(None, None, **kw)
        cfg.set_configs(wgan=True, pggan=False, grad_pen_mode="gp", grad_pen_interval=1)
        cfg.validate_configs()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)


def test_make_trainer_forwards_mode_and_interval(ngan, monkeypatch):
    train = ngan.train
    seen = []
    monkeypatch.setattr(train, "PGGANTrainer", lambda G, D, **kw: seen.append(kw) or "pg")
    base = dict(wgan=False, pggan=True, RMSprop=False, learning_rate=1e-4, grad_pen_lambda=10.0, drift_epsilon=0.001, n_critic=1,
                alpha_step=0.05, beta1=0.5)
    assert train.make_trainer(types.SimpleNamespace(**base), None, None) == "pg"             # a configuration from before the names
    assert train.make_trainer(types.SimpleNamespace(**base, grad_pen_mode="gp", grad_pen_interval=1), None, None) == "pg"
    assert train.make_trainer(types.SimpleNamespace(**base, grad_pen_mode="r1", grad_pen_interval=1), None, None) == "pg"
    assert train.make_trainer(types.SimpleNamespace(**base, grad_pen_mode="gp", grad_pen_interval=4, lsgan=True), None, None) == "pg"
    assert [(kw.get("grad_pen_mode"), kw.get("grad_pen_interval")) for kw in seen] == [(None, None), (None, None), ("r1", 1), ("gp", 4)]
    assert seen[3]["objective"] == "lsgan" and all(kw["grad_pen_lambda"] == 10.0 for kw in seen)


def test_trainer_validates_and_weights_the_penalty(ngan):
    train, LF = ngan.train, ngan.loss_functions
    assert LF.PENALTY_MODES == ("gp", "lp", "r1")
    tr = train.PGGANTrainer(*nets(ngan))
    assert (tr.grad_pen_mode, tr.grad_pen_interval, tr.grad_pen_iteration) == ("gp", 1, 0)
    assert tr.gp_loss.mode == "gp" and tr.gp_loss.Lambda == 10.0 and tr._graph_key((4, 1, 8, 8)) == (4, 1, 8, 8)
    tr = train.PGGANTrainer(*nets(ngan), grad_pen_mode="r1", grad_pen_interval=4, grad_pen_lambda=2.5)
    assert tr.gp_loss.mode == "r1" and tr.gp_loss.Lambda == 10.0                               # k times the weight
    for bad in ("r2", "", None, 1):
        with pytest.raises(ValueError, match="grad_pen_mode"):
            train.PGGANTrainer(*nets(ngan), grad_pen_mode=bad)
        with pytest.raises(ValueError, match="mode"):
            LF.D_grad_pen_loss(None, None, 10.0, mode=bad)
    for bad in (0, -3, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="grad_pen_interval"):
            train.PGGANTrainer(*nets(ngan), grad_pen_interval=bad)
    # lambda = 0: both arguments are accepted and nothing is due, ever; the graph key is the plain one
    tr = train.PGGANTrainer(*nets(ngan), grad_pen_lambda=0.0, grad_pen_mode="lp", grad_pen_interval=3)
    assert not tr.penalty_due and tr._graph_key((4, 1, 8, 8)) == (4, 1, 8, 8)


@pytest.mark.parametrize("k", [1, 3, 4])
def test_the_schedule_is_every_kth_iteration(ngan, k):
    train = ngan.train
    assert [i for i in range(10) if train.grad_pen_due(i, k)] == list(range(0, 10, k))
    tr = train.PGGANTrainer(*nets(ngan), grad_pen_interval=k)
    due, keys = [], set()
    for i in range(10):
        assert tr.grad_pen_iteration == i
        if tr.penalty_due:
            due.append(i)
        keys.add(tr._graph_key((4, 1, 8, 8)))
        with tr._penalty_phase_held():               # what capture() does around its warm-up iterations and the capture
            tr._advance_penalty_phase()
        assert tr.grad_pen_iteration == i
        tr._advance_penalty_phase()                  # what train_iteration and replay do after the iteration
    assert due == list(range(0, 10, k))
    assert keys == ({(4, 1, 8, 8)} if k == 1 else {(4, 1, 8, 8, "penalty", True), (4, 1, 8, 8, "penalty", False)})


def test_checkpoint_carries_mode_interval_and_count(ngan, tmp_path):
    utils, train = ngan.utils, ngan.train
    assert utils.PENALTY_KEYS == {"grad_pen_mode": "gp", "grad_pen_interval": 1, "grad_pen_iteration": 0}

    def save(name, iteration, **kw):
        G, D = nets(ngan)
        tr = train.PGGANTrainer(G, D, **kw)
        tr.grad_pen_iteration = iteration
        f = str(tmp_path / f"GenDisc_{name}.pth")
        utils.Checkpointer(G, D, 1e-4, f, N_epochs=10, verbose=False, trainer=tr).save_state(2)
        return f

    files = {"gp1": save("gp1", 5), "r13": save("r13", 7, grad_pen_mode="r1", grad_pen_interval=3),
             "lp1": save("lp1", 2, grad_pen_mode="lp")}
    d = utils.load_checkpoint_dict(files["r13"])                                       # the weights-only unpickler takes the keys
    assert (d["grad_pen_mode"], d["grad_pen_interval"], d["grad_pen_iteration"]) == ("r1", 3, 7)
    d = utils.load_checkpoint_dict(files["gp1"])
    assert (d["grad_pen_mode"], d["grad_pen_interval"], d["grad_pen_iteration"]) == ("gp", 1, 5)
    for k in utils.PENALTY_KEYS:                                                       # a file from before the keys is gp / 1 / 0
        del d[k]
    files["old"] = str(tmp_path / "GenDisc_old.pth")
    torch.save(d, files["old"])

    def load(name, weights_only=False, **kw):
        G, D = nets(ngan, 2)
        tr = train.PGGANTrainer(G, D, **kw)
        tr.grad_pen_iteration = 1
        ck = utils.Checkpointer(G, D, 1e-4, str(tmp_path / "x.pth") if weights_only else files[name], N_epochs=10, verbose=False, trainer=tr)
        ck.load_state(files[name] if weights_only else None)
        return tr, ck

    tr, ck = load("r13", grad_pen_mode="r1", grad_pen_interval=3)
    assert ck.epoch == 2 and tr.grad_pen_iteration == 7 and not tr.penalty_due
    due = []
    for i in range(7, 13):                                                             # the resumed run continues the schedule
        due += [i] if tr.penalty_due else []
        tr._advance_penalty_phase()
    assert due == [9, 12]
    assert load("gp1")[0].grad_pen_iteration == 5 and load("old")[0].grad_pen_iteration == 0
    for name, kw, words in (("r13", {}, ("r1", "gp", "3", "1")), ("r13", dict(grad_pen_mode="r1"), ("3", "1")),
                            ("r13", dict(grad_pen_mode="lp", grad_pen_interval=3), ("r1", "lp")),
                            ("gp1", dict(grad_pen_interval=2), ("1", "2")), ("old", dict(grad_pen_mode="lp"), ("gp", "lp")),
                            ("lp1", {}, ("lp", "gp"))):
        G, D = nets(ngan, 2)
        ck = utils.Checkpointer(G, D, 1e-4, files[name], N_epochs=10, verbose=False, trainer=train.PGGANTrainer(G, D, **kw))
        with pytest.raises(ValueError, match="grad_pen_mode") as e:
            ck.load_state()
        assert all(w in str(e.value) for w in words) and ck.epoch == 0                 # names both; nothing was loaded
    # weights alone (the --weights_init path) load across modes and intervals and do not restore the count
    tr, _ = load("r13", weights_only=True)
    assert tr.grad_pen_iteration == 1
    tr, _ = load("gp1", weights_only=True, grad_pen_mode="lp", grad_pen_interval=4)
    assert tr.grad_pen_iteration == 1
    G, D = nets(ngan, 3)
    utils.Checkpointer(G, D, 1e-4, files["r13"], N_epochs=10, verbose=False).load_state()      # and a checkpointer without a trainer
