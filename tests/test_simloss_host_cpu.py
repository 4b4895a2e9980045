"""CPU-only checks of the similarity switch's host side: the extension ABI (include/nganx.h against _C.EXT_SIGNATURES /
_C.EXT_NON_STATUS and the library's nganx_ symbols, with the comparison of tests/test_host_cpu.py), configuration and command line,
the default trainer's attribute set, and the per-epoch weight the epoch driver hands to the trainer."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_epoch_dist_cpu import StubCheckpoint, StubTrainer, _cfg, _dataset
from test_host_cpu import _abi_mismatches, _dynamic_symbols, built  # noqa: F401  (built: the session fixture that builds the library)


def _ext_prototypes():
    """{name: (return type, [(type, parameter name), ...])} of every prototype of include/nganx.h, as test_host_cpu._abi_prototypes
    reads ngan.h: types without `const`, the `*` attached; every `nganx_...(` of the header has to be one of them"""
    text = open(os.path.join(ROOT, "include", "nganx.h")).read()
    mentioned = set(re.findall(r"\b(nganx_[a-z0-9_]+)\s*\(", text))
    code = re.sub(r"(?m)^\s*#.*$", " ", re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))

    def ctype(t):
        t = " ".join(re.sub(r"\bconst\b", " ", t).replace("*", " * ").split())
        return t.replace(" *", "*")

    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s*]+)(nganx_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code):
        assert name not in protos, f"{name} is declared twice"
        plist = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"\s*(.*[\s*])([A-Za-z_]\w*)\s*", p, flags=re.S)
            assert m and ctype(m.group(1)), f"{name}: cannot parse the parameter {p!r}"
            plist.append((ctype(m.group(1)), m.group(2)))
        protos[name] = (ctype(ret), plist)
    assert mentioned == set(protos), f"named with a '(' in the header but not declared: {sorted(mentioned - set(protos))}"
    return protos


def test_extension_table_follows_its_header(built):  # noqa: F811
    """nganx.h == the extension tables == the library's nganx_ symbols, argument by argument; the core tables hold none of them, ngan.h
    does not include the header, and lib() binds both"""
    C = built._C
    protos = _ext_prototypes()
    exported = {n for n in _dynamic_symbols(C.LIB_PATH) if n.startswith("nganx_")}
    assert _abi_mismatches(protos, C.EXT_SIGNATURES, C.EXT_NON_STATUS, exported) == []
    assert set(protos) == {"nganx_pair_gram", "nganx_pair_gram_workspace_bytes", "nganx_simloss_head", "nganx_pair_mix"}
    assert not any(n.startswith("nganx_") for n in C.exported_symbols()) and len(C.exported_symbols()) == 185
    assert "nganx" not in open(os.path.join(ROOT, "include", "ngan.h")).read()
    lib = C.lib()
    for name, row in C.EXT_SIGNATURES.items():
        assert getattr(lib, name).argtypes == row and getattr(lib, name).restype is ctypes.c_int, name
    for name, (row, ret) in C.EXT_NON_STATUS.items():
        assert getattr(lib, name).argtypes == row and getattr(lib, name).restype is ret, name


@pytest.mark.parametrize("name, perturb, word", [
    ("nganx_pair_gram", lambda row: [ctypes.c_int if t is ctypes.c_long else t for t in row], "`long "),       # a long as int
    ("nganx_simloss_head", lambda row: row[:4] + row[5:], "11 in the table"),                                    # one int dropped
    ("nganx_pair_mix", lambda row: row[:-1], "8 in the table"),                                                  # the stream dropped
])
def test_a_drifted_extension_row_is_reported(built, name, perturb, word):  # noqa: F811
    C = built._C
    protos = _ext_prototypes()
    drifted = dict(C.EXT_SIGNATURES, **{name: perturb(list(C.EXT_SIGNATURES[name]))})
    assert drifted[name] != C.EXT_SIGNATURES[name]
    bad = _abi_mismatches(protos, drifted, C.EXT_NON_STATUS, set(protos))
    assert bad and all(line.startswith(name + ":") for line in bad) and any(word in line for line in bad), bad
    wrong_ret = {"nganx_pair_gram_workspace_bytes": (C.EXT_NON_STATUS["nganx_pair_gram_workspace_bytes"][0], ctypes.c_int)}
    assert [b.split(":")[0] for b in _abi_mismatches(protos, C.EXT_SIGNATURES, wrong_ret, set(protos))] == ["nganx_pair_gram_workspace_bytes"]


def test_refusals_and_the_workspace_query_need_no_gpu(built):  # noqa: F811
    lib = built._C.lib()
    assert lib.nganx_pair_gram_workspace_bytes(16, 512 * 512) == 1024 * (16 * 16 + 16) * 8
    assert lib.nganx_pair_gram_workspace_bytes(2, 16) == (2 * 2 + 2) * 8
    for b, n in ((1, 64), (65, 64), (2, 18), (2, 12), (2, 1 << 31)):
        assert lib.nganx_pair_gram_workspace_bytes(b, n) == 0, (b, n)
    one = ctypes.c_void_p(64)            # any aligned non-null address: the checks come before the launch
    assert lib.nganx_pair_gram(None, one, one, one, 2, 64, None) == -1 and b"rows is a null" in lib.ngan_last_error()
    assert lib.nganx_pair_gram(one, one, one, one, 65, 64, None) == -2 and b"B=65" in lib.ngan_last_error()
    assert lib.nganx_pair_mix(one, one, one, one, None, one, 2, 18, None) == -2 and b"N=18" in lib.ngan_last_error()
    assert lib.nganx_pair_mix(ctypes.c_void_p(68), one, one, one, None, one, 2, 64, None) == -1 and b"rows must start on a 16-byte" in lib.ngan_last_error()
    assert lib.nganx_simloss_head(one, one, one, None, 2, 64, 0, one, one, one, one, None) == -1 and b"lambda" in lib.ngan_last_error()


def test_config_validation_and_command_line(ngan):
    config = ngan.configs.config
    keep = {k: getattr(config, k) for k in config.configs_name}
    try:
        assert config.configs_name["sim_loss_on"] == "real" and config.configs_name["sim_loss_center"] is False
        config.set_configs(sim_loss_on="generated", sim_loss_center=True, sim_loss_lambda=0.0)      # lambda = 0: accepted and inert
        config.validate_configs(create_dirs=False)
        for bad in (dict(sim_loss_on="fake"), dict(sim_loss_on="generated", sim_loss_center=1),
                    dict(sim_loss_on="generated", wgan=True, pggan=False)):
            config.set_configs(**dict(dict(sim_loss_on="real", sim_loss_center=False), **bad))
            with pytest.raises(ValueError, match="sim_loss"):
                config.validate_configs(create_dirs=False)
    finally:
        config.set_configs(**keep)
    T = ngan.train
    p = T.build_arg_parser()
    o = p.parse_args([])
    assert (o.sim_loss_on, o.sim_loss_center) == ("real", False)
    argv = ["--sim_loss_on", "generated", "--sim_loss_center", "--sim_loss_lambda", "0.5"]
    o = p.parse_args(argv)
    assert T.cli_overrides(argv, o, config.configs_name) == {"sim_loss_on": "generated", "sim_loss_center": True, "sim_loss_lambda": 0.5}
    with pytest.raises(SystemExit):
        p.parse_args(["--sim_loss_on", "fake"])
    wgan = types.SimpleNamespace(wgan=True, pggan=False, sim_loss_on="generated")
    with pytest.raises(ValueError, match="sim_loss_on='generated' is not available for the WGAN nets"):
        T.make_trainer(wgan, None, None)


def _nets(ngan):
    torch.manual_seed(2)
    return ngan.models.Generator_PG([16, 8], image_size_init=4, latent_dim=16), ngan.models.Discriminator_PG([8, 16], image_size_init=4)


def test_the_default_trainer_gains_no_attribute(ngan):
    """sim_loss_on="real" sets nothing on the instance: its attribute set is that of a trainer built without the arguments, it holds
    no buffer for the term, and its hook is None; "generated" adds the device scalar and the two settings"""
    T = ngan.train
    plain, real = T.PGGANTrainer(*_nets(ngan)), T.PGGANTrainer(*_nets(ngan), sim_loss_on="real", sim_loss_center=False)
    assert set(vars(plain)) == set(vars(real)) and not any("sim" in k for k in vars(real))
    assert (real.sim_loss_on, real.sim_loss_center, real._sim_lambda) == ("real", False, None)
    assert not real.similarity_enabled and real._similarity_hook(4) is None
    with pytest.raises(ValueError, match="real"):
        real.set_sim_lambda(0.5)
    gen = T.PGGANTrainer(*_nets(ngan), sim_loss_on="generated", sim_loss_center=True)
    assert set(vars(gen)) - set(vars(plain)) == {"sim_loss_on", "sim_loss_center", "_sim_lambda"}
    assert gen.similarity_enabled and float(gen._sim_lambda) == 0.0 and gen._sim_lambda.dtype == torch.float32
    gen.set_sim_lambda(0.25)
    hook = gen._similarity_hook(4)
    assert float(gen._sim_lambda) == 0.25 and hook.lam is gen._sim_lambda and hook.center is True
    with pytest.raises(ValueError, match="at most 64"):
        gen._similarity_hook(65)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite number >= 0"):
            gen.set_sim_lambda(bad)
    with pytest.raises(ValueError, match="sim_loss_on"):
        T.PGGANTrainer(*_nets(ngan), sim_loss_on="fake")
    with pytest.raises(ValueError, match="sim_loss_center"):
        T.PGGANTrainer(*_nets(ngan), sim_loss_on="generated", sim_loss_center="yes")


class _SimStub(StubTrainer):
    """a stub with sim_loss_on="generated": records the weights it is handed and reports a term proportional to the weight"""
    similarity_enabled = True

    def __init__(self, steps):
        super().__init__(steps)
        self.lambdas, self.lam = [], None

    def set_sim_lambda(self, value):
        self.lam = float(value)
        self.lambdas.append(self.lam)

    def step(self, real, use_graph=True, global_batch=None):
        out = super().step(real, use_graph, global_batch)
        out["G_sim_loss"] = torch.tensor(2.0 * self.lam)
        return out


def reference_schedule(lam0, decay, epochs):
    """reference train.py:343-348, epoch by epoch"""
    lam, out = lam0, []
    for epoch in range(1, epochs + 1):
        if decay > 0 and lam > 0:
            if lam > 1e-5:
                lam = lam0 * (1 - decay) ** (epoch - 1)
            else:
                lam = 0.0
        out.append(lam)
    return out


@pytest.mark.parametrize("lam0, decay", [(0.5, 0.1), (0.5, 0.0), (0.0, 0.1), (1e-3, 0.99)])
def test_the_epoch_driver_hands_the_decayed_weight_to_the_trainer(ngan, lam0, decay):
    """six epochs: set_sim_lambda once per epoch with the reference's schedule (the cut to 0 below 1e-5 included: 1e-3 decaying by
    0.99); G_sim_loss is a monitor, the monitored G_loss is G_loss + G_sim_loss, and the real-image path is not taken"""
    cfg = _cfg(N_epochs=6, sim_loss_lambda=lam0, sim_loss_lambda_decay_rate=decay)
    tr = _SimStub(2)
    series = ngan.train.pggan_train(tr, _dataset(ngan, 8), cfg, checkpoint=StubCheckpoint(6), use_graph=False, log=lambda *a: None)
    want = reference_schedule(lam0, decay, 6)
    assert tr.lambdas == want and (decay < 0.9 or want[-1] == 0.0)
    np.testing.assert_allclose(series["G_sim_loss"], [2.0 * v for v in want], rtol=1e-6)
    plain_tr = StubTrainer(2)
    plain = ngan.train.pggan_train(plain_tr, _dataset(ngan, 8), _cfg(N_epochs=6), checkpoint=StubCheckpoint(6), use_graph=False,
                                   log=lambda *a: None)
    assert "G_sim_loss" not in plain and not hasattr(plain_tr, "lambdas")
    np.testing.assert_allclose(series["G_loss"], np.array(plain["G_loss"]) + 2.0 * np.array(want), rtol=1e-5)
