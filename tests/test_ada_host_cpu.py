"""CPU-only checks of the adaptive augmentation switch: the third ABI surface (include/ngada.h against _C.ADA_SIGNATURES and the
library's ngada_ symbols, with the comparison of tests/test_host_cpu.py), refusals that need no GPU,
configuration and command line, the trainers' refusals and the default trainer's attribute set, and the cases of tests/ada_cases.py:
the emulation against the integer / fp64 oracle, exactly."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import ada_cases as A
from conftest import ROOT
from test_host_cpu import _abi_mismatches, _dynamic_symbols, built  # noqa: F401  (built: the session fixture that builds the library)

NAMES = {"ngada_accumulate", "ngada_update", "ngada_diffaug_params", "ngada_diffgeo_params"}


def _ada_prototypes():
    """{name: (return type, [(type, parameter name), ...])} of every prototype of include/ngada.h, as test_host_cpu._abi_prototypes reads
    ngan.h: types without `const`, the `*` attached; every `ngada_...(` of the header has to be one of them"""
    text = open(os.path.join(ROOT, "include", "ngada.h")).read()
    mentioned = set(re.findall(r"\b(ngada_[a-z0-9_]+)\s*\(", text))
    code = re.sub(r"(?m)^\s*#.*$", " ", re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))

    def ctype(t):
        t = " ".join(re.sub(r"\bconst\b", " ", t).replace("*", " * ").split())
        return t.replace(" *", "*")

    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ ]*?[\s*]+)(ngada_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code):
        assert name not in protos, f"{name} is declared twice"
        plist = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"\s*(.*[\s*])([A-Za-z_]\w*)\s*", p, flags=re.S)
            assert m and ctype(m.group(1)), f"{name}: cannot parse the parameter {p!r}"
            plist.append((ctype(m.group(1)), m.group(2)))
        protos[name] = (ctype(ret), plist)
    assert mentioned == set(protos), f"named with a '(' in the header but not declared: {sorted(mentioned - set(protos))}"
    return protos


def test_ada_table_follows_its_header(built):  # noqa: F811
    """ngada.h == the ADA tables == the library's ngada_ symbols, argument by argument; the other tables hold none of them, neither
    ngan.h nor nganx.h includes the header, and lib() binds the rows"""
    C = built._C
    protos = _ada_prototypes()
    exported = {n for n in _dynamic_symbols(C.LIB_PATH) if n.startswith("ngada_")}
    assert _abi_mismatches(protos, C.ADA_SIGNATURES, {}, exported) == []
    assert set(protos) == NAMES
    others = list(C.exported_symbols()) + list(C.EXT_SIGNATURES) + list(C.EXT_NON_STATUS)
    assert not any(n.startswith("ngada_") for n in others) and len(C.exported_symbols()) == 185
    for header in ("ngan.h", "nganx.h"):
        assert "ngada" not in open(os.path.join(ROOT, "include", header)).read(), header
    lib = C.lib()
    for name, row in C.ADA_SIGNATURES.items():
        assert getattr(lib, name).argtypes == row and getattr(lib, name).restype is ctypes.c_int, name


@pytest.mark.parametrize("name, perturb, word", [
    ("ngada_update", lambda row: [ctypes.c_float if t is ctypes.c_double else t for t in row], "`double span`"),    # the span as a float
    ("ngada_accumulate", lambda row: row[:2] + row[3:], "7 in the table"),                                         # one int dropped
    ("ngada_diffaug_params", lambda row: row[:7] + [ctypes.c_float] + row[8:], "`float* p`"),                      # p by value again
    ("ngada_diffgeo_params", lambda row: row[:-1], "8 in the table"),                                              # the stream dropped
])
def test_a_drifted_ada_row_is_reported(built, name, perturb, word):  # noqa: F811
    C = built._C
    protos = _ada_prototypes()
    drifted = dict(C.ADA_SIGNATURES, **{name: perturb(list(C.ADA_SIGNATURES[name]))})
    assert drifted[name] != C.ADA_SIGNATURES[name]
    bad = _abi_mismatches(protos, drifted, {}, set(protos))
    assert bad and all(line.startswith(name + ":") for line in bad) and any(word in line for line in bad), bad


def test_refusals_need_no_gpu(built):  # noqa: F811
    """null pointers and arguments outside the domain return the documented status before anything is launched"""
    lib = built._C.lib()
    one = ctypes.c_void_p(64)            # any aligned non-null address: the checks come before the launch
    err = lambda: lib.ngan_last_error()  # noqa: E731
    assert lib.ngada_accumulate(None, one, 4, 4, 1, 0.0, one, None) == -1 and b"real_scores is a null" in err()
    assert lib.ngada_accumulate(one, None, 4, 4, 1, 0.0, one, None) == -1 and b"mode 1 needs fake_scores" in err()
    assert lib.ngada_accumulate(one, one, 4, 4, 1, 0.0, None, None) == -1 and b"counters is a null" in err()
    assert lib.ngada_accumulate(one, one, 4, 4, 1, 0.0, ctypes.c_void_p(68), None) == -1 and b"8-byte" in err()
    for mode in (-1, 2):
        assert lib.ngada_accumulate(one, one, 4, 4, mode, 0.0, one, None) == -1 and b"mode" in err()
    for n in (0, -3, 65537):
        assert lib.ngada_accumulate(one, None, n, 0, 0, 0.0, one, None) == -2 and b"n_real" in err()
        assert lib.ngada_accumulate(one, one, 4, n, 1, 0.0, one, None) == -2 and b"n_fake" in err()
    assert lib.ngada_update(None, one, 0.6, 1e3, 1.0, None) == -1 and b"counters is a null" in err()
    assert lib.ngada_update(one, None, 0.6, 1e3, 1.0, None) == -1 and b"p is a null" in err()
    for span in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.ngada_update(one, one, 0.6, span, 1.0, None) == -1 and b"span" in err()
    for target in (1.5, -1.5, float("nan")):
        assert lib.ngada_update(one, one, target, 1e3, 1.0, None) == -1 and b"target" in err()
    for p_max in (-0.1, 1.1, float("nan")):
        assert lib.ngada_update(one, one, 0.6, 1e3, p_max, None) == -1 and b"p_max" in err()
    for fn, top in ((lib.ngada_diffaug_params, 8), (lib.ngada_diffgeo_params, 4)):
        assert fn(one, one, 4, 16, 16, 4, 1, None, None) == -1 and b"p is a null" in err()
        assert fn(None, one, 4, 16, 16, 4, 1, one, None) == -1 and b"null pointer" in err()
        assert fn(one, one, 4, 16, 16, 4, top, one, None) == -1 and b"policy mask" in err()
        assert fn(one, one, 4, 18, 18, 4, 1, one, None) == -2 and b"R=18" in err()
        assert fn(one, one, 4, 16, 16, 3, 1, one, None) == -1 and b"3 rows" in err()


def test_config_validation_and_command_line(ngan):
    config = ngan.configs.config
    keep = {k: getattr(config, k) for k in config.configs_name}
    try:
        assert {k: config.configs_name[k] for k in ngan.train.ADA_DEFAULTS} == ngan.train.ADA_DEFAULTS == dict(
            ada_target=0.0, ada_interval=4, ada_kimg=500.0, ada_p_init=0.0)
        config.set_configs(diffaug="color,cutout", ada_target=0.6, ada_interval=2, ada_kimg=10.0, ada_p_init=0.25, diffaug_p=0.5)
        config.validate_configs(create_dirs=False)
        good = dict(diffaug="color", diffaug_p=1.0, ada_target=0.6, ada_interval=4, ada_kimg=500.0, ada_p_init=0.0, wgan=False, pggan=True)
        for bad, word in ((dict(ada_target=1.0), "ada_target"), (dict(ada_target=-0.1), "ada_target"), (dict(ada_target=True), "ada_target"),
                          (dict(ada_interval=0), "ada_interval"), (dict(ada_interval=2.0), "ada_interval"), (dict(ada_kimg=0.0), "ada_kimg"),
                          (dict(ada_kimg=float("inf")), "ada_kimg"), (dict(ada_p_init=-0.1), "ada_p_init"),
                          (dict(ada_p_init=0.6, diffaug_p=0.5), "ada_p_init"), (dict(diffaug=""), "none is named"),
                          (dict(diffaug="", wgan=True, pggan=False), "ada_target")):
            config.set_configs(**dict(good, **bad))
            with pytest.raises(ValueError, match=word):
                config.validate_configs(create_dirs=False)
        config.set_configs(**dict(good, ada_target=0.0, diffaug=""))              # off needs no policy
        config.validate_configs(create_dirs=False)
    finally:
        config.set_configs(**keep)
    T = ngan.train
    p = T.build_arg_parser()
    o = p.parse_args([])
    assert (o.ada_target, o.ada_interval, o.ada_kimg, o.ada_p_init) == (0.0, 4, 500.0, 0.0)
    argv = ["--diffaug", "color", "--ada_target", "0.6", "--ada_interval", "2", "--ada_kimg", "20", "--ada_p_init", "0.1"]
    o = p.parse_args(argv)
    assert T.cli_overrides(argv, o, config.configs_name) == {"diffaug": "color", "ada_target": 0.6, "ada_interval": 2, "ada_kimg": 20.0,
                                                             "ada_p_init": 0.1}
    assert "0.6" in p.format_help()                                                # the help recommends Karras et al.'s target
    wgan = types.SimpleNamespace(wgan=True, pggan=False, ada_target=0.6)
    with pytest.raises(ValueError, match="ada_target > 0 is not available for the WGAN nets"):
        T.make_trainer(wgan, None, None)


def _nets(ngan):
    torch.manual_seed(2)
    return ngan.models.Generator_PG([16, 8], image_size_init=4, latent_dim=16), ngan.models.Discriminator_PG([8, 16], image_size_init=4)


def test_trainer_refusals_and_the_default_attribute_set(ngan):
    """ada_target = 0 sets nothing on the instance and allocates nothing; a target adds the controller alone, keeps the policy on at
    p = 0 and makes diffaug_p the clamp; every documented refusal raises ValueError"""
    T = ngan.train
    plain, off = T.PGGANTrainer(*_nets(ngan)), T.PGGANTrainer(*_nets(ngan), ada_target=0.0, ada_interval=4, ada_kimg=500.0, ada_p_init=0.0)
    assert set(vars(plain)) == set(vars(off)) and not any("ada" in k for k in vars(off))
    assert not off.ada_enabled and off.ada_target == 0.0 and off.ada_iteration == 0 and off._ada is None
    assert len(off._training_state()) == len(plain._training_state())
    with pytest.raises(ValueError, match="ada_target = 0"):
        off.ada_state()
    fixed = T.PGGANTrainer(*_nets(ngan), diffaug="color", diffaug_p=0.0)
    assert not fixed.diffaug_enabled                                               # p = 0 still switches a fixed policy off
    on = T.PGGANTrainer(*_nets(ngan), diffaug="color,geometry", diffaug_p=0.75, ada_target=0.6, ada_interval=2, ada_kimg=0.5, ada_p_init=0.25)
    assert set(vars(on)) - set(vars(plain)) == {"_ada"} and on.ada_enabled and on.diffaug_enabled
    ada = on._ada
    assert (ada.target, ada.interval, ada.kimg, ada.span, ada.p_max, ada.iteration) == (0.6, 2, 0.5, 500.0, 0.75, 0)
    assert ada.counters.dtype == torch.int64 and ada.counters.tolist() == [0, 0, 0, 0]
    assert ada.p.dtype == torch.float32 and ada.p.tolist() == [0.25, 0.0] and on._aug.live_p is ada.p and on._aug.p == 0.75
    assert (ada.mode, ada.threshold) == (ngan.ops.ADA_MODE_MIDPOINT, 0.0)
    assert len(on._training_state()) == len(plain._training_state()) + 2
    ls = T.PGGANTrainer(*_nets(ngan), diffaug="cutout", ada_target=0.6, objective="lsgan")
    assert (ls._ada.mode, ls._ada.threshold) == (ngan.ops.ADA_MODE_THRESHOLD, 0.5)
    zero = T.PGGANTrainer(*_nets(ngan), diffaug="color", diffaug_p=0.0, ada_target=0.6)
    assert zero.diffaug_enabled and zero._ada.p_max == 0.0                         # the policy stays on although p cannot leave 0
    state = on.ada_state()
    assert set(state) == set(ngan.utils.ADA_KEYS) and state["ada_counters"].tolist() == [0, 0, 0, 0] and state["ada_p"].tolist() == [0.25, 0.0]
    on.load_ada_state(dict(state, ada_iteration=7, ada_counters=torch.tensor([5, 3, 8, 2]), ada_p=torch.tensor([0.9, -0.5])))
    assert on.ada_iteration == 7 and ada.counters.tolist() == [5, 3, 8, 2] and ada.p.tolist() == [0.75, -0.5]      # p clamped to p_max
    for kw, word in ((dict(ada_target=1.0), "ada_target"), (dict(ada_target=-0.5), "ada_target"), (dict(ada_target=float("nan")), "ada_target"),
                     (dict(ada_target=0.6, diffaug=""), "none is named"), (dict(ada_interval=0), "ada_interval"),
                     (dict(ada_interval=1.5), "ada_interval"), (dict(ada_kimg=0), "ada_kimg"), (dict(ada_kimg=-1.0), "ada_kimg"),
                     (dict(ada_p_init=-0.01), "ada_p_init"), (dict(ada_p_init=0.8, diffaug_p=0.75), "ada_p_init"),
                     (dict(ada_p_init=1.5), "ada_p_init")):
        with pytest.raises(ValueError, match=word):
            T.PGGANTrainer(*_nets(ngan), **dict(dict(diffaug="color", ada_target=0.6), **kw))
    with pytest.raises(ValueError, match="ada_target"):                            # (refused before the nets are looked at)
        T.WGANTrainer(None, None, ada_target=0.6)


def test_the_wrappers_refuse_wrong_state_before_the_library(ngan):
    ops = ngan.ops
    counters, p = ops.ada_state("cpu", 0.5)
    assert counters.tolist() == [0, 0, 0, 0] and p.tolist() == [0.5, 0.0]
    with pytest.raises(ValueError, match="int64"):
        ops.ada_accumulate(torch.zeros(4), None, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="fp32"):
        ops.ada_update(counters, torch.zeros(2, dtype=torch.float64), 0.6, 1e3)
    with pytest.raises(NotImplementedError, match="fp32 scores"):
        ops.ada_accumulate(torch.zeros(4, dtype=torch.bfloat16), None, counters)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # host tensors never fall back to eager PyTorch
        ops.ada_accumulate(torch.zeros(4), None, counters)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ada_update(counters, p, 0.6, 1e3)
    with pytest.raises(ValueError, match="device tensor"):
        ops.diffaug_params_live(torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.int32), 16, 7, 0.5)


# ---- the cases: emulation against the oracle, exactly -----------------------------------------------------------------------------
CASES = A.score_cases()


def test_the_score_cases_cover_what_they_claim():
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names)
    for b in A.SIZES:
        assert {f"dyadic_mid_{b}", "dyadic_thr_%d" % b, f"far_mid_{b}", f"far_thr_{b}"} <= set(names)
    assert {len(c[1]) for c in CASES} >= set(A.SIZES) and {c[3] for c in CASES} == {0, 1}
    ties = [n for n, real, fake, mode, thr in CASES if n.startswith("dyadic") and sum(A.oracle_counts(real, fake, mode, thr)[:2]) < len(real)]
    assert len(ties) >= len(A.SIZES), "the dyadic cases hold no ties"
    special = {c[0]: c for c in A.special_cases()}
    assert A.oracle_counts(*special["nan_threshold"][1:]) == (0, 0, 10) and A.oracle_counts(*special["nan_in_fakes"][1:]) == (0, 0, 3)
    assert A.oracle_counts(*special["nan_inf_threshold"][1:]) == (2, 4, 10)       # {inf, 2} above 0.5; {-1, .25, -inf, 0} below; 2 ties, 2 NaN
    assert A.oracle_counts(*special["posinf_in_reals"][1:]) == (0, 2, 4) and A.oracle_counts(*special["both_inf"][1:]) == (0, 0, 3)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_accumulate_emulation_agrees_with_the_oracle(case):
    """the kernel's summation order and the exactly rounded sums give the same counts on every case, and a second call adds"""
    _, real, fake, mode, thr = case
    pos, neg, n = A.oracle_counts(real, fake, mode, thr)
    start = [7, 1 << 40, (1 << 40) + 9, 3]
    once = A.emulate_accumulate(start, real, fake, mode, thr)
    assert once == [7 + pos, (1 << 40) + neg, (1 << 40) + 9 + n, 3]
    assert A.emulate_accumulate(once, real, fake, mode, thr) == [7 + 2 * pos, (1 << 40) + 2 * neg, (1 << 40) + 9 + 2 * n, 3]
    assert pos + neg <= n == len(real)


def test_update_emulation_agrees_with_the_oracle():
    for case in A.update_cases():
        want, got = A.oracle_update(*case), A.emulate_update(*case)
        assert (A.bits(want[0]), A.bits(want[1])) == (A.bits(got[0]), A.bits(got[1])), (case, want, got)
        pos, neg, n, p, last_r, target, span, p_max = case
        assert 0.0 <= float(got[0]) <= float(np.float32(p_max)), case                              # p never leaves [0, p_max]
        if n == 0:
            assert A.bits(got[1]) == A.bits(last_r) and (A.bits(got[0]) == A.bits(p) or np.isnan(p)), case


def test_one_update_moves_p_by_n_over_span_towards_the_target():
    """away from the clamps: p' = fp32(p + sign(r - target) n / span) exactly, for r above, below and on the target"""
    for pos, neg, n, target in ((7, 1, 8, 0.6), (5, 3, 8, 0.6), (6, 2, 8, 0.5), (3, 1, 4, 0.25), (100, 28, 128, 0.5625)):
        r = (pos - neg) / n
        sign = (r > float(np.float32(target))) - (r < float(np.float32(target)))
        for p, span in ((0.5, 1000.0), (0.25, 64.0), (0.3, 500000.0)):
            got_p, got_r = A.emulate_update(pos, neg, n, p, 0.0, target, span, 1.0)
            assert A.bits(got_p) == A.bits(np.float32(float(np.float32(p)) + sign * n / span)), (pos, neg, n, target, p, span)
            assert A.bits(got_r) == A.bits(np.float32(r))
    assert (6 - 2) / 8 == 0.5                                                                     # the on-target row has sign 0


def test_p_stays_inside_its_range_over_a_long_random_walk():
    rng = np.random.default_rng(5)
    for p_max in (1.0, 0.3, 0.0):
        p, last = np.float32(0.0), np.float32(0.0)
        for _ in range(2000):
            n = int(rng.integers(0, 64))
            pos = int(rng.integers(0, n + 1))
            neg = int(rng.integers(0, n - pos + 1))
            p, last = A.emulate_update(pos, neg, n, p, last, 0.6, float(rng.choice([8.0, 100.0, 5e5])), p_max)
            assert 0.0 <= float(p) <= float(np.float32(p_max)) and -1.0 <= float(last) <= 1.0


def test_checkpoint_keys_round_trip_and_the_eval_side_loader_ignores_them(ngan, tmp_path, capsys):
    """a checkpoint written by a trainer with the controller carries the keys; Checkpointer.load_state restores count, counters and p
    (clamped to the new run's diffaug_p, other settings logged); Generator_PG.from_state_dict, the one call through which eval.py reads a
    checkpoint, loads the same file to the same weights; a trainer without the controller writes none of the keys"""
    T, U = ngan.train, ngan.utils
    f = str(tmp_path / "ada.pth")
    G, D = _nets(ngan)
    tr = T.PGGANTrainer(G, D, diffaug="color", ada_target=0.6, ada_interval=2, ada_kimg=0.5, ada_p_init=0.25)
    tr.load_ada_state(dict(ada_iteration=7, ada_counters=torch.tensor([5, 3, 8, 2]), ada_p=torch.tensor([0.625, -0.5])))
    ck = U.Checkpointer(G, D, 1e-3, f, N_epochs=4, verbose=False, trainer=tr)
    ck.ADA = [(1, 0.25, 0.0), (2, 0.625, -0.5)]
    ck.save_state(2)
    saved = U.load_checkpoint_dict(f)
    assert set(U.ADA_KEYS) <= set(saved) and saved[U.ADA_SERIES_KEY] == ck.ADA
    assert (saved["ada_target"], saved["ada_interval"], saved["ada_kimg"], saved["ada_iteration"]) == (0.6, 2, 0.5, 7)
    assert saved["ada_counters"].tolist() == [5, 3, 8, 2] and saved["ada_p"].tolist() == [0.625, -0.5]
    G2, D2 = _nets(ngan)
    tr2 = T.PGGANTrainer(G2, D2, diffaug="color", diffaug_p=0.5, ada_target=0.5, ada_interval=4, ada_kimg=0.5)
    ck2 = U.Checkpointer(G2, D2, 1e-3, f, N_epochs=4, verbose=False, trainer=tr2)
    capsys.readouterr()
    ck2.load_state()
    assert "ada_target=0.6, ada_interval=2" in capsys.readouterr().out                     # other settings: allowed, and said
    assert tr2.ada_iteration == 7 and tr2._ada.counters.tolist() == [5, 3, 8, 2] and tr2._ada.p.tolist() == [0.5, -0.5] and ck2.ADA == ck.ADA
    assert (tr2._ada.target, tr2._ada.interval) == (0.5, 4)                                # the settings stay the new run's
    loaded = ngan.models.Generator_PG.from_state_dict(f, verbose=False)                    # eval.py's reader
    want = G.state_dict()
    assert all(torch.equal(v, want[k]) for k, v in loaded.state_dict().items())
    h = str(tmp_path / "plain.pth")
    G3, D3 = _nets(ngan)
    U.Checkpointer(G3, D3, 1e-3, h, N_epochs=4, verbose=False, trainer=T.PGGANTrainer(G3, D3, diffaug="color")).save_state(1)
    assert not any(k.startswith("ada") or k == "ADA" for k in U.load_checkpoint_dict(h))
    tr4 = T.PGGANTrainer(*_nets(ngan), diffaug="color", ada_target=0.6, ada_p_init=0.125)    # a file without the keys is off: p starts fresh
    U.Checkpointer(tr4.G, tr4.D, 1e-3, h, N_epochs=4, verbose=False, trainer=tr4).load_state()
    assert "no adaptive augmentation state" in capsys.readouterr().out and tr4._ada.p.tolist() == [0.125, 0.0] and tr4.ada_iteration == 0
