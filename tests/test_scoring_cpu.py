"""The plumbing around the seven checkpoint metrics (swd, msssim, spectrum, morph, skeleton, sholl, branch), on the CPU and without the
library: what `train.score_*` hands to `metrics.evaluate_*`, logs and stores, when `pggan_train` scores, what `eval.main` runs and
prints, the order of a checkpoint's keys, and the text of the four arbor tables.  Every expected value below is a literal."""
import contextlib
import os
import types

import pytest
import torch

from test_epoch_dist_cpu import StubCheckpoint, StubTrainer, _cfg, _dataset

# name, train's scorer, metrics' evaluate and format, the checkpoint list, eval.py's switch
METRICS = (("swd", "score_swd", "evaluate_swd", "format_table", "SWD", "--swd"),
           ("msssim", "score_msssim", "evaluate_msssim", "format_msssim", "MSSSIM", "--msssim"),
           ("spectrum", "score_spectrum", "evaluate_spectrum", "format_spectrum", "SPECTRUM", "--spectrum"),
           ("morph", "score_morph", "evaluate_morphology", "format_morphology", "MORPH", "--morph"),
           ("skeleton", "score_skeleton", "evaluate_skeleton", "format_skeleton", "SKELETON", "--skeleton"),
           ("sholl", "score_sholl", "evaluate_sholl", "format_sholl", "SHOLL", "--sholl"),
           ("branch", "score_branches", "evaluate_branches", "format_branches", "BRANCH", "--branches"))
KEYS = tuple(m[4] for m in METRICS)
ARBOR = {"morph": ("MORPH_STATISTICS", None), "skeleton": ("SKELETON_STATISTICS", None), "sholl": ("SHOLL_STATISTICS", "radius"),
         "branch": ("BRANCH_STATISTICS", "length")}
NOTE = "8 x 8 images are too small"


# ---------------------------------------------------------------------------------------------------------------------
# canned results
# ---------------------------------------------------------------------------------------------------------------------
def _arbor_rows(names, shift):
    return {name: {"ks": 0.125 * (i + 1) + shift, "real": 0.5 + i, "real_sem": 0.01 * (i + 1), "fake": 0.25 + i + shift,
                   "fake_sem": None if i == 0 else 0.02 + shift} for i, name in enumerate(names)}


def _arbor(ngan, name, kind, averaged):
    """(result, metric.active) of one evaluate_* call of an arbor metric; kinds: full, note (a side without a scored image),
    inactive (a stage the kernels do not take) and ema_note (full, but the averaged generator's side has no scored image)"""
    names, axis = getattr(ngan.metrics, ARBOR[name][0]), ARBOR[name][1]
    if kind == "inactive":
        return {"images": 0, "skipped_real": 0, "skipped_fake": 0, "note": NOTE}, False
    if kind == "note" or (kind == "ema_note" and averaged):
        return {"images": 6, "skipped_real": 0, "skipped_fake": 6, "note": "no scored image on the generated side"}, True
    out = {"images": 6, "skipped_real": 0, "skipped_fake": 2 if averaged else 1}
    out.update(_arbor_rows(names, 0.0625 if averaged else 0.0))
    if axis:      # the averaged generator's profile is one ring shorter than the data's: the entry pads it
        out["profile"] = {axis: [0.0, 0.125], "real": [0.0, 1.5], "fake": [0.5]} if averaged else \
            {axis: [0.0, 0.125, 0.25], "real": [0.0, 1.5, 0.75], "fake": [0.25, 1.0, 0.5]}
    return out, True


def canned(ngan, name, kind, averaged):
    """what the stub of metrics.evaluate_<name> returns: (result, metric or None)"""
    if name in ARBOR:
        res, active = _arbor(ngan, name, kind, averaged)
        return res, types.SimpleNamespace(active=active)
    full = kind == "full"
    if name == "swd":
        return ({"levels": [16], "swd": [2.25 if averaged else 1.5], "mean": 2.25 if averaged else 1.5} if full else
                {"levels": [], "swd": [], "mean": None, "note": NOTE}), None
    if name == "msssim":
        return ({"scales": 1, "weights": [1.0], "real": 0.125, "real_sem": 0.01, "pairs": 5, "fake": 0.75 if averaged else 0.5,
                 "fake_sem": 0.02} if full else
                {"scales": 0, "weights": [], "fake": None, "fake_sem": None, "real": None, "real_sem": None, "pairs": 0, "note": NOTE}), None
    assert name == "spectrum"
    if not full:
        return {"k": [], "real": [], "fake": [], "real_sem": [], "fake_sem": [], "ratio_db": [], "distance_db": None, "high_db": None,
                "skipped_bins": 0, "images": 0, "note": NOTE}, types.SimpleNamespace()
    return {"k": [0, 1, 2], "real": [1.0, 0.5, 0.25], "fake": [1.0, 0.25, 0.125], "real_sem": [None] * 3, "fake_sem": [None] * 3,
            "ratio_db": [0.0, -3.0, -3.0], "distance_db": 1.5 if averaged else 3.0, "high_db": None if averaged else -3.0,
            "skipped_bins": 0, "images": 6}, types.SimpleNamespace()


class Recorder:
    """a stand-in for metrics.evaluate_<name>: keeps (dataset, keyword arguments) of every call, with the data set and the metric of
    the first call spelt as strings so that the record compares against a literal"""

    def __init__(self, ngan, name, kind, events=None):
        self.ngan, self.name, self.kind, self.events = ngan, name, kind, events
        self.calls, self.metric, self.generators = [], None, []

    def __call__(self, generator, dataset=None, **kw):
        averaged = bool(self.calls)
        res, metric = canned(self.ngan, self.name, self.kind, averaged)
        if "real_from" in kw:
            kw["real_from"] = "METRIC" if kw["real_from"] is self.metric and self.metric is not None else kw["real_from"]
        self.calls.append((dataset, kw))
        self.generators.append(generator)
        if self.events is not None:
            self.events.append(self.name)
        if kw.get("return_metric"):
            self.metric = metric
            return res, metric
        return res


# ---------------------------------------------------------------------------------------------------------------------
# train.score_*
# ---------------------------------------------------------------------------------------------------------------------
class _Trainer:
    def __init__(self, ema):
        self.G = types.SimpleNamespace(image_size=16)
        self.ema_enabled, self.entered = ema, 0

    @contextlib.contextmanager
    def averaged_generator(self):
        self.entered += 1
        yield self.G


def score_cfg(**kw):
    base = dict(batch_size=4, swd_images=6, swd_seed=3, msssim_pairs=5, msssim_seed=4, spectrum_images=6, spectrum_seed=5,
                morph_images=6, morph_seed=6, morph_min_size=2, skeleton_images=6, skeleton_seed=7, skeleton_min_size=3,
                sholl_images=6, sholl_seed=8, sholl_min_size=4, branch_images=6, branch_seed=9, branch_min_size=5, branch_spur=0)
    base.update(kw)
    return types.SimpleNamespace(**base)


def run_score(ngan, monkeypatch, name, kind, ema, cfg=None):
    """(log lines, entry, calls of the evaluate, entries of averaged_generator(), names of the lists that grew)"""
    _, scorer, evaluate, _, key, _ = next(m for m in METRICS if m[0] == name)
    rec = Recorder(ngan, name, kind)
    monkeypatch.setattr(ngan.metrics, evaluate, rec)
    trainer, lines = _Trainer(ema), []
    ck = types.SimpleNamespace(**{k: [] for k in KEYS})
    entry = getattr(ngan.train, scorer)(trainer, "DATASET", cfg or score_cfg(), 12, checkpoint=ck, log=lines.append)
    assert getattr(ck, key) == [entry] and getattr(ck, key)[0] is entry
    assert all(g is trainer.G for g in rec.generators)
    return lines, entry, rec.calls, trainer.entered, [k for k in KEYS if getattr(ck, k)]


SCORE_CASES = [(name, kind, ema) for name, *_ in METRICS for kind in (("full", "note", "inactive", "ema_note") if name in ARBOR
                                                                      else ("full", "inactive")) for ema in (False, True)]


@pytest.mark.parametrize("name,kind,ema", SCORE_CASES, ids=["-".join((n, k, "ema" if e else "plain")) for n, k, e in SCORE_CASES])
def test_score_logs_stores_and_calls(ngan, monkeypatch, name, kind, ema):
    lines, entry, calls, entered, grown = run_score(ngan, monkeypatch, name, kind, ema)
    want = SCORED[name, kind, ema]
    assert lines == [want["line"]]
    assert entry == want["entry"] and list(entry) == list(want["entry"])
    assert [list(v) for v in entry.values() if isinstance(v, dict)] == [list(v) for v in want["entry"].values() if isinstance(v, dict)]
    assert calls == want["calls"]
    assert entered == len(calls) - 1 and len(calls) == want["passes"]
    assert grown == [next(m[4] for m in METRICS if m[0] == name)]
    if len(calls) == 2:                                                   # the averaged pass
        dataset, kw = calls[1]
        assert (dataset is None) == (name != "swd")
        assert name in ("swd", "msssim") or kw["real_from"] == "METRIC"


def test_score_without_a_checkpoint_and_with_a_given_spur(ngan, monkeypatch):
    rec = Recorder(ngan, "branch", "full")
    monkeypatch.setattr(ngan.metrics, "evaluate_branches", rec)
    lines = []
    entry = ngan.train.score_branches(_Trainer(False), "DATASET", score_cfg(branch_spur=7), 3, log=lines.append)
    assert entry["spur"] == 7 and rec.calls[0][1]["spur"] == 7 and ", spur 7: " in lines[0]
    rec = Recorder(ngan, "swd", "full")
    monkeypatch.setattr(ngan.metrics, "evaluate_swd", rec)
    ngan.train.score_swd(_Trainer(False), "DATASET", types.SimpleNamespace(batch_size=2), 3, log=lines.append)    # the defaults
    assert rec.calls == [("DATASET", {"n_images": 8192, "batch_size": 2, "seed": 0})]
    rec = Recorder(ngan, "msssim", "full")
    monkeypatch.setattr(ngan.metrics, "evaluate_msssim", rec)
    ngan.train.score_msssim(_Trainer(False), "DATASET", types.SimpleNamespace(batch_size=2), 3, log=lines.append)
    assert rec.calls == [("DATASET", {"n_pairs": 10000, "batch_size": 2, "seed": 0})]


# ---------------------------------------------------------------------------------------------------------------------
# pggan_train
# ---------------------------------------------------------------------------------------------------------------------
def test_the_epoch_driver_scores_by_period_before_it_saves(ngan, monkeypatch):
    events = []
    for name, _, evaluate, *_ in METRICS:
        monkeypatch.setattr(ngan.metrics, evaluate, Recorder(ngan, name, "inactive", events))

    class Checkpoint(StubCheckpoint):
        def __init__(self, n):
            super().__init__(n)
            for k in KEYS:
                setattr(self, k, [])

        def save_state(self, epoch):
            super().save_state(epoch)
            events.append(("save", epoch))

    cfg = _cfg(swd_period=2, msssim_period=0, spectrum_period=0, morph_period=4, skeleton_period=0, sholl_period=0, branch_period=1)
    ck = Checkpoint(cfg.N_epochs)
    ngan.train.pggan_train(StubTrainer(2), _dataset(ngan, 8), cfg, checkpoint=ck, use_graph=False, log=lambda *a: None)
    assert events == ["swd", "branch", ("save", 2), "swd", "morph", "branch", ("save", 4)]
    assert [[e["epoch"] for e in getattr(ck, k)] for k in KEYS] == [[2, 4], [], [], [4], [], [], [2, 4]]


# ---------------------------------------------------------------------------------------------------------------------
# eval.main
# ---------------------------------------------------------------------------------------------------------------------
class _EvalStubs:
    def __init__(self, ngan, monkeypatch, tmp_path):
        self.events, self.evaluates = [], {}
        monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
        monkeypatch.setattr(ngan.models.Generator_PG, "from_state_dict", self.from_state_dict)
        monkeypatch.setattr(ngan.eval, "load_dataset", lambda options, config, device: self.events.append("load_dataset") or "DATASET")
        monkeypatch.setattr(ngan.utils, "plot_gen_samples", lambda G, **kw: self.events.append(("grid", G.use_ema, kw["N_images"])))
        for name, _, evaluate, fmt, *_ in METRICS:
            self.evaluates[name] = Recorder(ngan, name, "inactive", self.events)
            monkeypatch.setattr(ngan.metrics, evaluate, self.evaluates[name])
            monkeypatch.setattr(ngan.metrics, fmt, lambda res, title, name=name: "[{}] {}".format(name, title))
        self.weights = tmp_path / "GenDisc_x.pth"
        self.weights.write_bytes(b"")

    def from_state_dict(self, filename, device=None, use_ema=False, verbose=True):
        assert filename == str(self.weights) and device == torch.device("cuda")
        self.events.append(("G", use_ema))
        G = types.SimpleNamespace(use_ema=use_ema)
        G.to = lambda device: G
        return G

    def argv(self, *flags):
        return ["-weights", str(self.weights), *flags]


def test_eval_runs_every_requested_metric_in_table_order(ngan, monkeypatch, tmp_path, capsys):
    s = _EvalStubs(ngan, monkeypatch, tmp_path)
    argv = s.argv("--branches", "9", "--sholl", "8", "--skeleton", "7", "--morph", "6", "--spectrum", "5", "--msssim", "4", "--swd", "3",
                  "--ema", "--dataset_dir", "d", "--swd_seed", "11", "--msssim_seed", "12", "--spectrum_seed", "13", "--morph_seed", "14",
                  "--skeleton_seed", "15", "--sholl_seed", "16", "--branch_seed", "17", "--morph_min_size", "2", "--skeleton_min_size",
                  "3", "--sholl_min_size", "4", "--branch_min_size", "5", "--branch_spur", "6")
    assert ngan.eval.main(argv) == 0
    per_metric = lambda name: ["load_dataset", ("G", False), name, ("G", True), name]   # noqa: E731
    assert s.events == [e for name, *_ in METRICS for e in per_metric(name)]                # (and no grid)
    assert {name: rec.calls for name, rec in s.evaluates.items()} == {
        "swd": [("DATASET", {"n_images": 3, "batch_size": 3, "seed": 11})] * 2,
        "msssim": [("DATASET", {"n_pairs": 4, "batch_size": 4, "seed": 12})] * 2,
        "spectrum": [("DATASET", {"n_images": 5, "batch_size": 5, "seed": 13})] * 2,
        "morph": [("DATASET", {"n_images": 6, "batch_size": 6, "seed": 14, "min_size": 2})] * 2,
        "skeleton": [("DATASET", {"n_images": 7, "batch_size": 7, "seed": 15, "min_size": 3})] * 2,
        "sholl": [("DATASET", {"n_images": 8, "batch_size": 8, "seed": 16, "min_size": 4})] * 2,
        "branch": [("DATASET", {"n_images": 9, "batch_size": 9, "seed": 17, "min_size": 5, "spur": 6})] * 2}
    w = str(s.weights)
    assert capsys.readouterr().out.splitlines() == [
        f"[swd] SWD x 1e3, training generator of {w} against 3 images", f"[swd] SWD x 1e3, averaged generator of {w} against 3 images",
        f"[msssim] MS-SSIM between pairs, training generator of {w}", f"[msssim] MS-SSIM between pairs, averaged generator of {w}",
        f"[spectrum] Radial power spectrum, training generator of {w}", f"[spectrum] Radial power spectrum, averaged generator of {w}",
        f"[morph] Arbor morphology, training generator of {w}", f"[morph] Arbor morphology, averaged generator of {w}",
        f"[skeleton] Arbor skeleton, training generator of {w}", f"[skeleton] Arbor skeleton, averaged generator of {w}",
        f"[sholl] Arbor geometry, training generator of {w}", f"[sholl] Arbor geometry, averaged generator of {w}",
        f"[branch] Arbor branches, training generator of {w}", f"[branch] Arbor branches, averaged generator of {w}"]


def test_eval_runs_one_metric_alone_or_the_grid(ngan, monkeypatch, tmp_path, capsys):
    s = _EvalStubs(ngan, monkeypatch, tmp_path)
    assert ngan.eval.main(s.argv("--sholl", "40", "--dataset_dir", "d")) == 0
    assert s.events == ["load_dataset", ("G", False), "sholl"]
    assert s.evaluates["sholl"].calls == [("DATASET", {"n_images": 40, "batch_size": 32, "seed": 0, "min_size": 1})]
    assert capsys.readouterr().out == f"[sholl] Arbor geometry, training generator of {s.weights}\n"
    del s.events[:]
    assert ngan.eval.main(s.argv("--branches", "--dataset_dir", "d")) == 0               # no --branch_spur: the metric's default
    assert s.events == ["load_dataset", ("G", False), "branch"]
    assert s.evaluates["branch"].calls == [("DATASET", {"n_images": 8192, "batch_size": 32, "seed": 0, "min_size": 1, "spur": None})]
    del s.events[:]
    assert ngan.eval.main(s.argv("--msssim")) == 0                                         # MS-SSIM alone needs no data set
    named = os.path.exists(ngan.config.dataset_dir)
    assert s.events == (["load_dataset"] if named else []) + [("G", False), "msssim"]
    assert s.evaluates["msssim"].calls == [("DATASET" if named else None, {"n_pairs": 10000, "batch_size": 32, "seed": 0})]
    del s.events[:]
    capsys.readouterr()
    assert ngan.eval.main(s.argv("-n", "9", "--ema", "-output", str(tmp_path / "grid.png"))) == 0
    assert s.events == [("G", True), ("grid", True, 9)] and capsys.readouterr().out == ""


@pytest.mark.parametrize("flags,match", [(("--msssim", "0"), "--msssim"), (("--spectrum", "0"), "--spectrum"), (("--swd", "0"), "--swd"),
                                         (("--morph", "8", "--morph_min_size", "0"), "--morph_min_size"), (("--morph", "0"), "--morph"),
                                         (("--skeleton", "8", "--skeleton_min_size", "0"), "--skeleton_min_size"),
                                         (("--sholl", "8", "--sholl_min_size", "0"), "--sholl_min_size"),
                                         (("--branches", "8", "--branch_min_size", "0"), "--branch_min_size"),
                                         (("--branches", "8", "--branch_spur", "-1"), "--branch_spur")])
def test_eval_refuses_counts_and_sizes_below_their_lowest(ngan, monkeypatch, tmp_path, flags, match):
    s = _EvalStubs(ngan, monkeypatch, tmp_path)
    with pytest.raises(ValueError, match=match):
        ngan.eval.main(s.argv(*flags, "--dataset_dir", "d"))
    assert not any(e in dict.fromkeys(m[0] for m in METRICS) for e in s.events)           # nothing was scored
    ngan.eval.main(s.argv("--morph", "8", "--skeleton_min_size", "0", "--branch_spur", "-1", "--dataset_dir", "d"))   # switches not given


# ---------------------------------------------------------------------------------------------------------------------
# Checkpointer
# ---------------------------------------------------------------------------------------------------------------------
def test_checkpoint_keys_keep_their_order_and_lists_stay_apart(ngan, tmp_path):
    utils = ngan.utils
    assert tuple(getattr(utils, k + "_KEY") for k in KEYS) == KEYS
    torch.manual_seed(1)
    G = ngan.models.Generator_PG([16, 16, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 16, 16], image_size_init=4)
    f = str(tmp_path / "GenDisc_s.pth")
    ck = utils.Checkpointer(G, D, 1e-4, f, N_epochs=10, verbose=False)
    assert all(getattr(ck, k) == [] for k in KEYS) and len({id(getattr(ck, k)) for k in KEYS}) == 7
    for i, k in reversed(list(enumerate(KEYS))):                          # filled in another order than they are written in
        getattr(ck, k).extend([{"epoch": 2, "image_size": 16, "which": k, "nested": {"fake": [0.5, i]}}, {"epoch": 4, "note": k}])
    ck.save_state(4)
    saved = utils.load_checkpoint_dict(f)
    assert list(saved) == ["epoch", "Generator_state", "Generator_attrs", "Discriminator_state", "Discriminator_attrs", "lr", "Loss_real",
                           "Loss_fake", "Loss_G", "Loss_D", "SWD", "MSSSIM", "SPECTRUM", "MORPH", "SKELETON", "SHOLL", "BRANCH"]
    ck.MORPH.clear()
    ck.save_state(5)
    assert list(utils.load_checkpoint_dict(f))[10:] == ["SWD", "MSSSIM", "SPECTRUM", "SKELETON", "SHOLL", "BRANCH"]   # empty: omitted
    ck2 = utils.Checkpointer(G, D, 1e-4, f, N_epochs=10, verbose=False)
    ck2.load_state()
    assert len({id(getattr(ck2, k)) for k in KEYS}) == 7
    for k in KEYS:
        mine, theirs = getattr(ck, k), getattr(ck2, k)
        assert theirs == mine and theirs is not mine and (k == "MORPH" or theirs == saved[k])
        assert all(a is not b for a, b in zip(mine, theirs))
        assert [list(e) for e in theirs] == [list(e) for e in mine]


# ---------------------------------------------------------------------------------------------------------------------
# the arbor tables
# ---------------------------------------------------------------------------------------------------------------------
def table_result(ngan, name, case):
    res, _ = _arbor(ngan, name, "note" if case == "note" else "full", False)
    if case == "no_sem":
        for row in res.values():
            if isinstance(row, dict) and "real_sem" in row:
                row["real_sem"] = None
    if case == "empty_profile" and "profile" in res:
        res["profile"] = {k: [] for k in res["profile"]}
    return res


TABLE_CASES = [(name, case) for name in ARBOR for case in ("profile", "empty_profile", "no_sem", "note")
               if not (case == "empty_profile" and ARBOR[name][1] is None)]


@pytest.mark.parametrize("name,case", TABLE_CASES, ids=["-".join(c) for c in TABLE_CASES])
def test_arbor_tables(ngan, name, case):
    fmt = getattr(ngan.metrics, next(m[3] for m in METRICS if m[0] == name))
    assert fmt(table_result(ngan, name, case), "Title of " + name) == TABLES[name, case]
    if case == "profile":
        default = fmt(table_result(ngan, name, case))
        assert default.split(" (")[0] == {"morph": "Arbor morphology", "skeleton": "Arbor skeleton", "sholl": "Arbor geometry",
                                          "branch": "Arbor branches"}[name]
        assert default.split(" (", 1)[1] == TABLES[name, case].split(" (", 1)[1]


# ---------------------------------------------------------------------------------------------------------------------
# expected values: recorded from the code as it stood before the seven copies were folded into one table
# ---------------------------------------------------------------------------------------------------------------------
SCORED = {('swd', 'full', False): {'line': 'Epoch:12, SWD x1e3 at [16]: [1.500]',
                          'entry': {'epoch': 12, 'image_size': 16, 'levels': [16], 'swd': [1.5], 'swd_ema': None},
                          'calls': [('DATASET', {'n_images': 6, 'batch_size': 4, 'seed': 3})],
                          'passes': 1},
 ('swd', 'full', True): {'line': 'Epoch:12, SWD x1e3 at [16]: [1.500], averaged generator: [2.250]',
                         'entry': {'epoch': 12, 'image_size': 16, 'levels': [16], 'swd': [1.5], 'swd_ema': [2.25]},
                         'calls': [('DATASET', {'n_images': 6, 'batch_size': 4, 'seed': 3}), ('DATASET', {'n_images': 6, 'batch_size': 4, 'seed': 3})],
                         'passes': 2},
 ('swd', 'inactive', False): {'line': 'Epoch:12, SWD: 8 x 8 images are too small',
                              'entry': {'epoch': 12, 'image_size': 16, 'levels': [], 'swd': [], 'swd_ema': None},
                              'calls': [('DATASET', {'n_images': 6, 'batch_size': 4, 'seed': 3})],
                              'passes': 1},
 ('swd', 'inactive', True): {'line': 'Epoch:12, SWD: 8 x 8 images are too small',
                             'entry': {'epoch': 12, 'image_size': 16, 'levels': [], 'swd': [], 'swd_ema': []},
                             'calls': [('DATASET', {'n_images': 6, 'batch_size': 4, 'seed': 3}), ('DATASET', {'n_images': 6, 'batch_size': 4, 'seed': 3})],
                             'passes': 2},
 ('msssim', 'full', False): {'line': 'Epoch:12, MS-SSIM over 5 pairs, 1 scales: generated 0.50000, data 0.12500',
                             'entry': {'epoch': 12, 'image_size': 16, 'scales': 1, 'fake': 0.5, 'fake_ema': None, 'real': 0.125, 'pairs': 5},
                             'calls': [('DATASET', {'n_pairs': 5, 'batch_size': 4, 'seed': 4})],
                             'passes': 1},
 ('msssim', 'full', True): {'line': 'Epoch:12, MS-SSIM over 5 pairs, 1 scales: generated 0.50000, averaged generator 0.75000, data 0.12500',
                            'entry': {'epoch': 12, 'image_size': 16, 'scales': 1, 'fake': 0.5, 'fake_ema': 0.75, 'real': 0.125, 'pairs': 5},
                            'calls': [('DATASET', {'n_pairs': 5, 'batch_size': 4, 'seed': 4}), (None, {'n_pairs': 5, 'batch_size': 4, 'seed': 4})],
                            'passes': 2},
 ('msssim', 'inactive', False): {'line': 'Epoch:12, MS-SSIM: 8 x 8 images are too small',
                                 'entry': {'epoch': 12, 'image_size': 16, 'scales': 0, 'fake': None, 'fake_ema': None, 'real': None, 'pairs': 0},
                                 'calls': [('DATASET', {'n_pairs': 5, 'batch_size': 4, 'seed': 4})],
                                 'passes': 1},
 ('msssim', 'inactive', True): {'line': 'Epoch:12, MS-SSIM: 8 x 8 images are too small',
                                'entry': {'epoch': 12, 'image_size': 16, 'scales': 0, 'fake': None, 'fake_ema': None, 'real': None, 'pairs': 0},
                                'calls': [('DATASET', {'n_pairs': 5, 'batch_size': 4, 'seed': 4})],
                                'passes': 1},
 ('spectrum', 'full', False): {'line': 'Epoch:12, spectrum over 6 images: distance +3.00 dB, top octave -3.00 dB',
                               'entry': {'epoch': 12,
                                         'image_size': 16,
                                         'images': 6,
                                         'k': [0, 1, 2],
                                         'real': [1.0, 0.5, 0.25],
                                         'fake': [1.0, 0.25, 0.125],
                                         'ratio_db': [0.0, -3.0, -3.0],
                                         'distance_db': 3.0,
                                         'high_db': -3.0},
                               'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 5})],
                               'passes': 1},
 ('spectrum', 'full', True): {'line': 'Epoch:12, spectrum over 6 images: distance +3.00 dB, top octave -3.00 dB, averaged generator: distance +1.50 dB, top '
                                      'octave -',
                              'entry': {'epoch': 12,
                                        'image_size': 16,
                                        'images': 6,
                                        'k': [0, 1, 2],
                                        'real': [1.0, 0.5, 0.25],
                                        'fake': [1.0, 0.25, 0.125],
                                        'ratio_db': [0.0, -3.0, -3.0],
                                        'distance_db': 3.0,
                                        'high_db': -3.0,
                                        'distance_db_ema': 1.5,
                                        'high_db_ema': None},
                              'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 5}),
                                        (None, {'real_from': 'METRIC', 'n_images': 6, 'batch_size': 4, 'seed': 5})],
                              'passes': 2},
 ('spectrum', 'inactive', False): {'line': 'Epoch:12, spectrum: 8 x 8 images are too small',
                                   'entry': {'epoch': 12,
                                             'image_size': 16,
                                             'images': 0,
                                             'k': [],
                                             'real': [],
                                             'fake': [],
                                             'ratio_db': [],
                                             'distance_db': None,
                                             'high_db': None},
                                   'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 5})],
                                   'passes': 1},
 ('spectrum', 'inactive', True): {'line': 'Epoch:12, spectrum: 8 x 8 images are too small',
                                  'entry': {'epoch': 12,
                                            'image_size': 16,
                                            'images': 0,
                                            'k': [],
                                            'real': [],
                                            'fake': [],
                                            'ratio_db': [],
                                            'distance_db': None,
                                            'high_db': None},
                                  'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 5})],
                                  'passes': 1},
 ('morph', 'full', False): {'line': 'Epoch:12, morphology over 6 images: components 1.25, largest share 2.250 (KS 0.375), fill 0.2500, dimension 3.250; data: '
                                    'components 1.50, largest share 2.500, fill 0.5000, dimension 3.500',
                            'entry': {'epoch': 12,
                                      'image_size': 16,
                                      'min_size': 2,
                                      'images': 6,
                                      'skipped_real': 0,
                                      'skipped_fake': 1,
                                      'fill': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                      'components': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                      'largest_share': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                      'dimension': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02}},
                            'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 6, 'min_size': 2})],
                            'passes': 1},
 ('morph', 'full', True): {'line': 'Epoch:12, morphology over 6 images: components 1.25, largest share 2.250 (KS 0.375), fill 0.2500, dimension 3.250; data: '
                                   'components 1.50, largest share 2.500, fill 0.5000, dimension 3.500; averaged generator: components 1.31, largest share '
                                   '2.312 (KS 0.438), fill 0.3125, dimension 3.312',
                           'entry': {'epoch': 12,
                                     'image_size': 16,
                                     'min_size': 2,
                                     'images': 6,
                                     'skipped_real': 0,
                                     'skipped_fake': 1,
                                     'fill': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                     'components': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                     'largest_share': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                     'dimension': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02},
                                     'skipped_fake_ema': 2,
                                     'fill_ema': {'fake': 0.3125, 'fake_sem': None, 'ks': 0.1875},
                                     'components_ema': {'fake': 1.3125, 'fake_sem': 0.0825, 'ks': 0.3125},
                                     'largest_share_ema': {'fake': 2.3125, 'fake_sem': 0.0825, 'ks': 0.4375},
                                     'dimension_ema': {'fake': 3.3125, 'fake_sem': 0.0825, 'ks': 0.5625}},
                           'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 6, 'min_size': 2}),
                                     (None, {'real_from': 'METRIC', 'n_images': 6, 'batch_size': 4, 'seed': 6, 'min_size': 2})],
                           'passes': 2},
 ('morph', 'note', False): {'line': 'Epoch:12, morphology: no scored image on the generated side',
                            'entry': {'epoch': 12,
                                      'image_size': 16,
                                      'min_size': 2,
                                      'images': 6,
                                      'skipped_real': 0,
                                      'skipped_fake': 6,
                                      'note': 'no scored image on the generated side'},
                            'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 6, 'min_size': 2})],
                            'passes': 1},
 ('morph', 'note', True): {'line': 'Epoch:12, morphology: no scored image on the generated side',
                           'entry': {'epoch': 12,
                                     'image_size': 16,
                                     'min_size': 2,
                                     'images': 6,
                                     'skipped_real': 0,
                                     'skipped_fake': 6,
                                     'note': 'no scored image on the generated side',
                                     'skipped_fake_ema': 6},
                           'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 6, 'min_size': 2}),
                                     (None, {'real_from': 'METRIC', 'n_images': 6, 'batch_size': 4, 'seed': 6, 'min_size': 2})],
                           'passes': 2},
 ('morph', 'inactive', False): {'line': 'Epoch:12, morphology: 8 x 8 images are too small',
                                'entry': {'epoch': 12,
                                          'image_size': 16,
                                          'min_size': 2,
                                          'images': 0,
                                          'skipped_real': 0,
                                          'skipped_fake': 0,
                                          'note': '8 x 8 images are too small'},
                                'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 6, 'min_size': 2})],
                                'passes': 1},
 ('morph', 'inactive', True): {'line': 'Epoch:12, morphology: 8 x 8 images are too small',
                               'entry': {'epoch': 12,
                                         'image_size': 16,
                                         'min_size': 2,
                                         'images': 0,
                                         'skipped_real': 0,
                                         'skipped_fake': 0,
                                         'note': '8 x 8 images are too small'},
                               'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 6, 'min_size': 2})],
                               'passes': 1},
 ('morph', 'ema_note', False): {'line': 'Epoch:12, morphology over 6 images: components 1.25, largest share 2.250 (KS 0.375), fill 0.2500, dimension 3.250; '
                                        'data: components 1.50, largest share 2.500, fill 0.5000, dimension 3.500',
                                'entry': {'epoch': 12,
                                          'image_size': 16,
                                          'min_size': 2,
                                          'images': 6,
                                          'skipped_real': 0,
                                          'skipped_fake': 1,
                                          'fill': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                          'components': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                          'largest_share': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                          'dimension': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02}},
                                'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 6, 'min_size': 2})],
                                'passes': 1},
 ('morph', 'ema_note', True): {'line': 'Epoch:12, morphology over 6 images: components 1.25, largest share 2.250 (KS 0.375), fill 0.2500, dimension 3.250; '
                                       'data: components 1.50, largest share 2.500, fill 0.5000, dimension 3.500',
                               'entry': {'epoch': 12,
                                         'image_size': 16,
                                         'min_size': 2,
                                         'images': 6,
                                         'skipped_real': 0,
                                         'skipped_fake': 1,
                                         'fill': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                         'components': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                         'largest_share': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                         'dimension': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02},
                                         'skipped_fake_ema': 6},
                               'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 6, 'min_size': 2}),
                                         (None, {'real_from': 'METRIC', 'n_images': 6, 'batch_size': 4, 'seed': 6, 'min_size': 2})],
                               'passes': 2},
 ('skeleton', 'full', False): {'line': 'Epoch:12, skeleton over 6 images: length 0.250, tips 1.25 (KS 0.250), junctions 2.25, width 3.250; data: length 0.500, '
                                       'tips 1.50, junctions 2.50, width 3.500',
                               'entry': {'epoch': 12,
                                         'image_size': 16,
                                         'min_size': 3,
                                         'images': 6,
                                         'skipped_real': 0,
                                         'skipped_fake': 1,
                                         'length': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                         'tips': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                         'junctions': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                         'width': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02}},
                               'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 7, 'min_size': 3})],
                               'passes': 1},
 ('skeleton', 'full', True): {'line': 'Epoch:12, skeleton over 6 images: length 0.250, tips 1.25 (KS 0.250), junctions 2.25, width 3.250; data: length 0.500, '
                                      'tips 1.50, junctions 2.50, width 3.500; averaged generator: length 0.312, tips 1.31 (KS 0.312), junctions 2.31, width '
                                      '3.312',
                              'entry': {'epoch': 12,
                                        'image_size': 16,
                                        'min_size': 3,
                                        'images': 6,
                                        'skipped_real': 0,
                                        'skipped_fake': 1,
                                        'length': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                        'tips': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                        'junctions': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                        'width': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02},
                                        'skipped_fake_ema': 2,
                                        'length_ema': {'fake': 0.3125, 'fake_sem': None, 'ks': 0.1875},
                                        'tips_ema': {'fake': 1.3125, 'fake_sem': 0.0825, 'ks': 0.3125},
                                        'junctions_ema': {'fake': 2.3125, 'fake_sem': 0.0825, 'ks': 0.4375},
                                        'width_ema': {'fake': 3.3125, 'fake_sem': 0.0825, 'ks': 0.5625}},
                              'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 7, 'min_size': 3}),
                                        (None, {'real_from': 'METRIC', 'n_images': 6, 'batch_size': 4, 'seed': 7, 'min_size': 3})],
                              'passes': 2},
 ('skeleton', 'note', False): {'line': 'Epoch:12, skeleton: no scored image on the generated side',
                               'entry': {'epoch': 12,
                                         'image_size': 16,
                                         'min_size': 3,
                                         'images': 6,
                                         'skipped_real': 0,
                                         'skipped_fake': 6,
                                         'note': 'no scored image on the generated side'},
                               'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 7, 'min_size': 3})],
                               'passes': 1},
 ('skeleton', 'note', True): {'line': 'Epoch:12, skeleton: no scored image on the generated side',
                              'entry': {'epoch': 12,
                                        'image_size': 16,
                                        'min_size': 3,
                                        'images': 6,
                                        'skipped_real': 0,
                                        'skipped_fake': 6,
                                        'note': 'no scored image on the generated side',
                                        'skipped_fake_ema': 6},
                              'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 7, 'min_size': 3}),
                                        (None, {'real_from': 'METRIC', 'n_images': 6, 'batch_size': 4, 'seed': 7, 'min_size': 3})],
                              'passes': 2},
 ('skeleton', 'inactive', False): {'line': 'Epoch:12, skeleton: 8 x 8 images are too small',
                                   'entry': {'epoch': 12,
                                             'image_size': 16,
                                             'min_size': 3,
                                             'images': 0,
                                             'skipped_real': 0,
                                             'skipped_fake': 0,
                                             'note': '8 x 8 images are too small'},
                                   'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 7, 'min_size': 3})],
                                   'passes': 1},
 ('skeleton', 'inactive', True): {'line': 'Epoch:12, skeleton: 8 x 8 images are too small',
                                  'entry': {'epoch': 12,
                                            'image_size': 16,
                                            'min_size': 3,
                                            'images': 0,
                                            'skipped_real': 0,
                                            'skipped_fake': 0,
                                            'note': '8 x 8 images are too small'},
                                  'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 7, 'min_size': 3})],
                                  'passes': 1},
 ('skeleton', 'ema_note', False): {'line': 'Epoch:12, skeleton over 6 images: length 0.250, tips 1.25 (KS 0.250), junctions 2.25, width 3.250; data: length '
                                           '0.500, tips 1.50, junctions 2.50, width 3.500',
                                   'entry': {'epoch': 12,
                                             'image_size': 16,
                                             'min_size': 3,
                                             'images': 6,
                                             'skipped_real': 0,
                                             'skipped_fake': 1,
                                             'length': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                             'tips': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                             'junctions': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                             'width': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02}},
                                   'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 7, 'min_size': 3})],
                                   'passes': 1},
 ('skeleton', 'ema_note', True): {'line': 'Epoch:12, skeleton over 6 images: length 0.250, tips 1.25 (KS 0.250), junctions 2.25, width 3.250; data: length '
                                          '0.500, tips 1.50, junctions 2.50, width 3.500',
                                  'entry': {'epoch': 12,
                                            'image_size': 16,
                                            'min_size': 3,
                                            'images': 6,
                                            'skipped_real': 0,
                                            'skipped_fake': 1,
                                            'length': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                            'tips': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                            'junctions': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                            'width': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02},
                                            'skipped_fake_ema': 6},
                                  'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 7, 'min_size': 3}),
                                            (None, {'real_from': 'METRIC', 'n_images': 6, 'batch_size': 4, 'seed': 7, 'min_size': 3})],
                                  'passes': 2},
 ('sholl', 'full', False): {'line': 'Epoch:12, sholl over 6 images: calibre 0.250 (KS 0.125), soma 1.25, peak 2.25 at 3.250, reach 4.250 (KS 0.625); data: '
                                    'calibre 0.500, soma 1.50, peak 2.50 at 3.500, reach 4.500',
                            'entry': {'epoch': 12,
                                      'image_size': 16,
                                      'min_size': 4,
                                      'images': 6,
                                      'skipped_real': 0,
                                      'skipped_fake': 1,
                                      'calibre': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                      'soma': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                      'sholl_peak': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                      'sholl_radius': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02},
                                      'reach': {'ks': 0.625, 'real': 4.5, 'real_sem': 0.05, 'fake': 4.25, 'fake_sem': 0.02},
                                      'profile': {'radius': [0.0, 0.125, 0.25], 'real': [0.0, 1.5, 0.75], 'fake': [0.25, 1.0, 0.5]}},
                            'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 8, 'min_size': 4})],
                            'passes': 1},
 ('sholl', 'full', True): {'line': 'Epoch:12, sholl over 6 images: calibre 0.250 (KS 0.125), soma 1.25, peak 2.25 at 3.250, reach 4.250 (KS 0.625); data: '
                                   'calibre 0.500, soma 1.50, peak 2.50 at 3.500, reach 4.500; averaged generator: calibre 0.312 (KS 0.188), soma 1.31, peak '
                                   '2.31 at 3.312, reach 4.312 (KS 0.688)',
                           'entry': {'epoch': 12,
                                     'image_size': 16,
                                     'min_size': 4,
                                     'images': 6,
                                     'skipped_real': 0,
                                     'skipped_fake': 1,
                                     'calibre': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                     'soma': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                     'sholl_peak': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                     'sholl_radius': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02},
                                     'reach': {'ks': 0.625, 'real': 4.5, 'real_sem': 0.05, 'fake': 4.25, 'fake_sem': 0.02},
                                     'profile': {'radius': [0.0, 0.125, 0.25], 'real': [0.0, 1.5, 0.75], 'fake': [0.25, 1.0, 0.5]},
                                     'skipped_fake_ema': 2,
                                     'calibre_ema': {'fake': 0.3125, 'fake_sem': None, 'ks': 0.1875},
                                     'soma_ema': {'fake': 1.3125, 'fake_sem': 0.0825, 'ks': 0.3125},
                                     'sholl_peak_ema': {'fake': 2.3125, 'fake_sem': 0.0825, 'ks': 0.4375},
                                     'sholl_radius_ema': {'fake': 3.3125, 'fake_sem': 0.0825, 'ks': 0.5625},
                                     'reach_ema': {'fake': 4.3125, 'fake_sem': 0.0825, 'ks': 0.6875},
                                     'profile_ema': {'fake': [0.5, 0.0, 0.0]}},
                           'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 8, 'min_size': 4}),
                                     (None, {'real_from': 'METRIC', 'n_images': 6, 'batch_size': 4, 'seed': 8, 'min_size': 4})],
                           'passes': 2},
 ('sholl', 'note', False): {'line': 'Epoch:12, sholl: no scored image on the generated side',
                            'entry': {'epoch': 12,
                                      'image_size': 16,
                                      'min_size': 4,
                                      'images': 6,
                                      'skipped_real': 0,
                                      'skipped_fake': 6,
                                      'note': 'no scored image on the generated side'},
                            'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 8, 'min_size': 4})],
                            'passes': 1},
 ('sholl', 'note', True): {'line': 'Epoch:12, sholl: no scored image on the generated side',
                           'entry': {'epoch': 12,
                                     'image_size': 16,
                                     'min_size': 4,
                                     'images': 6,
                                     'skipped_real': 0,
                                     'skipped_fake': 6,
                                     'note': 'no scored image on the generated side',
                                     'skipped_fake_ema': 6},
                           'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 8, 'min_size': 4}),
                                     (None, {'real_from': 'METRIC', 'n_images': 6, 'batch_size': 4, 'seed': 8, 'min_size': 4})],
                           'passes': 2},
 ('sholl', 'inactive', False): {'line': 'Epoch:12, sholl: 8 x 8 images are too small',
                                'entry': {'epoch': 12,
                                          'image_size': 16,
                                          'min_size': 4,
                                          'images': 0,
                                          'skipped_real': 0,
                                          'skipped_fake': 0,
                                          'note': '8 x 8 images are too small'},
                                'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 8, 'min_size': 4})],
                                'passes': 1},
 ('sholl', 'inactive', True): {'line': 'Epoch:12, sholl: 8 x 8 images are too small',
                               'entry': {'epoch': 12,
                                         'image_size': 16,
                                         'min_size': 4,
                                         'images': 0,
                                         'skipped_real': 0,
                                         'skipped_fake': 0,
                                         'note': '8 x 8 images are too small'},
                               'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 8, 'min_size': 4})],
                               'passes': 1},
 ('sholl', 'ema_note', False): {'line': 'Epoch:12, sholl over 6 images: calibre 0.250 (KS 0.125), soma 1.25, peak 2.25 at 3.250, reach 4.250 (KS 0.625); data: '
                                        'calibre 0.500, soma 1.50, peak 2.50 at 3.500, reach 4.500',
                                'entry': {'epoch': 12,
                                          'image_size': 16,
                                          'min_size': 4,
                                          'images': 6,
                                          'skipped_real': 0,
                                          'skipped_fake': 1,
                                          'calibre': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                          'soma': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                          'sholl_peak': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                          'sholl_radius': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02},
                                          'reach': {'ks': 0.625, 'real': 4.5, 'real_sem': 0.05, 'fake': 4.25, 'fake_sem': 0.02},
                                          'profile': {'radius': [0.0, 0.125, 0.25], 'real': [0.0, 1.5, 0.75], 'fake': [0.25, 1.0, 0.5]}},
                                'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 8, 'min_size': 4})],
                                'passes': 1},
 ('sholl', 'ema_note', True): {'line': 'Epoch:12, sholl over 6 images: calibre 0.250 (KS 0.125), soma 1.25, peak 2.25 at 3.250, reach 4.250 (KS 0.625); data: '
                                       'calibre 0.500, soma 1.50, peak 2.50 at 3.500, reach 4.500',
                               'entry': {'epoch': 12,
                                         'image_size': 16,
                                         'min_size': 4,
                                         'images': 6,
                                         'skipped_real': 0,
                                         'skipped_fake': 1,
                                         'calibre': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                         'soma': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                         'sholl_peak': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                         'sholl_radius': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02},
                                         'reach': {'ks': 0.625, 'real': 4.5, 'real_sem': 0.05, 'fake': 4.25, 'fake_sem': 0.02},
                                         'profile': {'radius': [0.0, 0.125, 0.25], 'real': [0.0, 1.5, 0.75], 'fake': [0.25, 1.0, 0.5]},
                                         'skipped_fake_ema': 6},
                               'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 8, 'min_size': 4}),
                                         (None, {'real_from': 'METRIC', 'n_images': 6, 'batch_size': 4, 'seed': 8, 'min_size': 4})],
                               'passes': 2},
 ('branch', 'full', False): {'line': 'Epoch:12, branches over 6 images, spur 2: forks 0.25 (KS 0.125), terminals 2.25 of 4.2500, spurs 3.25 (KS 0.500), links '
                                     'of 5.2500; data: forks 0.50, terminals 2.50 of 4.5000, spurs 3.50, links of 5.5000',
                             'entry': {'epoch': 12,
                                       'image_size': 16,
                                       'min_size': 5,
                                       'spur': 2,
                                       'images': 6,
                                       'skipped_real': 0,
                                       'skipped_fake': 1,
                                       'forks': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                       'nodes': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                       'terminals': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                       'spurs': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02},
                                       'terminal_length': {'ks': 0.625, 'real': 4.5, 'real_sem': 0.05, 'fake': 4.25, 'fake_sem': 0.02},
                                       'link_length': {'ks': 0.75, 'real': 5.5, 'real_sem': 0.06, 'fake': 5.25, 'fake_sem': 0.02},
                                       'longest': {'ks': 0.875, 'real': 6.5, 'real_sem': 0.07, 'fake': 6.25, 'fake_sem': 0.02},
                                       'profile': {'length': [0.0, 0.125, 0.25], 'real': [0.0, 1.5, 0.75], 'fake': [0.25, 1.0, 0.5]}},
                             'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 9, 'min_size': 5, 'spur': 2})],
                             'passes': 1},
 ('branch', 'full', True): {'line': 'Epoch:12, branches over 6 images, spur 2: forks 0.25 (KS 0.125), terminals 2.25 of 4.2500, spurs 3.25 (KS 0.500), links '
                                    'of 5.2500; data: forks 0.50, terminals 2.50 of 4.5000, spurs 3.50, links of 5.5000; averaged generator: forks 0.31 (KS '
                                    '0.188), terminals 2.31 of 4.3125, spurs 3.31 (KS 0.562), links of 5.3125',
                            'entry': {'epoch': 12,
                                      'image_size': 16,
                                      'min_size': 5,
                                      'spur': 2,
                                      'images': 6,
                                      'skipped_real': 0,
                                      'skipped_fake': 1,
                                      'forks': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                      'nodes': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                      'terminals': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                      'spurs': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02},
                                      'terminal_length': {'ks': 0.625, 'real': 4.5, 'real_sem': 0.05, 'fake': 4.25, 'fake_sem': 0.02},
                                      'link_length': {'ks': 0.75, 'real': 5.5, 'real_sem': 0.06, 'fake': 5.25, 'fake_sem': 0.02},
                                      'longest': {'ks': 0.875, 'real': 6.5, 'real_sem': 0.07, 'fake': 6.25, 'fake_sem': 0.02},
                                      'profile': {'length': [0.0, 0.125, 0.25], 'real': [0.0, 1.5, 0.75], 'fake': [0.25, 1.0, 0.5]},
                                      'skipped_fake_ema': 2,
                                      'forks_ema': {'fake': 0.3125, 'fake_sem': None, 'ks': 0.1875},
                                      'nodes_ema': {'fake': 1.3125, 'fake_sem': 0.0825, 'ks': 0.3125},
                                      'terminals_ema': {'fake': 2.3125, 'fake_sem': 0.0825, 'ks': 0.4375},
                                      'spurs_ema': {'fake': 3.3125, 'fake_sem': 0.0825, 'ks': 0.5625},
                                      'terminal_length_ema': {'fake': 4.3125, 'fake_sem': 0.0825, 'ks': 0.6875},
                                      'link_length_ema': {'fake': 5.3125, 'fake_sem': 0.0825, 'ks': 0.8125},
                                      'longest_ema': {'fake': 6.3125, 'fake_sem': 0.0825, 'ks': 0.9375},
                                      'profile_ema': {'fake': [0.5, 0.0, 0.0]}},
                            'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 9, 'min_size': 5, 'spur': 2}),
                                      (None, {'real_from': 'METRIC', 'n_images': 6, 'batch_size': 4, 'seed': 9, 'min_size': 5, 'spur': 2})],
                            'passes': 2},
 ('branch', 'note', False): {'line': 'Epoch:12, branches: no scored image on the generated side',
                             'entry': {'epoch': 12,
                                       'image_size': 16,
                                       'min_size': 5,
                                       'spur': 2,
                                       'images': 6,
                                       'skipped_real': 0,
                                       'skipped_fake': 6,
                                       'note': 'no scored image on the generated side'},
                             'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 9, 'min_size': 5, 'spur': 2})],
                             'passes': 1},
 ('branch', 'note', True): {'line': 'Epoch:12, branches: no scored image on the generated side',
                            'entry': {'epoch': 12,
                                      'image_size': 16,
                                      'min_size': 5,
                                      'spur': 2,
                                      'images': 6,
                                      'skipped_real': 0,
                                      'skipped_fake': 6,
                                      'note': 'no scored image on the generated side',
                                      'skipped_fake_ema': 6},
                            'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 9, 'min_size': 5, 'spur': 2}),
                                      (None, {'real_from': 'METRIC', 'n_images': 6, 'batch_size': 4, 'seed': 9, 'min_size': 5, 'spur': 2})],
                            'passes': 2},
 ('branch', 'inactive', False): {'line': 'Epoch:12, branches: 8 x 8 images are too small',
                                 'entry': {'epoch': 12,
                                           'image_size': 16,
                                           'min_size': 5,
                                           'spur': 2,
                                           'images': 0,
                                           'skipped_real': 0,
                                           'skipped_fake': 0,
                                           'note': '8 x 8 images are too small'},
                                 'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 9, 'min_size': 5, 'spur': 2})],
                                 'passes': 1},
 ('branch', 'inactive', True): {'line': 'Epoch:12, branches: 8 x 8 images are too small',
                                'entry': {'epoch': 12,
                                          'image_size': 16,
                                          'min_size': 5,
                                          'spur': 2,
                                          'images': 0,
                                          'skipped_real': 0,
                                          'skipped_fake': 0,
                                          'note': '8 x 8 images are too small'},
                                'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 9, 'min_size': 5, 'spur': 2})],
                                'passes': 1},
 ('branch', 'ema_note', False): {'line': 'Epoch:12, branches over 6 images, spur 2: forks 0.25 (KS 0.125), terminals 2.25 of 4.2500, spurs 3.25 (KS 0.500), '
                                         'links of 5.2500; data: forks 0.50, terminals 2.50 of 4.5000, spurs 3.50, links of 5.5000',
                                 'entry': {'epoch': 12,
                                           'image_size': 16,
                                           'min_size': 5,
                                           'spur': 2,
                                           'images': 6,
                                           'skipped_real': 0,
                                           'skipped_fake': 1,
                                           'forks': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                           'nodes': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                           'terminals': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                           'spurs': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02},
                                           'terminal_length': {'ks': 0.625, 'real': 4.5, 'real_sem': 0.05, 'fake': 4.25, 'fake_sem': 0.02},
                                           'link_length': {'ks': 0.75, 'real': 5.5, 'real_sem': 0.06, 'fake': 5.25, 'fake_sem': 0.02},
                                           'longest': {'ks': 0.875, 'real': 6.5, 'real_sem': 0.07, 'fake': 6.25, 'fake_sem': 0.02},
                                           'profile': {'length': [0.0, 0.125, 0.25], 'real': [0.0, 1.5, 0.75], 'fake': [0.25, 1.0, 0.5]}},
                                 'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 9, 'min_size': 5, 'spur': 2})],
                                 'passes': 1},
 ('branch', 'ema_note', True): {'line': 'Epoch:12, branches over 6 images, spur 2: forks 0.25 (KS 0.125), terminals 2.25 of 4.2500, spurs 3.25 (KS 0.500), '
                                        'links of 5.2500; data: forks 0.50, terminals 2.50 of 4.5000, spurs 3.50, links of 5.5000',
                                'entry': {'epoch': 12,
                                          'image_size': 16,
                                          'min_size': 5,
                                          'spur': 2,
                                          'images': 6,
                                          'skipped_real': 0,
                                          'skipped_fake': 1,
                                          'forks': {'ks': 0.125, 'real': 0.5, 'real_sem': 0.01, 'fake': 0.25, 'fake_sem': None},
                                          'nodes': {'ks': 0.25, 'real': 1.5, 'real_sem': 0.02, 'fake': 1.25, 'fake_sem': 0.02},
                                          'terminals': {'ks': 0.375, 'real': 2.5, 'real_sem': 0.03, 'fake': 2.25, 'fake_sem': 0.02},
                                          'spurs': {'ks': 0.5, 'real': 3.5, 'real_sem': 0.04, 'fake': 3.25, 'fake_sem': 0.02},
                                          'terminal_length': {'ks': 0.625, 'real': 4.5, 'real_sem': 0.05, 'fake': 4.25, 'fake_sem': 0.02},
                                          'link_length': {'ks': 0.75, 'real': 5.5, 'real_sem': 0.06, 'fake': 5.25, 'fake_sem': 0.02},
                                          'longest': {'ks': 0.875, 'real': 6.5, 'real_sem': 0.07, 'fake': 6.25, 'fake_sem': 0.02},
                                          'profile': {'length': [0.0, 0.125, 0.25], 'real': [0.0, 1.5, 0.75], 'fake': [0.25, 1.0, 0.5]},
                                          'skipped_fake_ema': 6},
                                'calls': [('DATASET', {'return_metric': True, 'n_images': 6, 'batch_size': 4, 'seed': 9, 'min_size': 5, 'spur': 2}),
                                          (None, {'real_from': 'METRIC', 'n_images': 6, 'batch_size': 4, 'seed': 9, 'min_size': 5, 'spur': 2})],
                                'passes': 2}}
TABLES = {('morph', 'profile'): 'Title of morph (6 images per side; not scored: 0 of the data, 1 generated)\n'
                       '                                 data              generated      KS\n'
                       '          fill     0.5000 +-   0.0100     0.2500               0.125\n'
                       '    components     1.5000 +-   0.0200     1.2500 +-   0.0200   0.250\n'
                       ' largest_share     2.5000 +-   0.0300     2.2500 +-   0.0200   0.375\n'
                       '     dimension     3.5000 +-   0.0400     3.2500 +-   0.0200   0.500',
 ('morph', 'no_sem'): 'Title of morph (6 images per side; not scored: 0 of the data, 1 generated)\n'
                      '                                 data              generated      KS\n'
                      '          fill     0.5000                 0.2500               0.125\n'
                      '    components     1.5000                 1.2500 +-   0.0200   0.250\n'
                      ' largest_share     2.5000                 2.2500 +-   0.0200   0.375\n'
                      '     dimension     3.5000                 3.2500 +-   0.0200   0.500',
 ('morph', 'note'): 'Title of morph: no scored image on the generated side',
 ('skeleton', 'profile'): 'Title of skeleton (6 images per side; not scored: 0 of the data, 1 generated)\n'
                          '                                 data              generated      KS\n'
                          '        length     0.5000 +-   0.0100     0.2500               0.125\n'
                          '          tips     1.5000 +-   0.0200     1.2500 +-   0.0200   0.250\n'
                          '     junctions     2.5000 +-   0.0300     2.2500 +-   0.0200   0.375\n'
                          '         width     3.5000 +-   0.0400     3.2500 +-   0.0200   0.500',
 ('skeleton', 'no_sem'): 'Title of skeleton (6 images per side; not scored: 0 of the data, 1 generated)\n'
                         '                                 data              generated      KS\n'
                         '        length     0.5000                 0.2500               0.125\n'
                         '          tips     1.5000                 1.2500 +-   0.0200   0.250\n'
                         '     junctions     2.5000                 2.2500 +-   0.0200   0.375\n'
                         '         width     3.5000                 3.2500 +-   0.0200   0.500',
 ('skeleton', 'note'): 'Title of skeleton: no scored image on the generated side',
 ('sholl', 'profile'): 'Title of sholl (6 images per side; not scored: 0 of the data, 1 generated)\n'
                       '                                 data              generated      KS\n'
                       '       calibre     0.5000 +-   0.0100     0.2500               0.125\n'
                       '          soma     1.5000 +-   0.0200     1.2500 +-   0.0200   0.250\n'
                       '    sholl_peak     2.5000 +-   0.0300     2.2500 +-   0.0200   0.375\n'
                       '  sholl_radius     3.5000 +-   0.0400     3.2500 +-   0.0200   0.500\n'
                       '         reach     4.5000 +-   0.0500     4.2500 +-   0.0200   0.625\n'
                       '  profile data 0.00 1.50 0.75   (mean crossings per ring, rings 0.1250 image widths apart)\n'
                       '     generated 0.25 1.00 0.50',
 ('sholl', 'empty_profile'): 'Title of sholl (6 images per side; not scored: 0 of the data, 1 generated)\n'
                             '                                 data              generated      KS\n'
                             '       calibre     0.5000 +-   0.0100     0.2500               0.125\n'
                             '          soma     1.5000 +-   0.0200     1.2500 +-   0.0200   0.250\n'
                             '    sholl_peak     2.5000 +-   0.0300     2.2500 +-   0.0200   0.375\n'
                             '  sholl_radius     3.5000 +-   0.0400     3.2500 +-   0.0200   0.500\n'
                             '         reach     4.5000 +-   0.0500     4.2500 +-   0.0200   0.625\n'
                             '  profile data    (mean crossings per ring, rings 0.0000 image widths apart)\n'
                             '     generated ',
 ('sholl', 'no_sem'): 'Title of sholl (6 images per side; not scored: 0 of the data, 1 generated)\n'
                      '                                 data              generated      KS\n'
                      '       calibre     0.5000                 0.2500               0.125\n'
                      '          soma     1.5000                 1.2500 +-   0.0200   0.250\n'
                      '    sholl_peak     2.5000                 2.2500 +-   0.0200   0.375\n'
                      '  sholl_radius     3.5000                 3.2500 +-   0.0200   0.500\n'
                      '         reach     4.5000                 4.2500 +-   0.0200   0.625\n'
                      '  profile data 0.00 1.50 0.75   (mean crossings per ring, rings 0.1250 image widths apart)\n'
                      '     generated 0.25 1.00 0.50',
 ('sholl', 'note'): 'Title of sholl: no scored image on the generated side',
 ('branch', 'profile'): 'Title of branch (6 images per side; not scored: 0 of the data, 1 generated)\n'
                        '                                   data              generated      KS\n'
                        '           forks     0.5000 +-   0.0100     0.2500               0.125\n'
                        '           nodes     1.5000 +-   0.0200     1.2500 +-   0.0200   0.250\n'
                        '       terminals     2.5000 +-   0.0300     2.2500 +-   0.0200   0.375\n'
                        '           spurs     3.5000 +-   0.0400     3.2500 +-   0.0200   0.500\n'
                        ' terminal_length     4.5000 +-   0.0500     4.2500 +-   0.0200   0.625\n'
                        '     link_length     5.5000 +-   0.0600     5.2500 +-   0.0200   0.750\n'
                        '         longest     6.5000 +-   0.0700     6.2500 +-   0.0200   0.875\n'
                        '    profile data 0.00 1.50 0.75   (mean branches per bin, bins 0.1250 image widths wide)\n'
                        '       generated 0.25 1.00 0.50',
 ('branch', 'empty_profile'): 'Title of branch (6 images per side; not scored: 0 of the data, 1 generated)\n'
                              '                                   data              generated      KS\n'
                              '           forks     0.5000 +-   0.0100     0.2500               0.125\n'
                              '           nodes     1.5000 +-   0.0200     1.2500 +-   0.0200   0.250\n'
                              '       terminals     2.5000 +-   0.0300     2.2500 +-   0.0200   0.375\n'
                              '           spurs     3.5000 +-   0.0400     3.2500 +-   0.0200   0.500\n'
                              ' terminal_length     4.5000 +-   0.0500     4.2500 +-   0.0200   0.625\n'
                              '     link_length     5.5000 +-   0.0600     5.2500 +-   0.0200   0.750\n'
                              '         longest     6.5000 +-   0.0700     6.2500 +-   0.0200   0.875\n'
                              '    profile data    (mean branches per bin, bins 0.0000 image widths wide)\n'
                              '       generated ',
 ('branch', 'no_sem'): 'Title of branch (6 images per side; not scored: 0 of the data, 1 generated)\n'
                       '                                   data              generated      KS\n'
                       '           forks     0.5000                 0.2500               0.125\n'
                       '           nodes     1.5000                 1.2500 +-   0.0200   0.250\n'
                       '       terminals     2.5000                 2.2500 +-   0.0200   0.375\n'
                       '           spurs     3.5000                 3.2500 +-   0.0200   0.500\n'
                       ' terminal_length     4.5000                 4.2500 +-   0.0200   0.625\n'
                       '     link_length     5.5000                 5.2500 +-   0.0200   0.750\n'
                       '         longest     6.5000                 6.2500 +-   0.0200   0.875\n'
                       '    profile data 0.00 1.50 0.75   (mean branches per bin, bins 0.1250 image widths wide)\n'
                       '       generated 0.25 1.00 0.50',
 ('branch', 'note'): 'Title of branch: no scored image on the generated side'}
