"""Scoring a checkpoint during training: one routine for every row of metric_table.METRICS.

`score(m, trainer, dataset, cfg, epoch, checkpoint, log)` evaluates the training generator with metrics.<m.evaluate> on
cfg.<prefix>_<count> images (or pairs) per side in minibatches of cfg.batch_size, seed cfg.<prefix>_seed, and, when the trainer
averages, the averaged generator under `trainer.averaged_generator()`; it logs one line and appends one entry {epoch, image_size, ...}
to checkpoint.<m.key>.  Eager, outside any captured graph, no collective; the evaluations draw from private generators only, so the run
trains on as if it had not happened.  What differs between metrics -- the fields of the entry, how the averaged pass is made and kept,
the wording of the line -- is one small piece per `m.kind` below.  `metrics.evaluate_*` is looked up when it is called."""
from .metric_table import METRICS


def evaluate_settings(m, cfg, image_size, metrics):
    """the keyword arguments of metrics.<m.evaluate> that the configuration decides"""
    kw = {"n_" + m.count: int(getattr(cfg, m.prefix + "_" + m.count, m.count_default)), "batch_size": int(cfg.batch_size),
          "seed": int(getattr(cfg, m.prefix + "_seed", 0))}
    for name, _, default, at_zero, _ in m.options:
        value = getattr(cfg, m.prefix + "_" + name, default)
        kw[name] = int(value) if at_zero is None else int(value or 0) or getattr(metrics, at_zero)(image_size)
    return kw


def _score_swd(m, metrics, run, dataset, averaged, kw, entry):
    """{levels, swd, swd_ema}; the averaged generator is scored against the data again: SWD's two sides share their patch corners' stream"""
    res = run(dataset)
    entry.update(levels=list(res["levels"]), swd=list(res["swd"]), swd_ema=None)
    if averaged is not None:
        with averaged():
            entry["swd_ema"] = list(run(dataset)["swd"])
    if not entry["levels"]:
        return "SWD: {}".format(res["note"])
    fmt = lambda v: "[" + ", ".join("{:.3f}".format(x) for x in v) + "]"   # noqa: E731
    return "SWD x1e3 at {}: {}{}".format(entry["levels"], fmt(entry["swd"]),
                                         "" if entry["swd_ema"] is None else ", averaged generator: " + fmt(entry["swd_ema"]))


def _score_msssim(m, metrics, run, dataset, averaged, kw, entry):
    """{scales, fake, fake_ema, real, pairs}, the data set's own pair similarity next to the generator's"""
    res = run(dataset)
    entry.update(scales=int(res["scales"]), fake=res["fake"], fake_ema=None, real=res["real"], pairs=int(res["pairs"]))
    if not res["scales"]:
        return "MS-SSIM: {}".format(res["note"])
    if averaged is not None:
        with averaged():
            entry["fake_ema"] = run(None)["fake"]                          # (the data's side is the same: not scored twice)
    return "MS-SSIM over {} pairs, {} scales: generated {:.5f}{}{}".format(
        entry["pairs"], entry["scales"], entry["fake"],
        "" if entry["fake_ema"] is None else ", averaged generator {:.5f}".format(entry["fake_ema"]),
        "" if entry["real"] is None else ", data {:.5f}".format(entry["real"]))


def _score_spectrum(m, metrics, run, dataset, averaged, kw, entry):
    """{images, k, real, fake, ratio_db, distance_db, high_db} plus {distance_db_ema, high_db_ema} with an averaged generator (the data's
    side is the same: it is not stored twice)"""
    res, metric = run(dataset, return_metric=True)
    entry.update(images=int(res["images"]), k=list(res["k"]), real=list(res["real"]), fake=list(res["fake"]),
                 ratio_db=list(res["ratio_db"]), distance_db=res["distance_db"], high_db=res["high_db"])
    if not res["k"]:
        return "spectrum: {}".format(res["note"])
    if averaged is not None:
        with averaged():
            ema = run(None, real_from=metric)                              # (the data's side is the same: not scored twice)
        entry["distance_db_ema"], entry["high_db_ema"] = ema["distance_db"], ema["high_db"]
    db = lambda v: "-" if v is None else "{:+.2f} dB".format(v)   # noqa: E731
    return "spectrum over {} images: distance {}, top octave {}{}".format(
        entry["images"], db(entry["distance_db"]), db(entry["high_db"]),
        "" if "high_db_ema" not in entry else ", averaged generator: distance {}, top octave {}".format(
            db(entry["distance_db_ema"]), db(entry["high_db_ema"])))


# per arbor metric: its name in the line, what follows the number of images (formatted with the evaluation's settings), and the
# statistics it shows, by name, with `<name>_ks` where the generated side's Kolmogorov-Smirnov distance follows
_ARBOR_LINES = {
    "morph": ("morphology", "", "components {components:.2f}, largest share {largest_share:.3f}{largest_share_ks}, fill {fill:.4f}, "
                                "dimension {dimension:.3f}"),
    "skeleton": ("skeleton", "", "length {length:.3f}, tips {tips:.2f}{tips_ks}, junctions {junctions:.2f}, width {width:.3f}"),
    "sholl": ("sholl", "", "calibre {calibre:.3f}{calibre_ks}, soma {soma:.2f}, peak {sholl_peak:.2f} at {sholl_radius:.3f}, "
                           "reach {reach:.3f}{reach_ks}"),
    "branch": ("branches", ", spur {spur}", "forks {forks:.2f}{forks_ks}, terminals {terminals:.2f} of {terminal_length:.4f}, "
                                            "spurs {spurs:.2f}{spurs_ks}, links of {link_length:.4f}"),
}


def _score_arbor(m, metrics, run, dataset, averaged, kw, entry):
    """{<option>..., images, skipped_real, skipped_fake[, note]} plus, per statistic, {real, real_sem, fake, fake_sem, ks} and, where the
    metric has one, profile: {<axis>, real, fake}; with an averaged generator also skipped_fake_ema, <statistic>_ema: {fake, fake_sem, ks}
    and profile_ema: {fake} over the bins of profile (the data's side is the same: it is not stored twice)"""
    names = getattr(metrics, m.statistics)
    label, after, wording = _ARBOR_LINES[m.prefix]
    res, metric = run(dataset, return_metric=True)
    entry.update({name: kw[name] for name, *_ in m.options})
    entry.update({k: ({a: (list(b) if isinstance(b, list) else b) for a, b in v.items()} if isinstance(v, dict) else v) for k, v in res.items()})
    if metric.active and averaged is not None:
        with averaged():
            ema = run(None, real_from=metric)                              # (the data's side is the same: not scored twice)
        entry["skipped_fake_ema"] = ema["skipped_fake"]
        for name in names:
            if name in ema:
                entry[name + "_ema"] = {k: ema[name][k] for k in ("fake", "fake_sem", "ks")}
        if "profile" in ema and "profile" in entry:
            n = len(entry["profile"][m.axis])
            entry["profile_ema"] = {"fake": (list(ema["profile"]["fake"]) + [0.0] * n)[:n]}
    if names[0] not in res:
        return "{}: {}".format(label, res["note"])
    one = lambda r: wording.format(**{n: r[n]["fake"] for n in names}, **{n + "_ks": " (KS {:.3f})".format(r[n]["ks"]) for n in names})  # noqa: E731
    line = "{} over {} images{}: {}; data: {}".format(label, res["images"], after.format(**kw), one(res), wording.format(
        **{n: res[n]["real"] for n in names}, **{n + "_ks": "" for n in names}))
    if names[0] + "_ema" in entry:
        line += "; averaged generator: " + one({n: entry[n + "_ema"] for n in names})
    return line


_PIECES = {"swd": _score_swd, "msssim": _score_msssim, "spectrum": _score_spectrum, "arbor": _score_arbor}


def score(m, trainer, dataset, cfg, epoch, checkpoint=None, log=print):
    """One evaluation of row `m` of METRICS at a checkpoint (see the module's text); returns the entry."""
    from . import metrics
    G = trainer.G
    evaluate = getattr(metrics, m.evaluate)
    kw = evaluate_settings(m, cfg, int(G.image_size), metrics)
    run = lambda data, **more: evaluate(G, data, **more, **kw)   # noqa: E731
    averaged = trainer.averaged_generator if getattr(trainer, "ema_enabled", False) else None
    entry = {"epoch": int(epoch), "image_size": int(G.image_size)}
    log("Epoch:{}, {}".format(epoch, _PIECES[m.kind](m, metrics, run, dataset, averaged, kw, entry)))
    if checkpoint is not None:
        getattr(checkpoint, m.key).append(entry)
    return entry


def score_due(trainer, dataset, cfg, epoch, checkpoint=None, log=print):
    """every metric whose cfg.<prefix>_period is positive and divides `epoch`, in table order"""
    for m in METRICS:
        period = int(getattr(cfg, m.prefix + "_period", 0) or 0)
        if period > 0 and epoch % period == 0:
            score(m, trainer, dataset, cfg, epoch, checkpoint=checkpoint, log=log)


# the rows by name, with the signature they have always had (train.py re-exports them)
_ROW = {m.prefix: m for m in METRICS}


def score_swd(trainer, dataset, cfg, epoch, checkpoint=None, log=print):
    return score(_ROW["swd"], trainer, dataset, cfg, epoch, checkpoint, log)


def score_msssim(trainer, dataset, cfg, epoch, checkpoint=None, log=print):
    return score(_ROW["msssim"], trainer, dataset, cfg, epoch, checkpoint, log)


def score_spectrum(trainer, dataset, cfg, epoch, checkpoint=None, log=print):
    return score(_ROW["spectrum"], trainer, dataset, cfg, epoch, checkpoint, log)


def score_morph(trainer, dataset, cfg, epoch, checkpoint=None, log=print):
    return score(_ROW["morph"], trainer, dataset, cfg, epoch, checkpoint, log)


def score_skeleton(trainer, dataset, cfg, epoch, checkpoint=None, log=print):
    return score(_ROW["skeleton"], trainer, dataset, cfg, epoch, checkpoint, log)


def score_sholl(trainer, dataset, cfg, epoch, checkpoint=None, log=print):
    return score(_ROW["sholl"], trainer, dataset, cfg, epoch, checkpoint, log)


def score_branches(trainer, dataset, cfg, epoch, checkpoint=None, log=print):
    return score(_ROW["branch"], trainer, dataset, cfg, epoch, checkpoint, log)
