"""The checkpoint metrics as one ordered table: what the configuration, the checkpoint file, both command lines and the scoring code
need to know about a metric, stated once.  Standard library only and nothing of the package: configs/config.py, utils.py, scoring.py,
train.py and eval.py all import it; the functions a row names are looked up on `metrics` when they are called.

A row gives a metric its settings `<prefix>_period` (0: off), `<prefix>_<count>`, `<prefix>_seed` and one `<prefix>_<option>` per
entry of `options`, in that order in the configuration and on train.py's command line; its switch on eval.py's; the key of its list of
entries in a checkpoint file, which is also the Checkpointer's attribute; and its table's title there."""
from collections import namedtuple

Metric = namedtuple("Metric", [
    "prefix",         # of its configuration names and flags
    "switch",         # eval.py: --<switch> [N]
    "key",            # of its list of entries in a checkpoint
    "count",          # what N counts: the configuration name after the prefix; evaluate_* takes it as n_<count>
    "count_default",
    "options",        # further integer settings: (name = keyword of evaluate_*, lowest legal value, default, the function of metrics.py
                      # that gives the value at an image size when the setting is 0, or None, the flag's help)
    "evaluate",       # metrics.<evaluate>(generator, dataset, ...)
    "format",         # metrics.<format>(result, title): the table eval.py prints
    "title",          # of that table, followed by which generator of which file and `title_tail`
    "title_tail",     # formatted with n = N
    "needs_data",     # eval.py: False if the metric also scores without a data set
    "kind",           # scoring.py: which of its pieces turns results into the checkpoint entry and the log line
    "statistics",     # metrics.<statistics>: the names of the per-image statistics of an arbor metric
    "axis",           # the key of the x axis of its result's `profile`, if it has one
])

_MIN_SIZE = ("min_size", 1, 1, None, "components below this many pixels are dropped (1 drops none)")
_SPUR = ("spur", 0, 0, "default_spur", "terminal branches below this many pixels are pruned as thinning spurs (0: max(2, image size / 32))")
_IMAGES = ("images", 8192)
_PLAIN = ("", True)

METRICS = (
    Metric("swd", "swd", "SWD", *_IMAGES, (), "evaluate_swd", "format_table", "SWD x 1e3", " against {n} images", True, "swd", None, None),
    Metric("msssim", "msssim", "MSSSIM", "pairs", 10000, (), "evaluate_msssim", "format_msssim", "MS-SSIM between pairs", "", False,
           "msssim", None, None),
    Metric("spectrum", "spectrum", "SPECTRUM", *_IMAGES, (), "evaluate_spectrum", "format_spectrum", "Radial power spectrum", *_PLAIN,
           "spectrum", None, None),
    Metric("morph", "morph", "MORPH", *_IMAGES, (_MIN_SIZE,), "evaluate_morphology", "format_morphology", "Arbor morphology", *_PLAIN,
           "arbor", "MORPH_STATISTICS", None),
    Metric("skeleton", "skeleton", "SKELETON", *_IMAGES, (_MIN_SIZE,), "evaluate_skeleton", "format_skeleton", "Arbor skeleton", *_PLAIN,
           "arbor", "SKELETON_STATISTICS", None),
    Metric("sholl", "sholl", "SHOLL", *_IMAGES, (_MIN_SIZE,), "evaluate_sholl", "format_sholl", "Arbor geometry", *_PLAIN,
           "arbor", "SHOLL_STATISTICS", "radius"),
    Metric("branch", "branches", "BRANCH", *_IMAGES, (_MIN_SIZE, _SPUR), "evaluate_branches", "format_branches",
           "Arbor branches", *_PLAIN, "arbor", "BRANCH_STATISTICS", "length"),
)


def settings(m):
    """[(configuration name, lowest legal value, default, help)] of a row, all integers, in the order they are listed and printed in"""
    what = m.title.split(" x ")[0]
    return [(m.prefix + "_period", 0, 0, f"score every checkpoint whose epoch is a multiple of this: {what} (metrics.py); 0: off"),
            (m.prefix + "_" + m.count, 1, m.count_default, f"{m.count} per side of one evaluation: {what}"),
            (m.prefix + "_seed", 0, 0, f"seed of the latents, augmentations and other draws: {what}")] + \
           [(m.prefix + "_" + name, lowest, default, text) for name, lowest, default, _, text in m.options]
