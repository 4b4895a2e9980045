"""The sliced Wasserstein distance on the GPU: every kernel of csrc/swd.hip per element against the fp64 restatement of
tests/swd_cases.py (bounds, shapes and emulations are described there), the whole metric, and its promise to leave a run alone.

Whole metric, measured on the CPU with the emulation in kernel order (tests/test_swd_cpu.py prints every figure): the worst emulated
err / bound over the 24 level values of the cases below is 0.0002 with C_ACC = 8 -- the bound is a worst case over one million
projections whose errors mostly cancel in the mean; the kernels are held to the same bound."""
import functools
import types

import numpy as np
import pytest
import torch

import swd_cases as S
from swd_cases import C_ACC, N_ROUND

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64 = np.float64


def err_over_bound(got, ref, absref, n_round):
    got, ref, absref = (np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=f64) for a in (got, ref, absref))
    assert got.shape == ref.shape == absref.shape, (got.shape, ref.shape, absref.shape)
    return np.abs(got - ref) / (n_round * 2.0 ** -23 * np.abs(ref) + C_ACC * 2.0 ** -24 * absref + 1e-30)


def assert_image_within(name, got, ref, absref, n_round):
    """borders and interior separately: a wrong mirror cannot hide in a maximum over the image"""
    r = err_over_bound(got, ref, absref, n_round)
    parts = {"top rows": r[:, :2], "bottom rows": r[:, -2:], "left columns": r[:, :, :2], "right columns": r[:, :, -2:],
             "interior": r[:, 2:-2, 2:-2]}
    for part, v in parts.items():
        assert v.max() <= 1.0, f"{name}, {part}: err / bound {v.max():.3f}"


# ---- pyramid ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.PYR_COLORS)
@pytest.mark.parametrize("size", S.PYR_SIZES)
def test_pyramid_stages_per_element(ngan, size, c):
    M = ngan.metrics
    x = S.images(S.seed_of(1, size, c), S.PYR_B, size, c)
    down = M.pyr_down(x.to(DEV))
    assert tuple(down.shape) == (S.PYR_B, size // 2, size // 2, c)
    assert_image_within(f"pyr_down {size} C={c}", down, S.pyr_down_ref(x), S.pyr_down_ref(x.abs()), N_ROUND["pyr_down"])
    lap = M.laplacian(x.to(DEV), down)
    coarse = down.cpu()                                    # the reference starts from the kernel's own input
    assert_image_within(f"laplacian {size} C={c}", lap, S.laplacian_ref(x, coarse), S.laplacian_abs(x, coarse), N_ROUND["laplacian"])
    # the pyramid is these stages chained: one, two, three levels for 16, 32, 64
    n_levels = len(S.levels_of(size)) if size in S.METRIC_SIZES else 2
    pyr = M.laplacian_pyramid(x.to(DEV), n_levels)
    assert [p.shape[1] for p in pyr] == [size >> l for l in range(n_levels)]
    if n_levels == 1:
        assert torch.equal(pyr[0], x.to(DEV))
    else:
        assert torch.equal(pyr[0], lap)
        assert torch.equal(pyr[-1], down if n_levels == 2 else M.pyr_down(down))


# ---- descriptors -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.PYR_COLORS)
@pytest.mark.parametrize("n", S.DESC_N)
def test_descriptors_gather_and_sums(ngan, n, c):
    M = ngan.metrics
    img = S.pyramid_ref(S.images(S.seed_of(2, c), 5, 32, c), 2)[0].float()
    pos = S.corner_positions(S.seed_of(3, c), 5, 32, 27)
    pos = torch.cat([pos[:n - 5], pos[-5:]])               # n rows, the first and the last image among them
    assert pos.shape[0] == n and {(0, 0), (25, 25), (0, 25), (25, 0)} <= {tuple(p) for p in pos[:, 1:].tolist()}
    want = S.descriptors_ref(img, pos)
    desc, sums = M.patch_descriptors(img.to(DEV), pos)
    assert torch.equal(desc.cpu(), want), "the gather is not bit-equal to indexing"
    ref = S.channel_sums_ref(want)
    tol = n * 49 * 2.0 ** -53 * torch.cat([want.double().abs().view(n, c, 49).sum((0, 2)), ref[c:]])
    assert ((sums.cpu() - ref).abs() <= tol).all(), (sums.cpu() - ref, tol)
    # minibatch after minibatch into one matrix and one pair of sums
    out = torch.full((n + 3, 49 * c), -7.0, device=DEV)
    acc, row = None, 0
    for cut in (pos[:50], pos[50:83], pos[83:]):
        _, acc = M.patch_descriptors(img.to(DEV), cut, out=out, sums=acc, row_offset=row, accumulate=row > 0)
        row += cut.shape[0]
    assert torch.equal(out[:n], desc) and bool((out[n:] == -7.0).all())
    assert ((acc.cpu() - ref).abs() <= tol).all()
    # the entry point refuses a corner outside the image through the wrapper too
    bad = pos.clone()
    bad[n // 2, 2] = 26
    with pytest.raises(RuntimeError, match="out of range"):
        M.patch_descriptors(img.to(DEV), bad)


# ---- projection ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.PYR_COLORS)
@pytest.mark.parametrize("n_dirs", S.PROJ_DIRS)
@pytest.mark.parametrize("n", S.DESC_N)
def test_projection_per_element_and_tail(ngan, n, n_dirs, c):
    M = ngan.metrics
    lap = S.pyramid_ref(S.images(S.seed_of(2, c), 5, 32, c), 2)[0].float()
    desc = S.descriptors_ref(lap, S.corner_positions(S.seed_of(3, c), 5, 32, 27)[:n])
    dirs = S.directions(S.seed_of(4, n_dirs, c), 49 * c, 1, n_dirs)
    ref, absref = S.project_ref(desc, dirs)
    n_pad = M.next_pow2(n)                                 # 128: a ragged last tile; 256: whole tiles of padding too
    got = M.project(desc.to(DEV), S.channel_sums_ref(desc).to(DEV), dirs.to(DEV), n_pad)
    assert tuple(got.shape) == (n_dirs, n_pad)
    r = err_over_bound(got[:, :n], ref, absref, N_ROUND["project"])
    assert r.max() <= 1.0, f"project n={n} n_dirs={n_dirs} C={c}: err / bound {r.max():.3f}"
    assert bool((got[:, n:] == float("inf")).all()), "the tail is not +inf"


# ---- sort ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sort_lengths():
    from __graft_entry__ import load_package
    blk = load_package().metrics.sort_block_elements()
    # 120 and 1024: one launch, shorter than a block; the block; block + 1: one pass over global memory; 8 blocks: single- and
    # double-stride passes (merge 2 blocks: 1; 4 blocks: 2 strides in one; 8 blocks: 2 strides in one, then 1)
    return (120, 1024, blk, blk + 1, 8 * blk)


@pytest.mark.parametrize("which", range(5))
def test_sort_columns_equals_torch_sort(ngan, which):
    M = ngan.metrics
    n = sort_lengths()[which]
    n_pad = M.next_pow2(n)
    g = torch.Generator().manual_seed(S.seed_of(5, n))
    cols = torch.full((6, n_pad), float("inf"))
    cols[0, :n] = torch.randn(n, generator=g)
    cols[1, :n] = torch.randint(0, 17, (n,), generator=g).float()                   # duplicates
    cols[2, :n] = torch.sort(torch.randn(n, generator=g)).values                     # already sorted
    cols[3, :n] = torch.sort(torch.randn(n, generator=g), descending=True).values    # reverse sorted
    cols[4, :n] = 2.5                                                                # all equal
    cols[5, :n] = torch.randn(n, generator=g).round() * 0.0                          # zeros of both signs
    cols[5, :n:3] = torch.randn(cols[5, :n:3].shape, generator=g)
    got = M.sort_columns(cols.to(DEV).clone()).cpu()
    want = torch.sort(cols, dim=1).values
    # equal to torch.sort of the same input, hence a permutation of it (== : the order of -0 and +0 is free)
    assert bool((got == want).all()), f"n={n}: {int((got != want).sum())} entries differ from torch.sort"
    assert bool((got[:, n:] == float("inf")).all())


# ---- whole metric ----------------------------------------------------------------------------------------------------------------------
def split_positions(pos, per_image, first):
    """the triples of the first `first` images and of the rest, the latter with image indices counted from the minibatch's start"""
    a, b = pos[:first * per_image].clone(), pos[first * per_image:].clone()
    b[:, 0] -= first
    return a, b


@pytest.mark.parametrize("kind", ("tanh", "smooth"))
@pytest.mark.parametrize("c", S.PYR_COLORS)
@pytest.mark.parametrize("size", S.METRIC_SIZES)
def test_whole_metric_against_fp64(ngan, size, c, kind):
    """emulated worst err / bound: 0.0002 (module docstring); the kernels are held to err / bound <= 1"""
    M = ngan.metrics
    x_a, x_b, pos_a, pos_b, dirs = S.metric_inputs(size, c, kind)
    ref = S.metric_ref(x_a, x_b, pos_a, pos_b, dirs)
    m = M.SWD(size, n_colors=c, nhoods_per_image=S.METRIC_PATCHES, dir_repeats=S.METRIC_DIRS[0], dirs_per_repeat=S.METRIC_DIRS[1],
              device=DEV)
    assert m.levels == S.levels_of(size)
    # the real side in one minibatch, as (B, C, R, R); the generated side in two, channels-last
    m.feed("real", x_a.permute(0, 3, 1, 2).contiguous().to(DEV), positions=pos_a)
    halves = [split_positions(p, S.METRIC_PATCHES, 3) for p in pos_b]
    m.feed("fake", x_b[:3].to(DEV), positions=[h[0] for h in halves])
    m.feed("fake", x_b[3:].to(DEV), positions=[h[1] for h in halves])
    res = m.result(dirs=dirs)
    assert res["levels"] == S.levels_of(size) and len(res["swd"]) == len(ref)
    assert abs(res["mean"] - sum(res["swd"]) / len(ref)) < 1e-12
    for level, got, (val, absref) in zip(res["levels"], res["swd"], ref):
        r = float(err_over_bound(np.array([got]), np.array([val]), np.array([absref]), N_ROUND["metric"])[0])
        print(f"metric {size} C={c} {kind} level {level}: ref {val:.6f} got {got:.6f} err/bound {r:.4f}")
        assert r <= 1.0, f"level {level}: {got} against {val}, err / bound {r:.3f}"


def test_identical_sets_give_exactly_zero_and_flat_channels_are_refused(ngan):
    M = ngan.metrics
    x = S.images(21, 5, 32, 3)
    pos = [S.corner_positions(22 + s, 5, s, 24) for s in (32, 16)]
    m = M.SWD(32, n_colors=3, nhoods_per_image=24, dir_repeats=2, dirs_per_repeat=128, seed=3, device=DEV)
    m.feed("real", x.to(DEV), positions=pos)
    m.feed("fake", x.to(DEV), positions=pos)
    res = m.result()
    assert res["swd"] == [0.0, 0.0] and res["mean"] == 0.0
    # drawn positions: a valid result, and the same one for the same seed
    runs = []
    for _ in range(2):
        m = M.SWD(32, n_colors=3, nhoods_per_image=24, dir_repeats=2, dirs_per_repeat=128, seed=3, device=DEV)
        m.feed("real", x.to(DEV))
        m.feed("fake", S.images(23, 5, 32, 3, "tanh").to(DEV))
        runs.append(m.result())
    assert runs[0] == runs[1] and all(v > 0 and np.isfinite(v) for v in runs[0]["swd"])
    # a channel without variance: the level is named
    flat = M.SWD(32, n_colors=1, nhoods_per_image=4, dir_repeats=1, dirs_per_repeat=16, device=DEV)
    flat.feed("real", S.images(24, 2, 32, 1).to(DEV))
    flat.feed("fake", torch.zeros(2, 1, 32, 32, device=DEV))
    with pytest.raises(ValueError, match="level 32.*fake.*zero variance"):
        flat.result()


# ---- no side effects -------------------------------------------------------------------------------------------------------------------
def small_nets(ngan):
    G = ngan.models.Generator_PG([32, 16], image_size_init=8, latent_dim=32).to(DEV)
    D = ngan.models.Discriminator_PG([16, 32], image_size_init=8).to(DEV)
    return G, D


def small_dataset(ngan):
    g = torch.Generator().manual_seed(9)
    return ngan.data.NeuronDataset(torch.rand(8, 1, 16, 16, generator=g), augmentations=True, im_translation=0.05, device=DEV, seed=3)


def test_evaluate_swd_consumes_no_shared_random_stream(ngan):
    torch.manual_seed(7)
    G, _ = small_nets(ngan)
    G.set_resolution(16, 1.0)
    data = small_dataset(ngan)
    data.set_image_size(8)
    host, device, aug = torch.get_rng_state(), torch.cuda.get_rng_state(DEV), data.gen.get_state()
    kw = dict(n_images=12, batch_size=8, seed=2, nhoods_per_image=16, dir_repeats=2, dirs_per_repeat=16)
    first = ngan.metrics.evaluate_swd(G, data, **kw)
    assert first["levels"] == [16] and first["swd"][0] > 0 and np.isfinite(first["swd"][0])
    assert torch.equal(torch.get_rng_state(), host), "torch's global generator was consumed"
    assert torch.equal(torch.cuda.get_rng_state(DEV), device), "the device generator was consumed"
    assert torch.equal(data.gen.get_state(), aug) and data.image_size == 8, "the data set's augmentation stream or stage moved"
    assert ngan.metrics.evaluate_swd(G, data, **kw) == first                    # seeded: the same number again
    G8, _ = small_nets(ngan)                                                    # a stage below 16 x 16: said, not raised
    below = ngan.metrics.evaluate_swd(G8, data, **kw)
    assert below["levels"] == [] and below["mean"] is None and "16 x 16" in below["note"]


def two_epochs(ngan, tmp_path, tag, swd_period, ema_beta):
    cfg = types.SimpleNamespace(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[1], N_epochs=2,
                                alpha_step=0.5, learning_rate=2e-3, checkpointing_period=1, ID=tag, swd_period=swd_period, swd_images=8,
                                swd_seed=1)
    torch.manual_seed(5)
    G, D = small_nets(ngan)
    data = small_dataset(ngan)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, alpha_step=cfg.alpha_step, device_latents=True, ema_beta=ema_beta)
    f = str(tmp_path / f"GenDisc_{tag}.pth")
    ck = ngan.utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=torch.device(DEV), trainer=tr,
                                 extra_checkpoint_period=1e3)
    lines = []
    series = ngan.train.pggan_train(tr, data, cfg, checkpoint=ck, epoch_final=3, log=lambda *a: lines.append(" ".join(map(str, a))))
    return series, ngan.utils.load_checkpoint_dict(f), lines, tr, f


@pytest.mark.parametrize("ema_beta", (0.0, 0.9))
def test_a_scored_run_trains_bit_identically(ngan, tmp_path, ema_beta, capsys):
    """two epochs at 16 x 16 (grown at epoch 1, fading in; captured graphs replayed) with a checkpoint and a score after each"""
    plain, saved0, lines0, _, _ = two_epochs(ngan, tmp_path, "s000", 0, ema_beta)
    scored, saved1, lines1, tr, f = two_epochs(ngan, tmp_path, "s001", 1, ema_beta)
    assert tr.G.image_size == 16 and tr.has_graph((4, 1, 16, 16)), "the run did not train through a captured graph"
    assert plain == scored, "the monitor series changed when the metric was turned on"
    for k, v in saved0["Generator_state"].items():
        assert torch.equal(v, saved1["Generator_state"][k]), k
    assert "SWD" not in saved0 and not any("SWD" in l for l in lines0)
    entries = saved1["SWD"]
    assert [e["epoch"] for e in entries] == [1, 2] and all(e["image_size"] == 16 and e["levels"] == [16] for e in entries)
    assert all(len(e["swd"]) == 1 and e["swd"][0] > 0 and np.isfinite(e["swd"][0]) for e in entries)
    if ema_beta:
        assert all(len(e["swd_ema"]) == 1 and np.isfinite(e["swd_ema"][0]) and e["swd_ema"] != e["swd"] for e in entries)
    else:
        assert all(e["swd_ema"] is None for e in entries)
    assert sum("SWD" in l for l in lines1) == 2 and all(("averaged generator" in l) == bool(ema_beta) for l in lines1 if "SWD" in l)
    # the eval tool prints the table for the checkpoint, and the averaged generator's after it when asked
    images = str(tmp_path / "images.pt")
    torch.save(torch.rand(8, 1, 16, 16, generator=torch.Generator().manual_seed(9)) * 2 - 1, images)
    capsys.readouterr()
    assert ngan.eval.main(["-weights", f, "--swd", "8", "--images", images] + (["--ema"] if ema_beta else [])) == 0
    out = capsys.readouterr().out
    assert out.count("SWD x 1e3") == (2 if ema_beta else 1) and ("averaged generator" in out) == bool(ema_beta)
    assert all(len(line.split()) == 2 for line in out.splitlines() if line.strip().startswith("16"))      # one level, and the mean
