"""The sliced Wasserstein distance without a GPU: the restatement of tests/swd_cases.py against scipy and a hand-worked case, host-side
validation of the new entry points, the configuration names and flags, the checkpoint key, and the fp32 emulations of the kernels
against the fp64 restatement (every emulated err / bound is at most 0.5: the constants are settled here, before a kernel is looked
at).  The kernels themselves are tested on the GPU (tests/test_gpu_swd.py)."""
import ctypes

import numpy as np
import pytest
import torch

import swd_cases as S
from swd_cases import N_ROUND, ratio

f32 = np.float32


def test_filter_and_boundary_agree_with_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    x = S.images(3, 2, 16, 3).double()
    k1 = np.array(S.GAUSS) / 16.0
    want = np.stack([np.stack([ndimage.convolve(x[b, :, :, c].numpy(), np.outer(k1, k1), mode="mirror") for c in range(3)], -1)
                     for b in range(2)])
    got = S.gauss_filter(x).numpy()
    assert np.abs(got - want).max() < 1e-14
    # the edge sample is not repeated: row 0 of the filtered image weighs rows 2 1 0 1 2
    col = torch.zeros(1, 16, 16, 1, dtype=torch.float64)
    col[0, 1] = 1.0
    assert abs(float(S.gauss_filter(col)[0, 0, 8, 0]) - 8.0 / 16.0) < 1e-15        # rows -1 and 1 both read row 1: 4/16 + 4/16
    # the fused upsample's parity taps are the zero-insert filter's: even 1/8 6/8 1/8, odd 1/2 1/2, the last even sample mirrors inwards
    c = torch.arange(8, dtype=torch.float64).view(1, 8, 1, 1).expand(1, 8, 8, 1)
    up = S.pyr_up_ref(c)[0, :, 0, 0]
    assert torch.allclose(up[2:13:2], torch.arange(1, 7, dtype=torch.float64), atol=1e-14)
    assert torch.allclose(up[1:14:2], torch.arange(7, dtype=torch.float64) + 0.5, atol=1e-14)
    assert abs(float(up[0]) - 0.25) < 1e-14 and abs(float(up[14]) - (6 * 7 + 6 + 7) / 8) < 1e-14 and abs(float(up[15]) - 7.0) < 1e-14


def test_hand_worked_one_dimensional_case():
    """two sets of three descriptors, one direction: sorted 1 3 6 against 2 5 6 -> (1 + 2 + 0) / 3 = 1"""
    a, b = torch.tensor([[3.0, 1.0, 6.0]]), torch.tensor([[6.0, 2.0, 5.0]])
    assert S.sorted_distance(a, b) == 1.0
    assert S.sorted_distance(a, a) == 0.0
    # through the whole restatement: descriptors whose 49 values all equal t project on the direction e / 7 to 7 (t - mean) / std
    t_a, t_b = torch.tensor([3.0, 1.0, 6.0], dtype=torch.float64), torch.tensor([6.0, 2.0, 5.0], dtype=torch.float64)
    da, db = t_a[:, None].expand(3, 49).contiguous(), t_b[:, None].expand(3, 49).contiguous()
    dirs = torch.full((49, 1), 1.0 / 7.0, dtype=torch.float64)
    na = (t_a - t_a.mean()) / t_a.var(unbiased=False).sqrt()
    nb = (t_b - t_b.mean()) / t_b.var(unbiased=False).sqrt()
    want = 7.0 * float((na.sort().values - nb.sort().values).abs().mean())
    assert abs(S.swd_ref(da, db, dirs) - want) < 1e-12


def test_entry_points_are_bound_and_validate_on_the_host(ngan):
    lib = ngan._C.lib()
    one = ctypes.c_void_p(64)            # any non-null 16-byte aligned address: every check below comes before the launch
    N = None
    err = lambda: lib.ngan_last_error()  # noqa: E731
    # null pointers
    assert lib.ngan_swd_pyr_down(N, one, 1, 16, 16, 1, None) < 0 and b"null" in err()
    assert lib.ngan_swd_laplacian(one, N, one, 1, 16, 16, 1, None) < 0 and b"null" in err()
    pos = (ctypes.c_int * 6)(0, 0, 0, 0, 9, 9)
    pos_p = ctypes.cast(pos, ctypes.c_void_p)
    assert lib.ngan_swd_descriptors(one, pos_p, one, one, N, one, 2, 0, 0, 1, 16, 16, 1, None) < 0 and b"null" in err()
    assert lib.ngan_swd_descriptors(one, N, one, one, one, one, 2, 0, 0, 1, 16, 16, 1, None) < 0 and b"null" in err()
    assert lib.ngan_swd_project(one, one, N, one, 4, 4, 1, 1, None) < 0 and b"null" in err()
    assert lib.ngan_swd_sort_columns(N, 1, 4, None) < 0 and b"null" in err()
    assert lib.ngan_swd_l1(one, one, N, one, 4, 4, 1, None) < 0 and b"null" in err()
    # colour counts other than 1 and 3
    for c in (0, 2, 4):
        assert lib.ngan_swd_pyr_down(one, one, 1, 16, 16, c, None) < 0 and b"C=" in err()
        assert lib.ngan_swd_laplacian(one, one, one, 1, 16, 16, c, None) < 0 and b"C=" in err()
        assert lib.ngan_swd_descriptors(one, pos_p, one, one, one, one, 2, 0, 0, 1, 16, 16, c, None) < 0 and b"C=" in err()
        assert lib.ngan_swd_project(one, one, one, one, 4, 4, 1, c, None) < 0 and b"C=" in err()
        assert lib.ngan_swd_descriptors_workspace_bytes(4, c) == 0
    # odd sizes
    assert lib.ngan_swd_pyr_down(one, one, 1, 17, 16, 1, None) < 0 and b"H=17" in err()
    assert lib.ngan_swd_pyr_down(one, one, 1, 16, 15, 1, None) < 0 and b"W=15" in err()
    assert lib.ngan_swd_laplacian(one, one, one, 1, 17, 16, 3, None) < 0 and b"H=17" in err()
    # n_pad not a power of two, or below n
    assert lib.ngan_swd_project(one, one, one, one, 5, 6, 1, 1, None) < 0 and b"n_pad=6" in err()
    assert lib.ngan_swd_project(one, one, one, one, 5, 4, 1, 1, None) < 0 and b"n_pad=4" in err()
    assert lib.ngan_swd_sort_columns(one, 1, 12, None) < 0 and b"n_pad=12" in err()
    assert lib.ngan_swd_sort_columns(ctypes.c_void_p(68), 1, 16, None) < 0 and b"aligned" in err()
    # patch corners out of range: the second patch (0, 9, 9) is legal in a 16 x 16 image, (0, 10, 9) is not, nor is image 1 of 1
    for bad in ((0, 10, 9), (0, 9, 10), (0, -1, 0), (1, 0, 0), (-1, 0, 0)):
        pos[3], pos[4], pos[5] = bad
        assert lib.ngan_swd_descriptors(one, pos_p, one, one, one, one, 2, 0, 0, 1, 16, 16, 1, None) == -1
        assert b"patch 1" in err() and b"out of range" in err()
    assert lib.ngan_swd_descriptors(one, pos_p, one, one, one, one, 2, -1, 0, 1, 16, 16, 1, None) < 0
    assert lib.ngan_swd_descriptors(one, pos_p, one, one, one, one, 2, 0, 0, 1, 6, 16, 1, None) < 0 and b"7 x 7" in err()
    # sizes of the workspaces and of the LDS block
    assert lib.ngan_swd_descriptors_workspace_bytes(64, 1) == 16 and lib.ngan_swd_descriptors_workspace_bytes(65, 3) == 96
    assert lib.ngan_swd_l1_workspace_bytes(4096, 3) == 24 and lib.ngan_swd_l1_workspace_bytes(4097, 3) == 48
    blk = lib.ngan_swd_sort_block_elements()
    assert blk & (blk - 1) == 0 and 4 * blk <= 160 * 1024
    # the Python wrappers refuse host tensors (no CPU fallback) and malformed arguments
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ngan.metrics.pyr_down(torch.zeros(1, 16, 16, 1))
    with pytest.raises(ValueError):
        ngan.metrics.pyr_down(torch.zeros(1, 16, 16, 2))
    with pytest.raises(ValueError):
        ngan.metrics.SWD(64, nhood_size=5)
    with pytest.raises(ValueError):
        ngan.metrics.SWD(48)


def test_metric_object_on_the_host(ngan):
    """levels, the private generator and the answer for a stage below 16 x 16 need no GPU"""
    M = ngan.metrics
    state = torch.get_rng_state()
    m = M.SWD(64, n_colors=3, nhoods_per_image=5, dir_repeats=2, dirs_per_repeat=8, seed=4, device="cpu")
    assert m.levels == [64, 32, 16] and [tuple(d.shape) for d in m.dirs] == [(147, 16)] * 3
    for d in m.dirs:
        assert d.dtype == torch.float32 and torch.allclose(d.square().sum(0), torch.ones(16), atol=1e-6)
    pos = m.draw_positions(3, 16)
    assert tuple(pos.shape) == (15, 3) and pos.dtype == torch.int32
    assert pos[:, 0].tolist() == [0] * 5 + [1] * 5 + [2] * 5 and int(pos[:, 1:].min()) >= 0 and int(pos[:, 1:].max()) <= 9
    m2 = M.SWD(64, n_colors=3, nhoods_per_image=5, dir_repeats=2, dirs_per_repeat=8, seed=4, device="cpu")
    assert all(torch.equal(a, b) for a, b in zip(m.dirs, m2.dirs)) and torch.equal(m2.draw_positions(3, 16), pos)
    assert torch.equal(torch.get_rng_state(), state), "the global generator was consumed"
    small = M.SWD(8, device="cpu")
    small.feed("real", torch.zeros(2, 1, 8, 8))
    res = small.result()
    assert res["levels"] == [] and res["swd"] == [] and res["mean"] is None and "16 x 16" in res["note"]
    assert "16 x 16" in M.format_table(res)
    with pytest.raises(ValueError, match="feed both sets"):
        M.SWD(16, device="cpu").result()
    assert M.channels_last(torch.zeros(2, 1, 16, 16)).shape == (2, 16, 16, 1)
    x = torch.rand(2, 3, 16, 16)
    assert torch.equal(M.channels_last(x), x.permute(0, 2, 3, 1)) and torch.equal(M.channels_last(x.permute(0, 2, 3, 1)), x.permute(0, 2, 3, 1))
    assert M.next_pow2(120) == 128 and M.next_pow2(128) == 128 and M.next_pow2(1) == 1


def test_flags_and_configuration_names(ngan):
    cfg, train = ngan.config, ngan.train
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    try:
        assert (cfg.configs_name["swd_period"], cfg.configs_name["swd_images"], cfg.configs_name["swd_seed"]) == (0, 8192, 0)
        none = train.cli_overrides([], train.build_arg_parser().parse_args([]), cfg.configs_name)
        assert not any(k.startswith("swd") for k in none)
        argv = ["--swd_period", "2", "--swd_images", "256", "--swd_seed", "7"]
        over = train.cli_overrides(argv, train.build_arg_parser().parse_args(argv), cfg.configs_name)
        assert over == {"swd_period": 2, "swd_images": 256, "swd_seed": 7}
        cfg.set_configs(**over)
        cfg.validate_configs()
        assert (cfg.swd_period, cfg.swd_images, cfg.swd_seed) == (2, 256, 7)
        for name, bad in (("swd_period", -1), ("swd_images", 0), ("swd_seed", -3), ("swd_period", 1.5)):
            cfg.set_configs(**{**over, name: bad})
            with pytest.raises(ValueError, match=name):
                cfg.validate_configs()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    p = ngan.eval.build_arg_parser()
    d = p.parse_args([])
    assert (d.swd, d.dataset_dir, d.images, d.swd_seed) == (None, "", "", 0)
    assert p.parse_args(["--swd"]).swd == 8192
    o = p.parse_args(["--swd", "512", "--ema", "--dataset_dir", "d", "--images", "x.pt"])
    assert (o.swd, o.ema, o.dataset_dir, o.images) == (512, True, "d", "x.pt")


def nets(ngan, seed):
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([16, 16, 16], image_size_init=4, latent_dim=32)
    D = ngan.models.Discriminator_PG([16, 16, 16], image_size_init=4)
    return G, D


def test_checkpoint_key_round_trip(ngan, tmp_path):
    utils = ngan.utils
    G, D = nets(ngan, 1)
    f = str(tmp_path / "GenDisc_s.pth")
    ck = utils.Checkpointer(G, D, 1e-4, f, N_epochs=10, verbose=False)
    ck.save_state(1)
    assert "SWD" not in utils.load_checkpoint_dict(f)                 # nothing scored: the file of a build without the feature
    entries = [{"epoch": 2, "image_size": 16, "levels": [16], "swd": [151.25], "swd_ema": None},
               {"epoch": 4, "image_size": 32, "levels": [32, 16], "swd": [180.5, 160.0], "swd_ema": [170.5, 150.0]}]
    ck.SWD.extend(entries)
    ck.save_state(4)
    assert utils.load_checkpoint_dict(f)["SWD"] == entries             # the weights-only unpickler accepts the key
    G2, D2 = nets(ngan, 2)
    ck2 = utils.Checkpointer(G2, D2, 1e-4, f, N_epochs=10, verbose=False)
    ck2.load_state()
    assert ck2.SWD == entries and ck2.epoch == 4
    ck2.SWD.append({"epoch": 6, "image_size": 32, "levels": [32, 16], "swd": [1.0, 2.0], "swd_ema": None})
    ck2.save_state(6)                                                  # a resumed run continues the list
    assert [e["epoch"] for e in utils.load_checkpoint_dict(f)["SWD"]] == [2, 4, 6]
    # a checkpoint without the key loads as before, and loading weights only (weights_init) leaves the list alone
    f0 = str(tmp_path / "GenDisc_0.pth")
    utils.Checkpointer(G, D, 1e-4, f0, N_epochs=10, verbose=False).save_state(3)
    ck3 = utils.Checkpointer(G2, D2, 1e-4, f0, N_epochs=10, verbose=False)
    ck3.load_state()
    assert ck3.SWD == [] and ck3.epoch == 3
    ck3.load_state(f)
    assert ck3.SWD == [] and ck3.epoch == 3
    assert all(torch.equal(a, b) for a, b in zip(G2.state_dict().values(), G.state_dict().values()))


# ---- the emulations against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.PYR_COLORS)
@pytest.mark.parametrize("size", S.PYR_SIZES)
def test_pyramid_emulations_within_half_the_bound(size, c):
    x = S.images(S.seed_of(1, size, c), S.PYR_B, size, c)
    down = S.pyr_down_emu(x.numpy())
    r = ratio(down, S.pyr_down_ref(x).numpy(), S.pyr_down_ref(x.abs()).numpy(), N_ROUND["pyr_down"])
    assert r <= 0.5, f"pyr_down {size} C={c}: {r:.3f}"
    coarse = torch.from_numpy(down)                                    # the kernel's own input: the fp32 coarse image
    r = ratio(S.laplacian_emu(x.numpy(), down), S.laplacian_ref(x, coarse).numpy(), S.laplacian_abs(x, coarse).numpy(),
              N_ROUND["laplacian"])
    assert r <= 0.5, f"laplacian {size} C={c}: {r:.3f}"


@pytest.mark.parametrize("c", S.PYR_COLORS)
@pytest.mark.parametrize("n_dirs", S.PROJ_DIRS)
def test_projection_emulation_within_half_the_bound(n_dirs, c):
    lap = S.pyramid_ref(S.images(S.seed_of(2, c), 5, 32, c), 2)[0].float()
    desc = S.descriptors_ref(lap, S.corner_positions(S.seed_of(3, c), 5, 32, 24))
    dirs = S.directions(S.seed_of(4, n_dirs, c), 49 * c, 1, n_dirs)
    ref, absref = S.project_ref(desc, dirs)
    r = ratio(S.project_emu(desc.numpy(), dirs.numpy()), ref.numpy(), absref.numpy(), N_ROUND["project"])
    assert r <= 0.5, f"project n_dirs={n_dirs} C={c}: {r:.3f}"


@pytest.mark.parametrize("kind", ("tanh", "smooth"))
@pytest.mark.parametrize("c", S.PYR_COLORS)
@pytest.mark.parametrize("size", S.METRIC_SIZES)
def test_metric_emulation_within_half_the_bound(size, c, kind):
    args = S.metric_inputs(size, c, kind)
    ref = S.metric_ref(*args)
    emu = S.metric_emu(*args)
    for level, (val, absref), got in zip(S.levels_of(size), ref, emu):
        assert np.isfinite(val) and val > 0
        r = ratio(np.array([got]), np.array([val]), np.array([absref]), N_ROUND["metric"])
        print(f"metric {size} C={c} {kind} level {level}: ref {val:.6f} emu {got:.6f} err/bound {r:.4f}")
        assert r <= 0.5, f"metric {size} C={c} {kind} level {level}: {r:.3f}"
