"""Geometric differentiable augmentation without a GPU: the fp64 restatement of tests/diffgeo_cases.py against torch's grid_sample
(forward, and its adjoint against torch.autograd on that), the per-element bound against an emulation of the kernels' arithmetic,
the parameter arithmetic, the policy names, the host-side refusals of the new entry points, and the trainer's argument checks.  The
kernels themselves are tested on the GPU (test_gpu_diffgeo.py).

The tests that touch only tests/diffgeo_cases.py are self-checks of the reference and pass on any commit; those that take the `ngan`
fixture need the feature."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import diffgeo_cases as A

f64 = np.float64


@functools.lru_cache(maxsize=None)
def case(B, C, R):
    x, gy = A.inputs(B, C, R)
    return x, gy, [(name, rows, {fill: A.fwd_ref(x, rows, fill) for fill in A.FILLS}, A.bwd_ref(gy, rows)) for name, rows in A.tables(B, R)]


@pytest.mark.parametrize("B,C,R", A.SHAPES)
def test_the_restatement_agrees_with_grid_sample(B, C, R):
    """forward: the restatement equals affine_grid + grid_sample on the matching matrix; backward: its adjoint equals torch.autograd
    on that -- in fp64.  grid_sample forms the source position through normalised coordinates, (2 s / (R - 1) - 1 and back): a few
    units of 2^-53 R in the position, times a slope of at most 2 for images in [-1, 1] (1.8 + the fill here), times the summation."""
    x, gy, tabs = case(B, C, R)
    tol = 64 * 2.0 ** -53 * R
    for name, rows, fwd, (gref, _) in tabs:
        for fill in A.FILLS:
            xt = torch.from_numpy(x.astype(f64)).requires_grad_()
            yt = A.transcription(xt, rows, fill)
            (gxt,) = torch.autograd.grad(yt, xt, torch.from_numpy(gy.astype(f64)))
            assert np.abs(yt.detach().numpy() - fwd[fill][0]).max() <= tol * 4, (name, fill)
            assert np.abs(gxt.numpy() - gref).max() <= tol * 4 * np.abs(gy).max() * 16, (name, fill)


@pytest.mark.parametrize("B,C,R", A.SHAPES)
def test_forward_emulation_stays_within_half_the_bound(B, C, R):
    """The emulation of the forward kernel against the restatement, at half the bound, so that the bound is one the reference
    alone meets"""
    x, _, tabs = case(B, C, R)
    worst = max(A.ratio(A.fwd_emulate(x, rows, fill), *fwd[fill]) for _, rows, fwd, _ in tabs for fill in A.FILLS)
    print(f"STAT DIFFGEO emulation {(B, C, R)}: fwd err/bound {worst:.3f}")
    assert worst <= 0.5, worst


@pytest.mark.parametrize("B,C,R", A.SHAPES)
def test_adjoint_emulation_stays_within_half_the_bound(B, C, R):
    _, gy, tabs = case(B, C, R)
    worst = max(A.ratio(A.bwd_emulate(gy, rows), *bwd) for _, rows, _, bwd in tabs)
    print(f"STAT DIFFGEO emulation {(B, C, R)}: adjoint err/bound {worst:.3f}")
    assert worst <= 0.5, worst


@pytest.mark.parametrize("B,C,R", A.SHAPES)
def test_forward_emulation_is_inside_the_bound_and_exact_where_it_is_zero(B, C, R):
    x, gy, tabs = case(B, C, R)
    for name, rows, fwd, (gref, gbd) in tabs:
        for fill in A.FILLS:
            ref, bd = fwd[fill]
            emu = A.fwd_emulate(x, rows, fill)
            assert A.ratio(emu, ref, bd) <= 1.0, (name, fill)
            far = np.stack([np.broadcast_to(~A.plan(tuple(r), R)["near"], (C, R, R)) for r in rows])
            assert (emu[far & (bd == 0)] == np.float32(fill)).all() and (ref[far] == fill).all()
        for n, row in enumerate(rows):
            if A.is_exact(row):                                # zero fractions: bound 0, the values are copied
                assert not fwd[0.0][1][n].any() and not gbd[n].any()
                assert np.array_equal(A.fwd_emulate(x, rows)[n], fwd[0.0][0][n].astype(np.float32))
    x, _ = A.inputs(3, 1, 16)                                  # ... bit for bit, the sign of a zero included
    assert np.signbit(x[x == 0]).any()
    for f in (0, 1):
        for k in range(4):
            want = np.ascontiguousarray(np.rot90(np.flip(x, -1) if f else x, k, axes=(-2, -1)))
            assert np.array_equal(A.fwd_emulate(x, [A.affine_row(16, bool(f), k)] * 3, -1.0).view(np.uint32), want.view(np.uint32))


def test_the_case_tables_cover_what_they_are_named_for():
    for R in (4, 16, 64, 512):
        rows = A.master_rows(R)
        assert len(rows) == 19 and rows[0] == A.IDENTITY and rows[1:9] == A.blit_rows(R) and len(set(rows[1:9])) == 8
        assert all(A.is_exact(r) for r in rows[:9]) and not any(A.is_exact(r) for r in rows[9:])
        assert all(set(r[:2] + r[3:5]) <= {0.0, 1.0, -1.0} and set((r[2], r[5])) <= {0.0, float(R - 1)} for r in rows[:9])
        x = np.arange(R * R, dtype=np.float32).reshape(1, 1, R, R)
        for f in (0, 1):                                       # blit row (f, k) is rot90(flip(x), k)
            for k in range(4):
                want = np.rot90(np.flip(x, -1) if f else x, k, axes=(-2, -1))
                assert np.array_equal(A.fwd_ref(x, [rows[1 + 4 * f + k]])[0], want), (R, f, k)
        # the quarter and half turns through the general path: some coordinate a rounding away from an integer, fractions not all 0
        for r in rows[9:13]:
            pl = A.plan(r, R)
            off = np.minimum(pl["ti"], 1 - pl["ti"])
            assert 0 < off.max() < 1e-6
        sv = [np.linalg.svd(np.array([[r[0], r[1]], [r[3], r[4]]]), compute_uv=False) for r in rows]
        assert min(s.min() for s in sv) >= 2.0 ** -0.351 and max(s.max() for s in sv) <= 2.0 ** 0.351
        fills = [1 - A.plan(r, R)["near"].mean() for r in rows]
        assert R == 4 or (fills[14] > 0.2 and fills[16] > 0.2 and fills[13] < fills[14])       # zoomed out: a fifth or more is fill
    for B, C, R in A.SHAPES:
        used = [r for _, rows in A.tables(B, R) for r in rows]
        assert set(used) == set(A.master_rows(R)) and all(len(rows) == B for _, rows in A.tables(B, R))


def test_ratio_and_bound_behave():
    ref, bd = np.array([1.0, 2.0, -1.0]), np.array([0.5, 0.0, 0.0])
    assert A.ratio(np.array([1.25, 2.0, -1.0]), ref, bd) == 0.5
    assert A.ratio(np.array([1.0, 2.0 + 1e-12, -1.0]), ref, bd) == float("inf")
    x, _ = A.inputs(3, 1, 16)
    rows = A.master_rows(16)[13:16]
    ref, bd = A.fwd_ref(x, rows, -1.0)
    broken = ref.copy()
    broken[1, 0, 5, 5] += 1e-5                                 # two hundred units of 2^-24 in one element
    assert A.ratio(ref.astype(np.float32), ref, bd) <= 0.5 and A.ratio(broken, ref, bd) > 1.0
    transposed = A.fwd_ref(x, [(r[3], r[4], r[5], r[0], r[1], r[2]) for r in rows], -1.0)[0]
    assert A.ratio(transposed, ref, bd) > 1.0                  # the coordinates swapped


def test_parameter_arithmetic_in_numpy():
    R = 16
    one = 1.0 - 2.0 ** -24
    ident = A.params_ref([[0.9] * 8], R, 3, 0.5)
    assert ident == [A.IDENTITY]
    assert A.params_ref([[0.1, 0.1, 0.9, 0, 0, 0, 0, 0]], R, 1, 0.5) == [A.affine_row(R, flip=True)]
    assert A.params_ref([[0.1, 0.5, 0.9, 0, 0, 0, 0, 0]], R, 1, 0.5) == [A.IDENTITY]            # the coin is strict
    assert A.params_ref([[0.5, 0.1, 0.5, 0.9, 0.5, 0.9, 0.5, 0.9]], R, 3, 0.5) == [A.IDENTITY]  # gates at u = p are closed
    for u3, k in ((0.0, 0), (0.25, 1), (0.5, 2), (0.75, 3), (one, 3)):
        assert A.params_ref([[0.9, 0, 0.1, u3, 0.9, 0, 0.9, 0]], R, 3, 0.5) == [A.affine_row(R, k=k)]
    lo, hi = A.params_ref([[0.9, 0, 0.9, 0, 0.1, 0.0, 0.9, 0]], R, 2, 0.5)[0], A.params_ref([[0.9, 0, 0.9, 0, 0.1, one, 0.9, 0]], R, 2, 0.5)[0]
    assert abs(lo[0] - 2.0 ** 0.35) < 1e-6 and abs(hi[0] - 2.0 ** -0.35) < 1e-6 and lo[1] == 0.0 == hi[3]   # zoom in by s: 1 / s
    for u7, theta in ((0.0, -math.pi), (0.5, 0.0), (0.75, math.pi / 2), (one, math.pi)):
        got = A.params_ref([[0.9, 0, 0.9, 0, 0.9, 0, 0.1, u7]], R, 2, 0.5)[0]
        assert np.allclose(got, A.affine_row(R, theta=theta), atol=1e-5)
    assert A.params_ref([[0.1] * 8], R, 0, 1.0) == [A.IDENTITY] == A.params_ref([[0.1] * 8], R, 3, 0.0)
    # composition: blit, then scale, then rotation, about the centre
    got = np.array(A.params_ref([[0.1, 0.1, 0.1, 0.25, 0.1, 0.25, 0.1, 0.6]], R, 3, 0.5)[0])
    F, Q = np.array([[1.0, 0], [0, -1.0]]), np.array([[0.0, 1.0], [-1.0, 0]])
    th, inv = 0.2 * math.pi, 2.0 ** (0.5 * 0.35)
    Amat = F @ Q @ (inv * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]]))
    c = 0.5 * (R - 1)
    want = [Amat[0, 0], Amat[0, 1], c - Amat[0].sum() * c, Amat[1, 0], Amat[1, 1], c - Amat[1].sum() * c]
    assert np.allclose(got, want, atol=4e-6)
    U = A.chosen_uniforms(0.5)
    assert U.shape[1] == 8 and {0.25, 0.5, 0.75} <= set(U[:, 0].tolist())
    assert A.params_close(A.params_ref(U, R, 3, 0.5), A.params_ref(U, R, 3, 0.5), R)
    assert not A.params_close([tuple(v + 1e-5 for v in A.IDENTITY)], [A.IDENTITY], R)


# ---- the product ----------------------------------------------------------------------------------------------------------------------
def test_policy_names(ngan):
    ops = ngan.ops
    assert ops.DIFFAUG_GROUPS == A.GROUPS
    assert ops.diffaug_policy_mask("blit,geometry,color") == 25 == A.policy_mask("blit,geometry,color")
    assert ops.diffaug_policy_mask("blit") == 8 and ops.diffaug_policy_mask(" geometry , blit ") == 24
    assert ops.diffaug_policy_mask("color,translation,cutout,blit,geometry") == 31
    for bad in ("colour", "color;cutout", "saturation", "rotate", "blit geometry", 3):
        with pytest.raises(ValueError, match="diffaug"):
            ops.diffaug_policy_mask(bad)


def test_python_operator_checks_its_arguments(ngan):
    ops = ngan.ops
    rows = A.master_rows(16)
    t = ops.diffgeo_table(rows)
    assert t.dtype == torch.float32 and tuple(t.shape) == (len(rows), 8) and ops.diffgeo_table_rows(t) == rows
    assert bool((t[:, 6:] == 0).all()) and ops.diffgeo_table_rows(ops.diffgeo_table([ops.DIFFGEO_IDENTITY])) == [A.IDENTITY]
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(ValueError, match="table"):
        ops.diffgeo(x, t.int())
    with pytest.raises(ValueError, match="images"):
        ops.diffgeo(x[0], t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # a host tensor never falls back to eager PyTorch
        ops.diffgeo(x, t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.DiffGeometry.apply(x, t, 0.0)


def test_entry_points_are_bound_and_validate_on_the_host(ngan):
    lib = ngan._C.lib()
    err = lib.ngan_last_error
    one = ctypes.c_void_p(64)            # any non-null, 16-byte aligned address: every check below comes before the launch
    odd = ctypes.c_void_p(68)
    N = None
    assert {"ngan_diffgeo_params", "ngan_diffgeo_fwd", "ngan_diffgeo_bwd"} <= set(ngan._C.exported_symbols())
    for fn in (lambda *a: lib.ngan_diffgeo_fwd(*a[:-1], 0.0, a[-1]), lib.ngan_diffgeo_bwd):     # (fwd: fill in front of the stream)
        for args in ((N, one, one), (one, N, one), (one, one, N)):
            assert fn(*args, 2, 1, 16, 16, 2, None) == -1 and b"null" in err()
        assert fn(one, one, one, 2, 1, 16, 32, 2, None) == -2 and b"square" in err()
        for r in (0, 2, 6, 18, 16388):
            assert fn(one, one, one, 2, 1, r, r, 2, None) == -2 and b"R=" in err()
        for b in (0, -1, 65536):
            assert fn(one, one, one, b, 1, 16, 16, 65536, None) == -2 and b"B=" in err()
        assert fn(one, one, one, 2, 0, 16, 16, 2, None) == -2 and b"C=" in err()
        assert fn(one, one, one, 2, 8, 16384, 16384, 2, None) == -2 and b"2^31" in err()
        assert fn(one, one, one, 3, 1, 16, 16, 2, None) == -1 and b"holds 2 rows" in err()      # a table shorter than the batch
        for args in ((odd, one, one), (one, odd, one), (one, one, odd)):
            assert fn(*args, 2, 1, 16, 16, 2, None) == -1 and b"16-byte" in err()
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert lib.ngan_diffgeo_fwd(one, one, one, 2, 1, 16, 16, 2, bad, None) == -1 and b"fill" in err()
    p = lib.ngan_diffgeo_params
    assert p(N, one, 2, 16, 16, 2, 3, 1.0, None) == -1 and b"null" in err()
    assert p(one, N, 2, 16, 16, 2, 3, 1.0, None) == -1 and b"null" in err()
    assert p(one, odd, 2, 16, 16, 2, 3, 1.0, None) == -1 and b"16-byte" in err()
    assert p(one, one, 2, 16, 8, 2, 3, 1.0, None) == -2 and b"square" in err()
    assert p(one, one, 2, 18, 18, 2, 3, 1.0, None) == -2 and b"R=" in err()
    assert p(one, one, 3, 16, 16, 2, 3, 1.0, None) == -1 and b"holds 2 rows" in err()
    for mask in (-1, 4, 8):
        assert p(one, one, 2, 16, 16, 2, mask, 1.0, None) == -1 and b"policy" in err()
    for prob in (-0.1, 1.5, float("nan")):
        assert p(one, one, 2, 16, 16, 2, 3, prob, None) == -1 and b"p=" in err()
    assert lib.ngan_diffaug_params(one, one, 2, 16, 16, 2, 8, 1.0, None) == -1 and b"policy" in err()     # the older kernel's mask stays 0 .. 7


def test_flags_configuration_and_trainer_arguments(ngan):
    cfg, train = ngan.config, ngan.train
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    try:
        argv = ["--diffaug", "blit,geometry,cutout"]
        options = train.build_arg_parser().parse_args(argv)
        over = train.cli_overrides(argv, options, cfg.configs_name)
        assert over == {"diffaug": "blit,geometry,cutout"}
        cfg.set_configs(**over)
        cfg.validate_configs()
        for bad in ("rotate", "blit geometry"):
            cfg.set_configs(diffaug=bad)
            with pytest.raises(ValueError, match="diffaug"):
                cfg.validate_configs()
        cfg.set_configs(diffaug="blit", wgan=True, pggan=False)
        with pytest.raises(ValueError, match="diffaug"):
            cfg.validate_configs()
        with pytest.raises(ValueError, match="diffaug"):
            train.make_trainer(cfg, None, None)
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)
    help_text = train.build_arg_parser().format_help()
    assert all(name in help_text for name in ("color", "translation", "cutout", "blit", "geometry"))
    with pytest.raises(ValueError, match="diffaug"):
        train.WGANTrainer(None, None, diffaug="geometry")
    mk = lambda: (ngan.models.Generator_PG([16, 16], image_size_init=4, latent_dim=32),     # noqa: E731
                  ngan.models.Discriminator_PG([16, 16], image_size_init=4))
    tr = train.PGGANTrainer(*mk(), diffaug="blit,geometry", diffaug_p=0.0)
    assert not tr.diffaug_enabled and tr._aug is None
    tr = train.PGGANTrainer(*mk(), diffaug="geometry,cutout", diffaug_p=0.5, diffaug_seed=3)
    aug = tr._aug
    assert (aug.mask, aug.p, aug.seed, aug.colour) == (20, 0.5, 3, False)
    assert tuple(aug.geo_table.shape) == (train.DIFFAUG_ROWS, 8) == tuple(aug.table.shape) and aug.geo_table.dtype == torch.float32
    assert ngan.ops.diffgeo_table_rows(aug.geo_table[:3]) == [A.IDENTITY] * 3            # identity until the first draw
    ptr = lambda v: (v.data_ptr() - aug.geo_table.data_ptr()) // 32                      # noqa: E731  (the older table's row layout)
    assert [ptr(aug.geo_real(0, 4)), ptr(aug.geo_fake(0, 4)), ptr(aug.geo_real(1, 4)), ptr(aug.geo_gen(4, 2)), ptr(aug.geo_gen(4, 0))] == [0, 4, 12, 24, 12]
    only = train.PGGANTrainer(*mk(), diffaug="blit")._aug
    assert only.table is None and only.uniforms is None and only.real(0, 4) is None and only.gen(4, 1) is None
    old = train.PGGANTrainer(*mk(), diffaug="color")._aug
    assert old.geo_table is None and old.geo_uniforms is None and old.geo_fake(0, 4) is None
