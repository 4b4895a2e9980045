"""Differentiable augmentation without a GPU: the fp64 restatement of tests/diffaug_cases.py against a literal transcription of the
DiffAugment steps in torch operators (forward, and backward against torch.autograd), the per-element bound against an fp32
emulation of the kernels' arithmetic, the host-side refusals of the new entry points, the flags and configuration names, and the
trainers' argument checks, and -- on the CPU oracle, at a depth the small GPU nets do not have -- why the trainer does not fill with
DiffAugment's zeros.  The kernels themselves are tested on the GPU (test_gpu_diffaug.py).

The tests that touch only tests/diffaug_cases.py (restatement against transcription, emulation against restatement, the case tables,
`ratio`, the parameter arithmetic) are self-checks of the reference and pass on any commit; those that take the `ngan` fixture need
the feature."""
import ctypes

import numpy as np
import pytest
import torch

import diffaug_cases as A


def _cases():
    for B, C, R in A.SHAPES:
        for name, rows in A.tables(B, R):
            yield B, C, R, name, rows


def test_the_two_restatements_agree():
    """forward: the restatement equals the transcription; backward: its adjoint equals torch.autograd on the transcription -- in
    fp64, up to the summation order (a few units of 2^-53 of the sums of absolute values)"""
    for B, C, R in A.SHAPES:
        x, gy = A.inputs(B, C, R)
        for name, rows in A.tables(B, R):
          for fill in (0.0, -1.0):                # DiffAugment's own fill and the trainer's; the adjoint does not depend on it
            xt = torch.from_numpy(x.astype(np.float64)).requires_grad_()
            yt = A.transcription(xt, rows, fill)
            (gxt,) = torch.autograd.grad(yt, xt, torch.from_numpy(gy.astype(np.float64)))
            ref, absref = A.fwd_ref(x, rows, fill)
            gref, gabs = A.bwd_ref(gy, rows)
            tol = 64 * 2.0 ** -53
            assert (np.abs(yt.detach().numpy() - ref) <= tol * absref).all(), (B, C, R, name)
            assert (ref[absref == 0] == fill).all()
            assert (np.abs(gxt.numpy() - gref) <= tol * gabs).all(), (B, C, R, name)


def test_the_case_tables_cover_what_they_are_named_for():
    for R in (4, 16, 64, 512):
        S, K = A.shift_size(R), A.cutout_size(R)
        rows = A.master_rows(R)
        assert (S, K) == {4: (1, 2), 16: (2, 8), 64: (8, 32), 512: (64, 256)}[R]
        assert {(r[2], r[3]) for r in rows} >= {(S, -S), (-S, S), (S, S), (-S, -S)}
        assert {r[1] for r in rows} >= {0.5, 1.5} and {r[0] for r in rows} >= {0.5, -0.5}
        assert A.IDENTITY in rows
        boxes = [r[4:] for r in rows if r != A.IDENTITY]
        assert all(0 <= i0 < i1 <= R and 0 <= j0 < j1 <= R for i0, i1, j0, j1 in boxes)
        touches = {(i0 == 0, i1 == R, j0 == 0, j1 == R) for i0, i1, j0, j1 in boxes}
        corners = {(True, False, True, False), (True, False, False, True), (False, True, True, False), (False, True, False, True)}
        edges = {(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)}
        if R > 4:             # (at R = 4 the cutout is 2 x 2: "inside" and the edges coincide with fewer distinct boxes)
            assert touches >= corners | edges | {(False, False, False, False)}, (R, touches)
        # both read paths of the map kernel: a column shift that is a multiple of 4 and one that is not
        if R >= 32:
            assert any(r[3] % 4 == 0 and r[3] != 0 for r in rows) and any(r[3] % 4 for r in rows)
    for B, C, R in A.SHAPES:
        used = [r for _, rows in A.tables(B, R) for r in rows]
        assert set(A.master_rows(R)) <= set(used) and A.tables(B, R)[-1][1] == [A.IDENTITY] * B


@pytest.mark.parametrize("B,C,R", A.SHAPES)
def test_emulation_within_half_the_bound(B, C, R):
    x, gy = A.inputs(B, C, R)
    worst = {"fwd": 0.0, "bwd": 0.0}
    for name, rows in A.tables(B, R):
        for fill in (-1.0, 0.0):
            ref, absref = A.fwd_ref(x, rows, fill)
            em = A.fwd_emulate(x, rows, fill)
            worst["fwd"] = max(worst["fwd"], A.ratio(em, ref, absref))
        gref, gabs = A.bwd_ref(gy, rows)
        gem = A.bwd_emulate(gy, rows)
        worst["bwd"] = max(worst["bwd"], A.ratio(gem, gref, gabs))
        for n, row in enumerate(rows):
            if row == A.IDENTITY:
                assert np.array_equal(em[n], x[n]) and np.array_equal(gem[n], gy[n])
        # the pairing check of the GPU test, rehearsed on the emulation: <T x - T 0, g> = <x, T^T g>
        em0 = A.fwd_emulate(np.zeros_like(x), rows)
        assert A.pairing_defect(x, gy, em, em0, gem) <= A.pairing_slack(x, gy, rows), name
        # ... and it has teeth: the transposed shift is not the adjoint
        if any(r[2] or r[3] for r in rows):
            wrong = A.bwd_emulate(gy, [(r[0], r[1], -r[2], -r[3]) + tuple(r[4:]) for r in rows])
            assert A.pairing_defect(x, gy, em, em0, wrong) > A.pairing_slack(x, gy, rows), name
    print(f"EMULATED diffaug {(B, C, R)}: fwd {worst['fwd']:.3f}, bwd {worst['bwd']:.3f}")
    assert worst["fwd"] <= 0.5 and worst["bwd"] <= 0.5, worst


def test_ratio_rejects_a_nonzero_where_the_definition_says_zero():
    x, _ = A.inputs(3, 1, 16)
    rows = A.tables(3, 16)[0][1]
    ref, absref = A.fwd_ref(x, rows)
    em = A.fwd_emulate(x, rows)
    assert A.ratio(em, ref, absref) <= 0.5
    i = np.argwhere(absref == 0)[0]
    em[tuple(i)] = 1e-30
    assert A.ratio(em, ref, absref) == float("inf")


def test_params_reference_arithmetic():
    """the numpy restatement of ngan_diffaug_params itself: the last uniform below 1 never draws n, gates open below p"""
    top = np.float32(1.0 - 2.0 ** -24)
    for n in (3, 5, 9, 17, 129 * 129, 513):
        assert A.draw_int(np.asarray([0.0, 0.5, top], np.float32), n).tolist() == [0, n // 2 if n % 2 == 0 else int(np.floor(np.float32(0.5) * n)), n - 1]
    U = A.chosen_uniforms()
    for R in (4, 16, 512):
        S = A.shift_size(R)
        for rows in (A.params_ref(U, R, 7, 0.5), A.params_ref(U, R, 7, 1.0)):
            for b, c, tx, ty, i0, i1, j0, j1 in rows:
                assert -0.5 <= b < 0.5 and 0.5 <= c <= 1.5 and -S <= tx <= S and -S <= ty <= S
                assert 0 <= i0 <= i1 <= R and 0 <= j0 <= j1 <= R
        assert A.params_ref(U, R, 7, 0.0) == [A.IDENTITY] * len(U) == A.params_ref(U, R, 0, 1.0)
        half = A.params_ref(U, R, 7, 0.5)
        assert any(r[:2] == (0.0, 1.0) for r in half) and any(r[:2] != (0.0, 1.0) for r in half)


def test_entry_points_are_bound_and_validate_on_the_host(ngan):
    lib = ngan._C.lib()
    err = lib.ngan_last_error
    one = ctypes.c_void_p(64)            # any non-null, 16-byte aligned address: every check below comes before the launch
    odd = ctypes.c_void_p(68)
    N = None
    assert {"ngan_diffaug_params", "ngan_diffaug_fwd", "ngan_diffaug_bwd", "ngan_diffaug_workspace_bytes"} <= set(ngan._C.exported_symbols())
    for fn in (lambda *a: lib.ngan_diffaug_fwd(*a[:-1], 0.0, a[-1]), lib.ngan_diffaug_bwd):     # (fwd: fill in front of the stream)
        for args in ((N, one, one, one), (one, N, one, one), (one, one, N, one)):
            assert fn(*args, 2, 1, 16, 16, 2, 1, None) == -1 and b"null" in err()
        assert fn(one, one, one, N, 2, 1, 16, 16, 2, 1, None) == -1 and b"workspace" in err()       # ... which colour = 0 does not need
        assert fn(one, one, one, one, 2, 1, 16, 32, 2, 1, None) == -2 and b"square" in err()
        for r in (0, 2, 6, 18, 16388):
            assert fn(one, one, one, one, 2, 1, r, r, 2, 1, None) == -2 and b"R=" in err()
        for b in (0, -1, 65536):
            assert fn(one, one, one, one, b, 1, 16, 16, 65536, 1, None) == -2 and b"B=" in err()
        assert fn(one, one, one, one, 2, 0, 16, 16, 2, 1, None) == -2 and b"C=" in err()
        assert fn(one, one, one, one, 2, 8, 16384, 16384, 2, 1, None) == -2 and b"2^31" in err()
        assert fn(one, one, one, one, 3, 1, 16, 16, 2, 1, None) == -1 and b"holds 2 rows" in err()  # a table shorter than the batch
        assert fn(odd, one, one, one, 2, 1, 16, 16, 2, 1, None) == -1 and b"16-byte" in err()
        assert fn(one, one, odd, one, 2, 1, 16, 16, 2, 1, None) == -1 and b"16-byte" in err()
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert lib.ngan_diffaug_fwd(one, one, one, one, 2, 1, 16, 16, 2, 1, bad, None) == -1 and b"fill" in err()
    p = lib.ngan_diffaug_params
    assert p(N, one, 2, 16, 16, 2, 7, 1.0, None) == -1 and b"null" in err()
    assert p(one, N, 2, 16, 16, 2, 7, 1.0, None) == -1 and b"null" in err()
    assert p(one, one, 2, 16, 8, 2, 7, 1.0, None) == -2 and b"square" in err()
    assert p(one, one, 2, 18, 18, 2, 7, 1.0, None) == -2 and b"R=" in err()
    assert p(one, one, 3, 16, 16, 2, 7, 1.0, None) == -1 and b"holds 2 rows" in err()
    for mask in (-1, 8):
        assert p(one, one, 2, 16, 16, 2, mask, 1.0, None) == -1 and b"policy" in err()
    for prob in (-0.1, 1.5, float("nan")):
        assert p(one, one, 2, 16, 16, 2, 7, prob, None) == -1 and b"p=" in err()
    # one partial sum (a double) per 8192 values of a sample
    ws = lib.ngan_diffaug_workspace_bytes
    assert (ws(1, 1, 4), ws(2, 3, 4), ws(5, 1, 64), ws(2, 1, 512), ws(16, 1, 512), ws(3, 1, 128)) == (8, 16, 40, 512, 4096, 48)
    assert ws(0, 1, 16) == 0 and ws(1, 0, 16) == 0 and ws(1, 8, 16384) == 0


def test_python_operator_checks_its_arguments(ngan):
    ops = ngan.ops
    assert ops.diffaug_policy_mask("") == 0 and ops.diffaug_policy_mask(None) == 0
    assert ops.diffaug_policy_mask("color,translation,cutout") == 7 and ops.diffaug_policy_mask(" cutout , color") == 5
    for bad in ("colour", "color;cutout", "saturation", 3):
        with pytest.raises(ValueError, match="diffaug"):
            ops.diffaug_policy_mask(bad)
    rows = A.master_rows(16)
    t = ops.diffaug_table(rows)
    assert t.dtype == torch.int32 and tuple(t.shape) == (len(rows), 8) and ops.diffaug_table_rows(t) == [tuple(r) for r in rows]
    assert ops.diffaug_table_rows(ops.diffaug_table([ops.DIFFAUG_IDENTITY])) == [A.IDENTITY]
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(ValueError, match="table"):
        ops.diffaug(x, t.float())
    with pytest.raises(ValueError, match="images"):
        ops.diffaug(x[0], t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # a host tensor never falls back to eager PyTorch
        ops.diffaug(x, t)


def test_flags_and_configuration_names(ngan):
    cfg, train = ngan.config, ngan.train
    saved = {k: getattr(cfg, k) for k in cfg.configs_name}
    try:
        assert (cfg.configs_name["diffaug"], cfg.configs_name["diffaug_p"], cfg.configs_name["diffaug_seed"]) == ("", 1.0, 0)
        argv = ["--diffaug", "color,translation,cutout", "--diffaug_p", "0.5", "--diffaug_seed", "7"]
        options = train.build_arg_parser().parse_args(argv)
        over = train.cli_overrides(argv, options, cfg.configs_name)
        assert over == {"diffaug": "color,translation,cutout", "diffaug_p": 0.5, "diffaug_seed": 7}
        none = train.cli_overrides([], train.build_arg_parser().parse_args([]), cfg.configs_name)
        assert not {"diffaug", "diffaug_p", "diffaug_seed"} & set(none)
        cfg.set_configs(**over)
        cfg.validate_configs()
        assert (cfg.diffaug, cfg.diffaug_p, cfg.diffaug_seed) == ("color,translation,cutout", 0.5, 7)
        for name, bad in (("diffaug", "colour"), ("diffaug", "color cutout"), ("diffaug", None), ("diffaug_p", -0.1), ("diffaug_p", 1.5),
                          ("diffaug_p", True), ("diffaug_seed", -1), ("diffaug_seed", 0.5), ("diffaug_seed", True)):
            cfg.set_configs(**over)
            cfg.set_configs(**{name: bad})
            with pytest.raises(ValueError, match=name):
                cfg.validate_configs()
        # the WGAN nets: refused by the configuration and by the trainer that make_trainer would build
        cfg.set_configs(**over)
        cfg.set_configs(wgan=True, pggan=False)
        with pytest.raises(ValueError, match="diffaug"):
            cfg.validate_configs()
        with pytest.raises(ValueError, match="diffaug"):
            train.make_trainer(cfg, None, None)
        cfg.set_configs(diffaug="")
        cfg.validate_configs()
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)


def test_trainer_arguments_are_validated(ngan):
    train = ngan.train
    mk = lambda: (ngan.models.Generator_PG([16, 16], image_size_init=4, latent_dim=32),     # noqa: E731
                  ngan.models.Discriminator_PG([16, 16], image_size_init=4))
    for kw in ({}, {"diffaug": ""}, {"diffaug": "color,cutout", "diffaug_p": 0.0}, {"diffaug": " , "}):
        tr = train.PGGANTrainer(*mk(), **kw)
        assert not tr.diffaug_enabled and tr._aug is None                  # off: no buffer, no generator
        tr.reseed_diffaug(3)
        tr.draw_diffaug_tables(4)
        with pytest.raises(ValueError, match="without a diffaug policy"):
            tr.draw_diffaug_tables(4, {"gen": None})
    for kw in ({"diffaug": "colour"}, {"diffaug": "color", "diffaug_p": 1.5}, {"diffaug": "color", "diffaug_p": -1},
               {"diffaug": "color", "diffaug_seed": -1}, {"diffaug": "color", "diffaug_seed": 1.5}):
        with pytest.raises(ValueError, match="diffaug"):
            train.PGGANTrainer(*mk(), **kw)
    tr = train.PGGANTrainer(*mk(), diffaug="translation,cutout", diffaug_p=0.5, diffaug_seed=3)
    aug = tr._aug
    assert tr.diffaug_enabled and (aug.mask, aug.p, aug.seed, aug.colour) == (6, 0.5, 3, False)
    assert tuple(aug.table.shape) == (train.DIFFAUG_ROWS, 8) and aug.table.dtype == torch.int32
    assert ngan.ops.diffaug_table_rows(aug.table[:3]) == [A.IDENTITY] * 3                # identity until the first draw
    # the row layout of an iteration: per critic step b reals and 2 b generated, then the generator step's b
    ptr = lambda v: (v.data_ptr() - aug.table.data_ptr()) // 32                              # noqa: E731
    assert [ptr(aug.real(0, 4)), ptr(aug.fake(0, 4)), ptr(aug.real(1, 4)), ptr(aug.gen(4, 2)), ptr(aug.gen(4, 0))] == [0, 4, 12, 24, 12]
    assert (len(aug.real(1, 4)), len(aug.fake(1, 4)), len(aug.gen(4, 2)), aug.rows(4, 2), aug.rows(4, 0)) == (4, 8, 4, 28, 16)
    with pytest.raises(ValueError, match="table rows"):
        aug.prepare(train.DIFFAUG_ROWS // 4 + 1, 1, 4)
    # the private stream: seeded from (seed, epoch, rank), distinct per rank and epoch, and never the global one
    seeds = {train.diffaug_stream_seed(s, e, r) for s in (0, 3) for e in (0, 1, 2) for r in (0, 1)}
    assert len(seeds) == 12
    state = torch.get_rng_state()
    tr.reseed_diffaug(2)
    a = aug.generator.get_state()
    tr.reseed_diffaug(2, rank=0)
    assert torch.equal(a, aug.generator.get_state()) and aug.generator.initial_seed() == train.diffaug_stream_seed(3, 2, 0)
    tr.reseed_diffaug(2, rank=1)
    assert aug.generator.initial_seed() == train.diffaug_stream_seed(3, 2, 1)
    assert torch.equal(state, torch.get_rng_state())
    with pytest.raises(ValueError, match="diffaug"):
        train.WGANTrainer(None, None, diffaug="color")


def test_why_the_trainer_does_not_fill_with_zeros():
    """A critic of six blocks at 128 x 128 on the CPU oracle, T with a 64 x 64 cutout: with DiffAugment's zero fill the patch's pixels
    have all-zero feature vectors (the biases start at zero), PixelNorm's derivative there is rsqrt(eps) = 1e4 per block, and the
    penalty's input-gradient norm leaves every sane range; with the trainer's fill it stays where the un-augmented image's is."""
    from oracle import pggan_oracle as O
    from __graft_entry__ import load_package
    ngan = load_package()
    fill = ngan.loss_functions.DIFFAUG_FILL
    assert fill == -1.0 and ngan.loss_functions.DiffAugmentHook().fill == fill
    torch.manual_seed(3)
    D = ngan.models.Discriminator_PG([16, 16, 32, 32, 64, 128], image_size_init=4)
    D.set_resolution(128, 1.0)
    pd = O.as_leaf_params({k: v.detach().clone() for k, v in D.state_dict().items()})
    spec = O.NetSpec(image_size_init=4, slope=0.2, alpha=1.0)
    x = torch.rand(2, 1, 128, 128) * 2 - 1
    rows = [(0.25, 1.25, 16, -16) + A.cutout_box(64, 64, 128), (-0.5, 0.5, -3, 5) + A.cutout_box(40, 90, 128)]
    eps = torch.tensor([0.3, 0.7]).view(2, 1, 1, 1)

    def penalty_norms(f):
        # x_hat between two augmented images whose cutouts overlap (the same rows): the penalty's input (loss_functions.py:171-176)
        x_hat = (eps * A.transcription(x, rows, f) + (1 - eps) * A.transcription(-x, rows, f)).requires_grad_()
        (g,) = torch.autograd.grad(O.discriminator_forward(pd, x_hat, spec).sum(), x_hat)
        return g.norm(2, dim=(1, 2, 3))

    xr = x.clone().requires_grad_()
    (g0,) = torch.autograd.grad(O.discriminator_forward(pd, xr, spec).sum(), xr)
    plain = g0.norm(2, dim=(1, 2, 3))
    good, zero = penalty_norms(fill), penalty_norms(0.0)
    print("DIFFAUG depth: plain", plain.tolist(), "fill", good.tolist(), "zero fill", zero.tolist())
    assert bool(torch.isfinite(good).all()) and bool((good < 10 * plain.max()).all()), (good, plain)
    assert bool((zero > 1e4 * plain.max()).all()), (zero, plain)       # the failure the fill exists for
