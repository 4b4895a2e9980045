"""The index-width table of DESIGN.md section 2 against the library, without a GPU: every limit of tests/large_offset_cases.ROWS is
refused at its first bad shape with NGAN_ERR_SHAPE and a message that names it, every in-scope symbol of include/*.h has a row, and
the table printed in DESIGN.md is the one the tests enforce.

The entry points are called as tests/test_diffaug_cpu.py calls them: dummy non-null, 16-byte aligned pointers, because every check
under test comes before the launch.  Only REFUSED shapes are ever passed: an accepted one would launch on those pointers.  A guard
that is missing therefore shows up here as a status other than -2 (on a machine without a GPU: the launch error), never on a GPU.
The first bad shape is derived from the row's formula (Limit.first_bad), not from the library's message."""
import ctypes
import os

import pytest

import large_offset_cases as L
from conftest import ROOT
from test_host_cpu import _abi_prototypes

FLOATS = {"slope": 0.2, "eps": 1e-8, "scale": 1.0, "momentum": 0.1}


def _call(lib, protos, name, dims):
    """the entry point with dummy pointers, the named integer arguments of `dims` (0 for a name it does not give) and a null stream"""
    _, params = protos[name]
    assert params[-1] == ("void*", "stream"), name
    args = []
    for t, pname in params[:-1]:
        if t.endswith("*"):
            args.append(ctypes.c_void_p(64))
        elif t in ("float", "double"):
            args.append(FLOATS.get(pname, 1.0))
        else:
            args.append(int(dims.get(pname, 0)))
    return getattr(lib, name)(*args, None)


@pytest.fixture(scope="module")
def protos():
    return _abi_prototypes()


def test_every_in_scope_symbol_has_a_row_and_every_row_names_a_symbol(protos):
    launching = {n for n, (ret, params) in protos.items() if ret == "int" and params and params[-1] == ("void*", "stream")}
    scope = {n for n in launching if L.in_scope(n)}
    named = {s for r in L.ROWS for s in r.symbols}
    assert named - set(protos) == set(), "rows name symbols the headers do not declare"
    assert scope - named == set(), "in-scope entry points without a row"
    assert named - scope == set(), "rows for entry points outside the stated scope"
    # the scope patterns themselves: each matches something, and the families the issue lists are all there
    for p in L.IN_SCOPE:
        assert any(p.fullmatch(n) for n in launching), p.pattern
    assert len(scope) == 67, sorted(scope)
    for family in ("conv3x3_fwd_ex", "bf16_conv3x3_wgrad", "lrelu_pixelnorm_bwdbwd", "bf16_channel_sum_acc", "from_image_dw_acc", "to_image_bwd_pnbwd_acc",
                   "up2_adjoint_pnbwd", "bf16_pool2_adjoint", "bf16_lerp", "fade_bwd", "first_block_dx", "mbstd_bwdbwd", "stdfield_dw", "s2_wgrad",
                   "bn_stats", "bn_act_bwd", "chan_sum", "tanh_bwd"):
        assert "ngan_" + family in scope, family
    # out of scope by the module's statement: nothing of these families slipped in
    for n in scope:
        assert not any(k in n for k in ("diffaug", "diffgeo", "augment", "swd", "msssim", "spectrum", "morph", "specloss", "simloss", "ada",
                                        "adam", "rmsprop", "ema", "linear", "final_dot")), n


def test_the_design_table_is_the_one_under_test():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    for line in L.design_table().splitlines():
        assert line in text, f"DESIGN.md section 2 does not print this row of large_offset_cases.ROWS:\n{line}"


LIMITS = [(r, lim, v) for r in L.ROWS for lim in r.limits for v in lim.variants]


@pytest.mark.parametrize("row,lim,variant", LIMITS, ids=[f"{r.symbols[0][5:]}-{lim.vary}-{i}" for i, (r, lim, v) in enumerate(LIMITS)])
def test_first_shape_past_each_limit_is_refused(ngan, protos, row, lim, variant):
    lib = ngan._C.lib()
    bad, good = lim.first_bad(variant)
    assert lim.value(good) < lim.bound <= lim.value(bad) and bad[lim.vary] == good[lim.vary] + 1, (lim.text, good, bad)
    called = 0
    for name in row.symbols:
        _, params = protos[name]
        ints = {p for t, p in params if not t.endswith("*") and t not in ("float", "double")}
        if lim.vary not in ints:
            continue                                    # (a limit on an argument this member of the row does not take)
        status = _call(lib, protos, name, bad)
        err = lib.ngan_last_error()
        assert status == L.NGAN_ERR_SHAPE, (name, lim.text, bad, status, err)
        assert lim.token in err and L.message_is_of(name, err), (name, lim.text, bad, err)       # this guard of this entry point, by its own words
        called += 1
    assert called, (row.symbols, lim.text)


def test_the_crossing_shapes_cross_what_they_are_named_for():
    e = lambda s: s[1] * s[2] * s[3]                                                           # noqa: E731
    for shape in (L.LARGE, L.LARGE_32, L.RAGGED, L.SMALL, L.SMALL_WIDE):
        assert L.crosses(shape[0], e(shape), 4) == (True, True, True), shape
        assert L.crosses(shape[0] - 1, e(shape), 4)[2] is False or shape == L.RAGGED, shape     # the smallest batch that does
    assert L.crosses(L.LARGE[0], e(L.LARGE), 2) == (True, True, True)                            # bf16: T2 = T3 at image 32
    assert L.boundary_images(33, e(L.LARGE), 4) == [0, 7, 8, 15, 16, 31, 32]
    assert L.boundary_images(33, e(L.LARGE), 2) == [0, 15, 16, 31, 32]
    assert L.boundary_images(8193, e(L.SMALL), 4) == [0, 2047, 2048, 4095, 4096, 8191, 8192]
    assert L.boundary_images(34, e(L.LARGE), 4) == [0, 7, 8, 15, 16, 31, 32, 33]
    # the resampling operators' second case: the SMALLER side crosses T3, the larger holds 34 GB and stays below the memory cap
    small = L.BOTH_SIDES_B * e(L.LARGE_LOW)
    assert small > L.T3 and (L.BOTH_SIDES_B - 1) * e(L.LARGE_LOW) <= L.T3 and 4 * e(L.LARGE_LOW) == e(L.LARGE)
    assert (L.BOTH_SIDES_B + 2) * e(L.LARGE) * 4 + small * 4 + 2 * L.LARGE_CHUNK * e(L.LARGE) * 4 < L.MEMORY_CAP      # with guards and a chunk's twin
    # the grid edge: the last accepted row count of from_image_fwd, on a shape every other limit of its row accepts
    B, H, W, C = L.GRID_EDGE
    (row,) = L.rows_of("ngan_from_image_fwd")
    d = dict(B=B, H=H, W=W, C=C)
    assert B * H == 65535 and all(lim.value(d) < lim.bound for lim in row.limits)
    for shape, accepted in ((L.FROM_IMAGE, True), (L.LARGE, False)):          # the large-image shape FromImage takes, and the one it refuses
        d = dict(B=shape[0], H=shape[1], W=shape[2], C=shape[3])
        assert all(lim.value(d) < lim.bound for lim in row.limits) is accepted and e(shape) == e(L.LARGE), shape
    d = dict(zip("BHWC", L.FROM_IMAGE_WIDE))
    assert all(lim.value(d) < lim.bound for lim in row.limits) and L.crosses(d["B"], e(L.FROM_IMAGE_WIDE), 4)[2]
    assert (2 * 64 - 1) * e(L.FROM_IMAGE_WIDE) * 4 < L.T1
    # chunks of the twin launches stay below every threshold, the last one included (it takes the remainder: below two chunks)
    for chunk, shape in ((L.LARGE_CHUNK, L.RAGGED), (L.SMALL_CHUNK, L.SMALL), (L.SMALL_CHUNK, L.SMALL_WIDE)):
        assert (2 * chunk - 1) * e(shape) * 4 < L.T1, shape


@pytest.mark.parametrize("variant", ["int_elements", "int_bytes", "unsigned_bytes"])
def test_a_wrapped_index_moves_a_boundary_image(variant):
    """Arithmetic only, no operator emulation (the audit's fixes were refusals, so there is no value defect to plant): an index formed
    in 32 bits first goes wrong in an image that check (b) looks at (and check (c) sees every later one), and the image before it --
    which is right -- is looked at too: the test would tell "wraps at the threshold" from "wrong everywhere".  The suite's largest
    tensor before this module shows no variant anything."""
    for shape, itemsize in ((L.LARGE, 4), (L.LARGE, 2), (L.LARGE_32, 4), (L.SMALL, 4), (L.SMALL_WIDE, 4), (L.SMALL_WIDE, 2), (L.RAGGED, 4)):
        B, elems = shape[0], shape[1] * shape[2] * shape[3]
        if itemsize == 2 and shape == L.SMALL_WIDE:
            B = 2 * B - 1
        wrong = L.images_a_variant_gets_wrong(B, elems, itemsize, variant)
        looked_at = L.boundary_images(B, elems, itemsize)
        assert wrong and wrong[0] > 0, (variant, shape, itemsize)
        assert wrong[0] in looked_at and wrong[0] - 1 in looked_at, (variant, shape, itemsize, wrong[0], looked_at)
    assert L.images_a_variant_gets_wrong(32, 512 * 512 * 16, 4, variant) == []


def test_the_first_block_fold_steps_aside_at_its_limit(ngan):
    """ops.first_block_fusable asks the library (ngan_first_block_plan): a critic input the fold would refuse takes the unfused pair
    FromImage -> conv instead of failing.  At the 512^2 stage the binding limit of the row is the slab count (8 workgroups across an image
    row, 1024 slabs): 128 images are folded, 129 are not -- long before B*H*W*N reaches 2^31 at 512.  Shapes only, nothing is launched."""
    import torch
    ops = ngan.ops
    (row,) = L.rows_of("ngan_first_block_fwd")
    assert sorted(lim.first_bad(dict(H=512, W=512))[0]["B"] for lim in row.limits) == [129, 512, 1024]      # slabs, elements, grid rows
    w_from, w_conv = torch.empty(16, 1, 1, 1, device="meta"), torch.empty(16, 16, 3, 3, device="meta")
    for B, want in ((128, True), (129, False), (511, False), (512, False)):
        x = torch.empty(B, 512, 512, 1, device="meta")
        assert ops.first_block_fusable(x, w_from, w_conv, pool=False) is want, B
        x2 = torch.empty(B, 1024, 1024, 1, device="meta")
        assert ops.first_block_fusable(x2, w_from, w_conv, pool=True) is want, B


def test_the_row_split_weight_gradient_reference_is_the_reference():
    import torch
    import fp64_conv as R
    gen = torch.Generator().manual_seed(5)
    for res, (B, H, W, K, N) in ((0, (3, 6, 10, 4, 5)), (1, (2, 4, 6, 3, 2)), (2, (2, 8, 4, 2, 3))):
        hin, win = (2 * H, 2 * W) if res == 1 else ((H // 2, W // 2) if res == 2 else (H, W))
        x = torch.randn(B, hin, win, K, dtype=torch.float64, generator=gen)
        g = torch.randn(B, H, W, N, dtype=torch.float64, generator=gen)
        a, b = L.conv3x3_wgrad_ref(x, g, 0.37, res), R.conv3x3_wgrad(x, g, 0.37, res)
        assert a.shape == b.shape == (N, K, 3, 3) and float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())
    half = torch.randn(3, 4, 5, 6, dtype=torch.float64, generator=gen)
    full = torch.randn(3, 8, 10, 7, dtype=torch.float64, generator=gen)
    a, b = L.s2_wgrad_ref(half, full), R.s2_wgrad(half, full)
    assert a.shape == b.shape == (6, 7, 4, 4) and float((a - b).abs().max()) <= 1e-13 * float(b.abs().max())
