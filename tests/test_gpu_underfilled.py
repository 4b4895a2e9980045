"""The three launches whose grids were resized to fill the chip (csrc/pointwise.hip, csrc/linear.hip): none of them may change a value.

Bilinear x2 adjoint (`launch_up2_adjoint_strip`): the strip height YT is 16 where the grid has 512 workgroups, else halved down to 2.
ADJOINT_SHAPES (B, h, w, C) are the small ones -- all of them end at YT = 2, with h below the strip (1), a ragged last strip (3, 17, 33),
a width below one workgroup's columns, several column blocks (40 columns of 32 at C = 32) and several strips (128 rows).  STRIP_SHAPES
reach the other heights on tiny tensors: at C = 4 a workgroup spans 256 columns, so w = 1 leaves ceil(h / YT) * B workgroups, and B = 32
with h = 64 / 128 / 256 gives exactly 512 of them at YT = 4 / 8 / 16 (and 256 at the next height up, which the rule therefore refuses).
Every shape runs with and without the fused PixelNorm backward, in both storage types, against the fp64 references of
tests/lane_group_cases.py on that module's bounds, as tests/test_gpu_lane_group.py does; and the result on the whole batch must equal
bit for bit the results of its parts sent alone (every image for the small shapes; the two halves, the first and the last image for the
B = 32 ones): the batch size changes the grid -- for STRIP_SHAPES also YT -- and must not change a value.

Stem forward (`linear_fwd_kernel`): up to 32 samples per block on one pass over the weight, one accumulator per 16-sample chunk.
B = 1, 16 (one chunk), 17 (ragged second), 32 (two), 33 (a second block with one row), 48 (a second block with one chunk); K = 16 (the tail
loop only) and 512 (two groups of the load ring); C = 20 (two channel tiles, the second ragged) and 128 (a tile per wave).  Against
`linear_fwd_ref` on the bound of tests/stem_head_cases.py (the figure of `linear_fwd_emulate` on the same inputs is printed next to the
kernel's), and every 16-row chunk of a B = 32 / 48 call must equal the same rows sent alone, in y and in the norms.

One-channel pool (`pool2_fwd_img_kernel`): w = 1 and 5 stay on the scalar kernel, 130 takes two outputs per thread, 512 four; `torch.equal`
against 0.25 * ((a + b) + (c + d)) formed in torch in that association (rounded to bf16 once for the bf16 storage type).

Output buffers lie between NaN guards and start as NaN (`Kernels` of tests/test_gpu_lane_group.py)."""
import numpy as np
import pytest
import torch

import lane_group_cases as L
import stem_head_cases as S
from test_gpu_lane_group import DEV, Kernels

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

ADJOINT_SHAPES = [(2, 1, 1, 16), (2, 3, 5, 16), (1, 16, 16, 128), (3, 17, 9, 64), (2, 33, 40, 32), (1, 64, 64, 32), (1, 128, 24, 32)]
STRIP_SHAPES = [(32, 64, 1, 4), (32, 128, 1, 4), (32, 256, 1, 4)]


def strip_height(B, h, w, C):
    """the rule of launch_up2_adjoint_strip"""
    cols = 256 // (C // 4)
    yt = 16
    while yt > 2 and -(-w // cols) * -(-h // yt) * B < 512:
        yt //= 2
    return yt


def test_the_shapes_reach_every_strip_height():
    assert {strip_height(*s) for s in ADJOINT_SHAPES} == {2}
    assert [strip_height(*s) for s in STRIP_SHAPES] == [4, 8, 16]
    assert [strip_height(16, *s) for s in ((16, 16, 128), (32, 32, 64), (64, 64, 32), (128, 128, 32), (256, 256, 16))] == [2, 2, 4, 16, 16]


@pytest.fixture(scope="module")
def adjoint_refs():
    """shape -> storage -> (inputs, references): computed once per shape, shared by the parametrised cases"""
    cache = {}

    def get(shape, storage):
        if (shape, storage) not in cache:
            B, h, w, C = shape
            d = L.draws(S.seed_of(5, *shape), g=(B, 2 * h, 2 * w, C), y=(B, h, w, C), rn_pos=(B, h, w))
            if storage == "bf16":
                d["g"], d["y"] = L.rbf(d["g"]), L.rbf(d["y"])
            refs = {"up2_adjoint/gx": L.up2_adjoint_ref(d["g"])["gx"],
                    "up2_adjoint_pnbwd/out": L.up2_adjoint_pnbwd_ref(d["g"], d["y"], d["rn_pos"])["out"]}
            cache[shape, storage] = d, refs
        return cache[shape, storage]
    return get


def _parts(B):
    if B <= 4:
        return [slice(b, b + 1) for b in range(B)]
    return [slice(0, B // 2), slice(B // 2, B), slice(0, 1), slice(B - 1, B)]


@pytest.mark.parametrize("storage", L.STORAGES)
@pytest.mark.parametrize("shape", ADJOINT_SHAPES + STRIP_SHAPES)
def test_up2_adjoint_strip_heights(ngan, adjoint_refs, shape, storage):
    """ngan_[bf16_]up2_adjoint and _up2_adjoint_pnbwd per element against fp64, and the batch against its parts sent alone"""
    B, h, w, C = shape
    d, refs = adjoint_refs(shape, storage)
    k = Kernels(ngan._C.call, storage, C)
    bf = storage == "bf16"
    forms = {"up2_adjoint/gx": lambda s: k.up2_adjoint(d["g"][s])["gx"],
             "up2_adjoint_pnbwd/out": lambda s: k.up2_adjoint_pnbwd(d["g"][s], d["y"][s], d["rn_pos"][s])["out"]}
    bad = {}
    for name, run in forms.items():
        whole = run(slice(0, B))
        v = L.worst(name, C, whole, refs[name], bf)
        print(f"STAT underfilled {storage} {name} {shape} YT={strip_height(*shape)}: {v:.3f}")
        if not v <= 1.0:
            bad[name] = v
        for s in _parts(B):
            alone = run(s)
            assert torch.equal(torch.from_numpy(whole[s]), torch.from_numpy(alone)), (name, shape, storage, s, "the batch size changed a value")
    assert not bad, (shape, storage, bad)


STEM_B = [1, 16, 17, 32, 33, 48]
STEM_SHAPES = [(K, Sp, C) for K in (16, 512) for C, Sp in ((20, 9), (128, 4))]


@pytest.fixture(scope="module")
def stem_refs():
    """(K, S, C) -> inputs for 48 samples (tests/stem_head_cases.py draws 37)"""
    cache = {}

    def get(K, Sp, C):
        if (K, Sp, C) not in cache:
            cache[K, Sp, C] = S.draws(S.seed_of(13, K, Sp, C), z=(max(STEM_B), K), w=(C * Sp, K))
        return cache[K, Sp, C]
    return get


def _stem(ngan, z, w, Sp, C, bf):
    B, K = z.shape
    y = torch.full((B + 1, Sp, C), float("nan"), device=DEV, dtype=BF if bf else torch.float32)
    rn = torch.full((B + 1, Sp), float("nan"), device=DEV)
    y[B], rn[B] = 7.0, 7.0
    dz, dw = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (z, w))
    ngan._C.call("ngan_bf16_linear_lrelu_pn_fwd" if bf else "ngan_linear_lrelu_pn_fwd", dz, dw, y, rn, B, K, Sp, C, S.STEM_SCALE, S.SLOPE, S.EPS)
    assert bool((y[B] == 7.0).all()) and bool((rn[B] == 7.0).all()), ("wrote past the batch", bf)
    return y[:B], rn[:B]


@pytest.mark.parametrize("K,Sp,C", STEM_SHAPES)
@pytest.mark.parametrize("B", STEM_B)
def test_stem_forward_chunks(ngan, stem_refs, B, K, Sp, C):
    """ngan_[bf16_]linear_lrelu_pn_fwd against fp64 on the bound of tests/stem_head_cases.py"""
    d = stem_refs(K, Sp, C)
    z, w = d["z"][:B], d["w"]
    em = S.linear_fwd_emulate(z, w, Sp, C, S.STEM_SCALE, "seq")
    bad = []
    for bf in (False, True):
        y, rn = _stem(ngan, z, w, Sp, C, bf)
        yh, rh = y.float().cpu().numpy(), rn.cpu().numpy()
        ref = S.linear_fwd_ref(z, w, Sp, C, S.STEM_SCALE, yh)
        for name, got, r in (("y", yh, S.stored(ref["y"], S.BF16_STORE if bf else 0)), ("rn", rh, ref["rn"])):
            v = S.ratio(got, *r, S.c_acc("linear_lrelu_pn_fwd/" + name))
            e = S.ratio(em[name], *S.linear_fwd_ref(z, w, Sp, C, S.STEM_SCALE, em["y"])[name], S.c_acc("linear_lrelu_pn_fwd/" + name))
            print(f"STAT underfilled linear_lrelu_pn_fwd/{name}{' bf16' if bf else ''} {(B, K, Sp, C)}: {v:.3f} (emulated fp32 {e:.3f})")
            if not v <= 1.0:
                bad.append((name, bf, v))
    assert not bad, ((B, K, Sp, C), bad)


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("K,Sp,C", STEM_SHAPES)
@pytest.mark.parametrize("B", [32, 48])
def test_stem_forward_rows_do_not_depend_on_the_batch(ngan, stem_refs, B, K, Sp, C, bf):
    """every 16-row chunk of a two-chunk block, and of the block behind it, equals the same rows sent alone (rows 0-15 of B = 32 among them)"""
    d = stem_refs(K, Sp, C)
    y, rn = _stem(ngan, d["z"][:B], d["w"], Sp, C, bf)
    for b0 in range(0, B, 16):
        ya, ra = _stem(ngan, d["z"][b0:b0 + 16], d["w"], Sp, C, bf)
        assert torch.equal(y[b0:b0 + 16], ya) and torch.equal(rn[b0:b0 + 16], ra), (B, K, Sp, C, bf, b0)


@pytest.mark.parametrize("storage", L.STORAGES)
@pytest.mark.parametrize("B,h,w", [(1, 1, 1), (2, 3, 5), (3, 8, 130), (1, 16, 512)])
def test_one_channel_pool(ngan, B, h, w, storage):
    """ngan_[bf16_]pool2_fwd at C = 1 against 0.25 * ((a + b) + (c + d)) in torch"""
    x = L.draws(S.seed_of(17, B, h, w), x=(B, 2 * h, 2 * w, 1))["x"]
    if storage == "bf16":
        x = L.rbf(x)
    k = Kernels(ngan._C.call, storage, 1)
    got = torch.from_numpy(k.pool2_fwd(x)["y"])
    t = torch.from_numpy(x).to(DEV)
    a, b, c, d = t[:, 0::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 0::2], t[:, 1::2, 1::2]
    want = 0.25 * ((a + b) + (c + d))
    if storage == "bf16":
        want = want.to(BF).float()
    assert got.shape == want.shape and torch.equal(got, want.cpu()), (B, h, w, storage)
