"""The generator's spectral loss on the GPU: the kernels of csrc/specloss.hip through the entry points of include/ngan_spectral.h
against the fp64 restatement of tests/specloss_cases.py (definition, bounds, emulation and shapes are described there), the autograd
node and the public loss, the data's target, and the trainer, the epoch driver and the checkpoint with the switch on and off.

Measured on the CPU with the emulation in kernel order (tests/test_specloss_bounds_cpu.py prints every figure): the worst emulated
err / bound with C_INV = 8 is 0.01 per gradient element and 0.22 for a coefficient (its one fp32 rounding); the kernels are held to
err / bound <= 1 for every element.

measured on MI355X (a record, not a bound: worst err / bound over all cases; 1 is the bound): S 0.015, l 0.0087, L 0.15, c 0.34
(R = 1024, the impulse), gradient 0.0100; every gradient element equals the emulation's bits.  Two ranks with shares 4 + 4 and
5 + 3: worst deviation / scale of the generator gradient 9.6e-8 and 3.7e-7 against the bound 2e-4.  The module takes 19 s."""
import types

import numpy as np
import pytest
import torch

import specloss_cases as L
import spectrum_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64 = np.float64
PAD = 64                       # guard elements on either side of every output
SENTINEL = -7.0


def host(t):
    return t.detach().cpu().numpy().astype(f64)


class Guarded:
    """a device buffer of n elements with PAD sentinel elements on either side (16-byte alignment of the payload is kept)"""

    def __init__(self, n, dtype):
        self.whole = torch.full((n + 2 * PAD,), SENTINEL, device=DEV, dtype=dtype)
        self.view = self.whole[PAD:PAD + n]

    def intact(self):
        return bool((self.whole[:PAD] == SENTINEL).all()) and bool((self.whole[PAD + self.view.numel():] == SENTINEL).all())

    def untouched(self):
        return bool((self.whole == SENTINEL).all())


def raw(ngan, x, tgt, scale, floor=L.FLOOR, on=True, upstream=1.0, addend=None, backward=True):
    """the three entry points on guarded buffers: {'radial', 'transform', 'per_image', 'loss', 'c', 'coef', 'skipped', 'grad'} (device
    tensors) and the guards"""
    C = ngan._C
    lib = C.lib()
    x = x.to(DEV).contiguous()
    B, R = x.shape[0], x.shape[1]
    K = R // 2 + 1
    bufs = {"radial": Guarded(B * K, torch.float64), "transform": Guarded(B * K * R * 2, torch.float32), "ring_norm": Guarded(K, torch.float64),
            "ws_fwd": Guarded(lib.ngan_specloss_fwd_workspace_bytes(B, R, 1) // 8, torch.float64),
            "per_image": Guarded(B, torch.float64), "loss": Guarded(1, torch.float32), "c": Guarded(B * K, torch.float32),
            "coef": Guarded(B * K, torch.float32), "skipped": Guarded(1, torch.int32),
            "ws_bwd": Guarded(lib.ngan_specloss_bwd_workspace_bytes(B, R, 1) // 8, torch.float64),
            "grad": Guarded(B * R * R, torch.float32)}
    v = {k: b.view for k, b in bufs.items()}
    t = torch.as_tensor(np.asarray(tgt, f64), device=DEV)
    C.call("ngan_specloss_fwd", x, v["radial"], v["transform"], v["ring_norm"], v["ws_fwd"], B, R, 1, int(on))
    C.call("ngan_specloss_head", v["radial"], t, v["ring_norm"], B, R, float(scale), float(floor), v["per_image"], v["loss"], v["c"], v["coef"],
           v["skipped"])
    if backward:
        up = torch.tensor(float(upstream), device=DEV)
        C.call("ngan_specloss_bwd", v["transform"], v["coef"], up, None if addend is None else addend.to(DEV).contiguous(), v["grad"],
               v["ws_bwd"], B, R, 1, int(on))
    torch.cuda.synchronize()
    out = {"radial": v["radial"].view(B, K), "ring_norm": v["ring_norm"], "transform": v["transform"].view(B, K, R, 2), "per_image": v["per_image"],
           "loss": v["loss"][0], "c": v["c"].view(B, K), "coef": v["coef"].view(B, K), "skipped": int(v["skipped"][0]),
           "grad": v["grad"].view(B, R, R)}
    return out, bufs


def pin(got, ref, names, tag):
    """S, l, L, c and every element of the gradient against the restatement; STAT lines; err / bound <= 1"""
    B = got["radial"].shape[0]
    rows = {"S": [L.ratio(host(got["radial"][b]), ref["radial"][b], ref["radial_bound"][b]) for b in range(B)],
            "l": [L.ratio(host(got["per_image"][b]), ref["per_image"][b], ref["per_image_bound"][b]) for b in range(B)],
            "c": [L.ratio(host(got["c"][b]), ref["c"][b], ref["c_bound"][b]) for b in range(B)],
            "grad": [L.ratio(host(got["grad"][b]), ref["grad"][b], ref["grad_bound"][b]) for b in range(B)]}
    for b, name in enumerate(names):
        print(f"STAT {tag} {name:10s} err/bound: " + " ".join(f"{k} {v[b]:.4f}" for k, v in rows.items()))
    rl = L.ratio(host(got["loss"]), ref["loss"], ref["loss_bound"])
    print(f"STAT {tag} L {float(got['loss']):.6g} (reference {ref['loss']:.6g}) err/bound {rl:.4f}")
    for k, v in rows.items():
        assert max(v) <= 1.0, f"{tag}: {k} err / bound {max(v):.3f} ({names[int(np.argmax(v))]})"
    assert rl <= 1.0, f"{tag}: L err / bound {rl:.3f}"
    assert got["skipped"] == 0


# ---- the kernels against fp64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on", (True, False))
@pytest.mark.parametrize("size", S.SMALL_SIZES)
def test_loss_and_gradient_against_fp64(ngan, size, on):
    """all seven families in one batch: every bin, every coefficient, every pixel; guards intact; the forward's radial values are the
    metric's bits; 1, 3 and 7 images give the same per-image bits; two calls give the same bits"""
    x, tgt, scale, ref = L.case(size, on)
    tag = f"R={size} window={int(on)}"
    got, bufs = raw(ngan, x, tgt, scale, on=on)
    assert all(b.intact() for b in bufs.values()), [k for k, b in bufs.items() if not b.intact()]
    pin(got, ref, S.FAMILIES, tag)
    assert torch.equal(got["radial"], ngan.metrics.radial_spectrum(x.to(DEV), window=on)), f"{tag}: not the metric's radial values"
    if on:
        g = got["grad"]
        assert bool((g[:, 0, :] == 0).all()) and bool((g[:, :, 0] == 0).all()), "w = 0 on row 0 and column 0: exact zeros"
    emu = L.specloss_emu(x.numpy(), tgt, scale, L.FLOOR, on)
    same = float((got["grad"].cpu().numpy() == emu["grad"]).mean())
    print(f"STAT {tag} gradient elements equal to the emulation's bits: {100 * same:.2f} %")
    for n in (3, 1):
        part, _ = raw(ngan, x[:n], tgt, scale, on=on)
        for key in ("radial", "transform", "per_image", "c", "coef", "grad"):
            assert torch.equal(part[key], got[key][:n]), f"{tag} B={n}: {key} of an image depends on the rest of the batch"
    again, _ = raw(ngan, x, tgt, scale, on=on)
    for key in ("radial", "transform", "per_image", "loss", "c", "coef", "grad"):
        assert torch.equal(again[key], got[key]), f"{tag}: two calls differ in {key}"


@pytest.mark.parametrize("size", S.LARGE_SIZES)
def test_large_sizes_single_image(ngan, size):
    """B = 1: the sizes with 2, 4 and 8 butterflies per thread (1024: 76 KB of LDS per workgroup in every pass)"""
    tgt = L.target(size)
    for i, fam in enumerate(S.LARGE_FAMILIES):
        x = S.images(size, 1, S.LARGE_FAMILIES)[i:i + 1].contiguous()
        ref = L.specloss_ref(x.numpy(), tgt, L.LAMBDA, L.FLOOR, True)
        got, bufs = raw(ngan, x, tgt, L.LAMBDA)
        assert all(b.intact() for b in bufs.values())
        pin(got, ref, (fam,), f"R={size}")


def test_fused_addend_and_device_upstream(ngan):
    x, tgt, scale, _ = L.case(64)
    plain, _ = raw(ngan, x, tgt, scale)
    g = plain["grad"]
    add = torch.randn(g.shape, generator=torch.Generator().manual_seed(11)).to(DEV) * float(g.abs().mean())
    fused, _ = raw(ngan, x, tgt, scale, addend=add)
    want = add + g
    assert bool(((fused["grad"] - want).abs() <= 2.0 ** -23 * want.abs()).all()), "addend + gradient differs by more than an ulp of the sum"
    for up in (0.25, 4.0, -2.0):
        scaled, _ = raw(ngan, x, tgt, scale, upstream=up)
        assert torch.equal(scaled["grad"], g * up), f"the upstream scalar {up} read from the device does not scale exactly"
    both, _ = raw(ngan, x, tgt, scale, upstream=0.5, addend=add)
    assert torch.equal(both["grad"], add + g * 0.5)
    inplace = add.clone()                                                           # the addend may be the output itself
    ngan._C.call("ngan_specloss_bwd", plain["transform"].contiguous(), plain["coef"].contiguous(), torch.ones((), device=DEV), inplace, inplace,
                 torch.empty(ngan._C.lib().ngan_specloss_bwd_workspace_bytes(x.shape[0], 64, 1) // 8, device=DEV, dtype=torch.float64),
                 x.shape[0], 64, 1, 1)
    assert torch.equal(inplace, fused["grad"])


def test_target_bins_that_are_not_positive_take_no_weight(ngan):
    x, tgt, scale, _ = L.case(32)
    t = np.array(tgt)
    t[3], t[9] = 0.0, -1.0
    got, _ = raw(ngan, x, t, scale)
    q, ell, loss, c = L.head_ref(host(got["radial"]), t, scale, L.FLOOR)
    assert got["skipped"] == 2 and bool((got["c"][:, [0, 3, 9]] == 0).all()) and bool(torch.isfinite(got["grad"]).all())
    np.testing.assert_allclose(host(got["per_image"]), ell, rtol=1e-12)
    np.testing.assert_allclose(host(got["c"]), c, rtol=2.0 ** -23)


def test_refusals_return_a_status_and_write_nothing(ngan):
    lib = ngan._C.lib()
    B, R, K = 2, 32, 17
    x = torch.zeros(B, 3, R, R, device=DEV)
    tgt = torch.ones(K, device=DEV, dtype=torch.float64)
    up = torch.ones((), device=DEV)
    o = {k: Guarded(n, dt) for k, n, dt in (("radial", B * K, torch.float64), ("transform", B * K * R * 2, torch.float32), ("ring_norm", K, torch.float64),
                                            ("ws", 1 << 14, torch.float64), ("per_image", B, torch.float64), ("loss", 1, torch.float32),
                                            ("c", B * K, torch.float32), ("coef", B * K, torch.float32), ("skipped", 1, torch.int32),
                                            ("grad", B * R * R, torch.float32))}
    p = {k: b.view.data_ptr() for k, b in o.items()}
    s = torch.cuda.current_stream().cuda_stream

    def fwd(images=x.data_ptr(), radial=p["radial"], transform=p["transform"], ring_norm=p["ring_norm"], ws=p["ws"], B=B, R=R, C=1):
        return lib.ngan_specloss_fwd(images, radial, transform, ring_norm, ws, B, R, C, 1, s)

    def head(radial=p["radial"], target=tgt.data_ptr(), ring_norm=p["ring_norm"], B=B, R=R, floor=1e-3, loss=p["loss"], coef=p["coef"]):
        return lib.ngan_specloss_head(radial, target, ring_norm, B, R, 1.0, floor, p["per_image"], loss, p["c"], coef, p["skipped"], s)

    def bwd(transform=p["transform"], coef=p["coef"], upstream=up.data_ptr(), addend=None, grad=p["grad"], ws=p["ws"], B=B, R=R, C=1):
        return lib.ngan_specloss_bwd(transform, coef, upstream, addend, grad, ws, B, R, C, 1, s)

    shape, arg = -2, -1                                                             # NGAN_ERR_SHAPE, NGAN_ERR_ARG
    for fn, kw, status, word in ((fwd, {"R": 24}, shape, "R=24"), (fwd, {"R": 8}, shape, "R=8"), (fwd, {"R": 2048}, shape, "R=2048"),
                                 (fwd, {"C": 3}, shape, "C=3"), (fwd, {"B": 0}, shape, "B=0"), (fwd, {"B": 65536}, shape, "B=65536"),
                                 (fwd, {"images": x.data_ptr() + 4}, arg, "16-byte"), (fwd, {"transform": p["transform"] + 8}, arg, "16-byte"),
                                 (fwd, {"images": None}, arg, "null"), (fwd, {"radial": None}, arg, "null"), (fwd, {"ring_norm": None}, arg, "null"),
                                 (fwd, {"ws": None}, arg, "workspace"), (head, {"ring_norm": None}, arg, "null"),
                                 (head, {"R": 48}, shape, "R=48"), (head, {"B": 0}, shape, "B=0"), (head, {"floor": 0.0}, arg, "floor"),
                                 (head, {"target": None}, arg, "null"), (head, {"loss": None}, arg, "null"),
                                 (head, {"radial": p["radial"] + 4}, arg, "8-byte"),
                                 (bwd, {"R": 24}, shape, "R=24"), (bwd, {"C": 3}, shape, "C=3"), (bwd, {"B": 0}, shape, "B=0"),
                                 (bwd, {"grad": p["grad"] + 4}, arg, "16-byte"), (bwd, {"addend": p["grad"] + 8}, arg, "16-byte"),
                                 (bwd, {"upstream": None}, arg, "null"), (bwd, {"coef": None}, arg, "null"), (bwd, {"ws": None}, arg, "workspace")):
        assert fn(**kw) == status, (fn.__name__, kw)
        assert word in lib.ngan_last_error().decode(), (fn.__name__, kw, lib.ngan_last_error())
    torch.cuda.synchronize()
    assert all(b.untouched() for b in o.values()), "a refused call wrote something"
    assert fwd(B=1) == 0 and head(B=1) == 0 and bwd(B=1) == 0
    torch.cuda.synchronize()
    assert all(b.intact() for b in o.values())
    assert bool((o["radial"].view[:K] != SENTINEL).all()) and bool((o["radial"].view[K:] == SENTINEL).all())
    assert bool((o["grad"].view[:R * R] != SENTINEL).all()) and bool((o["grad"].view[R * R:] == SENTINEL).all())


@pytest.mark.parametrize("size,B", ((16, 3), (64, 2), (128, 1)))
def test_workspace_query_matches_what_a_run_touches(ngan, size, B):
    """the guarded run stays inside the queried bytes (raw() checks the guards) and reaches their last element"""
    x = S.white_set(size, B, 2)
    _, bufs = raw(ngan, x, L.target(size), 1.0)
    for key in ("ws_fwd", "ws_bwd"):
        assert bufs[key].intact() and float(bufs[key].view[-1]) != SENTINEL and float(bufs[key].view[0]) != SENTINEL, key


# ---- the autograd node and the public loss -----------------------------------------------------------------------------------------------
def test_autograd_node_and_public_loss(ngan):
    x, tgt, scale, ref = L.case(32)
    got, _ = raw(ngan, x, tgt, scale)
    t = torch.as_tensor(tgt, device=DEV)
    planar = x.permute(0, 3, 1, 2).contiguous().to(DEV).requires_grad_(True)
    loss = ngan.loss_functions.G_spectral_loss(planar, t, Lambda=L.LAMBDA, floor=L.FLOOR)
    assert loss.shape == () and loss.dtype == torch.float32 and torch.equal(loss.detach(), got["loss"])
    loss.backward()
    assert torch.equal(planar.grad[:, 0], got["grad"])
    half = ngan.loss_functions.G_spectral_loss(planar.detach(), t, Lambda=L.LAMBDA, floor=L.FLOOR, global_batch=2 * x.shape[0])
    assert abs(float(half) / float(loss.detach()) - 0.5) < 1e-6
    # the tap: images passed through, the gradient of what follows fused into the adjoint's store
    y = planar.detach().clone().requires_grad_(True)
    out, term, per_image = ngan.ops.SpectralLoss.apply(y, t, scale, L.FLOOR)
    assert torch.equal(out, y) and not per_image.requires_grad and per_image.dtype == torch.float64
    np.testing.assert_allclose(host(per_image), ref["per_image"], rtol=1e-6)
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).to(DEV) * 1e-3
    torch.autograd.backward([(out * w).sum(), term], [torch.ones((), device=DEV), torch.full((), 0.5, device=DEV)])
    assert torch.equal(y.grad[:, 0], w[:, 0] + got["grad"] * 0.5)
    y2 = planar.detach().clone().requires_grad_(True)                              # the term unused: the image gradient passes through
    out2, _, _ = ngan.ops.SpectralLoss.apply(y2, t, scale, L.FLOOR)
    (out2 * w).sum().backward()
    assert torch.equal(y2.grad, w)
    y3 = planar.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(ngan.ops.SpectralLoss.apply(y3, t, scale, L.FLOOR)[1], y3)
    assert torch.equal(g[:, 0], got["grad"])
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(ngan.ops.SpectralLoss.apply(y3, t, scale, L.FLOOR)[1], y3, create_graph=True)
    with pytest.raises(ValueError):
        ngan.loss_functions.G_spectral_loss(torch.zeros(2, 3, 32, 32, device=DEV), t)
    with pytest.raises(ValueError):
        ngan.loss_functions.G_spectral_loss(planar.detach(), t[:-1])


def test_descent_on_the_gpu(ngan):
    """the descent check of tests/test_specloss_bounds_cpu.py through G_spectral_loss: Adam on 32 upsampled fields against the
    spectrum of white ones takes the loss to a tenth and high_db from below -10 dB to above -3 dB"""
    start, tgt, real = L.descent_inputs()
    t = torch.as_tensor(tgt, device=DEV)

    def loss_and_grad(x):
        x = x.clone().requires_grad_(True)
        loss = ngan.loss_functions.G_spectral_loss(x, t, Lambda=L.LAMBDA, floor=L.FLOOR)
        loss.backward()
        return float(loss.detach()), x.grad

    before = L.high_db(real, start.numpy())
    first, last, final = L.descend(loss_and_grad, start.to(DEV))
    after = L.high_db(real, final)
    print(f"STAT descent on the GPU: loss {first:.4f} -> {last:.4f}, high_db {before:.2f} -> {after:.2f} dB")
    assert last <= L.DESCENT["loss_factor"] * first
    assert before <= L.DESCENT["high_before"] and after > L.DESCENT["high_after"]


def test_spectral_target_is_seeded_and_leaves_no_trace(ngan):
    M = ngan.metrics
    g = torch.Generator().manual_seed(9)
    data = ngan.data.NeuronDataset(torch.rand(8, 1, 32, 32, generator=g), augmentations=True, im_translation=0.05, device=DEV, seed=3)
    data.set_image_size(8)
    host_rng, device_rng, aug, own = torch.get_rng_state(), torch.cuda.get_rng_state(DEV), data.gen.get_state(), data.gen
    t = M.spectral_target(data, 32, n_images=7, seed=2, batch_size=3, device=DEV)
    assert t.dtype == torch.float64 and tuple(t.shape) == (17,) and bool((t > 0).all())
    assert torch.equal(torch.get_rng_state(), host_rng) and torch.equal(torch.cuda.get_rng_state(DEV), device_rng)
    assert data.gen is own and torch.equal(data.gen.get_state(), aug) and data.image_size == 8, "the data set's stream or stage moved"
    assert torch.equal(M.spectral_target(data, 32, n_images=7, seed=2, batch_size=3, device=DEV), t)
    assert not torch.equal(M.spectral_target(data, 32, n_images=7, seed=3, batch_size=3, device=DEV), t)
    # by hand: the same augmented batches, as evaluate_spectrum takes its data side
    data.gen = torch.Generator(device="cpu").manual_seed(2 + 1)
    data.set_image_size(32)
    vals = [M.radial_spectrum(M.channels_last(data.batch([(i + j) % len(data) for j in range(min(3, 7 - i))]))) for i in range(0, 7, 3)]
    data.gen = own
    data.set_image_size(8)
    np.testing.assert_allclose(host(t), host(torch.cat(vals)).mean(0), rtol=1e-12)
    with pytest.raises(ValueError):
        M.spectral_target(data, 8)


# ---- the trainer -------------------------------------------------------------------------------------------------------------------------
LATENT = 32


def small_nets(ngan, seed=6, res=16, mbstd_group=0):
    """tests/test_gpu_spectrum.py::small_nets (widths 32, 16 from 8 x 8), seeded, grown to `res`"""
    torch.manual_seed(seed)
    G = ngan.models.Generator_PG([32, 16], image_size_init=8, latent_dim=LATENT)
    D = ngan.models.Discriminator_PG([16, 32], image_size_init=8, **({"mbstd_group": mbstd_group} if mbstd_group else {}))
    if res != 8:
        G.set_resolution(res, 1.0)
        D.set_resolution(res, 1.0)
    return G.to(DEV), D.to(DEV)


def _unit(g, n):
    v = torch.randn(n, LATENT, generator=g)
    return v / v.norm(dim=1, keepdim=True)


def batch_draws(ngan, seed, n, mask=0, res=16):
    g = torch.Generator().manual_seed(seed)
    d = dict(real=(torch.rand(n, 1, res, res, generator=g) * 2 - 1).to(DEV), z_d=_unit(g, n).to(DEV), z_gp=_unit(g, n).to(DEV),
             eps=torch.rand(n, 1, 1, 1, generator=g).to(DEV), z_g=_unit(g, n).to(DEV), tables=None)
    if mask:
        u = torch.rand(4 * n, 8, generator=g).to(DEV)
        t = torch.empty((4 * n, 8), dtype=torch.int32, device=DEV)
        ngan.ops.diffaug_params(u, t, res, mask, 1.0)
        d["tables"] = dict(real=t[:n].clone(), fake=t[n:3 * n].clone(), gen=t[3 * n:].clone())
    return d


def state_of(tr):
    ts = [tr.flat_g.flat, tr.flat_d.flat, tr.flat_g.seg_step, tr.flat_d.seg_step]
    for flat in (tr.flat_g, tr.flat_d):
        ts += [getattr(flat, n) for n in ("exp_avg", "exp_avg_sq", "square_avg") if getattr(flat, n, None) is not None]
    return [t.detach().cpu().numpy().copy() for t in ts + ([tr.flat_g.ema] if tr.ema_enabled else [])]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def target16(shift=0.0):
    """a target for 16 x 16 images: the level of white noise in [-1, 1], tilted"""
    return torch.tensor([(1.0 / 3.0) * (1.0 + shift + 0.05 * k) for k in range(9)], dtype=torch.float64)


def trainer(ngan, lam=1.0, nets=None, **kw):
    tr = ngan.train.PGGANTrainer(*(nets or small_nets(ngan)), learning_rate=1e-3, device_latents=True,
                                 **({"spec_loss_lambda": lam} if lam is not None else {}), **kw)
    if lam:
        tr.set_spectral_target(16, target16())
    return tr


def test_the_switch_off_is_the_default_trainer(ngan):
    """spec_loss_lambda=0: bit-equal parameters and optimiser state after two iterations, eager and replayed, the same RNG states, no
    spectral buffer; with the weight on the run ends elsewhere and draws as much"""
    def run(replayed, lam):
        tr = trainer(ngan, lam)
        torch.manual_seed(21)
        x = batch_draws(ngan, 3, 4)["real"]
        stats = [tr.step(x) if replayed else tr.train_iteration(x) for _ in range(2)][-1]
        torch.cuda.synchronize()
        return state_of(tr), torch.cuda.get_rng_state(DEV), torch.get_rng_state(), tr, set(stats)
    for replayed in (False, True):
        want, off, on = run(replayed, None), run(replayed, 0.0), run(replayed, 1.0)
        assert same(off[0], want[0]) and torch.equal(off[1], want[1]) and torch.equal(off[2], want[2]), replayed
        assert off[3]._spec_targets is None and not off[3].spectral_enabled and off[4] == want[4] and "G_spec_loss" not in off[4]
        assert not same(on[0], want[0]) and torch.equal(on[1], want[1]) and torch.equal(on[2], want[2]), replayed
        assert on[4] == want[4] | {"G_spec_loss"} and all(np.isfinite(v).all() for v in on[0])
    with pytest.raises(ValueError, match="spec_loss_lambda = 0"):
        off[3].set_spectral_target(16, target16())
    for bad in (dict(spec_loss_lambda=-1.0), dict(spec_loss_lambda=float("nan")), dict(spec_loss_lambda=1.0, spec_loss_floor=0.0)):
        with pytest.raises(ValueError, match="spec_loss"):
            ngan.train.PGGANTrainer(*small_nets(ngan), **bad)


VARIANTS = {"plain": {}, "lsgan": dict(objective="lsgan"), "diffaug_ema": dict(diffaug="translation,cutout", ema_beta=0.999),
            "rmsprop": dict(optimizer="rmsprop"), "mbstd": dict(), "lp": dict(grad_pen_mode="lp"), "r1": dict(grad_pen_mode="r1"),
            "bf16": dict()}      # the bf16 storage mode: the generator's image tensor is fp32 there, so the term runs as it is


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_eager_and_replayed_iterations_are_bit_equal(ngan, variant):
    """two eager iterations against capture + two replays with injected draws, the term on, under every switch it must work with"""
    if variant == "bf16":
        ngan.ops.set_conv_precision("bf16")
    try:
        _eager_against_replayed(ngan, variant)
    finally:
        ngan.ops.set_conv_precision("f32")


def _eager_against_replayed(ngan, variant):
    kw = VARIANTS[variant]
    mask = 6 if "diffaug" in kw else 0
    nets = lambda: small_nets(ngan, mbstd_group=4 if variant == "mbstd" else 0)      # noqa: E731
    batches = [batch_draws(ngan, 40 + i, 4, mask=mask) for i in range(2)]
    eager = trainer(ngan, nets=nets(), **kw)
    stats_e = []
    for d in batches:
        s = eager.train_iteration(d["real"], d["z_d"], d["z_gp"], d["eps"], d["z_g"], tables=d["tables"])
        stats_e.append({k: float(v) for k, v in s.items()})
    tr = trainer(ngan, nets=nets(), **kw)
    static, stats_r = None, []
    for d in batches:
        own = {k: d[k] for k in ("z_d", "z_gp", "eps", "z_g")}
        if static is None:
            static = {k: v.clone() for k, v in own.items()}
            tr.capture(d["real"], draws=static, tables=d["tables"])
        for k, v in own.items():
            static[k].copy_(v)
        stats_r.append({k: float(v) for k, v in tr.replay(d["real"], tables=d["tables"]).items()})
    torch.cuda.synchronize()
    assert stats_e == stats_r and all(np.isfinite(list(s.values())).all() for s in stats_e), (stats_e, stats_r)
    assert same(state_of(eager), state_of(tr))
    assert all(s["G_spec_loss"] > 0 for s in stats_e)


def test_a_fresh_target_changes_the_next_replay_without_a_capture(ngan):
    d = batch_draws(ngan, 50, 4)
    draws = {k: d[k] for k in ("z_d", "z_gp", "eps", "z_g")}

    def replayed(second_target):
        tr = trainer(ngan)
        tr.capture(d["real"], draws=draws)
        tr.replay(d["real"])
        graphs = dict(tr._graphs)
        if second_target is not None:
            tr.set_spectral_target(16, second_target)
        stats = tr.replay(d["real"])
        torch.cuda.synchronize()
        assert dict(tr._graphs) == graphs and len(graphs) == 1, "the graphs were captured again"
        return state_of(tr), float(stats["G_spec_loss"])
    eager = trainer(ngan)
    eager.train_iteration(d["real"], **draws)
    eager.set_spectral_target(16, target16(0.5))
    stats = eager.train_iteration(d["real"], **draws)
    kept, moved = replayed(None), replayed(target16(0.5))
    assert same(moved[0], state_of(eager)) and moved[1] == float(stats["G_spec_loss"])
    assert not same(kept[0], moved[0]) and kept[1] != moved[1]
    with pytest.raises(ValueError):
        eager.set_spectral_target(16, target16()[:-1])
    with pytest.raises(ValueError):
        eager.set_spectral_target(24, torch.ones(13, dtype=torch.float64))


def test_the_term_equals_the_restatement_and_the_gradients_add_up(ngan):
    """G_spec_loss on given latents against the fp64 restatement on the generator's own images, within its bound; the generator's
    parameter gradient with the term on equals the critic's part (a trainer without the term) plus the spectral part (a backward
    pass of G_spectral_loss alone) at the tolerance of tests/test_gpu_lsgan.py's gradient pins"""
    lam, d = 2.5, batch_draws(ngan, 60, 4)
    tr = trainer(ngan, lam)
    tr.fused_stem = False
    stats = tr.g_compute(d["real"], d["z_g"])
    with torch.no_grad():
        images = tr.G(d["z_g"])
    assert images.dtype == torch.float32 and tuple(images.shape) == (4, 1, 16, 16)
    ref = L.specloss_ref(images.permute(0, 2, 3, 1).cpu().numpy(), target16().numpy(), lam / 4, tr.spec_loss_floor, True)
    r = L.ratio(float(stats["G_spec_loss"]), ref["loss"], ref["loss_bound"])
    print(f"STAT trainer G_spec_loss {float(stats['G_spec_loss']):.6g} (reference {ref['loss']:.6g}) err/bound {r:.4f}")
    assert r <= 1.0 and ref["loss"] > 0
    both = [p.grad.detach().clone() for p in tr.flat_g.params]
    plain = trainer(ngan, None)
    plain.fused_stem = False
    assert float(plain.g_compute(d["real"], d["z_g"])["G_loss"]) == float(stats["G_loss"])      # G_loss stays the adversarial term
    critic = [p.grad.detach().clone() for p in plain.flat_g.params]
    alone = trainer(ngan, None)                                                   # (its flat views: the same tensors in the same order)
    alone.flat_g.ensure_grad_views()
    alone.flat_g.zero_grad()
    ngan.loss_functions.G_spectral_loss(alone.G(d["z_g"]), target16().to(DEV), Lambda=lam, floor=tr.spec_loss_floor).backward()
    assert list(tr.flat_g.names) == list(plain.flat_g.names) == list(alone.flat_g.names)
    spectral = [p.grad.detach().clone() for p in alone.flat_g.params]
    assert len(both) == len(critic) == len(spectral)
    gmax = max(float((c + s).abs().max()) for c, s in zip(critic, spectral))
    worst = 0.0
    for name, got, c, s in zip(tr.flat_g.names, both, critic, spectral):
        want = (c + s).double()
        diff = got.double() - want
        l2 = float(diff.norm() / (want.norm() + 1e-2 * gmax))
        outliers = float((diff.abs() > 1e-2 * (float(want.abs().max()) + 1e-2 * gmax)).double().mean())
        worst = max(worst, l2)
        assert l2 < 2e-3 and outliers <= 1e-3, (name, l2, outliers)
    assert max(float(s.abs().max()) for s in spectral) > 0 and max(float(c.abs().max()) for c in critic) > 0
    print(f"STAT critic part + spectral part against one backward pass: worst relative l2 {worst:.3e}")


def test_a_missing_target_raises_and_a_small_stage_trains_without_the_term(ngan, capsys):
    d = batch_draws(ngan, 70, 4)
    tr = ngan.train.PGGANTrainer(*small_nets(ngan), learning_rate=1e-3, spec_loss_lambda=1.0)
    with pytest.raises(RuntimeError, match="no spectral target for 16 x 16"):
        tr.g_compute(d["real"], d["z_g"])
    d8 = batch_draws(ngan, 71, 4, res=8)
    small = ngan.train.PGGANTrainer(*small_nets(ngan, res=8), learning_rate=1e-3, spec_loss_lambda=1.0)
    plain = ngan.train.PGGANTrainer(*small_nets(ngan, res=8), learning_rate=1e-3)
    capsys.readouterr()
    for _ in range(2):
        stats = small.train_iteration(d8["real"], d8["z_d"], d8["z_gp"], d8["eps"], d8["z_g"])
        plain.train_iteration(d8["real"], d8["z_d"], d8["z_gp"], d8["eps"], d8["z_g"])
    assert float(stats["G_spec_loss"]) == 0.0 and same(state_of(small), state_of(plain))
    assert "below 16 x 16" in small.spectral_note and capsys.readouterr().out.count("below 16 x 16") == 1      # said once, not raised


# ---- epoch driver and checkpoint ---------------------------------------------------------------------------------------------------------
DRIVER_CFG = dict(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[2], N_epochs=4, alpha_step=0.5,
                  learning_rate=1e-3, checkpointing_period=1, ID="sp", seed=3, spec_loss_images=6, spec_loss_seed=1)


def driver_draws(epoch, k, n):
    g = torch.Generator().manual_seed(10007 * epoch + k)
    return dict(z_d=_unit(g, n), z_gp=_unit(g, n), eps=torch.rand(n, 1, 1, 1, generator=g), z_g=_unit(g, n))


def driver_run(ngan, f, lam, epochs=(1, 3), resume=False):
    """pggan_train on four synthetic 16 x 16 images, one batch per epoch, replayed graphs, given latents: epoch 1 at 8 x 8, the growth
    step to 16 x 16 (fading in) at epoch 2"""
    cfg = types.SimpleNamespace(**DRIVER_CFG)
    G, D = small_nets(ngan, res=8)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, device_latents=True, alpha_step=cfg.alpha_step,
                                 **({} if lam is None else {"spec_loss_lambda": lam}))
    data = ngan.train.TensorImageDataset.synthetic(4, 16, device=DEV, seed=8)
    ck = ngan.utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=torch.device(DEV), trainer=tr,
                                 extra_checkpoint_period=1e3)
    if resume:
        ck.load_state()
    lines = []
    series = ngan.train.pggan_train(tr, data, cfg, checkpoint=ck, epoch_init=epochs[0], epoch_final=epochs[1], use_graph=True,
                                    log=lambda *a: lines.append(" ".join(map(str, a))), draws=driver_draws,
                                    on_epoch=lambda ep, t: torch.manual_seed(100 + ep))
    torch.cuda.synchronize()
    return series, state_of(tr), tr, lines


def test_epoch_driver_sets_the_target_and_carries_the_sixth_monitor(ngan, tmp_path, capsys):
    five = ["score_real", "score_fake", "D_loss", "G_loss", "D_grad_pen"]
    plain, state0, _, lines0 = driver_run(ngan, str(tmp_path / "a.pth"), None)
    off, state1, tr1, lines1 = driver_run(ngan, str(tmp_path / "b.pth"), 0.0)
    assert list(plain) == list(off) == five and plain == off and same(state0, state1), "the switch off is not the default run"
    assert not any("spectral" in l for l in lines0 + lines1) and tr1._spec_targets is None
    f = str(tmp_path / "c.pth")
    on, state2, tr, lines = driver_run(ngan, f, 0.5)
    assert list(on) == five + ["G_spec_loss"] and all(len(v) == 2 and np.isfinite(v).all() for v in on.values()), on
    assert tr.G.image_size == 16 and tr.has_graph((4, 1, 16, 16)), "the run did not train through a captured graph"
    assert on["G_spec_loss"][0] == 0.0 and on["G_spec_loss"][1] > 0.0          # 8 x 8: the term is off; 16 x 16: on
    assert [l for l in lines if "spectral target" in l] == [l for l in lines if "spectral target at 16x16" in l] and \
        sum("spectral target" in l for l in lines) == 1, lines                 # one fresh target, after the growth event
    assert sorted(tr._spec_targets) == [16] and not same(state2, state0)
    data = ngan.train.TensorImageDataset.synthetic(4, 16, device=DEV, seed=8)
    want = ngan.metrics.spectral_target(data, 16, n_images=6, seed=1, device=DEV)
    assert torch.equal(tr._spec_targets[16], want)
    saved = ngan.utils.load_checkpoint_dict(f)
    assert saved["spec_loss_lambda"] == 0.5 and saved["spec_loss_floor"] == 1e-3
    assert ngan.utils.load_checkpoint_dict(str(tmp_path / "a.pth"))["spec_loss_lambda"] == 0.0
    capsys.readouterr()                                                        # resuming under another weight is allowed, and said
    more, _, tr3, _ = driver_run(ngan, f, 2.0, epochs=(3, 4), resume=True)
    assert "spec_loss_lambda=0.5" in capsys.readouterr().out and list(more) == five + ["G_spec_loss"] and len(more["G_loss"]) == 1
    assert ngan.utils.load_checkpoint_dict(f)["spec_loss_lambda"] == 2.0


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------------------
def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _share_worker(rank, world, port, q):
    """tests/test_gpu_lsgan.py::_share_worker with the spectral term on: a batch of 8 in shares 4 + 4 and 5 + 3 against one rank on the
    whole batch"""
    import datetime
    import os
    import sys
    import traceback
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    try:
        from __graft_entry__ import load_package
        ngan = load_package()
        own = [dist.new_group([r]) for r in range(world)][rank]          # a one-rank group: the single-process reference
        d = batch_draws(ngan, 80, 8)
        tr = ngan.train.PGGANTrainer(*small_nets(ngan), spec_loss_lambda=1.5)                    # world = 2: exchanges on
        ref = ngan.train.PGGANTrainer(*small_nets(ngan), process_group=own, spec_loss_lambda=1.5)
        assert tr.world == world and ref.world == 1
        for t in (tr, ref):
            t.set_spectral_target(16, target16())
        worst = []
        for shares in ([4, 4], [5, 3]):
            sl = slice(sum(shares[:rank]), sum(shares[:rank + 1]))
            s = tr.g_compute(d["real"][sl], d["z_g"][sl], global_batch=shares)
            tr._exchange(tr.flat_g)
            s_ref = ref.g_compute(d["real"], d["z_g"])
            w = 0.0
            for name, p, pr, a in zip(tr.flat_g.names, tr.flat_g.params, ref.flat_g.params, tr.flat_g.active_host):
                if not a:
                    assert float(p.grad.abs().max()) == 0.0, name
                    continue
                got, want = p.grad / world, pr.grad                      # the fused Adam applies the 1/world factor
                scale = float(want.abs().max()) + 1e-3 * max(float(v.grad.abs().max()) for v in ref.flat_g.params)
                w = max(w, float((got - want).abs().max()) / scale)
            assert w < 2e-4, (shares, w)
            assert float(s["G_spec_loss"]) > 0 and float(s_ref["G_spec_loss"]) > 0
            worst.append(w)
        torch.cuda.synchronize()
        q.put((rank, "ok", worst))
    except Exception:  # noqa: BLE001
        q.put((rank, traceback.format_exc(), None))
        raise
    finally:
        dist.destroy_process_group()


def test_two_ranks_with_equal_and_unequal_shares_match_the_whole_batch():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_share_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
    results = sorted(q.get(timeout=5) for _ in range(2))
    print("STAT spectral term, shares 4 + 4 and 5 + 3, worst deviation / scale of the generator gradient per rank:", [r[2] for r in results])
    assert [r[:2] for r in results] == [(0, "ok"), (1, "ok")], results
    assert all(p.exitcode == 0 for p in procs)
