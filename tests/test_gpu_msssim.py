"""MS-SSIM between pairs on the GPU: the kernels of csrc/msssim.hip against the fp64 restatement of tests/msssim_cases.py (bound,
input families and shapes are described there), the whole metric, its accumulation, `evaluate_msssim`, and its promise to leave a
run alone.

Measured on the CPU with the emulation in kernel order (tests/test_msssim_cpu.py prints every figure): the worst emulated err / bound
with C_ACC = 8 is 0.06 per scale (constant images of different level: every entry carries the same rounding, nothing cancels in the
mean) and 0.005 for the whole metric; the kernels are held to err / bound <= 1 for every pair."""
import types

import numpy as np
import pytest
import torch

import msssim_cases as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f64 = np.float64


def host(t):
    return t.detach().cpu().numpy().astype(f64)


# ---- one scale -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.COLORS)
@pytest.mark.parametrize("size", S.SCALE_SIZES)
def test_scale_per_pair_against_fp64(ngan, size, c):
    """every family of inputs (the flat-background, constant and corner-only ones among them), cs and ssim separately, every pair;
    1, 3 and all 12 pairs in one launch (the grid takes one pair per workgroup row: no granularity to step over)"""
    M = ngan.metrics
    a, b, ref = S.scale_case(size, c)
    full = None
    for p in (len(S.FAMILIES), 3, 1):
        got = M.msssim_scale(a[:p].to(DEV), b[:p].to(DEV))
        assert tuple(got.shape) == (p, 2) and got.dtype == torch.float64
        if full is None:
            full = got
        assert torch.equal(got, full[:p]), f"P={p}: a pair's value depends on the rest of the batch"
        for col, name in enumerate(("cs", "ssim")):
            val, bound = ref[name]
            r = np.abs(host(got[:, col]) - val[:p]) / bound[:p]
            if p == len(S.FAMILIES):
                for fam, ri, v in zip(S.FAMILIES, r, val):
                    print(f"scale {size} C={c} {name:4s} {fam:20s} ref {v:+.6f} err/bound {ri:.4f}")
            assert r.shape == (p,) and r.max() <= 1.0, f"{name} {size} C={c} P={p}: err / bound {r.max():.3f} ({S.FAMILIES[int(r.argmax())]})"
    # the corner-only pair differs from an equal pair by far more than its bound: a dropped last tile or a short halo would show
    i = S.FAMILIES.index("corner")
    assert 1.0 - ref["cs"][0][i] > 100 * ref["cs"][1][i]
    # equal images: exactly 1, flat background included
    for fam in ("same", "neuron same", "constant equal"):
        assert full[S.FAMILIES.index(fam)].tolist() == [1.0, 1.0], fam
    assert torch.equal(M.msssim_scale(a.to(DEV), b.to(DEV)), full), "two calls differ"


@pytest.mark.parametrize("c", S.COLORS)
def test_pooled_images_at_one_rounding(ngan, c):
    a, b = S.pairs(32, c)
    ao, bo = ngan.metrics.msssim_pool2(a.to(DEV), b.to(DEV))
    for got, x in ((ao, a), (bo, b)):
        ref = S.pool2_ref(x.double()).numpy()
        assert tuple(got.shape) == ref.shape and got.dtype == torch.float32
        assert (np.abs(host(got) - ref) <= 2.0 ** -24 * np.abs(ref)).all()


# ---- whole metric ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.COLORS)
@pytest.mark.parametrize("size", S.METRIC_SIZES)
def test_whole_metric_against_fp64(ngan, size, c):
    M = ngan.metrics
    a, b, ref, bound = S.metric_case(size, c)
    ad, bd = a.to(DEV), b.to(DEV)
    got = M.msssim(ad, bd)
    assert tuple(got.shape) == (4,) and got.dtype == torch.float64
    err = np.abs(host(got) - ref)
    for i in range(4):
        print(f"metric {size} C={c} pair {i}: ref {ref[i]:.6f} got {float(got[i]):.6f} bound {bound[i]:.2e} "
              f"err/bound {err[i] / (bound[i] + 1e-300):.4f}")
    assert (err <= bound).all(), (err, bound)
    same = M.msssim(ad, ad)
    _, same_bound = S.msssim_ref(a, a)
    assert (np.abs(host(same) - 1.0) <= same_bound).all(), same
    assert torch.equal(M.msssim(ad, bd), got), "two calls differ"
    halves = torch.cat([M.msssim(ad[:1], bd[:1]), M.msssim(ad[1:], bd[1:])])
    assert torch.equal(halves, got), "a batch split in two gives other values"
    assert torch.equal(M.msssim(bd, ad), got), "not symmetric (the kernel's order is: contraction is off, every operation is one)"


def test_accumulation_over_uneven_minibatches(ngan):
    M = ngan.metrics
    a, b = S.pairs(32, 3)
    ad, bd = a.to(DEV), b.to(DEV)
    once = M.msssim(ad, bd)
    m = M.MSSSIM(32, n_colors=3, device=DEV)
    assert m.scales == 2
    for lo, hi in ((0, 1), (1, 6), (6, 12)):
        m.feed("fake", ad[lo:hi].permute(0, 3, 1, 2).contiguous(), bd[lo:hi].permute(0, 3, 1, 2).contiguous())      # as (B, C, R, R)
    m.feed("real", ad[:5], ad[:5])
    assert torch.equal(m.per_pair("fake"), once)
    res = m.result()
    v = host(once)
    assert res["scales"] == 2 and res["weights"] == M.msssim_weights(2) and res["pairs"] == 12
    assert abs(res["fake"] - v.mean()) < 1e-15 and abs(res["fake_sem"] - v.std(ddof=1) / 12 ** 0.5) < 1e-15
    assert res["real"] == 1.0 and res["real_sem"] == 0.0
    assert "generated" in M.format_msssim(res) and "data" in M.format_msssim(res)


# ---- evaluate_msssim ---------------------------------------------------------------------------------------------------------------------
def small_nets(ngan, widths=(32, 16)):
    G = ngan.models.Generator_PG(list(widths), image_size_init=8, latent_dim=32).to(DEV)
    D = ngan.models.Discriminator_PG(list(widths)[::-1], image_size_init=8).to(DEV)
    return G, D


def small_dataset(ngan, size=16):
    g = torch.Generator().manual_seed(9)
    return ngan.data.NeuronDataset(torch.rand(8, 1, size, size, generator=g), augmentations=True, im_translation=0.05, device=DEV, seed=3)


@pytest.mark.parametrize("size", (16, 32))
def test_evaluate_msssim_is_seeded_and_leaves_no_trace(ngan, size):
    M = ngan.metrics
    torch.manual_seed(7)
    G, _ = small_nets(ngan, (32, 16) if size == 16 else (32, 16, 16))
    G.set_resolution(size, 1.0)
    data = small_dataset(ngan, 32)
    data.set_image_size(8)
    host_rng, device_rng, aug = torch.get_rng_state(), torch.cuda.get_rng_state(DEV), data.gen.get_state()
    own = data.gen
    kw = dict(n_pairs=7, batch_size=3, seed=2)
    first = M.evaluate_msssim(G, data, **kw)
    assert first["scales"] == S.n_scales(size) and first["pairs"] == 7 and first["weights"] == M.msssim_weights(first["scales"])
    assert 0.0 <= first["fake"] <= 1.0 and 0.0 <= first["real"] <= 1.0 and first["fake_sem"] >= 0 and first["real_sem"] > 0
    assert torch.equal(torch.get_rng_state(), host_rng), "torch's global generator was consumed"
    assert torch.equal(torch.cuda.get_rng_state(DEV), device_rng), "the device generator was consumed"
    assert data.gen is own and torch.equal(data.gen.get_state(), aug) and data.image_size == 8, "the data set's stream or stage moved"
    assert M.evaluate_msssim(G, data, **kw) == first                              # seeded: the same numbers again
    other = M.evaluate_msssim(G, data, **{**kw, "seed": 3})
    assert other["fake"] != first["fake"] and other["real"] != first["real"]
    alone = M.evaluate_msssim(G, None, **kw)                                      # no data set: the generated side alone
    assert alone["fake"] == first["fake"] and alone["real"] is None and alone["real_sem"] is None
    # the real side by hand: the same augmented batches, paired (2 i, 2 i + 1)
    data.gen = torch.Generator(device="cpu").manual_seed(2 + 1)
    data.set_image_size(size)
    vals = []
    for i in range(0, 7, 3):
        n = 2 * min(3, 7 - i)
        x = M.channels_last(data.batch([(2 * i + j) % len(data) for j in range(n)]))
        vals.append(M.msssim(x[0::2].contiguous(), x[1::2].contiguous()))
    data.gen = own
    data.set_image_size(8)
    vals = torch.cat(vals)
    assert vals.numel() == 7 and first["real"] == float(vals.mean())
    # the generated side by hand
    lat = torch.Generator(device="cpu").manual_seed(2 + 2)
    vals = []
    for i in range(0, 7, 3):
        z = torch.randn(2 * min(3, 7 - i), G.latent_dim, generator=lat).clamp(-5, 5)
        with torch.no_grad():
            x = M.channels_last(G((z / z.norm(p=2, dim=1, keepdim=True)).to(DEV)))
        vals.append(M.msssim(x[0::2].contiguous(), x[1::2].contiguous()))
    assert first["fake"] == float(torch.cat(vals).mean())
    G8, _ = small_nets(ngan)                                                      # a stage below 16 x 16: said, not raised
    below = M.evaluate_msssim(G8, data, **kw)
    assert below["scales"] == 0 and below["fake"] is None and "16 x 16" in below["note"]


# ---- no side effects ---------------------------------------------------------------------------------------------------------------------
def same(x, y):
    if torch.is_tensor(x):
        return torch.is_tensor(y) and torch.equal(x, y)
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return isinstance(y, (list, tuple)) and len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    return x == y


def two_epochs(ngan, tmp_path, tag, msssim_period, ema_beta):
    cfg = types.SimpleNamespace(adapt_critic=False, sim_loss_lambda=0.0, n_critic=1, batch_size=4, transit_sch=[1], N_epochs=2,
                                alpha_step=0.5, learning_rate=2e-3, checkpointing_period=1, ID=tag, msssim_period=msssim_period,
                                msssim_pairs=6, msssim_seed=1)
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    G, D = small_nets(ngan)
    data = small_dataset(ngan)
    tr = ngan.train.PGGANTrainer(G, D, learning_rate=cfg.learning_rate, alpha_step=cfg.alpha_step, device_latents=True, ema_beta=ema_beta)
    f = str(tmp_path / f"GenDisc_{tag}.pth")
    ck = ngan.utils.Checkpointer(G, D, cfg.learning_rate, f, N_epochs=cfg.N_epochs, verbose=False, device=torch.device(DEV), trainer=tr,
                                 extra_checkpoint_period=1e3)
    lines = []
    series = ngan.train.pggan_train(tr, data, cfg, checkpoint=ck, epoch_final=3, log=lambda *a: lines.append(" ".join(map(str, a))))
    torch.cuda.synchronize()
    rng = (torch.get_rng_state(), torch.cuda.get_rng_state(DEV), data.gen.get_state())
    return series, ngan.utils.load_checkpoint_dict(f), lines, tr, f, rng


@pytest.mark.parametrize("ema_beta", (0.0, 0.9))
def test_a_scored_run_trains_bit_identically(ngan, tmp_path, ema_beta, capsys):
    """two epochs at 16 x 16 (grown at epoch 1, fading in; captured graphs replayed) with a checkpoint and a score after each"""
    plain, saved0, lines0, _, _, rng0 = two_epochs(ngan, tmp_path, "m000", 0, ema_beta)
    scored, saved1, lines1, tr, f, rng1 = two_epochs(ngan, tmp_path, "m001", 1, ema_beta)
    assert tr.G.image_size == 16 and tr.has_graph((4, 1, 16, 16)), "the run did not train through a captured graph"
    assert plain == scored, "the monitor series changed when the metric was turned on"
    for key in ("Generator_state", "Discriminator_state", "optimizer_state") + (("Generator_ema_state",) if ema_beta else ()):
        assert key in saved0 and same(saved0[key], saved1[key]), f"{key} changed when the metric was turned on"
    for name, x, y in zip(("torch's CPU generator", "the device generator", "the data set's generator"), rng0, rng1):
        assert torch.equal(x, y), f"{name} ended in another state"
    assert "MSSSIM" not in saved0 and not any("MS-SSIM" in l for l in lines0)
    entries = saved1["MSSSIM"]
    assert [e["epoch"] for e in entries] == [1, 2] and "SWD" not in saved1
    assert all(e["image_size"] == 16 and e["scales"] == S.n_scales(16) == 1 and e["pairs"] == 6 for e in entries)
    assert all(set(e) == {"epoch", "image_size", "scales", "fake", "fake_ema", "real", "pairs"} for e in entries)
    assert all(0.0 <= e["fake"] <= 1.0 and 0.0 <= e["real"] <= 1.0 for e in entries)
    assert entries[0]["real"] == entries[1]["real"] and entries[0]["fake"] != entries[1]["fake"]     # the same seed, another generator
    if ema_beta:
        assert all(0.0 <= e["fake_ema"] <= 1.0 and e["fake_ema"] != e["fake"] for e in entries)
    else:
        assert all(e["fake_ema"] is None for e in entries)
    scored_lines = [l for l in lines1 if "MS-SSIM" in l]
    assert len(scored_lines) == 2 and all(("averaged generator" in l) == bool(ema_beta) and "data" in l for l in scored_lines)
    # the eval tool prints the table for the checkpoint, and the averaged generator's after it when asked
    images = str(tmp_path / "images.pt")
    torch.save(torch.rand(8, 1, 16, 16, generator=torch.Generator().manual_seed(9)) * 2 - 1, images)
    capsys.readouterr()
    assert ngan.eval.main(["-weights", f, "--msssim", "8", "--images", images] + (["--ema"] if ema_beta else [])) == 0
    out = capsys.readouterr().out
    assert out.count("MS-SSIM between pairs") == (2 if ema_beta else 1) and ("averaged generator" in out) == bool(ema_beta)
    assert out.count("(1 scale, 8 pairs)") == (2 if ema_beta else 1)
    assert sum(l.strip().startswith("generated") for l in out.splitlines()) == (2 if ema_beta else 1)
    assert sum(l.strip().startswith("data") for l in out.splitlines()) == (2 if ema_beta else 1)
