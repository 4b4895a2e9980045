"""Golden vectors of the WGAN path from the REFERENCE's own Generator_wgan / Discriminator_wgan (models.py:728-790).

Runs in the build container only (needs the reference sources; see oracle/make_golden.py, whose helpers it imports and does not
edit).  The reference's loss modules do not import here, so its WGAN iteration (train.py:470-506, losses loss_functions.py:14-74) is
replayed over the reference's modules by `ref_iteration`, once in fp32 and once in fp64 from the same start.  init_weights is the
reference's rule (utils.py:96-101: its utils module does not import here either), applied as neuron_gan_amd.utils.init_weights.

    wgan_small.npz  G [16, 8, 8] / D [8, 8, 16], 64^2, latent 8, batch 4, n_critic 2, 2 iterations, Adam and RMSprop:
                    seed-1 state dicts after construction + init_weights; real images and every latent draw; per iteration the
                    scores and losses (fp32 and fp64); after the last iteration the critic's gradients (last critic step), the
                    generator's gradients, the parameters and BatchNorm buffers (fp64 values stored as fp32, plus the fp32 replay's
                    max deviation per tensor); an eval-mode sample.
    wgan_full.npz   the default widths at 512^2, batch 8, one Adam iteration: per tensor sum / sum|.| checksums and 16 element
                    pins of the parameters after the step and of both nets' gradients, fp64, with the fp32 replay's deviation; the
                    scalars.  Inputs are regenerated from their seeds (`inputs_full`).

    python tools/make_golden_wgan.py [--small] [--full]
"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import OUT, import_reference, latent  # noqa: E402

SMALL = dict(gw=[16, 8, 8], dw=[8, 8, 16], latent=8, size=64, colors=1, b=4, n_critic=2, iters=2, lr=1e-3)
FULL = dict(gw=[128, 64, 32, 32, 16, 16], dw=[16, 16, 32, 32, 64, 128], latent=512, size=512, colors=1, b=8, n_critic=1, iters=1,
            lr=1e-4)
N_PINS = 16


def init_weights(m):
    import __graft_entry__ as graft
    return graft.load_package().utils.init_weights(m)


def build(models, cfg, seed=1):
    torch.manual_seed(seed)
    G = models.Generator_wgan(cfg["gw"], latent_dim=cfg["latent"], image_size=cfg["size"], N_colors=cfg["colors"])
    D = models.Discriminator_wgan(cfg["dw"], image_size=cfg["size"], N_colors=cfg["colors"])
    G.apply(init_weights)
    D.apply(init_weights)
    return G, D


def inputs(cfg, seed=11):
    """real images and latents of every draw: [iteration] -> (real, [z per critic step], z_g)"""
    torch.manual_seed(seed)
    out = []
    for _ in range(cfg["iters"]):
        real = torch.rand(cfg["b"], cfg["colors"], cfg["size"], cfg["size"]) * 2 - 1
        zs = [latent(cfg["b"], cfg["latent"]) for _ in range(cfg["n_critic"])]
        out.append((real, zs, latent(cfg["b"], cfg["latent"])))
    return out


def make_opts(G, D, kind, lr):
    if kind == "adam":
        return torch.optim.Adam(G.parameters(), lr=lr, betas=(0.5, 0.999)), torch.optim.Adam(D.parameters(), lr=lr, betas=(0.5, 0.999))
    return torch.optim.RMSprop(G.parameters(), lr=lr), torch.optim.RMSprop(D.parameters(), lr=lr)


def ref_iteration(G, D, optG, optD, real, zs, z_g, drift=0.001, clip=0.01):
    """train.py:470-506 over the reference modules; returns the scalars and the critic's gradients of the last critic step"""
    out = {}
    d_grads = None
    for z in zs:
        real_score = D(real)
        s_real = real_score.mean()
        s_fake = D(G(z).detach()).mean()
        loss = -s_real + s_fake + drift * torch.square(real_score).mean()
        D.zero_grad()
        loss.backward()
        d_grads = {k: p.grad.detach().clone() for k, p in D.named_parameters()}
        optD.step()
        for p in D.parameters():
            p.data.clamp_(-clip, clip)
        out.update(D_loss=loss.item(), score_real=s_real.item(), score_fake=s_fake.item())
    G.zero_grad()
    g_loss = -D(G(z_g)).mean()
    g_loss.backward()
    optG.step()
    out["G_loss"] = g_loss.item()
    return out, d_grads, {k: p.grad.detach().clone() for k, p in G.named_parameters()}


def replay(models, cfg, kind, dtype, data):
    G, D = build(models, cfg)
    G, D = G.to(dtype), D.to(dtype)
    optG, optD = make_opts(G, D, kind, cfg["lr"])
    scalars = []
    for real, zs, zg in data:
        s, dg, gg = ref_iteration(G, D, optG, optD, real.to(dtype), [z.to(dtype) for z in zs], zg.to(dtype))
        scalars.append(s)
    return G, D, scalars, dg, gg


def states(G, D, dg, gg):
    """name -> tensor of everything compared after the last iteration"""
    out = {}
    for tag, net in (("G", G), ("D", D)):
        for k, v in net.state_dict().items():
            out[f"{tag}.{k}"] = v.detach()
    for tag, gr in (("gradD", dg), ("gradG", gg)):
        for k, v in gr.items():
            out[f"{tag}.{k}"] = v
    return out


def small(models, out_dir=OUT):
    torch.set_num_threads(1)
    cfg = SMALL
    data = inputs(cfg)
    G0, D0 = build(models, cfg)
    arrays = {}
    for tag, net in (("init_G", G0), ("init_D", D0)):
        for k, v in net.state_dict().items():
            arrays[f"{tag}.{k}"] = v.numpy()
    for i, (real, zs, zg) in enumerate(data):
        arrays[f"real.{i}"] = real.numpy()
        arrays[f"z_d.{i}"] = torch.stack(zs).numpy()
        arrays[f"z_g.{i}"] = zg.numpy()
    torch.manual_seed(21)
    z_eval = latent(4, cfg["latent"])
    arrays["z_eval"] = z_eval.numpy()
    for kind in ("adam", "rmsprop"):
        r = {}
        for dtype in (torch.float32, torch.float64):
            G, D, scalars, dg, gg = replay(models, cfg, kind, dtype, data)
            G.eval()
            with torch.no_grad():
                sample = G(z_eval.to(dtype))
            r[dtype] = (scalars, states(G, D, dg, gg), sample)
        (s32, st32, smp32), (s64, st64, smp64) = r[torch.float32], r[torch.float64]
        for name in s64[0]:
            arrays[f"{kind}.scalar64.{name}"] = np.array([s[name] for s in s64])
            arrays[f"{kind}.scalar32.{name}"] = np.array([s[name] for s in s32])
        for k, v in st64.items():
            if v.dtype == torch.int64:
                arrays[f"{kind}.{k}"] = v.numpy()
                continue
            arrays[f"{kind}.{k}"] = v.float().numpy()
            arrays[f"{kind}.dev.{k}"] = np.array(float((st32[k].double() - v).abs().max()))
        arrays[f"{kind}.sample"] = smp64.float().numpy()
        arrays[f"{kind}.dev.sample"] = np.array(float((smp32.double() - smp64).abs().max()))
    path = os.path.join(out_dir, "wgan_small.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


def inputs_full(cfg=FULL):
    return inputs(cfg, seed=13)


def pin_index(n, name):
    g = torch.Generator().manual_seed(sum(map(ord, name)) % 100003)
    return torch.randint(0, n, (N_PINS,), generator=g)


def full(models):
    cfg = FULL
    data = inputs_full(cfg)
    arrays = {}
    r = {}
    for dtype in (torch.float32, torch.float64):
        G, D, scalars, dg, gg = replay(models, cfg, "adam", dtype, data)
        r[dtype] = (scalars, states(G, D, dg, gg))
    (s32, st32), (s64, st64) = r[torch.float32], r[torch.float64]
    for name in s64[0]:
        arrays[f"scalar64.{name}"] = np.array([s[name] for s in s64])
        arrays[f"scalar32.{name}"] = np.array([s[name] for s in s32])
    for k, v in st64.items():
        if v.dtype == torch.int64:
            arrays[f"int.{k}"] = v.numpy()
            continue
        flat64, flat32 = v.reshape(-1), st32[k].double().reshape(-1)
        idx = pin_index(flat64.numel(), k)
        arrays[f"idx.{k}"] = idx.numpy()
        arrays[f"pin.{k}"] = flat64[idx].numpy()
        arrays[f"sum.{k}"] = np.array([float(flat64.sum()), float(flat64.abs().sum())])
        arrays[f"sumdev.{k}"] = np.array([abs(float(flat32.sum() - flat64.sum())), abs(float(flat32.abs().sum() - flat64.abs().sum()))])
        arrays[f"dev.{k}"] = np.array(float((flat32 - flat64).abs().max()))
        arrays[f"amax.{k}"] = np.array(float(flat64.abs().max()))
    path = os.path.join(OUT, "wgan_full.npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--full", action="store_true")
    a = ap.parse_args()
    models, _ = import_reference()
    if a.small or not a.full:
        small(models)
    if a.full or not a.small:
        full(models)
