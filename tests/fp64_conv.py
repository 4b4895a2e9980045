"""fp64 references of the convolution family of the hot path, for the element-wise tests at full size (tests/test_gpu_full_size.py).

Every operator is written as shifted slices and matrix products on channels-last tensors: no MIOpen, no F.conv2d, so the same code
runs on the CPU (where tests/test_fp64_conv_cpu.py checks it against torch's own fp64 operators) and on the GPU (where a full-size
reference takes well under a second).  A 3x3 pad-1 convolution is nine shifted (P x K)(K x N) products, a 4x4 stride-2 one sixteen.

    resample codes (ops.RES_*):  0 plain, 1 2x2 average pool on load, 2 bilinear x2 on load (align_corners=False)
    3x3:        conv3x3 / conv3x3_dgrad / conv3x3_wgrad, lrelu_pixelnorm (epilogue 1), pixelnorm_bwd (epilogue 2), pool2 (side output),
                pool_adjoint (out_mode 1), to_image (epilogue 3's tanh colour projection)
    stride 2:   s2_down (Conv2d k4 s2 p1), s2_up (ConvTranspose2d k4 s2 p1), s2_wgrad, act_on_load (BatchNorm -> LeakyReLU on load)
    BatchNorm:  bn_stats (batch statistics, folded transform, running buffers), bn_fold_eval, bn_act_backward (with / without the
                activation), act_backward (no BatchNorm), each with its absolute-value twin (*_abs) for tests/wgan_cases.py
    stem:       stem, stem_grads (Generator_wgan's Linear, outputs in NHWC order)
    adjoint identities: identity_margins (the noise-scaled statistic of test_full_size_layers_satisfy_the_adjoint_identities)
"""
import torch
import torch.nn.functional as F


def _pad1(x):
    return F.pad(x, (0, 0, 1, 1, 1, 1))


def pool2(x):
    """2x2 average (B, H, W, C) -> (B, H/2, W/2, C)"""
    b, h, w, c = x.shape
    return x.reshape(b, h // 2, 2, w // 2, 2, c).mean(dim=(2, 4))


def _up2_axis(x, dim):
    """bilinear x2 along one axis, align_corners=False: out[2i] = x[i-1]/4 + 3x[i]/4, out[2i+1] = 3x[i]/4 + x[i+1]/4, edges clamped"""
    n = x.shape[dim]
    prev = torch.cat([x.narrow(dim, 0, 1), x.narrow(dim, 0, n - 1)], dim)
    nxt = torch.cat([x.narrow(dim, 1, n - 1), x.narrow(dim, n - 1, 1)], dim)
    return torch.stack([0.25 * prev + 0.75 * x, 0.75 * x + 0.25 * nxt], dim + 1).flatten(dim, dim + 1)


def up2(x):
    """bilinear x2 (B, H, W, C) -> (B, 2H, 2W, C)"""
    return _up2_axis(_up2_axis(x, 1), 2)


def resample(x, code):
    if code == 1:
        return pool2(x)
    if code == 2:
        return up2(x)
    return x


def resample_adjoint(g, code):
    """adjoint of resample(., code) applied to g (given at the resampled size)"""
    if code == 1:
        return g.repeat_interleave(2, 1).repeat_interleave(2, 2) * 0.25
    if code == 2:
        b, h, w, c = g.shape
        with torch.enable_grad():
            z = torch.zeros(b, h // 2, w // 2, c, dtype=g.dtype, device=g.device, requires_grad=True)
            (gz,) = torch.autograd.grad(up2(z), z, g)
        return gz
    return g


def conv3x3(x, w, scale=1.0, res=0, bias=None):
    """y = conv3x3(resample(x), scale * w) + bias, zero padding 1; x (B, H, W, K), w (N, K, 3, 3) -> (B, H', W', N)"""
    x = resample(x, res)
    b, h, wd, k = x.shape
    n = w.shape[0]
    xp = _pad1(x)
    wt = (scale * w).permute(2, 3, 1, 0)                    # [dy][dx] (K x N)
    y = torch.zeros(b * h * wd, n, dtype=x.dtype, device=x.device)
    for dy in range(3):
        for dx in range(3):
            y.addmm_(xp[:, dy:dy + h, dx:dx + wd, :].reshape(-1, k), wt[dy, dx])
    y = y.view(b, h, wd, n)
    return y if bias is None else y + bias


def conv3x3_dgrad(g, w, scale=1.0, res=0):
    """input gradient of conv3x3(., w, scale, res) for the output gradient g (B, H, W, N) -> the input's shape"""
    b, h, wd, n = g.shape
    k = w.shape[1]
    gp = _pad1(g)
    wt = (scale * w).permute(2, 3, 0, 1)                    # [dy][dx] (N x K)
    gx = torch.zeros(b * h * wd, k, dtype=g.dtype, device=g.device)
    for dy in range(3):
        for dx in range(3):                                 # y[i] takes x[i + dy - 1]: x[a] receives g[a + 1 - dy]
            gx.addmm_(gp[:, 2 - dy:2 - dy + h, 2 - dx:2 - dx + wd, :].reshape(-1, n), wt[dy, dx])
    return resample_adjoint(gx.view(b, h, wd, k), res)


def conv3x3_wgrad(x, g, scale=1.0, res=0):
    """weight gradient (N, K, 3, 3) = scale * sum over pixels of g (x) the shifted resample(x) (ops._run_wgrad: a pooled input is
    pooled first)"""
    x = resample(x, res)
    b, h, wd, k = x.shape
    n = g.shape[3]
    xp = _pad1(x)
    g2 = g.reshape(-1, n).t()
    gw = torch.empty(n, k, 3, 3, dtype=x.dtype, device=x.device)
    for dy in range(3):
        for dx in range(3):
            gw[:, :, dy, dx] = scale * (g2 @ xp[:, dy:dy + h, dx:dx + wd, :].reshape(-1, k))
    return gw


def lrelu_pixelnorm(c, slope, eps=1e-8):
    """epilogue 1: (y, r) with a = LeakyReLU(c), r = sqrt(mean_c(a^2) + eps), y = a / r"""
    a = torch.where(c > 0, c, slope * c)
    r = torch.sqrt((a * a).mean(-1, keepdim=True) + eps)
    return a / r, r[..., 0]


def pixelnorm_bwd(g, y, r, slope):
    """epilogue 2: gradient w.r.t. the pre-activation of the producer (y, r) = lrelu_pixelnorm(c), given g w.r.t. y"""
    m = torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))
    return m * (g - y * (g * y).mean(-1, keepdim=True)) / r.unsqueeze(-1)


def pool_adjoint(c):
    """the pool-adjoint store (out_mode 1): c (B, H, W, N) -> (B, 2H, 2W, N), 0.25 c to each pixel of the 2x2 block; 0.25 is exact, so the
    absolute-value twin is pool_adjoint(|c|)"""
    return resample_adjoint(c, 1)


def to_image(y, wimg):
    """the tanh colour projection of epilogue 3 (one colour): (t, sum_c |y_c| |wimg_c|) with t = tanh(sum_c y_c wimg_c); y (B, H, W, N),
    wimg (N,) -> (B, H, W) each; the second value is the dot product's absolute-value twin (|tanh'| <= 1)"""
    return torch.tanh((y * wimg).sum(-1)), (y.abs() * wimg.abs()).sum(-1)


# ---- 4x4 stride-2 pad-1 (csrc/stride2.hip) ------------------------------------------------------------------------------------
def act_on_load(x, scale=None, shift=None, act=0, slope=0.0):
    """the per-channel transform a stride-2 kernel applies while it loads: act(scale * x + shift), act = LeakyReLU(slope) if set"""
    if scale is not None:
        x = x * scale + shift
    return torch.where(x > 0, x, slope * x) if act else x


def s2_down(x, w, bias=None):
    """Conv2d(k4, s2, p1): x (B, H, W, C), w (M, C, 4, 4) -> (B, H/2, W/2, M)"""
    b, h, wd, c = x.shape
    ho, wo, m = h // 2, wd // 2, w.shape[0]
    xp = _pad1(x)
    y = torch.zeros(b * ho * wo, m, dtype=x.dtype, device=x.device)
    for ky in range(4):
        for kx in range(4):
            y.addmm_(xp[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2, :].reshape(-1, c), w[:, :, ky, kx].t())
    y = y.view(b, ho, wo, m)
    return y if bias is None else y + bias


def s2_up(x, w, bias=None):
    """ConvTranspose2d(k4, s2, p1): x (B, H, W, C), w (C, M, 4, 4) -> (B, 2H, 2W, M)"""
    b, h, wd, c = x.shape
    m = w.shape[1]
    yp = torch.zeros(b, 2 * h + 2, 2 * wd + 2, m, dtype=x.dtype, device=x.device)
    x2 = x.reshape(-1, c)
    for ky in range(4):
        for kx in range(4):                                 # output row o = 2i - 1 + ky, i.e. padded row 2i + ky
            yp[:, ky:ky + 2 * h:2, kx:kx + 2 * wd:2, :] += (x2 @ w[:, :, ky, kx]).view(b, h, wd, m)
    y = yp[:, 1:-1, 1:-1, :]
    return y if bias is None else y + bias


def s2_wgrad(half, full):
    """dW[h][f][ky][kx] = sum_{b,i,j} half[b,i,j,h] * full[b, 2i-1+ky, 2j-1+kx, f] (zero outside): the weight gradient of a Conv2d
    (half = output gradient, full = its input) or of a ConvTranspose2d (half = its input, full = output gradient)"""
    b, hh, wh, ch = half.shape
    cf = full.shape[3]
    fp = _pad1(full)
    h2 = half.reshape(-1, ch).t()
    dw = torch.empty(ch, cf, 4, 4, dtype=half.dtype, device=half.device)
    for ky in range(4):
        for kx in range(4):
            dw[:, :, ky, kx] = h2 @ fp[:, ky:ky + 2 * hh:2, kx:kx + 2 * wh:2, :].reshape(-1, cf)
    return dw


def bn_stats(y, gamma, beta, eps=1e-5, momentum=0.1, running_mean=None, running_var=None):
    """training-mode BatchNorm2d on channels-last y: dict(mean, var (biased), rstd, scale = gamma * rstd, shift = beta - mean * scale,
    and the momentum-updated running buffers (unbiased variance) when given)"""
    c = y.shape[-1]
    y2 = y.reshape(-1, c)
    n = y2.shape[0]
    mean = y2.mean(0)
    var = ((y2 - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    out = dict(mean=mean, var=var, rstd=rstd, scale=gamma * rstd, shift=beta - mean * gamma * rstd)
    if running_mean is not None:
        out["running_mean"] = (1 - momentum) * running_mean + momentum * mean
        # one pixel per channel has no unbiased variance (torch refuses the batch): the kernels keep the biased one, 0
        out["running_var"] = (1 - momentum) * running_var + momentum * var * n / max(n - 1, 1)
    return out


def bn_stats_abs(y, gamma, beta, eps=1e-5, momentum=0.1, running_mean=None, running_var=None):
    """absolute-value twin of bn_stats: the mean's is mean|y|; the variance is a sum of squares about the mean, so it, rstd and scale are
    their own twins; shift and the running buffers add the magnitudes of their terms"""
    c = y.shape[-1]
    n = y.reshape(-1, c).shape[0]
    s = bn_stats(y, gamma, beta, eps)
    amean = y.reshape(-1, c).abs().mean(0)
    out = dict(mean=amean, var=s["var"], rstd=s["rstd"], scale=s["scale"].abs(), shift=beta.abs() + amean * s["scale"].abs())
    if running_mean is not None:
        out["running_mean"] = abs(1 - momentum) * running_mean.abs() + momentum * amean
        out["running_var"] = abs(1 - momentum) * running_var.abs() + momentum * s["var"] * n / max(n - 1, 1)
    return out


def bn_fold_eval(gamma, beta, running_mean, running_var, eps=1e-5):
    """eval-mode BatchNorm2d as an on-load transform: (scale, shift) = (gamma / sqrt(running_var + eps), beta - running_mean * scale)"""
    scale = gamma / torch.sqrt(running_var + eps)
    return scale, beta - running_mean * scale


def bn_fold_eval_abs(gamma, beta, running_mean, running_var, eps=1e-5):
    scale = gamma.abs() / torch.sqrt(running_var + eps)
    return scale, beta.abs() + running_mean.abs() * scale


def bn_act_backward(y, ga, gamma, beta, mean, rstd, slope, act=True, mask=None):
    """gradient of act(BatchNorm(y)) in training mode, act = LeakyReLU(slope) or (act=False) the identity: (gy, dgamma, dbeta) given ga
    w.r.t. the activation.  mask, when given, is act' per element (1 or slope) and replaces the sign of z computed here."""
    c = y.shape[-1]
    xhat = (y - mean) * rstd
    if mask is None:
        z = xhat * gamma + beta
        mask = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope)) if act else torch.ones_like(z)
    gz = ga * mask
    g2, x2 = gz.reshape(-1, c), xhat.reshape(-1, c)
    dbeta, dgamma = g2.sum(0), (g2 * x2).sum(0)
    gy = gamma * rstd * (gz - g2.mean(0) - xhat * (g2 * x2).mean(0))
    return gy, dgamma, dbeta


def bn_act_backward_abs(y, ga, gamma, mean, rstd, mask):
    """absolute-value twin of bn_act_backward: |gz|, |xhat| and the sums of absolute values through the same formula, every term added"""
    c = y.shape[-1]
    xhat = ((y - mean) * rstd).abs()
    gz = (ga * mask).abs()
    g2, x2 = gz.reshape(-1, c), xhat.reshape(-1, c)
    dbeta, dgamma = g2.sum(0), (g2 * x2).sum(0)
    gy = (gamma * rstd).abs() * (gz + g2.mean(0) + xhat * (g2 * x2).mean(0))
    return gy, dgamma, dbeta


def act_backward(y, ga, slope):
    """gradient of LeakyReLU(y) without BatchNorm; a single product, so its absolute-value twin is |result|"""
    return ga * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, slope))


# ---- the stem Linear of Generator_wgan, outputs permuted NCHW -> NHWC (csrc/stride2.hip) ------------------------------------------
def stem(z, w, bias, s, c):
    """y[b, p, c] = bias[c S + p] + sum_k z[b, k] w[c S + p, k]: z (B, K), w (C S, K) -> (B, S, C).  Linear in every operand with
    non-negative coefficients: its absolute-value twin is stem(|z|, |w|, |bias|)."""
    return (z @ w.t() + bias).view(z.shape[0], c, s).permute(0, 2, 1).contiguous()


def stem_grads(z, g, s, c):
    """(gW, gb) of stem for the output gradient g (B, S, C): gW[c S + p, k] = sum_b g[b, p, c] z[b, k], gb[c S + p] = sum_b g[b, p, c];
    twin: stem_grads(|z|, |g|)"""
    g2 = g.permute(0, 2, 1).reshape(g.shape[0], c * s)
    return g2.t() @ z, g2.sum(0)


# ---- adjoint identities -------------------------------------------------------------------------------------------------------
def identity_margins(x, w, y, g, gx, gw, eps):
    """<y, g> = <x, gx> = <w, gw> for y = conv(x; w), gx = dgrad(g; w), gw = wgrad(x, g): (|a0 - a1| / tau1, |a0 - a2| / tau2), each < 1
    for a result within eps (the mode's element-wise bound) of the exact one.  A local error in y of size eps * max|y| moves <y, g> by at
    most eps * max|y| * |g| when it is random over the pixels (a random-sign sum grows like the square root of the number of terms, so
    the bound grows like the L2 norm, not like the number of elements); 6x covers both tails of two such sums.
        tau1 = 6 eps (max|y| |g| + max|gx| |x|),   tau2 = 6 eps (max|y| |g| + max|gw| |w|)   (|.| the L2 norm)"""
    d = lambda a, b: float((a.double() * b.double()).sum())
    nrm = lambda a: float(a.double().norm())
    amax = lambda a: float(a.double().abs().max())
    a0, a1, a2 = d(y, g), d(x, gx), d(w, gw)
    tau1 = 6 * eps * (amax(y) * nrm(g) + amax(gx) * nrm(x))
    tau2 = 6 * eps * (amax(y) * nrm(g) + amax(gw) * nrm(w))
    return abs(a0 - a1) / tau1, abs(a0 - a2) / tau2
