/*
 * ngan.h -- C ABI of libngan_hip.so: hand-written gfx950 (MI355X) kernels for the PGGAN / WGAN-GP
 * training step of oliviertrottier/neuron-gan.
 *
 * The reference has no FFI of its own: its hot path dispatches torch ATen operators from Python
 * (SURVEY.md 2.1).  Each entry point below replaces one of those dispatch sites; the reference
 * call site it stands in for is cited as file:line into /root/reference.  The reference-side
 * binding a maintainer would add is a ctypes stub, shown in INTEGRATION.md.
 *
 * Conventions
 *   - every tensor is fp32, device memory, pixel-major / channels-last: (B, H, W, C) contiguous.
 *     Images with C == 1 have the same bytes as the reference's NCHW tensors.  (The last section, "bf16 activation
 *     storage", adds entry points whose activation tensors are bf16; everything before it is the fp32 contract.)
 *   - weights keep the reference's parameter layouts (OIHW for convs, (out, in) for Linear), so
 *     state_dict tensors are passed as they are.
 *   - the caller allocates every output and workspace; the library never allocates, frees or
 *     synchronises.  `stream` is a hipStream_t (PyTorch's current stream), passed as void*.
 *   - return value: 0 ok; < 0 invalid argument / unsupported shape (see ngan_last_error());
 *     > 0 a hipError_t from the launch.
 *   - resample codes:  0 none, 1 avg-pool 2x2 on load, 2 bilinear x2 (align_corners=False) on load.
 */
#ifndef NGAN_H
#define NGAN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGAN_OK 0
#define NGAN_ERR_ARG (-1)
#define NGAN_ERR_SHAPE (-2)

#define NGAN_RESAMPLE_NONE 0
#define NGAN_RESAMPLE_POOL2 1
#define NGAN_RESAMPLE_UP2 2
/* flags of ngan_conv3x3_fwd / ngan_conv3x3_fwd_ex (per call; the library keeps no mutable global state) */
#define NGAN_CONV_SKIP_BORDER 1   /* precision 3 only: do not launch the border-ring kernel, the caller follows up with ngan_conv3x3_up2_border */

const char* ngan_version(void);
const char* ngan_last_error(void);

/* ---- 3x3 convolution, pad 1, stride 1: Conv2d_normalized.forward, models.py:203-204 (ATen conv2d) ---------
 * The kernels are an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32).  Weights are first re-ordered
 * into MFMA fragment order and pre-multiplied by the equalised-LR constant `scale` (models.py:201).
 *   mode 0 (forward):  k = Cin, n = Cout.
 *   mode 1 (dgrad):    k = Cout, n = Cin, taps flipped: the same kernel then computes the input gradient.
 * `packed` holds ngan_conv3x3_packed_floats(...) floats.  Cin and Cout must be multiples of 16. */
int ngan_conv3x3_pack_weights(const float* w_oihw, float* packed, int Cout, int Cin, int mode, float scale, int precision,
                              void* stream);
/* precision 0: exact fp32 MFMA (v_mfma_f32_16x16x4_f32).  precision 1: "bf16x3" -- every fp32 operand is split into
 * hi = bf16(v), lo = bf16(v - hi) and a product is hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_bf16 with fp32
 * accumulation (relative error ~1e-5 per product instead of ~1e-7; ~5x the fp32 MFMA rate, which makes these layers
 * HBM-bound).  Ask before packing / calling -- the answer is the precision CODE to pack with and to pass to the conv call:
 *   0 exact fp32;  1 split-bf16;  2 split-bf16 with a K = 16 contraction zero-padded to 32 (its own packed layout);
 *   3 split-bf16 with the bilinear x2 of `resample` 2 folded into the weights (N = 16, K in {16, 32}, large images): `packed` then
 *     holds four 3x3 weight sets over the LOW-resolution input, one per output parity (py, px),
 *     W_eff[dr][dc] = sum_{ky,kx} W[ky][kx] * E[py][ky][dr] * E[px][kx][dc]  (E: the .25/.75 blend rows of upsample_bilinear2d,
 *     align_corners = False), followed by the scaled fp32 weights for the one-pixel border ring (mode 0 only);
 *   4 exact fp32 by Winograd F(2x2, 3x3) (answered for a REQUESTED precision 0 on large images: the 16 -> 16 layers with plain or
 *     bilinear input, and -- on widths that are multiples of 32 -- every shape with K, N in {16, 32}, plain or bilinear input):
 *     `packed` holds the 16 transformed weight sets G g G^T (16 * Cin * Cout floats), the kernel transforms 4x4 input patches
 *     (B^T d B; bilinear input: (B^T E) L (B^T E)^T straight from the 3x3 low-resolution patch) and 2x2 output tiles (A^T M A) per
 *     lane and spends 16 instead of 36 v_mfma_f32_16x16x4_f32 per 16 pixels and 16 x 16 channel pair.  fp32 arithmetic throughout;
 *     its error against an fp64 evaluation of the fused operator is below 1e-6 relative L2 (tests/test_gpu_ops.py::
 *     test_winograd_kernels_against_fp64; the direct form: 2.6e-7 against 1.5e-7 on the same operands).
 * The answer depends on the shape only: the library reads no environment variable. */
int ngan_conv3x3_algorithm(int B, int H, int W, int K, int N, int resample, int precision);
long ngan_conv3x3_packed_floats(int Cout, int Cin, int precision);   /* size of `packed` in floats */

/* Re-pack many weights with ONE launch (after an optimiser step).  `table` is a device array of n_entries records
 *   { const float* src; float* dst; int Cout, Cin, mode, precision; float scale; int pad; long first; }          (48 bytes)
 * where `first` is the running sum of ngan_conv3x3_pack_elements(...) over the preceding entries (the unit is one packed
 * element: a float for precision 0 / 4, a bf16 for precision 1 / 2, precision 3: bf16 for the four sets, then one per raw fp32
 * weight) and total_elements is the sum over all entries. */
long ngan_conv3x3_pack_elements(int Cout, int Cin, int mode, int precision);
int ngan_conv3x3_pack_many(const void* table, int n_entries, long total_elements, void* stream);

/* y = epilogue(conv3x3(resample(x), packed) + bias)      (models.py:252-268 fused: resample, conv, LReLU, PixelNorm)
 *   x        resample 0: (B,H,W,K)   1: (B,2H,2W,K)   2: (B,H/2,W/2,K)       (H, W: conv/output resolution)
 *   bias     N floats or NULL
 *   epilogue 0: y = conv (+bias)            1: y = PixelNorm(LeakyReLU(conv + bias)), rnorm (B,H,W) = sqrt(mean_c a^2 + eps)
 *   out_mode 0: y is (B,H,W,N)              1: avg-pool adjoint store: y is (B,2H,2W,N), each value * 0.25 to its 2x2 block
 * K = contraction channels (any multiple of 16), N = output channels: 16, 32, 64 or 128 per call (the Python layer runs wider
 * layers as output-channel chunks of these sizes, ops._n_chunks). */
int ngan_conv3x3_fwd(const float* x, const float* packed, const float* bias, float* y, float* rnorm,
                     int B, int H, int W, int K, int N, int resample, int epilogue, int out_mode,
                     float slope, float eps, int precision, int flags, void* stream);

/* The same kernels with two more fused epilogues (what the hand-scheduled first-order passes of train.py:365, 384 use):
 *   epilogue 2: the call computes an input gradient g (packed = flipped weights) and applies the backward of the
 *               LeakyReLU -> PixelNorm that produced the layer's input: y = m*(g - aux_in*mean_c(g*aux_in))/aux_rn with
 *               m = aux_in > 0 ? 1 : slope.  aux_in (same shape as y, also with out_mode 1) is that input, aux_rn its norms.
 *               No resampling, no bias.  Always available: shapes without a fused kernel run the PixelNorm backward in place
 *               as a second launch (ngan_conv3x3_epilogue_fused tells which).
 *   epilogue 3: epilogue 1 followed by ToImage (models.py:141-146, one colour): aux_out (B,H,W) = tanh(sum_c aux_in[c]*y[c]);
 *               aux_in = the N colour weights.  y / rnorm may be NULL (inference: the activation is never written).
 *               Only where ngan_conv3x3_epilogue_fused(...) returns 1. */
/* Precision 3 (bilinear x2 folded into the weights): the one-pixel border ring of the output is written by a second, small kernel.
 * By default ngan_conv3x3_fwd / _fwd_ex launch it themselves.  With flags & NGAN_CONV_SKIP_BORDER a call launches the main kernel
 * only and the caller follows it with ngan_conv3x3_up2_border on the same stream (the Python layer does, so that a per-call timer
 * around ngan_conv3x3_fwd brackets exactly one kernel).  The choice is per call: nothing is remembered between calls. */
int ngan_conv3x3_up2_border(const float* x, const float* packed, const float* bias, float* y, float* rnorm,
                            int B, int H, int W, int K, int N, int epilogue, float slope, float eps, void* stream);
int ngan_conv3x3_epilogue_fused(int B, int H, int W, int K, int N, int resample, int epilogue, int out_mode, int precision);
/* Pooled side output of epilogue 1: where this returns 1 (the Winograd kernels, precision code 4, on whole 32-pixel tiles and even
 * H), ngan_conv3x3_fwd_ex with epilogue 1 and aux_out != NULL also writes aux_out (B, H/2, W/2, N) = the 2x2 average of y -- the
 * input of the next block's AvgPool2d(2) + conv (models.py:252-254) -- with the association of ngan_pool2_fwd, i.e. the same
 * bits a separate pooling pass over y would give.  Elsewhere aux_out must be NULL for epilogue 1. */
int ngan_conv3x3_pooled_output(int B, int H, int W, int K, int N, int resample, int precision);
int ngan_conv3x3_fwd_ex(const float* x, const float* packed, const float* bias, float* y, float* rnorm,
                        const float* aux_in, const float* aux_rn, float* aux_out,
                        int B, int H, int W, int K, int N, int resample, int epilogue, int out_mode,
                        float slope, float eps, int precision, int flags, void* stream);

/* name of the kernel template instance ngan_conv3x3_fwd dispatches to for these arguments, as rocprofv3 prints it
 * (profiling aid: lets bench.py label its HIP-event timings with the same names as the kernel trace) */
int ngan_conv3x3_kernel_name(int B, int H, int W, int K, int N, int resample, int epilogue, int out_mode, int precision,
                             char* buf, int len);
/* the same for ngan_conv3x3_wgrad (its main kernel; the slab reduction is a second kernel) */
int ngan_conv3x3_wgrad_kernel_name(int B, int H, int W, int Cin, int Cout, int resample, int precision, char* buf, int len);

/* weight gradient (ATen convolution_backward, weight part):
 *   gw[co][ci][ky][kx] = scale * sum_{b,y,x} g[b,y,x,co] * resample(x)[b,y+ky-1,x+kx-1,ci]      gw is OIHW
 * precision 1 requests the split-bf16 kernel (used when the image is at least 32 pixels wide, else exact fp32).
 * accumulate != 0: gw += ... (adds into an existing gradient buffer).  workspace: ngan_conv3x3_wgrad_workspace_bytes(...) bytes.
 * precision 0 on images wider than 16 pixels contracts in Winograd form, dW = G^T [ sum over 2x2 output tiles (A dY A^T) . (B^T d B) ] G
 * (fp32 arithmetic, 16 position accumulators instead of 9 taps, the back-transform applied to every partial sum before it is written:
 * same slabs, same fixed-order reduction). */
size_t ngan_conv3x3_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int ngan_conv3x3_wgrad(const float* x, const float* g, float* gw, float* workspace,
                       int B, int H, int W, int Cin, int Cout, int resample, float scale, int accumulate, int precision,
                       void* stream);

/* Deferred reduction.  ngan_conv3x3_wgrad(..., accumulate = 2, ...) writes the slabs only; later ONE call reduces the slabs of many
 * such calls (a whole backward pass) and merges up to 4 contributions to the same gradient tensor in a fixed order.
 * `entries`: host array of n records
 *   { const float* partial[4]; float* gw; int nparts[4]; int nsrc, nslices, n_ci_slices, co_s, ci_s, K, accumulate, reserved;
 *     float scale[4]; }                                                                                     (104 bytes)
 * with (nparts, nslices, n_ci_slices, co_s, ci_s) from ngan_conv3x3_wgrad_plan (out5).  accumulate != 0: gw += sum.
 * Several records may name the same gw (more than 4 contributions: the later records accumulate): they are applied in their order,
 * each in a launch after the previous one's. */
int ngan_conv3x3_wgrad_plan(int B, int H, int W, int Cin, int Cout, int precision, int* out5);
int ngan_conv3x3_wgrad_reduce_many(const void* entries, int n, void* stream);

/* ---- LeakyReLU -> PixelNorm: models.py:263-264, 118-126 (ATen leaky_relu, pow, mean, sqrt, div) ---------------
 * fwd:    a = lrelu(c + bias); r = sqrt(mean_c(a^2) + eps); y = a / r
 * bwd:    gc = m * ((gy - y*mean_c(gy*y)) / r + gr*y/C),  m = (y > 0 ? 1 : slope); gr (npix) may be NULL
 * bwdbwd: given h = dL/d(gc) of a bwd call made with gr == NULL:
 *           ggy = (h' - y*t)/r,  gy_out = -(s*h' + t*gy)/r,  gr_out = -C*(u - s*t)/r^2
 *           with h' = m*h, s = mean_c(gy*y), t = mean_c(h'*y), u = mean_c(h'*gy)
 * C is any multiple of 4.  C/4 a power of two <= 64 (C = 4, 8, 16 ... 256) runs in the lane-group kernels (C/4 consecutive lanes per
 * pixel, butterfly reductions); every other C -- 48, 96, 320, 512, 1024 ... -- in csrc/wide.hip: one thread per pixel walking the
 * channels, fixed summation order, meant for the wide presets' small images.  y may alias c and gc may alias gy (in-place calls). */
int ngan_lrelu_pixelnorm_fwd(const float* c, const float* bias, float* y, float* rnorm, long npix, int C,
                             float slope, float eps, void* stream);
int ngan_lrelu_pixelnorm_bwd(const float* gy, const float* gr, const float* y, const float* rnorm, float* gc,
                             long npix, int C, float slope, void* stream);
/* bwd with the incoming gradient given as a sum of two tensors (gy + gy2; gy2 may be NULL): in the gradient-penalty pass the
 * gradient w.r.t. a layer output has two contributions, and summing them here saves a separate elementwise pass */
int ngan_lrelu_pixelnorm_bwd2(const float* gy, const float* gy2, const float* gr, const float* y, const float* rnorm, float* gc,
                              long npix, int C, float slope, void* stream);
int ngan_lrelu_pixelnorm_bwdbwd(const float* h, const float* gy, const float* y, const float* rnorm,
                                float* ggy, float* gy_out, float* gr_out, long npix, int C, float slope, void* stream);

/* column sums over pixels: out[c] = scale * sum_p g[p][c]   (bias gradient of conv2d).  workspace: 1024*C floats */
int ngan_channel_sum(const float* g, float* out, float* workspace, long npix, int C, float scale, void* stream);
/* Small parameter gradients added straight into an existing gradient buffer (the step driver's flat .grad views) instead of being
 * returned and added by a separate elementwise launch: the `_acc` forms take `accumulate`, a bit mask over the function's outputs
 * (bit i set: output i is added into, clear: written).  channel_sum: out (bit 0). */
int ngan_channel_sum_acc(const float* g, float* out, float* workspace, long npix, int C, float scale, int accumulate, void* stream);

/* ---- FromImage 1x1 conv + bias: models.py:161-165 ---------------------------------------------------------------
 * fwd: y[p][c] = sum_k w[c][k]*x[p][k] + b[c];  pool=1: x is (B,2H,2W,Ncol) and is 2x2-averaged on load (models.py:519)
 * dx:  gx[p][k] = sum_c w[c][k]*g[p][c];        pool=1: gx is (B,2H,2W,Ncol), avg-pool adjoint store
 * dw:  gw[c][k] = sum_p g[p][c]*x[p][k], gb[c] = sum_p g[p][c] (gb may be NULL).  workspace: 1024*C*(Ncol+1) floats */
int ngan_from_image_fwd(const float* x, const float* w, const float* b, float* y, int B, int H, int W, int Ncol, int C,
                        int pool, void* stream);
int ngan_from_image_dx(const float* g, const float* w, float* gx, int B, int H, int W, int Ncol, int C, int pool, void* stream);
int ngan_from_image_dw(const float* x, const float* g, float* gw, float* gb, float* workspace,
                       int B, int H, int W, int Ncol, int C, int pool, void* stream);
int ngan_from_image_dw_acc(const float* x, const float* g, float* gw, float* gb, float* workspace,
                           int B, int H, int W, int Ncol, int C, int pool, int accumulate, void* stream);   /* accumulate: bit 0 gw, bit 1 gb */

/* ---- ToImage 1x1 conv + tanh: models.py:141-149 ------------------------------------------------------------------
 * fwd: t[p][k] = tanh(sum_c w[k][c]*x[p][c])
 * bwd: q = g*(1-t^2); gx[p][c] = sum_k q[p][k]*w[k][c]; gw[k][c] = sum_p q[p][k]*x[p][c].  workspace: 1024*C*Ncol floats */
int ngan_to_image_fwd(const float* x, const float* w, float* t, long npix, int C, int Ncol, void* stream);
int ngan_to_image_bwd(const float* g, const float* t, const float* x, const float* w, float* gx, float* gw,
                      float* workspace, long npix, int C, int Ncol, void* stream);
/* to_image_bwd where the ToImage input is the output y of a LeakyReLU -> PixelNorm (norms rnorm): gc receives the gradient w.r.t.
 * that operator's input, i.e. the PixelNorm/LeakyReLU backward is applied before the store (one pass over the activation) */
int ngan_to_image_bwd_pnbwd(const float* g, const float* t, const float* y, const float* rnorm, const float* w, float* gc,
                            float* gw, float* workspace, long npix, int C, int Ncol, float slope, void* stream);
int ngan_to_image_bwd_pnbwd_acc(const float* g, const float* t, const float* y, const float* rnorm, const float* w, float* gc,
                                float* gw, float* workspace, long npix, int C, int Ncol, float slope, int accumulate, void* stream);   /* accumulate != 0: gw += */

/* ---- resampling: models.py:87-89 (F.interpolate bilinear, align_corners=None) and models.py:254 (AvgPool2d(2)) --
 * (h, w) is always the LOW resolution; adjoint = transpose of the linear map. */
int ngan_up2_fwd(const float* x, float* y, int B, int h, int w, int C, void* stream);
int ngan_up2_adjoint(const float* gy, float* gx, int B, int h, int w, int C, void* stream);
/* up2_adjoint followed by the backward of the LeakyReLU -> PixelNorm that produced the low-resolution tensor `yprev` (B,h,w,C) with
 * norms `rnorm`: out = m*(g' - yprev*mean_c(g'*yprev))/rnorm, g' = up2_adjoint(g).  C is any multiple of 4: one fused kernel where C/4
 * is a power of two <= 64, otherwise two launches (ngan_up2_adjoint into `out`, then the PixelNorm backward of csrc/wide.hip in place). */
int ngan_up2_adjoint_pnbwd(const float* g, const float* yprev, const float* rnorm, float* out, int B, int h, int w, int C,
                           float slope, void* stream);
int ngan_pool2_fwd(const float* x, float* y, int B, int h, int w, int C, void* stream);
int ngan_pool2_adjoint(const float* gy, float* gx, int B, int h, int w, int C, void* stream);

/* ---- fade-in and interpolation arithmetic: models.py:350, 521; loss_functions.py:171 -----------------------------
 * lerp:   out = a + alpha*(b - a), alpha read from device memory (so a captured graph follows the transition)
 * axpby:  out = ca*a + cb*b with host scalars (b may be NULL -> out = ca*a)
 * fade_bwd: ga = (1-alpha)*g, gb = alpha*g
 * xhat:   out[b,:] = eps[b]*real[b,:] + (1-eps[b])*fake[b,:] */
int ngan_lerp(const float* a, const float* b, const float* alpha, float* out, long n, void* stream);
int ngan_axpby(const float* a, const float* b, float ca, float cb, float* out, long n, void* stream);
int ngan_fade_bwd(const float* g, const float* alpha, float* ga, float* gb, long n, void* stream);
int ngan_xhat(const float* real, const float* fake, const float* eps, float* out, int B, long n, void* stream);

/* ---- gradient penalty pieces: loss_functions.py:176 (ATen linalg_vector_norm) ----------------------------------
 * norms[b] = ||g[b,:]||_2 (two fixed-order stages; g 16-byte aligned and n a multiple of 4 so that every row is, or B = 1 with any n:
 * NGAN_ERR_SHAPE otherwise);   scale_rows: out[b,:] = coef[b] * g[b,:] */
int ngan_sample_l2norm(const float* g, float* norms, float* workspace /* 64*B floats */, int B, long n, void* stream);
int ngan_scale_rows(const float* g, const float* coef, float* out, int B, long n, void* stream);
/* the penalty's scalar head and its adjoint: out1 = lambda * mean((norms - 1)^2);  coef[b] = g_out * 2 lambda (norms[b] - 1) / (B norms[b])
 * (feed coef to ngan_scale_rows to get the gradient w.r.t. g) */
int ngan_gp_head(const float* norms, int B, float lambda, float* out1, void* stream);
int ngan_gp_coef(const float* norms, int B, float lambda, const float* g_out /* 1 float */, float* coef, void* stream);

/* ---- scalar heads of the Wasserstein losses: loss_functions.py:21-45, 67 (ATen mean / neg / add / square chains) -----------
 * scores holds n_real real scores followed by n_fake fake scores.  loss = -mean(real) + mean(fake) + drift * mean(real^2), plus the two means
 * (three separate 1-float outputs);  n_fake = 0 gives -mean(scores), the generator loss.  bwd: gradient w.r.t. scores from the three
 * output gradients (device scalars, NULL = 0). */
int ngan_wloss_head(const float* scores, int n_real, int n_fake, float drift, float* loss, float* mean_real, float* mean_fake,
                    void* stream);
int ngan_wloss_head_bwd(const float* scores, int n_real, int n_fake, float drift, const float* g_loss, const float* g_real,
                        const float* g_fake, float* g_scores, void* stream);

/* ---- scalar heads of the objectives beside the Wasserstein one (least squares): declared in ngan_objectives.h, which this header
 * includes -- one ABI: a caller includes ngan.h alone, and _C.py binds this file and its extension sections from one table ---- */
#include "ngan_objectives.h"
/* ---- minibatch standard deviation of the PG critic's head (opt-in): declared in ngan_mbstd.h, an extension section likewise ---- */
#include "ngan_mbstd.h"
/* ---- geometric groups of the differentiable augmentation (blit, geometry): declared in ngan_geoaug.h, an extension section likewise ---- */
#include "ngan_geoaug.h"
/* ---- one-sided and zero-centred forms of the gradient penalty (opt-in): declared in ngan_penalty.h, an extension section likewise ---- */
#include "ngan_penalty.h"
/* ---- launch plan of the folded critic first block as a host query: declared in ngan_first_block.h, an extension section likewise ---- */
#include "ngan_first_block.h"
/* ---- spectral regularisation of the generator (opt-in): declared in ngan_spectral.h, an extension section likewise ---- */
#include "ngan_spectral.h"

/* ---- latent projection: utils.py:77-78 (clamp(-c, c), L2-normalise each row), in place on (rows, dim) normal draws ---------- */
int ngan_latent_normalize(float* z, int rows, int dim, float clamp, void* stream);

/* ---- generator stem: Linear_normalized -> Unflatten -> LeakyReLU -> PixelNorm, models.py:299-311 (ATen mm) --------
 * fwd:   y[b][p][c] = PN(LReLU(scale * sum_k z[b][k] * Wt[c*S + p][k])),  y (B,S,C), rnorm (B,S); W is (C*S, K)
 * wgrad: gW[c*S+p][k] = scale * sum_b gc[b][p][c] * z[b][k]
 * dgrad: gz[b][k] = scale * sum_{p,c} gc[b][p][c] * W[c*S+p][k]
 * Shapes (NGAN_ERR_SHAPE otherwise), any B > 0:
 *   fwd:   K a multiple of 16, and 64 * (K + C + 9) bytes of LDS (16 samples x (K + 4) latents and (C + 4) channels, 16 norms) at most
 *          160 KiB, i.e. K + C <= 2551; above 64 KiB (K + C > 1015) the launch raises the kernel's dynamic-LDS limit first.
 *   wgrad: K a multiple of 4, at most 1024.  K a multiple of 16 and at most 512 takes the MFMA form (one pass over the samples, the
 *          only form with accumulate and with the optimiser epilogues); every other K the row-streaming form (16-sample register
 *          chunks, fp32 read-modify-write across the chunks).
 *   dgrad: any K. */
int ngan_linear_lrelu_pn_fwd(const float* z, const float* Wt, float* y, float* rnorm, int B, int K, int S, int C,
                             float scale, float slope, float eps, void* stream);
int ngan_linear_wgrad(const float* z, const float* gc, float* gW, int B, int K, int S, int C, float scale, void* stream);
/* accumulate != 0: gW += ... (K <= 512, a multiple of 16; NGAN_ERR_SHAPE for any other K): adds straight into the parameter's gradient buffer */
int ngan_linear_wgrad_acc(const float* z, const float* gc, float* gW, int B, int K, int S, int C, float scale, int accumulate,
                          void* stream);
/* the same contraction with Adam applied in its epilogue instead of a stored gradient (K <= 512, a multiple of 16; any B -- the
 * data-parallel ranks pass the gathered factors): p, m, v are the stem weight's slices of the flat parameter / moment buffers,
 * seg_step points at its (already advanced) step count, hyper as in ngan_adam_step.  Replaces, for this tensor, the store in
 * ngan_linear_wgrad plus its chunks of ngan_adam_step: same arithmetic, same bits. */
int ngan_linear_wgrad_adam(const float* z, const float* gc, float* p, float* m, float* v, const float* seg_step,
                           const float* hyper, int n_hyper, int B, int K, int S, int C, float scale, void* stream);
int ngan_linear_dgrad(const float* gc, const float* Wt, float* gz, int B, int K, int S, int C, float scale, void* stream);

/* ---- critic head: Conv2d_normalized(C, 1, (S,S), padding 0) + Flatten, models.py:485-490 ------------------------
 * fwd: out[b] = scale * sum_{p,c} y[b][p][c]*W[c*S2+p] + bias[0]
 * dx:  gy[b][p][c] = scale * go[b] * W[c*S2+p]
 * dw:  gW[c*S2+p] = scale * sum_b go[b]*y[b][p][c];  gb[0] = sum_b go[b] */
int ngan_final_dot_fwd(const float* y, const float* W, const float* bias, float* out, int B, int S2, int C, float scale, void* stream);
int ngan_final_dot_dx(const float* go, const float* W, float* gy, int B, int S2, int C, float scale, void* stream);
int ngan_final_dot_dw(const float* y, const float* go, float* gW, float* gb, int B, int S2, int C, float scale, void* stream);
int ngan_final_dot_dw_acc(const float* y, const float* go, float* gW, float* gb, int B, int S2, int C, float scale, int accumulate,
                          void* stream);                                   /* accumulate: bit 0 gW, bit 1 gb */

/* ---- Adam: optim.Adam.step, train.py:224-225, 366, 385 (betas (beta1, 0.999), eps 1e-8, no weight decay) ---------
 * One launch updates every active segment of a flat parameter buffer.
 *   seg_off[i], seg_len[i]  element offset / length of tensor i inside p, g, m, v   (device, int64)
 *   seg_active[i]           1 if tensor i received a gradient this step (inactive tensors keep step and state)
 *   seg_step[i]             per-tensor step count (device float, incremented here for active tensors)
 *   hyper                   9 device floats {lr, beta1, beta2, eps, grad_scale, 1 - beta1, 1 - beta2, ln beta1, ln beta2} (the last
 *                           four rounded from the host's double values: torch forms `1 - beta` and its bias corrections in
 *                           double; here 1 - beta^t = -expm1(t ln beta)); the gradient is multiplied by grad_scale
 *                           (1/world_size after a SUM all-reduce across data-parallel ranks, otherwise 1)
 *   n_hyper                 the number of floats the caller put into `hyper`: must equal NGAN_ADAM_HYPER_FLOATS.  (`hyper` grew from 5
 *                           to 9 floats in round 3; the count is checked so that a binding written against the older layout gets
 *                           NGAN_ERR_ARG instead of a kernel that reads past its buffer.  ngan_linear_wgrad_adam takes the same pair.)
 * chunk_seg / chunk_off (device int32 / int64): work list, one entry per 4096-element chunk.
 * Non-finite gradients leave what torch leaves: NaN gives NaN in m, v and p; +-inf gives v = inf, p = NaN and m = +-inf, or NaN once
 * 1 - beta1 >= 0.5 (torch's lerp_ evaluates g - (g - m) beta1 from that weight on). */
#define NGAN_ADAM_HYPER_FLOATS 9
int ngan_adam_step(float* p, const float* g, float* m, float* v, const long* seg_off, const long* seg_len,
                   const int* seg_active, float* seg_step, int n_seg, const int* chunk_seg, const long* chunk_off,
                   int n_chunks, const float* hyper, int n_hyper, void* stream);

/* ---- RMSprop: optim.RMSprop.step, train.py:220-222 (the reference's RMSprop switch: alpha 0.99, eps 1e-8, no momentum, not centred,
 * no weight decay) --------------------------------------------------------------------------------------------------------------------
 * The work list, seg_active and seg_step are those of ngan_adam_step (step counts advance for active tensors; the update reads none).
 *   v                       square_avg, the one state buffer (fp32, laid out like p)
 *   hyper                   5 device floats {lr, alpha, eps, grad_scale, 1 - alpha} (1 - alpha rounded from the host's double, as torch
 *                           forms `value=1 - alpha`); per element  g *= grad_scale;  v = alpha*v + (1 - alpha)*g*g;  p -= lr*g/(sqrt(v) + eps)
 *   n_hyper                 must equal NGAN_RMSPROP_HYPER_FLOATS
 * ngan_linear_wgrad_rmsprop: the stem's weight-gradient contraction of ngan_linear_wgrad with this update in its epilogue instead of a
 * stored gradient (K <= 512, a multiple of 16; any B); p and v are the stem weight's slices of the flat buffers.  Same bits as
 * ngan_linear_wgrad followed by ngan_rmsprop_step on the stored gradient. */
#define NGAN_RMSPROP_HYPER_FLOATS 5
int ngan_rmsprop_step(float* p, const float* g, float* v, const long* seg_off, const long* seg_len, const int* seg_active,
                      float* seg_step, int n_seg, const int* chunk_seg, const long* chunk_off, int n_chunks, const float* hyper,
                      int n_hyper, void* stream);
int ngan_linear_wgrad_rmsprop(const float* z, const float* gc, float* p, float* v, const float* hyper, int n_hyper, int B, int K, int S,
                              int C, float scale, void* stream);

/* ---- the averaged generator: an exponential moving average of the parameters (an addition of this implementation with no reference
 * counterpart; opt-in, off by default) ------------------------------------------------------------------------------------------------
 * Update rule, the same in every entry point below:   e' = fmaf(w, p' - e, e)
 *   p'      the parameter value the step has just computed (the fp32 value it stores)
 *   ema     the average e, laid out like p; fp32 in every arithmetic mode (the parameters are fp32 masters in the bf16 mode too)
 *   ema_w   ONE device float, w = fp32(1 - beta) rounded on the host from the double: read by the kernel, so a captured graph replays
 *           with the decay of the moment (as `hyper` does for the learning rate)
 * The difference is rounded once and the fused multiply-add once, in every kernel, so all forms give the same bits.
 * ngan_adam_step_ema / ngan_rmsprop_step_ema: the arguments of ngan_adam_step / ngan_rmsprop_step plus ema, ema_w.  Same work list,
 *   same seg_active gating, same step-count launch; p, m, v and the step counts come out bit-identical to the plain entry points.  An
 *   inactive tensor keeps its average.
 * ngan_linear_wgrad_adam_ema / ngan_linear_wgrad_rmsprop_ema: the stem launches with the average updated in the same epilogue (ema is
 *   the stem weight's slice); same shape rules (K a multiple of 16, at most 512) and host-side validation.
 * ngan_ema_step: the update alone, e' = fmaf(w, p - e, e), for the active tensors of the same segment / chunk tables -- for a path
 *   that cannot use a folded form, and the yardstick of the folded ones (plain step + this = folded step, bit for bit). */
int ngan_adam_step_ema(float* p, const float* g, float* m, float* v, const long* seg_off, const long* seg_len,
                       const int* seg_active, float* seg_step, int n_seg, const int* chunk_seg, const long* chunk_off,
                       int n_chunks, const float* hyper, int n_hyper, float* ema, const float* ema_w, void* stream);
int ngan_rmsprop_step_ema(float* p, const float* g, float* v, const long* seg_off, const long* seg_len, const int* seg_active,
                          float* seg_step, int n_seg, const int* chunk_seg, const long* chunk_off, int n_chunks, const float* hyper,
                          int n_hyper, float* ema, const float* ema_w, void* stream);
int ngan_linear_wgrad_adam_ema(const float* z, const float* gc, float* p, float* m, float* v, const float* seg_step,
                               const float* hyper, int n_hyper, int B, int K, int S, int C, float scale, float* ema, const float* ema_w,
                               void* stream);
int ngan_linear_wgrad_rmsprop_ema(const float* z, const float* gc, float* p, float* v, const float* hyper, int n_hyper, int B, int K,
                                  int S, int C, float scale, float* ema, const float* ema_w, void* stream);
int ngan_ema_step(const float* p, float* ema, const long* seg_off, const long* seg_len, const int* seg_active, const int* chunk_seg,
                  const long* chunk_off, int n_chunks, const float* ema_w, void* stream);

/* ---- the critic's first layer pair as one operator (first-order passes): FromImage (ONE colour channel, models.py:161-165) folded
 * into the block's first 3x3 conv + LeakyReLU + PixelNorm (models.py:252-264).  f[c] = wf[c]*p + bf[c] is affine in one number per
 * pixel, so the conv over its C channels is a 3x3 conv over ONE channel with A[n][t] = scale*sum_c W[n][c][t]*wf[c] and a
 * border-aware bias sum_t Bv[n][t] (taps inside the image only); the C-channel tensor is never written.
 *   p (B,H,W) image (already pooled);  w_conv (N,C,3,3), b_conv (N) or NULL;  wf, bf (C);  y (B,H,W,N), rnorm (B,H,W);
 *   N in {16, 32}, C <= 64
 *   bwd: gw_conv (+)= dL/dW, gwf, gbf, gb_conv (or NULL) from gc = dL/d(pre-activation);  workspace: ngan_first_block_workspace_floats floats
 *   dx:  gx = dL/dp (pool = 0) or its avg-pool adjoint on the (B,2H,2W) image (pool = 1)
 *   the three refuse the same shapes (NGAN_ERR_SHAPE), those for which the plan query of ngan_first_block.h does */
size_t ngan_first_block_table_floats(int N);      /* = 2*9*N: the folded tables A, Bv (written by fwd, read by dx) */
int ngan_first_block_fwd(const float* p, const float* w_conv, const float* wf, const float* bf, const float* b_conv, float* y,
                         float* rnorm, float* tables, int B, int H, int W, int C, int N, float scale, float slope, float eps,
                         void* stream);
size_t ngan_first_block_workspace_floats(int B, int H, int N);
int ngan_first_block_bwd(const float* p, const float* gc, const float* w_conv, const float* wf, const float* bf,
                         float* gw_conv, float* gwf, float* gbf, float* gb_conv, float* workspace, int B, int H, int W, int C,
                         int N, float scale, int accumulate, void* stream);   /* accumulate: bit 0 gw_conv, 1 gwf, 2 gbf, 3 gb_conv */
int ngan_first_block_dx(const float* gc, const float* tables, float* gx, int B, int H, int W, int N, int pool, void* stream);

/* ---- on-device input pipeline: data/NeuronDataset.py:112-126, 149-164 (torchvision RandomAffine / RandomVerticalFlip /
 * ColorJitter / CenterCrop / Renormalize / Resize(antialias) per image) as two launches per batch, one colour channel.
 *   src     (N, P, P) padded images in [0, 1];  idx (B) int32: which image each sample uses
 *   params  B records { float cos, sin, tx, ty, brightness, contrast; int flip, contrast_first; }   (32 bytes)
 *           source pixel = nearest([cos, sin; -sin, cos] * (dst - (tx, ty))) in centred pixel coordinates, 0 outside
 *   out     (B, S, S) in [-1, 1]: centre crop R x R of the P x P canvas, renormalised, down-sampled to S x S (S divides R) with the
 *           antialiased bilinear (triangle) filter
 *   workspace  ngan_augment_workspace_bytes(B, P) bytes (0 for B <= 0 or P <= 0), fp32, every element overwritten by a call:
 *           B canvases of P x P floats -- canvas b = flip(affine(src[idx[b]])), with brightness (clamped to [0, 1]) applied iff
 *           contrast_first == 0 -- then B x nblk partial sums, nblk = ceil(P P / 2048): partial (b, t) is the sum of the elements
 *           [2048 t, min(2048 (t + 1), P P)) of canvas b in row-major order, added in a fixed order.  The contrast mean is the sum
 *           of a sample's nblk partials over P P.  After the call both are there to be read (tests/test_gpu_augment.py does). */
size_t ngan_augment_workspace_bytes(int B, int P);
int ngan_augment_batch(const float* src, const int* idx, const void* params, float* workspace, float* out,
                       int N, int B, int P, int R, int S, void* stream);

/* ---- data set: the load loop of data/NeuronDataset.py:84-107 for a whole folder of 8-bit, one-colour, square images of one size R
 * (decoded on the host): histogram, 4-class multi-Otsu thresholds (skimage.filters.threshold_multiotsu(img, classes=4)), mean and
 * standard deviation of the noise floor, pad by R / 4 and Gaussian noise in every zero pixel (replace_zero_with_noise, 13-19).
 * pixels = R * R <= 2^23, at most 65535 images per call (NGAN_ERR_SHAPE beyond).  Integer atomics only: results are reproducible.
 *   images     (N, pixels) unsigned bytes           hist    (N, 256) counts, overwritten
 *   thresholds (N, 3) levels t0 < t1 < t2: the lexicographically smallest triplet lo <= t0 < t1 < t2 <= hi - 1 (lo / hi: lowest /
 *              highest occupied level) with the largest sum over the classes lo..t0, t0+1..t1, t1+1..t2, t2+1..hi of S^2 / P, where
 *              P = sum h[v], S = sum v h[v] are exact integers, each term is evaluated in fp64 and an empty class contributes 0
 *   record     (N, 3) doubles { count, mean, std } of the pixels 0 < v < t0 (population standard deviation), in level units
 *   status     (N) 0 ok; 1 fewer than four occupied levels; 2 no pixel with 0 < v < t0 (thresholds and record are zeros for both)
 *   workspace  ngan_multiotsu_workspace_bytes(N) bytes
 *   normals    (N, P, P) standard-normal draws, P = R + 2 * (R / 4);  canvases (N, P, P) in [0, 1]: the source level (0 in the pad),
 *              a level of 0 replaced by trunc(min(max(mean + std * draw, 0), 255)) in fp64, divided by 255.  normals and canvases
 *              must be 16-byte aligned. */
size_t ngan_multiotsu_workspace_bytes(int n_images);
int ngan_u8_histogram(const unsigned char* images, unsigned int* hist, int n_images, long pixels, void* stream);
int ngan_multiotsu4_noise_stats(const unsigned int* hist, void* workspace, int* thresholds, double* record, int* status,
                                int n_images, void* stream);
int ngan_u8_pad_noise_fill(const unsigned char* images, const float* normals, const double* record, float* canvases, int n_images,
                           int R, void* stream);

/* ==== bf16 activation storage ("bf16" mode, precision code 5): BASELINE.json's C2 configuration ==================================
 * The reference computes in the default dtype (/root/reference/train.py:136-144: fp32); this mode is an addition with its OWN,
 * stated tolerance -- never the headline.  The bounds are the ones the tests assert (tests/test_gpu_bf16.py, tests/test_gpu_bf16_wide.py),
 * derived from the CPU emulation of the mode (tests/lowprec_budget.py) as DESIGN.md section 8 describes.
 *
 * What changes: every ACTIVATION tensor -- the (B,H,W,C) outputs of conv / stem / FromImage layers, LeakyReLU -> PixelNorm outputs, and
 * the gradients w.r.t. them -- is stored as bf16 (ngan_bf16 = the raw 16 bits, round-to-nearest-even on store), and the 3x3
 * convolutions multiply bf16 operands with ONE v_mfma_f32_16x16x32_bf16 per product group (the fp32 master weights are rounded to
 * bf16 by the packing kernel, scale folded in first).  What does not: accumulation, PixelNorm statistics and norms (rnorm), biases,
 * LeakyReLU / tanh, the scalar loss heads, images (C = colours: x, x_hat, G(z), dD/dx), latents, every parameter, every parameter
 * gradient and the Adam / RMSprop state are fp32, and those entry points are the ones above.
 *
 * Each ngan_bf16_<op> below has the arguments and semantics of ngan_<op> above; the pointers typed ngan_bf16 are the activation
 * tensors.  Channel counts: the 3x3 conv takes N in {16, 32, 64, 128} and any K that is a multiple of 16 up to 1024 -- K in
 * {16, 32, 64, 128} in the tuned kernels, every other K in 128-channel slices of one fp32 accumulation (the last slice zero-padded
 * in packing and staging; packed layout: bf16_weight in csrc/conv3x3_internal.h), one epilogue and one rounding on the store.  The
 * per-pixel operators take the channel counts of their fp32 twins: C with C/4 a power of two <= 64 in the lane-group kernels, any
 * other C % 4 == 0 in csrc/wide.hip (fp32 arithmetic, one rounding on the store; accumulate refused there, as in fp32).
 * ngan_bf16_up2_adjoint_pnbwd at such C fuses the adjoint and the PixelNorm backward (no bf16 intermediate).
 *
 * 3x3 convolution: ngan_conv3x3_algorithm(..., precision 5) answers 5 for the shapes the bf16 kernel takes (else 0: there is no
 * fallback), ngan_conv3x3_pack_weights / _pack_many / _packed_floats / _pack_elements take precision 5 (packed = bf16 MFMA
 * fragments), ngan_conv3x3_epilogue_fused(..., 5) answers for epilogues 2 and 3.  Resampling (avg-pool 2x2, bilinear x2) happens
 * while the input tile is staged: fp32 blend of the bf16 sources, one rounding.  aux_in: epilogue 2 -> the producer's output (bf16);
 * epilogue 3 -> the N colour weights (fp32).  There is no pooled side output in this mode (the consumer pools on load). */
typedef unsigned short ngan_bf16;
int ngan_bf16_conv3x3_fwd(const ngan_bf16* x, const float* packed, const float* bias, ngan_bf16* y, float* rnorm,
                          const void* aux_in, const float* aux_rn, float* aux_out,
                          int B, int H, int W, int K, int N, int resample, int epilogue, int out_mode,
                          float slope, float eps, void* stream);
/* weight gradient from bf16 x and g (fp32 slabs, fp32 gw; same workspace size, plan (precision 5) and deferred reduction as the
 * fp32 entry point: ngan_conv3x3_wgrad_workspace_bytes, ngan_conv3x3_wgrad_plan(..., 5, out5), ngan_conv3x3_wgrad_reduce_many) */
int ngan_bf16_conv3x3_wgrad(const ngan_bf16* x, const ngan_bf16* g, float* gw, float* workspace,
                            int B, int H, int W, int Cin, int Cout, int resample, float scale, int accumulate, void* stream);

int ngan_bf16_lrelu_pixelnorm_fwd(const ngan_bf16* c, const float* bias, ngan_bf16* y, float* rnorm, long npix, int C,
                                  float slope, float eps, void* stream);
int ngan_bf16_lrelu_pixelnorm_bwd(const ngan_bf16* gy, const float* gr, const ngan_bf16* y, const float* rnorm, ngan_bf16* gc,
                                  long npix, int C, float slope, void* stream);
int ngan_bf16_lrelu_pixelnorm_bwd2(const ngan_bf16* gy, const ngan_bf16* gy2, const float* gr, const ngan_bf16* y, const float* rnorm,
                                   ngan_bf16* gc, long npix, int C, float slope, void* stream);
int ngan_bf16_lrelu_pixelnorm_bwdbwd(const ngan_bf16* h, const ngan_bf16* gy, const ngan_bf16* y, const float* rnorm,
                                     ngan_bf16* ggy, ngan_bf16* gy_out, float* gr_out, long npix, int C, float slope, void* stream);
int ngan_bf16_channel_sum(const ngan_bf16* g, float* out, float* workspace, long npix, int C, float scale, void* stream);
int ngan_bf16_channel_sum_acc(const ngan_bf16* g, float* out, float* workspace, long npix, int C, float scale, int accumulate, void* stream);

int ngan_bf16_from_image_fwd(const float* x, const float* w, const float* b, ngan_bf16* y, int B, int H, int W, int Ncol, int C,
                             int pool, void* stream);
int ngan_bf16_from_image_dx(const ngan_bf16* g, const float* w, float* gx, int B, int H, int W, int Ncol, int C, int pool, void* stream);
int ngan_bf16_from_image_dw(const float* x, const ngan_bf16* g, float* gw, float* gb, float* workspace,
                            int B, int H, int W, int Ncol, int C, int pool, void* stream);
int ngan_bf16_from_image_dw_acc(const float* x, const ngan_bf16* g, float* gw, float* gb, float* workspace,
                                int B, int H, int W, int Ncol, int C, int pool, int accumulate, void* stream);
int ngan_bf16_to_image_fwd(const ngan_bf16* x, const float* w, float* t, long npix, int C, int Ncol, void* stream);
int ngan_bf16_to_image_bwd(const float* g, const float* t, const ngan_bf16* x, const float* w, ngan_bf16* gx, float* gw,
                           float* workspace, long npix, int C, int Ncol, void* stream);
int ngan_bf16_to_image_bwd_pnbwd(const float* g, const float* t, const ngan_bf16* y, const float* rnorm, const float* w, ngan_bf16* gc,
                                 float* gw, float* workspace, long npix, int C, int Ncol, float slope, void* stream);
int ngan_bf16_to_image_bwd_pnbwd_acc(const float* g, const float* t, const ngan_bf16* y, const float* rnorm, const float* w, ngan_bf16* gc,
                                     float* gw, float* workspace, long npix, int C, int Ncol, float slope, int accumulate, void* stream);

int ngan_bf16_up2_fwd(const ngan_bf16* x, ngan_bf16* y, int B, int h, int w, int C, void* stream);
int ngan_bf16_up2_adjoint(const ngan_bf16* gy, ngan_bf16* gx, int B, int h, int w, int C, void* stream);
int ngan_bf16_up2_adjoint_pnbwd(const ngan_bf16* g, const ngan_bf16* yprev, const float* rnorm, ngan_bf16* out, int B, int h, int w, int C,
                                float slope, void* stream);
int ngan_bf16_pool2_fwd(const ngan_bf16* x, ngan_bf16* y, int B, int h, int w, int C, void* stream);
int ngan_bf16_pool2_adjoint(const ngan_bf16* gy, ngan_bf16* gx, int B, int h, int w, int C, void* stream);
/* the critic's fade-in mixes two FEATURE tensors (models.py:521); the generator's mixes images (models.py:350: the fp32 ngan_lerp) */
int ngan_bf16_lerp(const ngan_bf16* a, const ngan_bf16* b, const float* alpha, ngan_bf16* out, long n, void* stream);
int ngan_bf16_fade_bwd(const ngan_bf16* g, const float* alpha, ngan_bf16* ga, ngan_bf16* gb, long n, void* stream);

/* stem and head: the contraction reads the fp32 master weight and fp32 latents (33 MFLOP per image: nothing to gain from a bf16
 * copy of a 67 MB weight that is read once); y / gc are bf16 */
int ngan_bf16_linear_lrelu_pn_fwd(const float* z, const float* Wt, ngan_bf16* y, float* rnorm, int B, int K, int S, int C,
                                  float scale, float slope, float eps, void* stream);
int ngan_bf16_linear_wgrad(const float* z, const ngan_bf16* gc, float* gW, int B, int K, int S, int C, float scale, void* stream);
int ngan_bf16_linear_wgrad_acc(const float* z, const ngan_bf16* gc, float* gW, int B, int K, int S, int C, float scale, int accumulate,
                               void* stream);
int ngan_bf16_linear_wgrad_adam(const float* z, const ngan_bf16* gc, float* p, float* m, float* v, const float* seg_step,
                                const float* hyper, int n_hyper, int B, int K, int S, int C, float scale, void* stream);
int ngan_bf16_linear_wgrad_rmsprop(const float* z, const ngan_bf16* gc, float* p, float* v, const float* hyper, int n_hyper, int B, int K,
                                   int S, int C, float scale, void* stream);
int ngan_bf16_linear_wgrad_adam_ema(const float* z, const ngan_bf16* gc, float* p, float* m, float* v, const float* seg_step,
                                    const float* hyper, int n_hyper, int B, int K, int S, int C, float scale, float* ema,
                                    const float* ema_w, void* stream);
int ngan_bf16_linear_wgrad_rmsprop_ema(const float* z, const ngan_bf16* gc, float* p, float* v, const float* hyper, int n_hyper, int B,
                                       int K, int S, int C, float scale, float* ema, const float* ema_w, void* stream);
int ngan_bf16_linear_dgrad(const ngan_bf16* gc, const float* Wt, float* gz, int B, int K, int S, int C, float scale, void* stream);
int ngan_bf16_final_dot_fwd(const ngan_bf16* y, const float* W, const float* bias, float* out, int B, int S2, int C, float scale, void* stream);
int ngan_bf16_final_dot_dx(const float* go, const float* W, ngan_bf16* gy, int B, int S2, int C, float scale, void* stream);
int ngan_bf16_final_dot_dw(const ngan_bf16* y, const float* go, float* gW, float* gb, int B, int S2, int C, float scale, void* stream);
int ngan_bf16_final_dot_dw_acc(const ngan_bf16* y, const float* go, float* gW, float* gb, int B, int S2, int C, float scale, int accumulate,
                               void* stream);

/* ---- weight clipping fused into the optimiser step (the WGAN critic, reference train.py:489-490) ---------------------------------
 * Arguments as ngan_adam_step / ngan_rmsprop_step, plus clip >= 0: each updated parameter is stored as min(max(p, -clip), clip) --
 * the same bits as the unclipped step followed by p.clamp_(-clip, clip) (NaN passes through, as with clamp_). */
int ngan_adam_step_clip(float* p, const float* g, float* m, float* v, const long* seg_off, const long* seg_len,
                        const int* seg_active, float* seg_step, int n_seg, const int* chunk_seg, const long* chunk_off,
                        int n_chunks, const float* hyper, int n_hyper, float clip, void* stream);
int ngan_rmsprop_step_clip(float* p, const float* g, float* v, const long* seg_off, const long* seg_len, const int* seg_active,
                           float* seg_step, int n_seg, const int* chunk_seg, const long* chunk_off, int n_chunks, const float* hyper,
                           int n_hyper, float clip, void* stream);

/* ---- WGAN nets (reference models.py:728-790): 4x4 stride-2 pad-1 convolutions and training-mode BatchNorm2d, exact fp32 ----------
 * Channels-last fp32 tensors.  W is a torch conv weight [d0][d1][4][4].
 * ngan_s2_pack: Wp (ngan_s2_packed_floats(M, C) floats) = W in the kernels' order for an M-output, C-input pass:
 *     up == 0 (down pass): W is [M][C] (a Conv2d weight, or a ConvTranspose2d weight in its input-gradient pass)
 *     up == 1 (up pass):   W is [C][M] (a ConvTranspose2d weight, or a Conv2d weight in its input-gradient pass)
 * ngan_s2_conv: up == 0: Conv2d(k4, s2, p1): x (B, Hin, Win, C) -> y (B, Hin/2, Win/2, M); Hin, Win even
 *               up == 1: ConvTranspose2d(k4, s2, p1): x (B, Hin, Win, C) -> y (B, 2Hin, 2Win, M)
 *     each input element is read as act(in_scale[c]*x + in_shift[c]) (no affine part when both are null; act = LeakyReLU(slope) when
 *     in_act != 0) -- BatchNorm -> LeakyReLU on load; zero padding applies after it.  y = conv + bias[m] (bias may be null), then
 *     tanh when tanh_out != 0.
 * ngan_s2_wgrad: dW[h][f][ky][kx] = sum_{b,i,j} H(half[b,i,j,h]) * F(full[b, 2i-1+ky, 2j-1+kx, f]), half (B, Hh, Wh, CH),
 *     full (B, 2Hh, 2Wh, CF), H / F the on-load transforms (scale, shift, act) of each operand; work holds
 *     ngan_s2_wgrad_workspace_floats(...) floats.  Conv2d: half = output gradient, full = input.  ConvTranspose2d: the reverse.
 * ngan_bn_stats: batch statistics of y (npix, C): mean, rstd = 1/sqrt(biased var + eps), the on-load transform scale = gamma*rstd,
 *     shift = beta - mean*scale; run_mean / run_var (may both be null) get the momentum update with the unbiased variance; *nbt += 1
 *     (nbt may be null).  The sums of the pixels (shifted by the channel's first) and of their squares are formed in fp32 and in
 *     fp64; the fp32 moments stand where the fp64 ones confirm them, so the variance does not depend on where the first pixel lies.
 *     work: ngan_chan_reduce_workspace_floats(npix, C) floats, 8-byte aligned (fp64 and fp32 partials; the fp32 reductions use a
 *     third of it).
 * ngan_bn_fold_eval: eval-mode BatchNorm as the on-load transform: scale = gamma/sqrt(run_var + eps), shift = beta - run_mean*scale.
 * ngan_bn_act_bwd: g is the gradient w.r.t. act(scale*y + shift); writes gy w.r.t. y.  gamma non-null: training-mode BatchNorm
 *     backward with its batch statistics (mean, rstd); dgamma / dbeta (each may be null) = sum gz*xhat, sum gz.  gamma null: only the
 *     activation (and the affine part, if scale is given, is treated as constant -- the D's first LeakyReLU passes null).
 *     work: ngan_bn_act_bwd_workspace_floats(npix, C) floats.
 * ngan_bn_act_apply: out = act(scale*y + shift) (the critic head's input).  ngan_chan_sum: out[c] = sum over pixels (bias gradients).
 * ngan_tanh_bwd: out = g * (1 - t*t).
 * ngan_wgan_stem_fwd: Linear(K -> C*S) with bias, output permuted from NCHW to NHWC: y[b][p][c] = bias[c*S+p] + sum_k z[b][k]*W[c*S+p][k]
 * ngan_wgan_stem_grad: gW[c*S+p][k] = sum_b g[b][p][c]*z[b][k], gb[c*S+p] = sum_b g[b][p][c] (either may be null).
 * Every reduction is two-stage in a fixed order (no float atomics): results are bit-reproducible. */
long ngan_s2_packed_floats(int M, int C);
int ngan_s2_pack(const float* W, float* Wp, int M, int C, int up, void* stream);
int ngan_s2_conv(const float* x, const float* Wp, const float* bias, const float* in_scale, const float* in_shift, int in_act, float slope,
                 float* y, int B, int Hin, int Win, int C, int M, int up, int tanh_out, void* stream);
long ngan_s2_wgrad_workspace_floats(int B, int Hh, int Wh, int CH, int CF);
int ngan_s2_wgrad(const float* half, const float* full, const float* h_scale, const float* h_shift, int h_act, const float* f_scale,
                  const float* f_shift, int f_act, float slope, float* dW, float* work, int B, int Hh, int Wh, int CH, int CF, void* stream);
long ngan_chan_reduce_workspace_floats(long npix, int C);
long ngan_bn_act_bwd_workspace_floats(long npix, int C);
int ngan_bn_stats(const float* y, long npix, int C, const float* gamma, const float* beta, float* mean, float* rstd, float* scale,
                  float* shift, float* run_mean, float* run_var, long long* nbt, float momentum, float eps, float* work, void* stream);
int ngan_bn_fold_eval(const float* gamma, const float* beta, const float* run_mean, const float* run_var, float eps, float* scale,
                      float* shift, int C, void* stream);
int ngan_bn_act_bwd(const float* y, const float* g, const float* scale, const float* shift, const float* mean, const float* rstd,
                    const float* gamma, int act, float slope, long npix, int C, float* gy, float* dgamma, float* dbeta, float* work,
                    void* stream);
int ngan_bn_act_apply(const float* y, const float* scale, const float* shift, int act, float slope, long npix, int C, float* out,
                      void* stream);
int ngan_chan_sum(const float* g, long npix, int C, float* out, float* work, void* stream);
int ngan_tanh_bwd(const float* t, const float* g, float* out, long n, void* stream);
int ngan_wgan_stem_fwd(const float* z, const float* W, const float* bias, float* y, int B, int K, int S, int C, void* stream);
int ngan_wgan_stem_grad(const float* z, const float* g, float* gW, float* gb, int B, int K, int S, int C, void* stream);

/* ---- synchronised BatchNorm2d for the data-parallel WGAN trainer (WGANTrainer(sync_batchnorm=True)) ----------------------------------
 * Each rank reduces its own pixels into an fp64 record, the caller all-gathers the records (rank order 0 .. world-1 in `recs`), and
 * every rank merges the same bytes in the same order: bit-identical statistics on every rank.  The single-GPU entry points above are
 * unchanged; no float atomics here either.
 * ngan_bn_moments: rec (1 + 2C doubles) = [count, mean[C], M2[C]] of y (npix, C), M2 = sum (y - mean)^2.  All of it is fp64
 *     arithmetic on the fp32 pixels: s0 = sum d and s1 = sum d^2 of d = y - y[0, c] (the channel's first pixel), every addition in
 *     fp64 from the first on, then mean = y[0, c] + s0/n and M2 = s1 - s0*s0/n.  That difference cancels by 1 + 2 (s0/n)^2 / var,
 *     which costs fp64 sums nothing an fp32 result can show, wherever the first pixel lies (fp32 sums per chunk lost tens of fp32
 *     roundings of rstd to a first pixel six sigma out).  work: ngan_chan_reduce_workspace_floats(npix, C) floats, 8-byte aligned
 *     (2 np C doubles of chunk partials).
 * ngan_bn_merge_fold: merges world records (world x (1 + 2C) doubles) in rank order, pairwise (Chan et al.): n = na + nb,
 *     d = mean_b - mean_a, mean = mean_a + d*nb/n, M2 = M2_a + M2_b + d^2*na*nb/n.  Then writes what ngan_bn_stats writes from the
 *     global N and M2: mean, rstd = 1/sqrt(M2/N + eps), scale, shift, running statistics (variance M2/(N-1)), *nbt += 1 -- and
 *     n_total[0] = N (one double on the device, for the backward).
 * ngan_bn_act_bwd_partial: rec (2C doubles) = [S0[C], S1[C]] = sum gz, sum gz*xhat over this rank's pixels, gz = g * act'(scale*y +
 *     shift), xhat = (y - mean)*rstd with the merged statistics.  work: ngan_chan_reduce_workspace_floats(npix, C) floats.
 * ngan_bn_act_bwd_merged: sums the world gathered backward records (world x 2C doubles) in rank order and writes
 *     gy = gamma*rstd*(gz - S0/N - xhat*S1/N), N = n_total[0]; dgamma / dbeta (each may be null) = S1 / S0 of record `rank` only --
 *     this rank's share, which the data-parallel gradient all-reduce adds up.  work: 3C floats. */
int ngan_bn_moments(const float* y, long npix, int C, double* rec, float* work, void* stream);
int ngan_bn_merge_fold(const double* recs, int world, int C, const float* gamma, const float* beta, float* mean, float* rstd, float* scale,
                       float* shift, float* run_mean, float* run_var, long long* nbt, float momentum, float eps, double* n_total, void* stream);
int ngan_bn_act_bwd_partial(const float* y, const float* g, const float* scale, const float* shift, const float* mean, const float* rstd,
                            int act, float slope, long npix, int C, double* rec, float* work, void* stream);
int ngan_bn_act_bwd_merged(const float* y, const float* g, const float* scale, const float* shift, const float* mean, const float* rstd,
                           const float* gamma, int act, float slope, long npix, int C, const double* recs, int world, int rank,
                           const double* n_total, float* gy, float* dgamma, float* dbeta, float* work, void* stream);

/* ---- sample quality: sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018, section 5; an addition of this
 * implementation, off by default; neuron-gan_amd/metrics.py drives it) -----------------------------------------------------------
 * Images are channels-last (B, H, W, C) fp32 with C = 1 or 3 (NGAN_ERR_SHAPE otherwise).  The Gaussian is separable, [1 4 6 4 1] / 16
 * per axis, with the MIRROR boundary `d c b | a b c d | c b a` (the edge sample is not repeated: scipy's mode='mirror', torch's
 * 'reflect').  fp32 arithmetic with explicit fused multiply-adds in a fixed order; every sum over many values is fp64 in two fixed
 * stages through a caller workspace (no floating-point atomics): all results are bit-reproducible.
 * pyr_down:    out (B, H/2, W/2, C) = the filtered input at its even rows and columns.  H, W even, at least 4.
 * laplacian:   lap = fine - up(coarse); fine, lap (B, H, W, C), coarse (B, H/2, W/2, C); up = zeros inserted at the odd positions,
 *              filtered with 4 x the same Gaussian, mirror boundary on the fine grid.  H, W even, at least 4.
 * descriptors: n patches (image, top row, left column) as int32 triples, given twice: `pos_host` in host memory, checked here
 *              (0 <= image < B, 0 <= row <= H - 7, 0 <= column <= W - 7, NGAN_ERR_ARG otherwise), and `pos`, the same triples in
 *              device memory, which the kernel reads.  Row row_offset + i of desc (any number of rows x 49 C) receives the 7 x 7 x C
 *              neighbourhood of patch i at column c * 49 + dy * 7 + dx.  sums (2 C doubles) = [sum d per channel, sum d^2 per
 *              channel] over the n * 49 values of each channel; accumulate != 0 adds to what sums holds, so one descriptor matrix
 *              and one pair of sums grow minibatch by minibatch.  workspace: the bytes the _workspace_bytes function names.
 * project:     proj[j][i] = sum_k ((desc[i][k] - mean_c(k)) / std_c(k)) * dirs[k][j], i < n; +inf for n <= i < n_pad.  desc (n, 49 C),
 *              dirs (49 C, n_dirs), proj (n_dirs, n_pad): one contiguous column per direction.  mean = S1 / (49 n) and the population
 *              standard deviation come from sums in fp64; (desc - mean) / std is formed in fp64 and rounded once, the sum runs over
 *              k = 0, 1, ... with one fmaf each.  n_pad: a power of two >= n (NGAN_ERR_SHAPE otherwise).
 * sort_columns: every one of the n_dirs columns of length n_pad (a power of two) ascending, in place: a bitonic network; the stages
 *              whose stride fits a block of sort_block_elements values run in LDS, larger strides as passes over global memory.
 * l1:          out[0] (one double) = (1 / (n n_dirs)) sum_j sum_{i < n} |a[j][i] - b[j][i]|; a, b (n_dirs, n_pad). */
int ngan_swd_pyr_down(const float* in, float* out, int B, int H, int W, int C, void* stream);
int ngan_swd_laplacian(const float* fine, const float* coarse, float* lap, int B, int H, int W, int C, void* stream);
size_t ngan_swd_descriptors_workspace_bytes(int n, int C);
int ngan_swd_descriptors(const float* images, const int* pos_host, const int* pos, float* desc, double* sums, void* workspace, int n,
                         long row_offset, int accumulate, int B, int H, int W, int C, void* stream);
int ngan_swd_project(const float* desc, const double* sums, const float* dirs, float* proj, int n, int n_pad, int n_dirs, int C,
                     void* stream);
int ngan_swd_sort_block_elements(void);
int ngan_swd_sort_columns(float* cols, int n_dirs, int n_pad, void* stream);
size_t ngan_swd_l1_workspace_bytes(int n, int n_dirs);
int ngan_swd_l1(const float* a, const float* b, double* out, void* workspace, int n, int n_pad, int n_dirs, void* stream);

/* ---- sample diversity: multi-scale structural similarity between pairs of images (Wang, Simoncelli and Bovik 2003, as reported by
 * Odena et al. 2017 and Karras et al. 2018; an addition of this implementation, off by default; neuron-gan_amd/metrics.py drives it) --
 * Images are channels-last (P, H, H, C) fp32, H a power of two, C = 1 or 3 (NGAN_ERR_SHAPE otherwise); pair p is (a[p], b[p]).
 * window:  the 11 taps of the separable Gaussian, sigma = 1.5: g[i] = exp(-(i - 5)^2 / 4.5), normalised to sum 1 in double and then
 *          rounded to float, written to host memory.  The scale kernel filters with exactly these values.
 * scale:   out[p] = {mean cs, mean ssim} (two doubles per pair) of one scale, the means over the (H - 10)^2 C entries of the "valid"
 *          filtering (no padding), H >= 16.  With the Gaussian-weighted moments mu_a, mu_b, E[a a], E[b b], E[a b] of a window,
 *          var_a = E[a a] - mu_a^2, cov = E[a b] - mu_a mu_b, C1 = (0.01 data_range)^2 and C2 = (0.03 data_range)^2:
 *              cs = (2 cov + C2) / (var_a + var_b + C2),   l = (2 mu_a mu_b + C1) / (mu_a^2 + mu_b^2 + C1),   ssim = l cs
 *          in fp32: each 11-tap sum is acc = fmaf(g[k], x[k], acc) for k = 0 .. 10 from acc = 0, rows first, then columns, the
 *          products a a, b b, a b rounded before the row pass; var and cov are one fmaf each (the difference is rounded once).  The
 *          per-pixel values are summed in fp64 in a fixed order through `workspace` (the bytes ngan_msssim_workspace_bytes names; no
 *          floating-point atomics): the result is bit-reproducible and a pair's value does not depend on the rest of the batch.
 *          P < 65536 pairs per call.
 * pool2:   the next scale: a_out, b_out (P, H/2, H/2, C) = the 2 x 2 averages of a, b, summed in double and rounded once. */
int ngan_msssim_window(float* window11);
size_t ngan_msssim_workspace_bytes(int P, int H);
int ngan_msssim_scale(const float* a, const float* b, double* out, void* workspace, int P, int H, int C, double data_range, void* stream);
int ngan_msssim_pool2(const float* a, const float* b, float* a_out, float* b_out, int P, int H, int C, void* stream);

/* ---- differentiable augmentation of the critic's inputs (Zhao et al. 2020; an addition of this implementation, off by default;
 * ops.DiffAugment and PGGANTrainer(diffaug=...) drive it) -----------------------------------------------------
 * Images here are contiguous fp32 (B, C, R, R) -- the reference's own layout, the same bytes as channels-last for C = 1 -- with
 * square images, R a multiple of 4 (NGAN_ERR_SHAPE otherwise), starting on a 16-byte boundary.  N = C R R.  Images and their
 * gradients are fp32 in every arithmetic mode.  Sample n has one parameter row of 32 bytes in `table`,
 *     struct { float b, c; int tx, ty, i0, i1, j0, j1; }
 * and `table_rows`, the rows the table holds, must be at least B (NGAN_ERR_ARG otherwise).
 * fwd:     m_n = (sum x[n]) / N                       (fp64 sum, fixed order)
 *          k_n = fp32(c b + (1 - c)(m_n + b))         (brightness x + b, then contrast c about the new mean; formed in double)
 *          u   = fmaf(c, x, k_n)
 *          y[n, ch, i, j] = u[n, ch, i + tx, j + ty]  if (i + tx, j + ty) lies inside the image and (i, j) outside [i0, i1) x [j0, j1),
 *                           `fill` otherwise (a finite constant: 0 is DiffAugment's own; its derivative is 0, so bwd does not take it)
 * bwd:     gu[q] = gy[q - t] where q - t lies inside the image and outside the cutout, else 0
 *          r_n = fp32((1 - c) / N * sum_q gu[q])      (fp64, fixed order: a masked sum of gy)
 *          gx  = fmaf(c, gu, r_n)
 *          The identity row {0, 1, 0, 0, 0, 0, 0, 0} reproduces x and gy bit for bit, whatever fill is.
 * colour:  0 -- the caller states that every row has b = 0, c = 1: the two columns are not read, the sum pass is not launched (one
 *          launch instead of two) and workspace may be NULL; otherwise workspace holds ngan_diffaug_workspace_bytes(B, C, R) bytes.
 *          y / gx may be a row range of a larger batch buffer (the pointer of its first row).  No atomics: bit-reproducible.
 * params:  uniforms (B, 8) in [0, 1) -> rows 0 .. B-1 of table, for R x R images.  policy: bits 1 colour, 2 translation, 4 cutout;
 *          a group outside the policy, or whose gate is closed, gets its identity values.  With S = int(R 0.125 + 0.5),
 *          K = int(R 0.5 + 0.5) and draw(u, n) = min(n - 1, floor(u n)) in fp32:
 *              colour       open if u0 < p:  b = u1 - 0.5, c = u2 + 0.5
 *              translation  open if u3 < p:  d = draw(u4, (2S + 1)^2), tx = d / (2S + 1) - S, ty = d % (2S + 1) - S
 *              cutout       open if u5 < p:  oi = draw(u6, R + 1 - K % 2), oj = draw(u7, R + 1 - K % 2),
 *                                            [i0, i1) = [oi - K/2, oi - K/2 + K) cut to [0, R), [j0, j1) likewise from oj
 *          (saturation, DiffAugment's third colour operation, is left out: the data are greyscale) */
size_t ngan_diffaug_workspace_bytes(int B, int C, int R);
int ngan_diffaug_params(const float* uniforms, void* table, int B, int H, int W, int table_rows, int policy, float p, void* stream);
int ngan_diffaug_fwd(const float* x, const void* table, float* y, void* workspace, int B, int C, int H, int W, int table_rows,
                     int colour, float fill, void* stream);
int ngan_diffaug_bwd(const float* gy, const void* table, float* gx, void* workspace, int B, int C, int H, int W, int table_rows,
                     int colour, void* stream);

/* ---- spectral fidelity: the radial power spectrum of images (Durall et al. 2020; an addition of this implementation, off by default;
 * neuron-gan_amd/metrics.py drives it) -- a batched 2-D real transform in LDS, no vendor FFT library ------------
 * Images are channels-last (B, R, R, C) fp32, R a power of two in 16 .. 1024, C = 1 or 3, 1 <= B <= 65535 (NGAN_ERR_SHAPE otherwise).
 * window:       the R taps of the periodic Hann window, h[i] = 0.5 - 0.5 cos(2 pi i / R) in double, rounded to float, to host memory.
 * ring_counts:  n_0 .. n_{R/2} to host memory: the number of signed frequencies (u, v) in [-R/2, R/2)^2 whose d = u^2 + v^2 lies in
 *               ring k, the integer with (2k-1)^2 <= 4d < (2k+1)^2 (k = 0 for d = 0), i.e. floor(sqrt(d) + 1/2) decided in integers.
 * radial:       per image and channel F = the 2-D DFT of x w, with w[y][x] = h[y] h[x] one fp32 product on load and x w one more
 *               (window = 0: w = 1, no product); P = |F|^2 / norm in fp32 (two products and one addition, no contraction), norm =
 *               (sum h^2)^2 of the taps in double (R^2 without the window);
 *                   radial[b][k] = sum over channels and the frequencies of ring k of P / (C n_k),   k = 0 .. R/2 (corners dropped)
 *               (B, R/2 + 1) doubles, summed in fp64 in a fixed order through `workspace` (ngan_spectrum_workspace_bytes names its
 *               size; it also holds the row pass's half spectrum): no atomics, bit-reproducible, and an image's values do not depend
 *               on the rest of the batch.  power_or_null: when given, P of the half plane, (B, C, R, R/2 + 1) fp32, the x frequency
 *               0 .. R/2 last, the y frequency in DFT order; `radial` is the same bits with and without it.  images, power and
 *               workspace start on a 16-byte boundary, radial on an 8-byte one (NGAN_ERR_ARG otherwise, as for a null pointer). */
int ngan_spectrum_window(float* taps, int R);
int ngan_spectrum_ring_counts(int* counts, int R);
size_t ngan_spectrum_workspace_bytes(int B, int R, int C);
int ngan_spectrum_radial(const float* images, double* radial, float* power_or_null, void* workspace, int B, int R, int C, int window,
                         void* stream);

/* ---- arbor morphology: connectivity and box counts of the thresholded image (an addition of this implementation, off by default;
 * neuron-gan_amd/metrics.py drives it) ------------------------------------------------------------------------------
 * Images are channels-last (B, R, R, C) fp32, R a power of two in 16 .. 1024, C = 1 or 3, 1 <= B <= 65535 (NGAN_ERR_SHAPE otherwise).
 * Every result is an integer, the only atomics are integer ones: every output is bit-reproducible, and an image's values do not
 * depend on the rest of the batch.  Pointers to images, levels, mask, labels, kept and workspace start on a 16-byte boundary, the
 * others on a 4-byte one (NGAN_ERR_ARG otherwise, as for a null pointer); a refused call writes nothing.
 * levels:    levels (B, R, R) bytes: (int) min(max(fmaf(g, 127.5f, 128.0f), 0), 255), truncated -- the 8-bit level of [-1, 1] rounded
 *            to nearest; g is the pixel for C = 1 and (x0 + x1 + x2) * (1.0f / 3.0f), summed left to right in fp32, for C = 3.
 *            hist (B, 256) counts of those levels, overwritten: what ngan_multiotsu4_noise_stats takes.
 * mask:      mask (B, R, R) bytes 0 / 1: level > cut[b]; cut (B) int32 on the device (255: an empty mask).
 * label:     8-connected components.  labels (B, R, R) int32: -1 on background, otherwise the smallest linear index row * R + col of
 *            the pixel's component.  stats (B, 4) int32 { area: foreground pixels, components: those of at least min_size pixels
 *            (min_size >= 1), largest: pixels of the largest component, kept_area: pixels in the counted components }.
 *            kept_or_null (B, R, R) bytes: the mask restricted to the counted components; labels and stats are the same bits with
 *            and without it.  workspace: ngan_morph_workspace_bytes(B, R) bytes (0 for an unsupported shape).
 * boxcount:  counts (B, log2 R + 1) int32, overwritten: counts[b][k] = aligned 2^k x 2^k boxes holding a foreground (non-zero) pixel;
 *            counts[b][0] is the area, counts[b][log2 R] is 0 or 1. */
size_t ngan_morph_workspace_bytes(int B, int R);
int ngan_morph_levels(const float* images, unsigned char* levels, unsigned int* hist, int B, int R, int C, void* stream);
int ngan_morph_mask(const unsigned char* levels, const int* cut, unsigned char* mask, int B, int R, void* stream);
int ngan_morph_label(const unsigned char* mask, int* labels, int* stats, unsigned char* kept_or_null, void* workspace, int B, int R,
                     int min_size, void* stream);
int ngan_morph_boxcount(const unsigned char* mask, int* counts, int B, int R, void* stream);

/* ---- arbor skeleton: thinning, tips, junctions and length of a mask (an addition of this implementation, off by default;
 * neuron-gan_amd/metrics.py drives it) ------------------------------------------------------------------------------
 * Masks are (B, R, R) bytes, any non-zero byte is foreground; R a power of two in 16 .. 512 (the bit rows of an image, 32 KiB at 512,
 * stay in one workgroup's LDS; 1024 is refused), 1 <= B <= 65535 (NGAN_ERR_SHAPE otherwise).  One workgroup per image, integers only,
 * no atomics: every output is bit-reproducible, and an image's values do not depend on the rest of the batch.  mask and skeleton start
 * on a 16-byte boundary, stats on a 4-byte one (NGAN_ERR_ARG otherwise, as for a null mask or stats); a refused call writes nothing.
 * Pixels outside the image are background.  The neighbours of a pixel P are named clockwise from north: P2 N (y-1, x), P3 NE, P4 E,
 * P5 SE, P6 S, P7 SW, P8 W, P9 NW.
 * thinning:  Guo and Hall 1989, algorithm A1.  With
 *                C  = [!P2 & (P3|P4)] + [!P4 & (P5|P6)] + [!P6 & (P7|P8)] + [!P8 & (P9|P2)]
 *                N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8),  N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9),  N = min(N1, N2)
 *            a foreground pixel is deleted in a sub-iteration when C == 1, 2 <= N <= 3 and, in sub-iteration 0, (P2|P3|!P5) & P4 == 0,
 *            in sub-iteration 1, (P6|P7|!P9) & P8 == 0; every deletion of a sub-iteration is decided on the state before it.
 *            Sub-iterations 0 and 1 alternate; the loop stops after the first pair in which neither deleted a pixel.  `passes` counts
 *            the sub-iterations run, that last pair included: it is even, and 2 for an already thin mask.
 * counts:    on any mask, with B the number of set neighbours and X the number of 0 -> 1 steps round the ring P2, P3, ..., P9, P2:
 *            pixels (set pixels), tips (X == 1 and B <= 2), junctions (X >= 3), isolated (B == 0), orth (pairs of set pixels that are
 *            horizontal or vertical neighbours), diag (pairs of set diagonal neighbours for which neither of the two pixels 4-adjacent
 *            to both is set: a staircase corner is not counted twice).  The length of a skeleton is orth + sqrt(2) diag pixels.
 * skel_thin:   skeleton_or_null (B, R, R) bytes 0 / 1; stats (B, 8) int32, overwritten: { pixels, tips, junctions, isolated, orth,
 *              diag: of the skeleton; passes; area: the mask's foreground pixels }; the same stats with and without the skeleton.
 * skel_counts: the six counts of the mask as it is; passes is 0 and area equals pixels. */
int ngan_skel_thin(const unsigned char* mask, unsigned char* skeleton_or_null, int* stats, int B, int R, void* stream);
int ngan_skel_counts(const unsigned char* mask, int* stats, int B, int R, void* stream);

/* ---- arbor geometry: distance transform, soma and Sholl crossings of a mask (an addition of this implementation, off by default;
 * neuron-gan_amd/metrics.py drives it) ------------------------------------------------------------------------------
 * Masks are (B, R, R) bytes, any non-zero byte is foreground, pixels outside the image are background; R a power of two in 16 .. 1024
 * (no image has to fit one workgroup's LDS, so there is no 512 limit), 1 <= B <= 65535 (NGAN_ERR_SHAPE otherwise).  Integers and integer
 * atomics only, but for `roots`, which is summed in fp64 in a fixed order: every output is bit-reproducible, an image's values do not
 * depend on the rest of the batch, and no workgroup waits on another.  mask, skeleton, dist2 and workspace start on a 16-byte boundary,
 * roots on an 8-byte one, soma, centre and crossings on a 4-byte one (NGAN_ERR_ARG otherwise, as for a null pointer); a refused call
 * writes nothing.
 * edt:    dist2 (B, R, R) int32, overwritten: 0 on the background; on a foreground pixel p the smallest (py-qy)^2 + (px-qx)^2 over all
 *         background pixels q, those of the one-pixel ring outside the image (rows and columns -1 and R) included -- the exact squared
 *         Euclidean distance.  soma (B, 3) int32, overwritten: {y, x, dist2} of the pixel with the largest dist2, among equals the one
 *         with the smallest linear index y * R + x; {-1, -1, 0} for an empty mask.  workspace: ngan_geom_workspace_bytes(B, R) bytes
 *         (0 for an unsupported shape).
 * sholl:  skeleton (B, R, R) bytes, any mask; dist2 as edt writes it; centre (B, 3) int32 of which {y, x} are read (the layout of
 *         soma).  With the ring step s = max(2, R / 64), the ring index k(p) of a pixel is the largest integer k with
 *         (k s)^2 <= (py-cy)^2 + (px-cx)^2, decided in integers.  The edges of the skeleton are those ngan_skel_counts counts (orth and
 *         diag).  crossings (B, 91) int32, overwritten: for every edge (p, q) with k(p) != k(q), crossings[b][max(k(p), k(q))] += 1
 *         (s >= 2 > sqrt 2: the two differ by one; k <= 90 for every centre inside the image; bin 0 stays 0).  roots (B) fp64,
 *         overwritten: the sum over the set skeleton pixels of sqrt((double) dist2[p]), per-thread partial sums added by a fixed tree.
 *         An image whose centre lies outside the image (y < 0: the soma of an empty mask) gets all-zero crossings and roots 0. */
size_t ngan_geom_workspace_bytes(int B, int R);
int ngan_geom_edt(const unsigned char* mask, int* dist2, int* soma, void* workspace, int B, int R, void* stream);
int ngan_geom_sholl(const unsigned char* skeleton, const int* dist2, const int* centre, int* crossings, double* roots, int B, int R,
                    void* stream);

/* ---- arbor branches: nodes, spur pruning and branch lengths of a skeleton (an addition of this implementation, off by default;
 * neuron-gan_amd/metrics.py drives it) ------------------------------------------------------------------------------
 * skeleton is (B, R, R) bytes, any mask: any non-zero byte is set, pixels outside the image are background, the linear index of a pixel
 * is y * R + x.  R a power of two in 16 .. 512 (the thinning's range), 1 <= B <= 65535 (NGAN_ERR_SHAPE otherwise); spur >= 1
 * (NGAN_ERR_ARG otherwise).  skeleton, labels and workspace must start on a 16-byte boundary, stats and hist on a 4-byte one; a null
 * (but for labels) or misaligned pointer is NGAN_ERR_ARG.  A refused call writes nothing.  Integers and integer atomics only: every
 * output is bit-reproducible and an image's values do not depend on the rest of the batch.
 * Graph: the vertices are the set pixels, the edges those ngan_skel_counts counts (orth: horizontal and vertical neighbours; diag:
 *         diagonal neighbours neither of whose two common 4-neighbours is set); deg(p) is the number of edges at p.  A node pixel has
 *         deg >= 3, a branch pixel deg <= 2.  An edge is a node edge (both ends node pixels), a branch edge (both branch pixels) or an
 *         attachment.  A node is a connected component of node pixels under node edges, a branch one of branch pixels under branch
 *         edges: a simple path or a cycle, an isolated pixel included.
 * Per branch: n pixels; a attachments at its pixels (0, 1 or 2); o and d its branch edges plus its attachments, orth and diag; the floor
 *         length L = o + isqrt(2 d d), an exact integer square root.  Class: free (a = 0), spur (a = 1 and n < spur), terminal (a = 1
 *         and n >= spur), link (a = 2).  spur = 1 prunes nothing.
 * Per node: strong, the number of attachments whose branch is no spur; a fork is a node with strong >= 3.  Pruning is one round.
 * labels (B, R, R) int32, optional (stats and hist are the same bits without): -1 on the background, on a branch pixel the smallest
 *         linear index of its branch, on a node pixel -2 - the smallest linear index of its node.
 * stats  (B, 20) int32, overwritten: {pixels, node_pixels, nodes, branches, terminal, links, free, spurs, term_orth, term_diag,
 *         link_orth, link_diag, free_orth, free_diag, spur_orth, spur_diag (the o and d sums of the branches of a class), node_orth,
 *         node_diag (the node edges), longest (the largest L over terminal, link and free branches, 0 without one), forks}.
 *         branches = terminal + links + free + spurs; the four *_orth plus node_orth are ngan_skel_counts' orth, and so for diag.
 * hist   (B, 64) int32, overwritten: every terminal and link branch adds one to bin min(63, L / max(1, R / 128)).
 * workspace: ngan_branch_workspace_bytes(B, R) bytes, 13 per pixel (0 for an unsupported shape). */
size_t ngan_branch_workspace_bytes(int B, int R);
int ngan_branch_graph(const unsigned char* skeleton, int* labels_or_null, int* stats, int* hist, void* workspace, int B, int R, int spur,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NGAN_H */
