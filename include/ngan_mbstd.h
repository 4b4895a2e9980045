/* ngan_mbstd.h -- extension section of ngan.h (which includes it: include ngan.h, not this file): the minibatch standard-deviation
 * layer of the PG critic's head (Karras et al. 2018, section 3), closed under double-backward.  Same conventions as ngan.h:
 * status-returning, the trailing void* is the hipStream_t, device pointers, fp32 channels-last tensors, no state between calls.
 * Python binding: _C.SIGNATURES / _C.NON_STATUS.
 *
 * x is (B, H, W, C), C a multiple of 4, J = H W C.  The batch holds `segments` critic calls of B / segments samples each; inside a
 * segment, consecutive runs of G_eff samples form a group (G_eff divides B / segments, so no group spans two segments).  Per group g
 * and feature j:  mu_j = mean_n x[n, j],  sigma_j = sqrt(mean_n (x[n, j] - mu_j)^2 + 1e-8),  s_g = mean_j sigma_j.
 * Per feature the arithmetic is fp32 (csrc/mbstd_bits.h); every sum over j is taken in fp64 in a fixed order: two calls give the same
 * bits, and a group's results do not depend on the other groups.  No atomics, no waiting between workgroups.
 * Activation pointers (x, gx, h, dx, c, out, g) must start on a 16-byte boundary.  NGAN_ERR_ARG for a null or misaligned pointer,
 * NGAN_ERR_SHAPE for B outside 1 .. 65535, C not a positive multiple of 4, or a segment / group size that does not divide. */
#ifndef NGAN_MBSTD_H
#define NGAN_MBSTD_H

#ifdef __cplusplus
extern "C" {
#endif

/* doubles of workspace ngan_mbstd_fwd / ngan_mbstd_bwdbwd need: one partial sum per group and block of 1024 features; 0 for a bad shape */
long ngan_mbstd_workspace_doubles(int B, int H, int W, int C, int G_eff);

/* s[n] = s_g of n's group, n = 0 .. B-1 */
int ngan_mbstd_fwd(const float* x, float* s, double* workspace, int B, int H, int W, int C, int segments, int G_eff, void* stream);
/* gx[n, j] = gs_g d[n, j] / (G J sigma_j), gs_g the sum of gs over the group's samples, d = x - mu */
int ngan_mbstd_bwd(const float* gs, const float* x, float* gx, int B, int H, int W, int C, int segments, int G_eff, void* stream);
/* backward of ngan_mbstd_bwd, cotangent h on gx, one pass over x:  dgs[n] = sum_j hd_j / (G J sigma_j)  (the same for every sample
 * of a group),  dx[m, j] = gs_g / (G J) ((h[m, j] - hbar_j) / sigma_j - d[m, j] hd_j / (G sigma_j^3)),  hbar_j = mean_n h[n, j],
 * hd_j = sum_n h[n, j] d[n, j] */
int ngan_mbstd_bwdbwd(const float* h, const float* gs, const float* x, float* dgs, float* dx, double* workspace, int B, int H, int W,
                      int C, int segments, int G_eff, void* stream);

/* The statistic as one extra, constant input plane of a zero-padded 3x3 convolution with weights w_std (C, 1, 3, 3):
 *   out[n, y, x, co] = c[n, y, x, co] + scale s[n] T[y, x, co],   T = sum of the taps of w_std[co] whose source pixel is inside the image
 * (nine position classes, formed on the fly; H = W = 1 leaves the centre tap).  A bilinear triple, like ngan_final_dot_*:
 *   ds:  gs[n] = scale sum_{y, x, co} g[n, y, x, co] T[y, x, co]
 *   dw:  gw[co, 0, ky, kx] = scale sum_{n} s[n] sum_{(y, x) whose tap (ky, kx) is inside} g[n, y, x, co]
 * Products are rounded to fp32 and summed in fp64 in a fixed order.  out may be c; c may be NULL (the field alone, c = 0). */
int ngan_stdfield_add(const float* c, const float* s, const float* w_std, float* out, int B, int H, int W, int C, float scale, void* stream);
int ngan_stdfield_ds(const float* g, const float* w_std, float* gs, int B, int H, int W, int C, float scale, void* stream);
int ngan_stdfield_dw(const float* g, const float* s, float* gw, int B, int H, int W, int C, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NGAN_MBSTD_H */
