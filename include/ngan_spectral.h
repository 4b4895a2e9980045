/* ngan_spectral.h -- extension section of ngan.h (which includes it: include ngan.h, not this file): the spectral regularisation of
 * the generator (Durall et al. 2020), a loss on the radial power spectrum of ngan_spectrum_radial.  Same conventions as ngan.h:
 * status-returning, the trailing void* is the hipStream_t, device pointers, no state between calls, fixed summation order, no atomics.
 * Python binding: _C.SIGNATURES / _C.NON_STATUS; kernels: csrc/specloss.hip.
 *
 * Images are fp32 (B, 1, R, R) -- one colour channel, so planar and channels-last coincide -- R a power of two in 16 .. 1024,
 * B = 1 .. 65535, K = R/2 + 1.  With S the radial spectrum (window as ngan_spectrum_radial's), a target t[k], a floor d > 0:
 *     r = S / t,  q = ln((r + d) / (1 + d)),  l[b] = sum_{k=1..R/2} q[b][k]^2 / (R/2),  L = scale * sum_b l[b]
 * (scale = lambda / global batch), c[b][k] = dL/dS[b][k] = scale / (R/2) * 2 q / (t (r + d)); bin 0 and every bin with t[k] <= 0 take
 * weight 0.  The gradient is dL/dx = 2 w Re(sum_f a[f] F[f] exp(+2 pi i f.p / R)), a[f] = c[ring(f)] / (n_ring(f) norm), 0 for the
 * corner frequencies beyond R/2.
 * NGAN_ERR_SHAPE for an unsupported R, B or C (C = 3 is refused: the generator's image tensor is planar greyscale); NGAN_ERR_ARG for
 * a null pointer, a misaligned one or a floor that is not positive.  Nothing is launched when a status other than NGAN_OK is returned. */
#ifndef NGAN_SPECTRAL_H
#define NGAN_SPECTRAL_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of workspace of the forward and of the adjoint; 0 for a shape the entry points refuse */
size_t ngan_specloss_fwd_workspace_bytes(int B, int R, int C);
size_t ngan_specloss_bwd_workspace_bytes(int B, int R, int C);

/* radial[b][k] (fp64, B x K): the bits of ngan_spectrum_radial on the same images;  transform (fp32 complex, B x K x R): the
 * half-plane transform F[b][v][fy], v = 0 .. R/2 the x frequency, fy the y frequency in DFT order;  ring_norm[k] (fp64, K): n_k norm,
 * the divisor of bin k (the number of frequencies in ring k times sum w^2).  Three launches.
 * images, transform and workspace on 16-byte boundaries. */
int ngan_specloss_fwd(const float* images, double* radial, float* transform, double* ring_norm, void* workspace, int B, int R, int C,
                      int window, void* stream);

/* From the forward's radial and ring_norm:  per_image[b] = l[b] (fp64);  loss[0] = L (fp32, rounded once from fp64);
 * dradial[b][k] = c (fp32, rounded once);  coef[b][k] = c / ring_norm[k] (fp32, divided in fp64 from the unrounded c, rounded once):
 * the table ngan_specloss_bwd reads;  skipped[0] = the number of bins k >= 1 with target[k] <= 0.  One launch of one workgroup. */
int ngan_specloss_head(const double* radial, const double* target, const double* ring_norm, int B, int R, double scale, double floor,
                       double* per_image, float* loss, float* dradial, float* coef, int* skipped, void* stream);

/* grad[b][y][x] = (addend, if given) + upstream[0] * dL/dx from the transform the forward kept and the head's coef.  upstream is a
 * DEVICE scalar (the gradient arriving at L): nothing is read back, the call can be captured.  addend_or_null may be grad itself.
 * Two launches.  transform, addend, grad and workspace on 16-byte boundaries. */
int ngan_specloss_bwd(const float* transform, const float* coef, const float* upstream, const float* addend_or_null, float* grad,
                      void* workspace, int B, int R, int C, int window, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NGAN_SPECTRAL_H */
