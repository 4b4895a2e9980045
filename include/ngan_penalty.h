/* ngan_penalty.h -- extension section of ngan.h (which includes it: include ngan.h, not this file): the selectable forms of the
 * gradient penalty beside the reference's two-sided one.  Same conventions as ngan.h: status-returning, the trailing void* is the
 * hipStream_t, device pointers, no state between calls.  Python binding: _C.SIGNATURES.
 *
 * form 1, one-sided (WGAN-LP, Petzka et al. 2018):   phi(n) = max(0, n - 1)^2
 * form 2, zero-centred (R1, Mescheder et al. 2018):  phi(n) = n^2 / 2
 * The two-sided form (n - 1)^2 of the reference stays on the sample_l2norm / gp_head / gp_coef / scale_rows chain of ngan.h.
 * g is the critic's input gradient, B rows of n fp32 elements; rows must start on 16-byte boundaries for the head (g aligned and
 * n % 4 == 0, or B == 1), as for the l2-norm entry point of ngan.h: NGAN_ERR_SHAPE otherwise.  NGAN_ERR_ARG for a null pointer, B <= 0,
 * n <= 0 or an unknown form.  Nothing is launched when a status other than NGAN_OK is returned.  Fixed summation order, no atomics. */
#ifndef NGAN_PENALTY_H
#define NGAN_PENALTY_H

#ifdef __cplusplus
extern "C" {
#endif

/* norms[b] = ||g[b,:]||_2;  out1 = lambda * mean_b phi(norms[b]).  workspace: 64 * B floats.  Two launches. */
int ngan_penalty_head(const float* g, int B, long n, int form, float lambda, float* workspace, float* norms, float* out1, void* stream);

/* out[b,:] = c_b * g[b,:], the gradient of out1 w.r.t. g times the device scalar g_out:
 *   form 1:  c_b = g_out * 2 lambda (n_b - 1) / (B n_b) where n_b > 1; elsewhere the row is +0.0 whatever g holds
 *   form 2:  c_b = g_out * lambda / B  (no division by a norm)
 * with n_b = norms[b] as the head wrote it.  One launch; 16-byte accesses where g and out are 16-byte aligned and n % 4 == 0 (or B == 1),
 * 4-byte ones elsewhere. */
int ngan_penalty_bwd(const float* g, const float* norms, int B, long n, int form, float lambda, const float* g_out, float* out,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NGAN_PENALTY_H */
