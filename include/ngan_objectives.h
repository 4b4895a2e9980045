/* ngan_objectives.h -- extension section of ngan.h (which includes it: include ngan.h, not this file): the scalar heads of the
 * objectives a trainer can select besides the Wasserstein one.  Same conventions as ngan.h: status-returning, the trailing void* is the
 * hipStream_t, device pointers, no state between calls.  Python binding: _C.SIGNATURES. */
#ifndef NGAN_OBJECTIVES_H
#define NGAN_OBJECTIVES_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- scalar heads of the least-squares losses (Mao et al. 2017): loss_functions.py:77-143, which the reference ships and never calls ----
 * scores holds n_real real scores followed by n_fake fake scores.
 * loss = mean((real - t_real)^2) + mean((fake - t_fake)^2), plus the two plain score means (three separate 1-float
 * outputs);  n_fake = 0 gives mean((scores - t_real)^2), the generator form, with mean_fake = 0.  One workgroup, fixed summation order.
 * bwd: g_scores[i] = (g_loss * 2 (s_i - t) + g_mean) / n of its half, from the three output gradients (device scalars, NULL = 0).
 * NGAN_ERR_ARG for a null pointer, n_real <= 0 or n_fake < 0.  The scores are fp32 in every conv precision. */
int ngan_lsloss_head(const float* scores, int n_real, int n_fake, float t_real, float t_fake, float* loss, float* mean_real,
                     float* mean_fake, void* stream);
int ngan_lsloss_head_bwd(const float* scores, int n_real, int n_fake, float t_real, float t_fake, const float* g_loss,
                         const float* g_real, const float* g_fake, float* g_scores, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NGAN_OBJECTIVES_H */
