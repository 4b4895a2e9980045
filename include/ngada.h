/* ngada.h -- adaptive discriminator augmentation (Karras et al. 2020, "Training generative adversarial networks with limited data",
 * section 3): entry points of libngan_hip.so under the prefix ngada_.  Neither ngan.h nor nganx.h includes this file: the core ABI and
 * the first extension header are both frozen.  Same library, same conventions as nganx.h: status-returning (NGAN_OK or an NGAN_ERR_*
 * of ngan.h, the message in ngan_last_error), the trailing void* is the hipStream_t, device pointers, no state inside the library,
 * fixed summation order, no atomics, and nothing is launched when a status other than NGAN_OK is returned.
 * Python binding: _C.ADA_SIGNATURES (every entry point returns a status); kernels: csrc/ada.hip (and the live parameter mappings beside the ones they mirror, in
 * csrc/diffaug.hip and csrc/diffgeo.hip); per-element arithmetic: csrc/ada_bits.h; DESIGN.md section 7 has the definition.
 *
 * Device state, owned by the caller and never reallocated (captured graphs hold the addresses):
 *     counters  int64[4] = {pos, neg, n, updates}        p  fp32[2] = {p, last_r}
 * pos / neg count the real scores above / below the threshold since the last update, n the real scores seen, updates the updates
 * made; p[0] is the augmentation probability every gate of the live parameter mappings compares against, p[1] the statistic
 * r = (pos - neg) / n the last update saw. */
#ifndef NGADA_H
#define NGADA_H

#ifdef __cplusplus
extern "C" {
#endif

/* Count the real scores on either side of a threshold t, over real_scores[0 .. n_real) only:
 *     pos += #{i : s_i > t},   neg += #{i : s_i < t},   n += n_real
 * mode 0: t = threshold (0.5 serves the least-squares objective, whose real target is 1 and fake target 0; 0 is Karras's choice);
 *         fake_scores_or_null and n_fake are not read.
 * mode 1: t = 0.5 (sum(real) / n_real + sum(fake) / n_fake), the midpoint of the two batch means: both sums in fp64 in an order that
 *         depends on the counts alone, the midpoint kept in fp64, the scores compared with it as doubles.  threshold is not read.
 * A NaN score, or a NaN t, compares neither way and counts in n alone.  The counts are integers added to what the counters hold:
 * bit-reproducible.  One launch of one workgroup.  Domain: 1 <= n_real <= 65536, and in mode 1 the same for n_fake (NGAN_ERR_SHAPE
 * outside it).  NGAN_ERR_ARG for a null real_scores or counters, a null fake_scores_or_null in mode 1, a mode outside {0, 1}, and
 * counters off an 8-byte boundary. */
int ngada_accumulate(const float* real_scores, const float* fake_scores_or_null, int n_real, int n_fake, int mode, float threshold,
                     long* counters, void* stream);

/* One step of the controller, one thread.  With d = (double)(pos - neg) - (double)target * (double)n and s = sign(d) (0 for d = 0, a
 * NaN d, or n = 0):
 *     p[0] = (float) min((double)p_max, max(0.0, (double)p[0] + s * (double)n / span))      (a NaN p[0] becomes 0)
 *     p[1] = n ? (float)((double)(pos - neg) / (double)n) : p[1]
 *     pos = neg = n = 0;  updates += 1
 * span is the number of real scores over which p may travel from 0 to 1.  NGAN_ERR_ARG for a null pointer, counters off an 8-byte
 * boundary, a target outside [-1, 1], a span that is not a finite number > 0, or a p_max outside [0, 1]. */
int ngada_update(long* counters, float* p, float target, double span, float p_max, void* stream);

/* ngan_diffaug_params (ngan.h) and ngan_diffgeo_params (ngan_geoaug.h) with the probability read from device memory: p[0] is loaded
 * by every thread, the expressions are the same and every gate is u < p[0].  A NaN closes every gate (identity rows), a value above
 * 1 opens them all; there is no host-side range check, because the host does not know the value.  With the same value the tables
 * are the by-value entry points' bit for bit.  Every other argument, check and status as documented there; NGAN_ERR_ARG for a null
 * p. */
int ngada_diffaug_params(const float* uniforms, void* table, int B, int H, int W, int table_rows, int policy, const float* p,
                         void* stream);
int ngada_diffgeo_params(const float* uniforms, void* table, int B, int H, int W, int table_rows, int policy, const float* p,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NGADA_H */
