/* nganx.h -- extension entry points of libngan_hip.so.  ngan.h does NOT include this file: the core ABI (ngan.h and the sections it
 * includes) is frozen at the reference's surface plus the additions made so far, and everything added outside the reference from now
 * on is declared here under the prefix nganx_.  Same library, same conventions as ngan.h: status-returning (NGAN_OK or an NGAN_ERR_*
 * of ngan.h, the message in ngan_last_error), the trailing void* is the hipStream_t, device pointers, no state between calls, fixed
 * summation order, no atomics, and nothing is launched when a status other than NGAN_OK is returned.
 * Python binding: _C.EXT_SIGNATURES / _C.EXT_NON_STATUS; kernels: csrc/simloss.hip; per-pair arithmetic: csrc/simloss_bits.h.
 *
 * ---- pairwise similarity loss of the generator (ops.SimilarityLoss) ----
 * X is a batch flattened to (B, N) fp32 rows, Z the latents (B, latent_dim).  With m_i the mean of row i (centring on) or 0,
 *     G_ij = sum_p (x_i[p] - m_i)(x_j[p] - m_j),   S_ij = G_ij / sqrt(G_ii G_jj),   T_ij the same for Z (never centred),
 *     L = lambda / (B (B - 1)) * sum_{i != j} (T_ij - S_ij)^2
 * and, with A_ij = -2 lambda (T_ij - S_ij) / (B (B - 1)) (zero diagonal) and n_i = sqrt(G_ii),
 *     dL/dx_i = sum_j M_ij x_j - r_i,   M_ij = 2 A_ij / (n_i n_j) (j != i),   M_ii = -2 sum_j A_ij S_ij / n_i^2,   r_i = sum_j M_ij m_j.
 * There is no epsilon: a row whose (centred) squared norm is 0 gives NaN, as the reference's division does.
 * Domain: B = 2 .. 64; N a multiple of 4, 16 <= N < 2^31; row pointers on 16-byte boundaries.  NGAN_ERR_SHAPE for B or N outside it,
 * NGAN_ERR_ARG for a null or misaligned pointer; the message names the argument. */
#ifndef NGANX_H
#define NGANX_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of workspace of nganx_pair_gram; 0 for a shape it refuses */
size_t nganx_pair_gram_workspace_bytes(int B, long N);

/* gram[i][j] = sum_p x_i[p] x_j[p] (fp64, B x B, every element written, symmetric bit for bit) and sums[i] = sum_p x_i[p] (fp64, B)
 * from fp32 rows.  The products are exact in fp64; they are added in fp64 in an order that depends on (B, N) alone.  Two launches:
 * slab partials into the workspace, one reduce.  Serves the images (N = C R R) and the latents (N = latent_dim) alike; centring is
 * applied by the head from the sums.  rows and workspace on 16-byte boundaries, gram and sums on 8-byte ones. */
int nganx_pair_gram(const float* rows, double* gram, double* sums, void* workspace, int B, long N, void* stream);

/* From the two Gram matrices (and the images' row sums, read when center != 0):  loss[0] = L (fp32, rounded once from fp64);
 * sim[i][j] = S_ij (fp64, B x B; the diagonal holds G_ii / sqrt(G_ii G_ii));  mix[i][j] = M_ij (fp32, B x B) and shift[i] = r_i
 * (fp32, B), each formed in fp64 and rounded once.  lambda is a DEVICE fp32 scalar: it decays per epoch and a captured graph reads
 * it live.  N is the images' row length.  One launch of one workgroup. */
int nganx_simloss_head(const double* gram_x, const double* sums_x, const double* gram_z, const float* lambda, int B, long N, int center,
                       float* loss, double* sim, float* mix, float* shift, void* stream);

/* grad[i][p] = (addend[i][p], if given) + upstream[0] * (sum_j mix[i][j] rows[j][p] - shift[i]): fp32 FMAs in the order j = 0 .. B-1,
 * then the subtraction, the product and the addition, one rounding each.  upstream is a DEVICE scalar; addend_or_null may be grad
 * itself.  One launch.  rows, addend and grad on 16-byte boundaries. */
int nganx_pair_mix(const float* rows, const float* mix, const float* shift, const float* upstream, const float* addend_or_null,
                   float* grad, int B, long N, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NGANX_H */
