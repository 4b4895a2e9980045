// Per-pair arithmetic of the pairwise similarity loss (include/nganx.h), shared by the head kernel of simloss.hip and by host code
// (tools/simloss_host_check.cpp compiles it under sanitizers).  Everything is fp64; every line is one operation per rounding, with
// contraction off, so the device, the host and the emulation of tests/simloss_cases.py form the same bits.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SIMLOSS_HD __host__ __device__ inline
#else
#define SIMLOSS_HD inline
#endif

namespace simloss {

constexpr int B_MIN = 2, B_MAX = 64;         // rows of a batch
constexpr long N_MIN = 16, N_LIMIT = 1L << 31;   // N a multiple of 4 in [N_MIN, N_LIMIT): what ngan_diffaug_* accept as a sample

inline bool shape_ok(int B, long N) { return B >= B_MIN && B <= B_MAX && N >= N_MIN && N < N_LIMIT && N % 4 == 0; }

// Slab plan of the Gram launch, a function of (B, N) alone: `lanes` rows-of-four per side (a power of two covering B), `groups` pixel
// groups of lanes^2 threads in a workgroup of 256, a tile of `tile` pixels, `chunk` pixels per slab (a multiple of the tile),
// `slabs` workgroups.  At most 1024 slabs; at least 256 pixels each.
struct GramPlan { int lanes, groups, tile; long chunk; int slabs; };
inline GramPlan gram_plan(int B, long N) {
    GramPlan p;
    p.lanes = 1;
    while (4 * p.lanes < B) p.lanes *= 2;
    p.groups = 256 / (p.lanes * p.lanes);
    p.tile = p.groups > 64 ? 256 : 64;
    long per = (N + 1023) / 1024;
    per = (per + p.tile - 1) / p.tile * p.tile;
    p.chunk = per < 256 ? 256 : per;
    p.slabs = (int)((N + p.chunk - 1) / p.chunk);
    return p;
}
SIMLOSS_HD long gram_elements(int B) { return (long)B * B + B; }        // one slab's partials: the matrix, then the row sums

// m_i: the mean of a row from its fp64 sum, or 0 without centring
SIMLOSS_HD double row_mean(double sum, long N, int center) { return center ? sum / (double)N : 0.0; }

// sum_p (x_i - m_i)(x_j - m_j) = G_ij - N m_i m_j: the product m_i m_j first (it commutes, so the centred matrix stays symmetric bit
// for bit), then times N, then the subtraction -- three roundings
SIMLOSS_HD double centred(double g, long N, double mi, double mj) {
#pragma clang fp contract(off)
    const double mm = mi * mj;
    const double nmm = (double)N * mm;
    return g - nmm;
}

// G_ij / sqrt(G_ii G_jj)
SIMLOSS_HD double cosine(double gij, double gii, double gjj) {
#pragma clang fp contract(off)
    const double q = gii * gjj;
    return gij / sqrt(q);
}

// lambda / (B (B - 1))
SIMLOSS_HD double pair_weight(double lambda, int B) { return lambda / ((double)B * (double)(B - 1)); }

// What pair (i, j) contributes: s = S_ij; d = T_ij - S_ij (exactly 0 on the diagonal); a = A_ij = -2 w d; m_off = 2 A_ij / (n_i n_j),
// the off-diagonal M; c = A_ij S_ij, whose row sum gives M_ii.
struct Pair { double s, d, a, m_off, c; };
SIMLOSS_HD Pair pair_terms(double gx_ij, double gx_ii, double gx_jj, double gz_ij, double gz_ii, double gz_jj, double w, bool diagonal) {
#pragma clang fp contract(off)
    Pair p;
    p.s = cosine(gx_ij, gx_ii, gx_jj);
    const double t = cosine(gz_ij, gz_ii, gz_jj);
    p.d = diagonal ? 0.0 : t - p.s;
    const double wd = w * p.d;
    p.a = -2.0 * wd;
    const double nn = sqrt(gx_ii) * sqrt(gx_jj);
    p.m_off = (2.0 * p.a) / nn;
    p.c = p.a * p.s;
    return p;
}

// M_ii = -2 (sum_j A_ij S_ij) / n_i^2, n_i^2 = G_ii
SIMLOSS_HD double mix_diagonal(double row_c, double gx_ii) { return (-2.0 * row_c) / gx_ii; }

}  // namespace simloss
