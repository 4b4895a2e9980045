// Adaptive discriminator augmentation (Karras et al. 2020, "Training generative adversarial networks with limited data", section 3; an
// addition of this implementation, off by default): how far the critic separates the reals, r = E[sign(D(real) - t)], is counted on
// the device and every few iterations the augmentation probability moves a fixed amount towards the value that holds r at a target.
// include/ngada.h and DESIGN.md section 7 hold the definition; the per-element arithmetic is csrc/ada_bits.h; tests/ada_cases.py
// restates both kernels.
//   ngada_accumulate  accumulate_kernel: one workgroup of 256 threads.  Mode 1 first sums both score vectors in fp64 -- thread k adds
//                     elements k, k + 256, ... in ascending order, then a butterfly inside each wave, then the four waves in order:
//                     an order that depends on the counts alone -- and forms the midpoint; every thread holds the same bits of it.
//                     Then each thread counts its real scores on either side, the integer counts are summed (exact in any order)
//                     and thread 0 adds them to the counters.
//   ngada_update      update_kernel: one thread applies ada::update and resets the counters.
// The live parameter mappings (ngada_diffaug_params, ngada_diffgeo_params) stand beside the kernels they mirror, in diffaug.hip and
// diffgeo.hip.  No atomics: one workgroup per call, and calls on one stream are ordered.
#include <cstdint>
#include "ngan_common.h"
#include "../../include/ngada.h"

#pragma clang fp contract(off)
#include "ada_bits.h"

namespace {

// sum over the workgroup's 256 threads in a fixed order: butterfly inside each wave, then the four waves in order; every thread gets it
__device__ __forceinline__ double block_sum256(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ int block_count256(int v, int* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

__device__ __forceinline__ double strided_sum(const float* __restrict__ x, int n) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += ada::THREADS) s += (double)x[i];
    return s;
}

__global__ __launch_bounds__(256) void accumulate_kernel(const float* __restrict__ real, const float* __restrict__ fake, int n_real,
                                                         int n_fake, int mode, float threshold, long* __restrict__ counters) {
    __shared__ double red_real[4], red_fake[4];
    __shared__ int red_pos[4], red_neg[4];
    double t = (double)threshold;
    if (mode == 1) {
        const double sr = block_sum256(strided_sum(real, n_real), red_real);
        const double sf = block_sum256(strided_sum(fake, n_fake), red_fake);
        t = ada::midpoint(sr, n_real, sf, n_fake);
    }
    int pos = 0, neg = 0;
    for (int i = threadIdx.x; i < n_real; i += ada::THREADS) {
        const int s = ada::side(real[i], t);
        pos += s > 0;
        neg += s < 0;
    }
    pos = block_count256(pos, red_pos);
    neg = block_count256(neg, red_neg);
    if (threadIdx.x == 0) {
        counters[0] += (long)pos;
        counters[1] += (long)neg;
        counters[2] += (long)n_real;
    }
}

__global__ void update_kernel(long* __restrict__ counters, float* __restrict__ p, float target, double span, float p_max) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const long pos = counters[0], neg = counters[1], n = counters[2];
    const ada::Step st = ada::update(pos, neg, n, p[0], p[1], target, span, p_max);
    p[0] = st.p;
    p[1] = st.r;
    counters[0] = 0;
    counters[1] = 0;
    counters[2] = 0;
    counters[3] += 1;
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

extern "C" int ngada_accumulate(const float* real_scores, const float* fake_scores_or_null, int n_real, int n_fake, int mode,
                                float threshold, long* counters, void* stream) {
    NGAN_REQUIRE(mode == 0 || mode == 1, NGAN_ERR_ARG, "ngada_accumulate: mode %d (0: the threshold argument, 1: the midpoint of the batch means)", mode);
    NGAN_REQUIRE(real_scores, NGAN_ERR_ARG, "ngada_accumulate: real_scores is a null pointer");
    NGAN_REQUIRE(counters, NGAN_ERR_ARG, "ngada_accumulate: counters is a null pointer");
    NGAN_REQUIRE(mode == 0 || fake_scores_or_null, NGAN_ERR_ARG, "ngada_accumulate: mode 1 needs fake_scores, got a null pointer");
    NGAN_REQUIRE(aligned8(counters), NGAN_ERR_ARG, "ngada_accumulate: counters must start on an 8-byte boundary");
    NGAN_REQUIRE(n_real >= ada::N_MIN && n_real <= ada::N_MAX, NGAN_ERR_SHAPE, "ngada_accumulate: n_real=%d unsupported (%d .. %d)", n_real,
                 ada::N_MIN, ada::N_MAX);
    NGAN_REQUIRE(mode == 0 || (n_fake >= ada::N_MIN && n_fake <= ada::N_MAX), NGAN_ERR_SHAPE, "ngada_accumulate: n_fake=%d unsupported (%d .. %d)",
                 n_fake, ada::N_MIN, ada::N_MAX);
    hipLaunchKernelGGL(accumulate_kernel, dim3(1), dim3(ada::THREADS), 0, (hipStream_t)stream, real_scores, fake_scores_or_null, n_real,
                       n_fake, mode, threshold, counters);
    return ngan::launch_status("ngada_accumulate");
}

extern "C" int ngada_update(long* counters, float* p, float target, double span, float p_max, void* stream) {
    NGAN_REQUIRE(counters, NGAN_ERR_ARG, "ngada_update: counters is a null pointer");
    NGAN_REQUIRE(p, NGAN_ERR_ARG, "ngada_update: p is a null pointer");
    NGAN_REQUIRE(aligned8(counters), NGAN_ERR_ARG, "ngada_update: counters must start on an 8-byte boundary");
    NGAN_REQUIRE(target >= -1.f && target <= 1.f, NGAN_ERR_ARG, "ngada_update: target=%g must lie in [-1, 1]", (double)target);
    NGAN_REQUIRE(span > 0.0 && span - span == 0.0, NGAN_ERR_ARG, "ngada_update: span=%g must be a finite number > 0", span);
    NGAN_REQUIRE(p_max >= 0.f && p_max <= 1.f, NGAN_ERR_ARG, "ngada_update: p_max=%g must lie in [0, 1]", (double)p_max);
    hipLaunchKernelGGL(update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counters, p, target, span, p_max);
    return ngan::launch_status("ngada_update");
}
