// The selectable forms of the gradient penalty (include/ngan_penalty.h): form 1, one-sided, max(0, ||g|| - 1)^2 (Petzka et al. 2018), and
// form 2, zero-centred, ||g||^2 / 2 (R1, Mescheder et al. 2018).  The reference's two-sided form stays on the chain of pointwise.hip
// (ngan_sample_l2norm, ngan_gp_head, ngan_gp_coef, ngan_scale_rows); the kernels here keep that chain's operation order, so that where
// the forms coincide (form 1 with every norm above 1) the bits coincide too.
//
// Head: two launches.  The partial sums of squares are sample_sumsq_kernel's, unchanged; one finishing workgroup then adds each
// sample's chunks (one wave per sample, four samples at a time, sample_l2norm_finish_kernel's order), takes the roots and, after a
// barrier, forms lambda * mean(phi) in gp_head_kernel's order.  Backward: one launch; every workgroup derives its row's scalar from
// norms[b] (gp_coef_kernel's order for form 1) and streams the row.  No atomics and no hand-off between workgroups inside a launch.
#include "ngan_common.h"

namespace {

constexpr int L2_CHUNKS = 64;
constexpr int FORM_ONE_SIDED = 1, FORM_ZERO_CENTRED = 2;

__global__ __launch_bounds__(256) void penalty_sumsq_kernel(const float* __restrict__ g, float* __restrict__ partial, long n) {
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* p = g + (long)b * n;
    const long n4 = n >> 2;
    float4 a = f4zero();
    for (long i = (long)blockIdx.x * 256 + tid; i < n4; i += (long)gridDim.x * 256) {
        const float4 v = ld4(p + i * 4);
        a.x = fmaf(v.x, v.x, a.x); a.y = fmaf(v.y, v.y, a.y); a.z = fmaf(v.z, v.z, a.z); a.w = fmaf(v.w, v.w, a.w);
    }
    float s = (a.x + a.y) + (a.z + a.w);
    if (blockIdx.x == 0)
        for (long i = n4 * 4 + tid; i < n; i += 256) s = fmaf(p[i], p[i], s);      // tail when n is not a multiple of 4
    s = group_sum<64>(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) partial[(long)b * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = group_sum<64>(v);
    const int tid = threadIdx.x;
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup: norms[b] = sqrt(sum of sample b's chunks); out = lambda * mean_b phi(norms[b])
__global__ __launch_bounds__(256) void penalty_finish_kernel(const float* __restrict__ partial, float* norms, int B, int nchunk, int form,
                                                             float lambda, float* __restrict__ out) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int b = tid >> 6; b < B; b += 4) {
        float s = 0.f;
        for (int i = lane; i < nchunk; i += 64) s += partial[(long)b * nchunk + i];
        s = group_sum<64>(s);
        if (lane == 0) norms[b] = sqrtf(s);
    }
    __threadfence_block();
    __syncthreads();
    float s = 0.f;
    if (form == FORM_ONE_SIDED) {
        for (int i = tid; i < B; i += 256) { const float e = norms[i] - 1.0f, d = e < 0.f ? 0.f : e; s += d * d; }     // (a NaN norm stays NaN)
    } else {
        for (int i = tid; i < B; i += 256) { const float v = norms[i]; s = fmaf(0.5f * v, v, s); }
    }
    s = block_sum_256(s, red);
    if (tid == 0) out[0] = lambda * s / (float)B;
}

// the row's scalar; `live` false: the row is +0.0 whatever g holds
__device__ __forceinline__ float row_coef(const float* __restrict__ norms, int b, int B, int form, float lambda, const float* __restrict__ g_out,
                                          bool& live) {
    if (form == FORM_ONE_SIDED) {
        const float nb = norms[b];
        live = nb > 1.0f;
        return live ? g_out[0] * 2.0f * lambda * (nb - 1.0f) / ((float)B * nb) : 0.f;
    }
    live = true;
    return g_out[0] * lambda / (float)B;
}

// VEC: rows are 16-byte aligned (n % 4 == 0 or one row); the up to three elements behind the last float4 go to block 0
template <bool VEC>
__global__ __launch_bounds__(256) void penalty_bwd_kernel(const float* __restrict__ g, const float* __restrict__ norms, int B, long n, int form,
                                                          float lambda, const float* __restrict__ g_out, float* __restrict__ out) {
    const int b = blockIdx.y;
    bool live;
    const float c = row_coef(norms, b, B, form, lambda, g_out, live);
    const float* p = g + (long)b * n;
    float* o = out + (long)b * n;
    const long start = (long)blockIdx.x * 256 + threadIdx.x, step = (long)gridDim.x * 256;
    if (VEC) {
        const long n4 = n >> 2;
        if (live) {
            for (long i = start; i < n4; i += step) st4(o + i * 4, f4scale(ld4(p + i * 4), c));
            if (blockIdx.x == 0)
                for (long i = n4 * 4 + threadIdx.x; i < n; i += 256) o[i] = c * p[i];
        } else {
            for (long i = start; i < n4; i += step) st4(o + i * 4, f4zero());
            if (blockIdx.x == 0)
                for (long i = n4 * 4 + threadIdx.x; i < n; i += 256) o[i] = 0.f;
        }
    } else if (live) {
        for (long i = start; i < n; i += step) o[i] = c * p[i];
    } else {
        for (long i = start; i < n; i += step) o[i] = 0.f;
    }
}

int row_blocks(long n) {      // ngan_scale_rows' grid: a block per 256 elements, at most 256 per row
    const long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 256 ? 256 : b));
}

bool form_ok(int form) { return form == FORM_ONE_SIDED || form == FORM_ZERO_CENTRED; }

}  // namespace

extern "C" int ngan_penalty_head(const float* g, int B, long n, int form, float lambda, float* workspace, float* norms, float* out1,
                                 void* stream) {
    NGAN_REQUIRE(g && workspace && norms && out1 && B > 0 && n > 0, NGAN_ERR_ARG, "penalty_head: bad argument");
    NGAN_REQUIRE(form_ok(form), NGAN_ERR_ARG, "penalty_head: unknown form %d (1: one-sided, 2: zero-centred)", form);
    NGAN_REQUIRE(((size_t)g & 15) == 0 && (n % 4 == 0 || B == 1) && B <= 65535, NGAN_ERR_SHAPE,
                 "penalty_head: rows must be 16-byte aligned and at most 65535 (B=%d, n=%ld)", B, n);
    NGAN_REQUIRE((((size_t)workspace | (size_t)norms | (size_t)out1) & 3) == 0, NGAN_ERR_SHAPE, "penalty_head: misaligned output");
    long want = (n / 4 + 255) / 256;
    const int nchunk = (int)(want < 1 ? 1 : (want > L2_CHUNKS ? L2_CHUNKS : want));
    hipLaunchKernelGGL(penalty_sumsq_kernel, dim3(nchunk, B), dim3(256), 0, (hipStream_t)stream, g, workspace, n);
    hipLaunchKernelGGL(penalty_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, workspace, norms, B, nchunk, form, lambda, out1);
    return ngan::launch_status("ngan_penalty_head");
}

extern "C" int ngan_penalty_bwd(const float* g, const float* norms, int B, long n, int form, float lambda, const float* g_out, float* out,
                                void* stream) {
    NGAN_REQUIRE(g && norms && g_out && out && B > 0 && n > 0, NGAN_ERR_ARG, "penalty_bwd: bad argument");
    NGAN_REQUIRE(form_ok(form), NGAN_ERR_ARG, "penalty_bwd: unknown form %d (1: one-sided, 2: zero-centred)", form);
    NGAN_REQUIRE((((size_t)g | (size_t)norms | (size_t)g_out | (size_t)out) & 3) == 0 && B <= 65535, NGAN_ERR_SHAPE,
                 "penalty_bwd: pointers must be 4-byte aligned and rows at most 65535 (B=%d)", B);
    const bool vec = (((size_t)g | (size_t)out) & 15) == 0 && (n % 4 == 0 || B == 1) && n >= 4;
    if (vec)
        hipLaunchKernelGGL(penalty_bwd_kernel<true>, dim3(row_blocks(n / 4), B), dim3(256), 0, (hipStream_t)stream, g, norms, B, n, form,
                           lambda, g_out, out);
    else
        hipLaunchKernelGGL(penalty_bwd_kernel<false>, dim3(row_blocks(n), B), dim3(256), 0, (hipStream_t)stream, g, norms, B, n, form,
                           lambda, g_out, out);
    return ngan::launch_status("ngan_penalty_bwd");
}
