// Sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al. 2018, section 5): the kernels behind metrics.py.
//   ngan_swd_pyr_down      pyr_down_kernel: a 16 x 16 output tile per workgroup; its 35 x 35 input tile with the mirrored halo is
//                          staged in LDS, filtered along the rows at the even columns only, then along the columns at the even rows
//   ngan_swd_laplacian     laplacian_kernel: one thread per coarse pixel and channel; its 3 x 3 coarse neighbourhood gives the four
//                          fine outputs of the 2 x 2 quad, each parity class with its own taps (even: 1/8 6/8 1/8, odd: 1/2 1/2)
//   ngan_swd_descriptors   descriptors_kernel (64 patches per workgroup: gather, fp64 partial sums) + reduce_doubles_kernel
//   ngan_swd_project       project_kernel: 64 descriptors per workgroup, normalised into LDS once, 16 directions per wave and pass
//   ngan_swd_sort_columns  sort_lds_kernel (every stage of stride < SORT_BLOCK on a block held in LDS) and sort_global_kernel<1|2>
//                          (one or two strides >= SORT_BLOCK per pass over global memory, 16-byte accesses)
//   ngan_swd_l1            l1_kernel + reduce_doubles_kernel
// Every multiply-add whose rounding matters is an explicit fmaf, so the order is the source's whatever the compiler contracts.
#include "ngan_common.h"

namespace {

constexpr int PD_T = 16;                 // pyr_down: output tile edge
constexpr int PD_IN = 2 * PD_T + 3;      // input tile edge with the halo of 2 on the low and 1 + 2 on the high side
constexpr int DESC_ROWS = 64;            // patches per workgroup of the gather
constexpr int PROJ_ROWS = 64;            // descriptors per workgroup of the projection (one per lane)
constexpr int PROJ_DJ = 16;              // directions per wave and pass
#ifndef NGAN_SWD_SORT_BLOCK
#define NGAN_SWD_SORT_BLOCK 16384      // (a power of two up to 32768; measured against 8192 and 32768: DESIGN.md section 7)
#endif
constexpr int SORT_BLOCK = NGAN_SWD_SORT_BLOCK;   // values of one LDS block: 64 KiB, two workgroups per CU
constexpr int SORT_THREADS = 1024;
constexpr int L1_PER_BLOCK = 256 * 16;   // values of one column per workgroup of the L1 sum

__device__ __forceinline__ int mirror(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);        // (only tile positions past the image, whose values nothing reads, reach the clamp)
}

// [1 4 6 4 1] / 16: the outer pairs are added first, the products with 1/16 and 1/4 are exact
__device__ __forceinline__ float gauss5(float x0, float x1, float x2, float x3, float x4) {
    return fmaf(0.375f, x2, fmaf(0.25f, x1 + x3, 0.0625f * (x0 + x4)));
}

template <int C>
__global__ __launch_bounds__(256) void pyr_down_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W) {
    __shared__ float tile[PD_IN * PD_IN * C];
    __shared__ float hb[PD_IN * PD_T * C];
    const int Ho = H >> 1, Wo = W >> 1;
    const int ox0 = blockIdx.x * PD_T, oy0 = blockIdx.y * PD_T;
    const float* im = in + (long)blockIdx.z * H * W * C;
    const int iy0 = 2 * oy0 - 2, ix0 = 2 * ox0 - 2;
    for (int e = threadIdx.x; e < PD_IN * PD_IN * C; e += 256) {
        const int r = e / (PD_IN * C), q = e - r * (PD_IN * C), x = q / C, c = q - x * C;
        tile[e] = im[((long)mirror(iy0 + r, H) * W + mirror(ix0 + x, W)) * C + c];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < PD_IN * PD_T * C; e += 256) {
        const int r = e / (PD_T * C), q = e - r * (PD_T * C), x = q / C, c = q - x * C;
        const float* t = tile + (r * PD_IN + 2 * x) * C + c;
        hb[e] = gauss5(t[0], t[C], t[2 * C], t[3 * C], t[4 * C]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < PD_T * PD_T * C; e += 256) {
        const int y = e / (PD_T * C), q = e - y * (PD_T * C), x = q / C, c = q - x * C;
        if (oy0 + y >= Ho || ox0 + x >= Wo) continue;
        const float* t = hb + (2 * y * PD_T + x) * C + c;
        constexpr int S = PD_T * C;
        out[(((long)blockIdx.z * Ho + oy0 + y) * Wo + ox0 + x) * C + c] = gauss5(t[0], t[S], t[2 * S], t[3 * S], t[4 * S]);
    }
}

// Zero-insert x2 filtered with 4 x the Gaussian, per axis (i: coarse index, n: coarse size; the mirror acts on the fine grid):
//   fine 2 i     = (c[i - 1] + c[i + 1]) / 8 + 6 c[i] / 8,   c[-1] -> c[1] and c[n] -> c[n - 1] (fine index 2 n mirrors to 2 n - 2)
//   fine 2 i + 1 = (c[i] + c[i + 1]) / 2,                    c[n] -> c[n - 1]
// (the other taps of each class fall on inserted zeros, before and after the mirror)
template <int C>
__global__ __launch_bounds__(256) void laplacian_kernel(const float* __restrict__ fine, const float* __restrict__ coarse,
                                                        float* __restrict__ lap, int Hc, int Wc, long total) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % C);
    long p = t / C;
    const int j = (int)(p % Wc);
    p /= Wc;
    const int i = (int)(p % Hc);
    const long b = p / Hc;
    const int rows[3] = {i == 0 ? 1 : i - 1, i, i == Hc - 1 ? i : i + 1};
    const int jm = j == 0 ? 1 : j - 1, jp = j == Wc - 1 ? j : j + 1;
    const float* cb = coarse + b * Hc * Wc * C + c;
    float he[3], ho[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* row = cb + (long)rows[k] * Wc * C;
        const float l = row[jm * C], m = row[j * C], r = row[jp * C];
        he[k] = fmaf(0.75f, m, 0.125f * (l + r));
        ho[k] = 0.5f * (m + r);
    }
    const float ee = fmaf(0.75f, he[1], 0.125f * (he[0] + he[2])), eo = fmaf(0.75f, ho[1], 0.125f * (ho[0] + ho[2]));
    const float oe = 0.5f * (he[1] + he[2]), oo = 0.5f * (ho[1] + ho[2]);
    const long W = 2L * Wc;
    const long base = ((b * 2 * Hc + 2 * i) * W + 2 * j) * C + c;
    lap[base] = fine[base] - ee;
    lap[base + C] = fine[base + C] - eo;
    lap[base + W * C] = fine[base + W * C] - oe;
    lap[base + W * C + C] = fine[base + W * C + C] - oo;
}

// sum over the workgroup's 256 threads in a fixed order: butterfly inside each wave, then the four waves in order; thread 0 holds it
__device__ __forceinline__ double block_sum256(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

template <int C>
__global__ __launch_bounds__(256) void descriptors_kernel(const float* __restrict__ img, const int* __restrict__ pos,
                                                          float* __restrict__ desc, double* __restrict__ partials, int n, int B, int H,
                                                          int W) {
    constexpr int K = 49 * C;
    __shared__ int sp[DESC_ROWS * 3];
    __shared__ double red[4];
    const int row0 = blockIdx.x * DESC_ROWS;
    const int rows = min(DESC_ROWS, n - row0);
    for (int t = threadIdx.x; t < rows * 3; t += 256) sp[t] = pos[(long)row0 * 3 + t];
    __syncthreads();
    double s[C], q[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = q[c] = 0.0;
    for (int e = threadIdx.x; e < rows * K; e += 256) {
        const int r = e / K, k = e - r * K, c = k / 49, kk = k - c * 49, dy = kk / 7, dx = kk - dy * 7;
        // the host has checked the triples; the clamps keep a caller whose two copies differ inside the images
        const int b = min(max(sp[3 * r], 0), B - 1), y = min(max(sp[3 * r + 1], 0), H - 7), x = min(max(sp[3 * r + 2], 0), W - 7);
        const float v = img[(((long)b * H + y + dy) * W + x + dx) * C + c];
        desc[(long)(row0 + r) * K + k] = v;
        const double d = (double)v;
#pragma unroll
        for (int cc = 0; cc < C; ++cc)
            if (c == cc) {
                s[cc] += d;
                q[cc] = fma(d, d, q[cc]);
            }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const double ts = block_sum256(s[c], red);
        const double tq = block_sum256(q[c], red);
        if (threadIdx.x == 0) {
            partials[(long)blockIdx.x * 2 * C + c] = ts;
            partials[(long)blockIdx.x * 2 * C + C + c] = tq;
        }
    }
}

// stage 2 of the fp64 reductions: out[i] = (accumulate ? out[i] : 0) + scale * sum_j partials[j * M + i], one workgroup, fixed order
__global__ __launch_bounds__(256) void reduce_doubles_kernel(const double* __restrict__ partials, long nparts, int M,
                                                             double* __restrict__ out, double scale, int accumulate) {
    __shared__ double red[4];
    for (int i = 0; i < M; ++i) {
        double v = 0.0;
        for (long j = threadIdx.x; j < nparts; j += 256) v += partials[j * M + i];
        const double t = block_sum256(v, red);
        if (threadIdx.x == 0) out[i] = (accumulate ? out[i] : 0.0) + scale * t;
    }
}

template <int C>
__global__ __launch_bounds__(256) void project_kernel(const float* __restrict__ desc, const double* __restrict__ sums,
                                                      const float* __restrict__ dirs, float* __restrict__ proj, int n, int n_pad,
                                                      int n_dirs) {
    constexpr int K = 49 * C, PITCH = PROJ_ROWS + 1;      // pitch 65: the transposing stores below hit 64 different banks
    __shared__ float vs[K * PITCH];
    const int row0 = blockIdx.x * PROJ_ROWS;
    double mean[C], inv[C];
    const double cnt = 49.0 * (double)n;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        mean[c] = sums[c] / cnt;
        inv[c] = 1.0 / sqrt(sums[C + c] / cnt - mean[c] * mean[c]);
    }
    const int rows = min(PROJ_ROWS, n - row0);
    if (rows <= 0) {                                       // a tile of the +inf tail: nothing to compute
        const int i = row0 + (threadIdx.x & 63);
        if (i < n_pad)
            for (int j = threadIdx.x >> 6; j < n_dirs; j += 4) proj[(long)j * n_pad + i] = __builtin_inff();
        return;
    }
    for (int e = threadIdx.x; e < PROJ_ROWS * K; e += 256) {
        const int r = e / K, k = e - r * K, c = k / 49;
        float v = 0.0f;
        if (r < rows) {
            double m = mean[0], s = inv[0];
#pragma unroll
            for (int cc = 1; cc < C; ++cc)
                if (c == cc) { m = mean[cc]; s = inv[cc]; }
            v = (float)(((double)desc[(long)(row0 + r) * K + k] - m) * s);
        }
        vs[k * PITCH + r] = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = row0 + lane;
    for (int j0 = wave * PROJ_DJ; j0 < n_dirs; j0 += 4 * PROJ_DJ) {      // wave-uniform: the directions come through scalar loads
        float acc[PROJ_DJ];
#pragma unroll
        for (int d = 0; d < PROJ_DJ; ++d) acc[d] = 0.0f;
        if (j0 + PROJ_DJ <= n_dirs) {
            // seven k in flight (K = 7 * 7 C): seven 16-dword scalar loads are issued before the first is waited for -- 1.05 ms
            // against 2.97 ms without the unroll for 2^20 descriptors x 512 directions; the order of the fmafs is unchanged
#pragma unroll 7
            for (int k = 0; k < K; ++k) {
                const float v = vs[k * PITCH + lane];
                const float* th = dirs + (long)k * n_dirs + j0;
#pragma unroll
                for (int d = 0; d < PROJ_DJ; ++d) acc[d] = fmaf(v, th[d], acc[d]);
            }
        } else {
            for (int k = 0; k < K; ++k) {
                const float v = vs[k * PITCH + lane];
                const float* th = dirs + (long)k * n_dirs;
#pragma unroll
                for (int d = 0; d < PROJ_DJ; ++d) acc[d] = fmaf(v, th[min(j0 + d, n_dirs - 1)], acc[d]);
            }
        }
        if (i < n_pad) {
#pragma unroll
            for (int d = 0; d < PROJ_DJ; ++d)
                if (j0 + d < n_dirs) proj[(long)(j0 + d) * n_pad + i] = i < n ? acc[d] : __builtin_inff();
        }
    }
}

// ---- bitonic sort of columns ---------------------------------------------------------------------------------------------------
// Element i of a column, merge size k, stride j: partner i ^ j, ascending where (i & k) == 0.  The network for a power-of-two length
// sorts any input; the +inf tail of the projection sorts to the end.
__device__ __forceinline__ void cmpx(float& a, float& b, bool asc) {
    if ((a > b) == asc) {
        const float t = a;
        a = b;
        b = t;
    }
}
__device__ __forceinline__ void cmpx4(float4& a, float4& b, bool asc) {
    cmpx(a.x, b.x, asc);
    cmpx(a.y, b.y, asc);
    cmpx(a.z, b.z, asc);
    cmpx(a.w, b.w, asc);
}

// One block of `len` values (a power of two <= SORT_BLOCK) of one column in LDS: for every merge size k = k_lo, 2 k_lo, ..., k_hi all
// strides min(k, len) / 2, ..., 1.  (k_lo = 2, k_hi = len: the block sorted from scratch; k_lo = k_hi = k > len: the tail of merge k.)
__global__ __launch_bounds__(SORT_THREADS) void sort_lds_kernel(float* __restrict__ cols, int n_pad, int len, long k_lo, long k_hi) {
    extern __shared__ float4 sm4[];       // (no static LDS in front: the base is 16-byte aligned)
    float* sm = reinterpret_cast<float*>(sm4);
    const long base = (long)blockIdx.x * len;
    float* g = cols + (long)blockIdx.y * n_pad + base;
    if (len >= 4) {
        for (int t = threadIdx.x; t < len / 4; t += SORT_THREADS) sm4[t] = reinterpret_cast<const float4*>(g)[t];
    } else {
        for (int t = threadIdx.x; t < len; t += SORT_THREADS) sm[t] = g[t];
    }
    __syncthreads();
    for (long k = k_lo; k <= k_hi; k <<= 1) {
        for (int j = (int)(k > len ? len : k) >> 1; j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < len / 2; p += SORT_THREADS) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                float a = sm[i], b = sm[i + j];
                cmpx(a, b, ((base + i) & k) == 0);
                sm[i] = a;
                sm[i + j] = b;
            }
            __syncthreads();
        }
    }
    if (len >= 4) {
        for (int t = threadIdx.x; t < len / 4; t += SORT_THREADS) reinterpret_cast<float4*>(g)[t] = sm4[t];
    } else {
        for (int t = threadIdx.x; t < len; t += SORT_THREADS) g[t] = sm[t];
    }
}

// STAGES = 1: stride j of merge k, one lane per pair of 16-byte groups.  STAGES = 2: strides j and j / 2 in one pass, one lane per
// four groups at i, i + j/2, i + j, i + 3j/2 (k > j, so the direction is the same for all of them).  j / STAGES >= 4.
template <int STAGES>
__global__ __launch_bounds__(256) void sort_global_kernel(float* __restrict__ cols, int n_pad, long k, int j) {
    float* g = cols + (long)blockIdx.y * n_pad;
    const long q = ((long)blockIdx.x * 256 + threadIdx.x) * 4;           // first element of this lane's lowest group, compacted
    if (STAGES == 1) {
        if (q >= n_pad / 2) return;
        const long i = ((q & ~(long)(j - 1)) << 1) | (q & (j - 1));
        const bool asc = (i & k) == 0;
        float4 a = ld4(g + i), b = ld4(g + i + j);
        cmpx4(a, b, asc);
        st4(g + i, a);
        st4(g + i + j, b);
    } else {
        if (q >= n_pad / 4) return;
        const int h = j >> 1;
        const long i = ((q & ~(long)(h - 1)) << 2) | (q & (h - 1));
        const bool asc = (i & k) == 0;
        float4 x0 = ld4(g + i), x1 = ld4(g + i + h), x2 = ld4(g + i + j), x3 = ld4(g + i + j + h);
        cmpx4(x0, x2, asc);
        cmpx4(x1, x3, asc);
        cmpx4(x0, x1, asc);
        cmpx4(x2, x3, asc);
        st4(g + i, x0);
        st4(g + i + h, x1);
        st4(g + i + j, x2);
        st4(g + i + j + h, x3);
    }
}

__global__ __launch_bounds__(256) void l1_kernel(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ partials,
                                                 int n, int n_pad) {
    __shared__ double red[4];
    const long col = (long)blockIdx.y * n_pad;
    const int i0 = blockIdx.x * L1_PER_BLOCK;
    const int i1 = min(i0 + L1_PER_BLOCK, n);
    double v = 0.0;
    for (int i = i0 + threadIdx.x; i < i1; i += 256) v += (double)fabsf(a[col + i] - b[col + i]);
    const double t = block_sum256(v, red);
    if (threadIdx.x == 0) partials[(long)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

bool pow2(long v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace

extern "C" int ngan_swd_pyr_down(const float* in, float* out, int B, int H, int W, int C, void* stream) {
    NGAN_REQUIRE(in && out, NGAN_ERR_ARG, "swd_pyr_down: null pointer");
    NGAN_REQUIRE(C == 1 || C == 3, NGAN_ERR_SHAPE, "swd_pyr_down: C=%d unsupported (1 or 3 colour channels)", C);
    NGAN_REQUIRE(B > 0 && B < 65536 && H >= 4 && W >= 4 && H % 2 == 0 && W % 2 == 0 && H <= 32768 && W <= 32768, NGAN_ERR_SHAPE,
                 "swd_pyr_down: B=%d H=%d W=%d unsupported (H and W even, 4 .. 32768; B < 65536)", B, H, W);
    const dim3 grid(ngan::ceil_div(W / 2, PD_T), ngan::ceil_div(H / 2, PD_T), B);
    if (C == 1) hipLaunchKernelGGL(pyr_down_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, in, out, H, W);
    else hipLaunchKernelGGL(pyr_down_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, in, out, H, W);
    return ngan::launch_status("ngan_swd_pyr_down");
}

extern "C" int ngan_swd_laplacian(const float* fine, const float* coarse, float* lap, int B, int H, int W, int C, void* stream) {
    NGAN_REQUIRE(fine && coarse && lap, NGAN_ERR_ARG, "swd_laplacian: null pointer");
    NGAN_REQUIRE(C == 1 || C == 3, NGAN_ERR_SHAPE, "swd_laplacian: C=%d unsupported (1 or 3 colour channels)", C);
    NGAN_REQUIRE(B > 0 && H >= 4 && W >= 4 && H % 2 == 0 && W % 2 == 0 && H <= 32768 && W <= 32768, NGAN_ERR_SHAPE,
                 "swd_laplacian: B=%d H=%d W=%d unsupported (H and W even, 4 .. 32768)", B, H, W);
    const int Hc = H / 2, Wc = W / 2;
    const long total = (long)B * Hc * Wc * C;
    NGAN_REQUIRE((total + 255) / 256 < (1L << 31), NGAN_ERR_SHAPE, "swd_laplacian: %ld coarse values in one call", total);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (C == 1) hipLaunchKernelGGL(laplacian_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, fine, coarse, lap, Hc, Wc, total);
    else hipLaunchKernelGGL(laplacian_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, fine, coarse, lap, Hc, Wc, total);
    return ngan::launch_status("ngan_swd_laplacian");
}

extern "C" size_t ngan_swd_descriptors_workspace_bytes(int n, int C) {
    if (n <= 0 || (C != 1 && C != 3)) return 0;
    return (size_t)ngan::ceil_div(n, DESC_ROWS) * 2 * C * sizeof(double);
}

extern "C" int ngan_swd_descriptors(const float* images, const int* pos_host, const int* pos, float* desc, double* sums, void* workspace,
                                    int n, long row_offset, int accumulate, int B, int H, int W, int C, void* stream) {
    NGAN_REQUIRE(images && pos_host && pos && desc && sums && workspace, NGAN_ERR_ARG, "swd_descriptors: null pointer");
    NGAN_REQUIRE(C == 1 || C == 3, NGAN_ERR_SHAPE, "swd_descriptors: C=%d unsupported (1 or 3 colour channels)", C);
    NGAN_REQUIRE(n > 0 && row_offset >= 0 && B > 0 && H >= 7 && W >= 7, NGAN_ERR_SHAPE,
                 "swd_descriptors: n=%d row_offset=%ld B=%d H=%d W=%d unsupported (a patch is 7 x 7)", n, row_offset, B, H, W);
    for (int i = 0; i < n; ++i) {
        const int b = pos_host[3 * i], y = pos_host[3 * i + 1], x = pos_host[3 * i + 2];
        NGAN_REQUIRE(b >= 0 && b < B && y >= 0 && y <= H - 7 && x >= 0 && x <= W - 7, NGAN_ERR_ARG,
                     "swd_descriptors: patch %d = (image %d, row %d, column %d) is out of range for %d images of %d x %d", i, b, y, x, B,
                     H, W);
    }
    hipStream_t s = (hipStream_t)stream;
    const int blocks = ngan::ceil_div(n, DESC_ROWS);
    double* partials = reinterpret_cast<double*>(workspace);
    float* out = desc + row_offset * 49 * C;
    if (C == 1) hipLaunchKernelGGL(descriptors_kernel<1>, dim3(blocks), dim3(256), 0, s, images, pos, out, partials, n, B, H, W);
    else hipLaunchKernelGGL(descriptors_kernel<3>, dim3(blocks), dim3(256), 0, s, images, pos, out, partials, n, B, H, W);
    hipLaunchKernelGGL(reduce_doubles_kernel, dim3(1), dim3(256), 0, s, partials, (long)blocks, 2 * C, sums, 1.0, accumulate);
    return ngan::launch_status("ngan_swd_descriptors");
}

extern "C" int ngan_swd_project(const float* desc, const double* sums, const float* dirs, float* proj, int n, int n_pad, int n_dirs,
                                int C, void* stream) {
    NGAN_REQUIRE(desc && sums && dirs && proj, NGAN_ERR_ARG, "swd_project: null pointer");
    NGAN_REQUIRE(C == 1 || C == 3, NGAN_ERR_SHAPE, "swd_project: C=%d unsupported (1 or 3 colour channels)", C);
    NGAN_REQUIRE(n > 0 && n_dirs > 0, NGAN_ERR_SHAPE, "swd_project: n=%d n_dirs=%d must be positive", n, n_dirs);
    NGAN_REQUIRE(pow2(n_pad) && n_pad >= n, NGAN_ERR_SHAPE, "swd_project: n_pad=%d must be a power of two >= n=%d", n_pad, n);
    const dim3 grid(ngan::ceil_div(n_pad, PROJ_ROWS));
    if (C == 1) hipLaunchKernelGGL(project_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, desc, sums, dirs, proj, n, n_pad, n_dirs);
    else hipLaunchKernelGGL(project_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, desc, sums, dirs, proj, n, n_pad, n_dirs);
    return ngan::launch_status("ngan_swd_project");
}

extern "C" int ngan_swd_sort_block_elements(void) { return SORT_BLOCK; }

extern "C" int ngan_swd_sort_columns(float* cols, int n_dirs, int n_pad, void* stream) {
    NGAN_REQUIRE(cols, NGAN_ERR_ARG, "swd_sort_columns: null pointer");
    NGAN_REQUIRE(n_dirs > 0 && n_dirs < 65536, NGAN_ERR_SHAPE, "swd_sort_columns: n_dirs=%d unsupported (1 .. 65535)", n_dirs);
    NGAN_REQUIRE(pow2(n_pad) && n_pad <= (1 << 30), NGAN_ERR_SHAPE, "swd_sort_columns: n_pad=%d must be a power of two <= 2^30", n_pad);
    NGAN_REQUIRE(n_pad < 4 || (reinterpret_cast<size_t>(cols) & 15) == 0, NGAN_ERR_ARG,
                 "swd_sort_columns: cols must be 16-byte aligned (16-byte loads and stores)");
    if (n_pad == 1) return NGAN_OK;
    hipStream_t s = (hipStream_t)stream;
    const int len = n_pad < SORT_BLOCK ? n_pad : SORT_BLOCK;
    const size_t lds = (size_t)len * sizeof(float);
    static bool attr_set = false;
    if (lds > 64 * 1024 && !attr_set) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sort_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 SORT_BLOCK * (int)sizeof(float));
        NGAN_REQUIRE(e == hipSuccess, (int)e, "swd_sort_columns: cannot raise the dynamic LDS limit: %s", hipGetErrorString(e));
        attr_set = true;
    }
    const dim3 lgrid(n_pad / len, n_dirs);
    hipLaunchKernelGGL(sort_lds_kernel, lgrid, dim3(SORT_THREADS), lds, s, cols, n_pad, len, 2L, (long)len);
    for (long k = 2L * len; k <= n_pad; k <<= 1) {
        int j = (int)(k >> 1);
        while (j >= len) {
            if (j / 2 >= len) {
                hipLaunchKernelGGL(sort_global_kernel<2>, dim3(ngan::ceil_div(n_pad / 16, 256), n_dirs), dim3(256), 0, s, cols, n_pad, k, j);
                j >>= 2;
            } else {
                hipLaunchKernelGGL(sort_global_kernel<1>, dim3(ngan::ceil_div(n_pad / 8, 256), n_dirs), dim3(256), 0, s, cols, n_pad, k, j);
                j >>= 1;
            }
        }
        hipLaunchKernelGGL(sort_lds_kernel, lgrid, dim3(SORT_THREADS), lds, s, cols, n_pad, len, k, k);
    }
    return ngan::launch_status("ngan_swd_sort_columns");
}

extern "C" size_t ngan_swd_l1_workspace_bytes(int n, int n_dirs) {
    if (n <= 0 || n_dirs <= 0) return 0;
    return (size_t)ngan::ceil_div(n, L1_PER_BLOCK) * n_dirs * sizeof(double);
}

extern "C" int ngan_swd_l1(const float* a, const float* b, double* out, void* workspace, int n, int n_pad, int n_dirs, void* stream) {
    NGAN_REQUIRE(a && b && out && workspace, NGAN_ERR_ARG, "swd_l1: null pointer");
    NGAN_REQUIRE(n > 0 && n_pad >= n && n_dirs > 0 && n_dirs < 65536, NGAN_ERR_SHAPE,
                 "swd_l1: n=%d n_pad=%d n_dirs=%d unsupported (0 < n <= n_pad, n_dirs 1 .. 65535)", n, n_pad, n_dirs);
    hipStream_t s = (hipStream_t)stream;
    const int blocks = ngan::ceil_div(n, L1_PER_BLOCK);
    double* partials = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(l1_kernel, dim3(blocks, n_dirs), dim3(256), 0, s, a, b, partials, n, n_pad);
    hipLaunchKernelGGL(reduce_doubles_kernel, dim3(1), dim3(256), 0, s, partials, (long)blocks * n_dirs, 1, out,
                       1.0 / ((double)n * (double)n_dirs), 0);
    return ngan::launch_status("ngan_swd_l1");
}
