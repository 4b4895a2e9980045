// Differentiable augmentation of the critic's inputs (Zhao et al. 2020, "Differentiable Augmentation for Data-Efficient GAN Training";
// an addition of this implementation, off by default): brightness, contrast, integer translation with a constant fill and one rectangular
// cutout per sample, applied alike to real and generated images, and the operator's adjoint for the generator step.  include/ngan.h
// ("differentiable augmentation") and DESIGN.md section 7 hold the definition; tests/diffaug_cases.py restates it in fp64.
//   ngan_diffaug_params  params_kernel: one thread per sample maps eight uniforms to the sample's parameter row.
//   ngan_diffaug_fwd     sum_kernel<false>: per-sample partial sums of x in fp64 (SUM_TILE elements per workgroup, so the number of
//                        workgroups per sample depends on C R R alone), skipped without the colour group;
//                        map_kernel<false>: folds the partials in a fixed order into k_n, then y = mask . shift(fmaf(c, x, k_n)), with
//                        the constant `fill` where the shift or the cutout leaves nothing (0 is DiffAugment's; the trainer fills
//                        with -1, the images' black: a critic whose blocks end in PixelNorm must not see exact zeros).
//   ngan_diffaug_bwd     sum_kernel<true>: the same sum over gy where the forward pass let a value through (a masked sum: no gather);
//                        map_kernel<true>: r_n from the partials, gx = fmaf(c, shift^T(mask . gy), r_n).
// Reductions go thread (fp64, ascending addresses) -> wave butterfly -> LDS (the four waves in order) -> workspace -> a second fixed
// fold; no atomics, so results are bit-reproducible and a sample's values do not depend on the rest of the batch.  Stores are float4
// along the image row; the shifted reads are aligned float4 loads when the column shift is a multiple of 4 and four predicated scalar
// loads otherwise, which also covers the head and tail of a row.  Contraction is off: the one fused multiply-add per element is the
// explicit fmaf, and k_n / r_n are formed in double and rounded once.
#include <cstdint>
#include "ngan_common.h"
#include "../../include/ngada.h"

#pragma clang fp contract(off)

namespace {

constexpr int SUM_TILE = 8192;             // elements per workgroup of the sum pass: 256 threads x 8 float4
constexpr int MAP_TILE = 4096;             // elements per workgroup of the map pass: 256 threads x 4 float4
constexpr int POLICY_COLOR = 1, POLICY_TRANSLATION = 2, POLICY_CUTOUT = 4;

struct Row {                               // one per sample, 32 bytes (include/ngan.h)
    float b, c;
    int tx, ty, i0, i1, j0, j1;
};
static_assert(sizeof(Row) == 32, "the parameter row is 32 bytes");

// min(n - 1, floor(u n)) in fp32: u = 1 - 2^-24 times n can round up to n
__device__ __forceinline__ int draw_int(float u, int n) { return min(n - 1, (int)floorf(u * (float)n)); }

// LIVE: the probability is the device scalar p_live[0] (include/ngada.h), read by every thread; otherwise the argument p_value
template <bool LIVE>
__global__ __launch_bounds__(256) void params_kernel(const float* __restrict__ u, Row* __restrict__ rows, int B, int R, int S, int K,
                                                     int policy, float p_value, const float* __restrict__ p_live) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= B) return;
    const float p = LIVE ? p_live[0] : p_value;
    const float* q = u + (long)n * 8;
    Row r{0.f, 1.f, 0, 0, 0, 0, 0, 0};                                      // every group's identity
    if ((policy & POLICY_COLOR) && q[0] < p) {
        r.b = q[1] - 0.5f;
        r.c = q[2] + 0.5f;
    }
    if ((policy & POLICY_TRANSLATION) && q[3] < p) {                        // one uniform, (2S + 1)^2 equally likely pairs
        const int side = 2 * S + 1, cell = draw_int(q[4], side * side);
        r.tx = cell / side - S;
        r.ty = cell % side - S;
    }
    if ((policy & POLICY_CUTOUT) && q[5] < p) {
        const int span = R + 1 - (K & 1);
        const int oi = draw_int(q[6], span), oj = draw_int(q[7], span);
        r.i0 = max(oi - K / 2, 0);
        r.i1 = min(oi - K / 2 + K, R);
        r.j0 = max(oj - K / 2, 0);
        r.j1 = min(oj - K / 2 + K, R);
    }
    rows[n] = r;
}

// sum over the workgroup's 256 threads in a fixed order: butterfly inside each wave, then the four waves in order; thread 0 holds it
__device__ __forceinline__ double block_sum256(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// does the forward pass let the value at output position (i, j) through?  (its source (i + tx, j + ty) lies inside the image and
// (i, j) outside the cutout)
__device__ __forceinline__ bool passes(const Row& r, int R, int i, int j) {
    return (unsigned)(i + r.tx) < (unsigned)R && (unsigned)(j + r.ty) < (unsigned)R && !(i >= r.i0 && i < r.i1 && j >= r.j0 && j < r.j1);
}

// partial[n][blk] = sum of the SUM_TILE elements blk covers (MASKED: of those the forward pass lets through)
template <bool MASKED>
__global__ __launch_bounds__(256) void sum_kernel(const float* __restrict__ x, const Row* __restrict__ rows, double* __restrict__ partial,
                                                  int N, int R) {
    __shared__ double red[4];
    const int n = blockIdx.y, tid = threadIdx.x;
    const float* im = x + (long)n * N;
    Row r{};
    if (MASKED) r = rows[n];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < SUM_TILE / 1024; ++k) {
        const int e = blockIdx.x * SUM_TILE + (k * 256 + tid) * 4;          // N is a multiple of 16: a float4 is inside or outside
        if (e < N) {
            const float4 v = ld4(im + e);
            if (MASKED) {
                const int row = e / R, j = e - row * R, i = row % R;        // (channel * R + i, j): R % 4 == 0, so one row per float4
                s += passes(r, R, i, j) ? (double)v.x : 0.0;
                s += passes(r, R, i, j + 1) ? (double)v.y : 0.0;
                s += passes(r, R, i, j + 2) ? (double)v.z : 0.0;
                s += passes(r, R, i, j + 3) ? (double)v.w : 0.0;
            } else {
                s += (double)v.x;
                s += (double)v.y;
                s += (double)v.z;
                s += (double)v.w;
            }
        }
    }
    const double t = block_sum256(s, red);
    if (tid == 0) partial[(long)n * gridDim.x + blockIdx.x] = t;
}

// BWD false: y = mask . shift(fmaf(c, x, k)), k = fp32(c b + (1 - c)(sum / N + b)); `fill` where the mask or the shift leaves nothing
// BWD true:  gx = fmaf(c, gu, r), gu[q] = gy[q - t] where the forward pass let position q - t through, r = fp32((1 - c) / N . sum)
// COLOUR false: b = 0 and c = 1 are taken for granted, the partials are not read and the values pass through untouched
template <bool BWD, bool COLOUR>
__global__ __launch_bounds__(256) void map_kernel(const float* __restrict__ in, const Row* __restrict__ rows, const double* __restrict__ partial,
                                                  float* __restrict__ out, int N, int R, int nblk, float fill) {
    __shared__ double red[4];
    const int n = blockIdx.y, tid = threadIdx.x;
    const Row r = rows[n];
    float c = 1.f, k = 0.f;
    if (COLOUR) {
        double s = 0.0;                                                     // the same fold in every workgroup of the sample
        for (int i = tid; i < nblk; i += 256) s += partial[(long)n * nblk + i];
        const double total = block_sum256(s, red);
        const double cd = (double)r.c, bd = (double)r.b;
        c = r.c;
        k = BWD ? (float)((1.0 - cd) / (double)N * total) : (float)(cd * bd + (1.0 - cd) * (total / (double)N + bd));
    }
    const bool plain = !COLOUR || (c == 1.f && k == 0.f);                   // the identity keeps every bit (the sign of a zero too)
    const int dx = BWD ? -r.tx : r.tx, dy = BWD ? -r.ty : r.ty;             // source = destination + (dx, dy)
    const float* im = in + (long)n * N;
    float* o = out + (long)n * N;
#pragma unroll
    for (int v = 0; v < MAP_TILE / 1024; ++v) {
        const int e = blockIdx.x * MAP_TILE + (v * 256 + tid) * 4;
        if (e >= N) continue;
        const int row = e / R, j = e - row * R, i = row % R;
        const int si = i + dx, sj = j + dy;
        const bool row_in = (unsigned)si < (unsigned)R;
        const long src = (long)(row + dx) * R + sj;                         // read only where row_in and the column is inside
        float g[4];
        if (row_in && (dy & 3) == 0 && (unsigned)sj < (unsigned)R) {        // aligned: sj % 4 == 0 and sj + 3 < R
            const float4 t = ld4(im + src);
            g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w;
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a) g[a] = (row_in && (unsigned)(sj + a) < (unsigned)R) ? im[src + a] : 0.f;
        }
        float w[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const bool col_in = (unsigned)(sj + a) < (unsigned)R;
            // the cutout is a set of forward OUTPUT positions: the destination going forward, the source going back
            const int mi = BWD ? si : i, mj = (BWD ? sj : j) + a;
            const bool cut = mi >= r.i0 && mi < r.i1 && mj >= r.j0 && mj < r.j1;
            const bool live = row_in && col_in && !cut;
            if (BWD) {
                const float gu = live ? g[a] : 0.f;
                w[a] = plain ? gu : fmaf(c, gu, k);
            } else {
                w[a] = live ? (plain ? g[a] : fmaf(c, g[a], k)) : fill;
            }
        }
        st4(o + e, make_float4(w[0], w[1], w[2], w[3]));
    }
}

int check_shape(const char* what, int B, int C, int H, int W, int table_rows) {
    NGAN_REQUIRE(H == W, NGAN_ERR_SHAPE, "%s: %d x %d images unsupported (square images only)", what, H, W);
    NGAN_REQUIRE(H >= 4 && H <= 16384 && H % 4 == 0, NGAN_ERR_SHAPE, "%s: R=%d unsupported (a multiple of 4, 4 .. 16384)", what, H);
    NGAN_REQUIRE(B > 0 && B < 65536, NGAN_ERR_SHAPE, "%s: B=%d unsupported (1 .. 65535 samples per call)", what, B);
    NGAN_REQUIRE(C > 0 && (long)C * H * H < (1L << 31), NGAN_ERR_SHAPE, "%s: C=%d, R=%d: a sample must hold fewer than 2^31 values", what, C, H);
    NGAN_REQUIRE(table_rows >= B, NGAN_ERR_ARG, "%s: the parameter table holds %d rows, the batch %d samples", what, table_rows, B);
    return NGAN_OK;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <bool BWD>
int run(const char* what, const float* in, const void* table, float* out, void* workspace, int B, int C, int H, int W, int table_rows,
        int colour, float fill, void* stream) {
    NGAN_REQUIRE(in && table && out, NGAN_ERR_ARG, "%s: null pointer", what);
    NGAN_REQUIRE(workspace || !colour, NGAN_ERR_ARG, "%s: the colour group needs the workspace", what);
    if (int st = check_shape(what, B, C, H, W, table_rows)) return st;
    NGAN_REQUIRE(fill == fill && fill - fill == 0.f, NGAN_ERR_ARG, "%s: fill=%g must be finite", what, (double)fill);
    NGAN_REQUIRE(aligned16(in) && aligned16(out), NGAN_ERR_ARG, "%s: images must start on a 16-byte boundary", what);
    const int N = C * H * H;
    const int nblk = ngan::ceil_div(N, SUM_TILE);
    const Row* rows = reinterpret_cast<const Row*>(table);
    double* partial = reinterpret_cast<double*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(ngan::ceil_div(N, MAP_TILE), B);
    if (colour) {
        hipLaunchKernelGGL(sum_kernel<BWD>, dim3(nblk, B), dim3(256), 0, s, in, rows, partial, N, H);
        hipLaunchKernelGGL((map_kernel<BWD, true>), grid, dim3(256), 0, s, in, rows, partial, out, N, H, nblk, fill);
    } else {
        hipLaunchKernelGGL((map_kernel<BWD, false>), grid, dim3(256), 0, s, in, rows, partial, out, N, H, nblk, fill);
    }
    return ngan::launch_status(what);
}

}  // namespace

extern "C" size_t ngan_diffaug_workspace_bytes(int B, int C, int R) {
    if (B <= 0 || C <= 0 || R <= 0 || (long)C * R * R >= (1L << 31)) return 0;
    return (size_t)B * (size_t)ngan::ceil_div((long)C * R * R, SUM_TILE) * sizeof(double);
}

extern "C" int ngan_diffaug_params(const float* uniforms, void* table, int B, int H, int W, int table_rows, int policy, float p,
                                   void* stream) {
    NGAN_REQUIRE(uniforms && table, NGAN_ERR_ARG, "diffaug_params: null pointer");
    if (int st = check_shape("diffaug_params", B, 1, H, W, table_rows)) return st;
    NGAN_REQUIRE(policy >= 0 && policy < 8, NGAN_ERR_ARG, "diffaug_params: policy mask %d (bits 1 colour, 2 translation, 4 cutout)", policy);
    NGAN_REQUIRE(p >= 0.f && p <= 1.f, NGAN_ERR_ARG, "diffaug_params: p=%g must lie in [0, 1]", (double)p);
    const int S = (int)(H * 0.125 + 0.5), K = (int)(H * 0.5 + 0.5);
    hipLaunchKernelGGL(params_kernel<false>, dim3(ngan::ceil_div(B, 256)), dim3(256), 0, (hipStream_t)stream, uniforms,
                       reinterpret_cast<Row*>(table), B, H, S, K, policy, p, (const float*)nullptr);
    return ngan::launch_status("ngan_diffaug_params");
}

// the same mapping with the probability in device memory (include/ngada.h): no range check, the host does not know the value
extern "C" int ngada_diffaug_params(const float* uniforms, void* table, int B, int H, int W, int table_rows, int policy, const float* p,
                                    void* stream) {
    NGAN_REQUIRE(uniforms && table, NGAN_ERR_ARG, "ngada_diffaug_params: null pointer");
    NGAN_REQUIRE(p, NGAN_ERR_ARG, "ngada_diffaug_params: p is a null pointer");
    if (int st = check_shape("ngada_diffaug_params", B, 1, H, W, table_rows)) return st;
    NGAN_REQUIRE(policy >= 0 && policy < 8, NGAN_ERR_ARG, "ngada_diffaug_params: policy mask %d (bits 1 colour, 2 translation, 4 cutout)", policy);
    const int S = (int)(H * 0.125 + 0.5), K = (int)(H * 0.5 + 0.5);
    hipLaunchKernelGGL(params_kernel<true>, dim3(ngan::ceil_div(B, 256)), dim3(256), 0, (hipStream_t)stream, uniforms,
                       reinterpret_cast<Row*>(table), B, H, S, K, policy, 0.f, p);
    return ngan::launch_status("ngada_diffaug_params");
}

extern "C" int ngan_diffaug_fwd(const float* x, const void* table, float* y, void* workspace, int B, int C, int H, int W,
                                int table_rows, int colour, float fill, void* stream) {
    return run<false>("ngan_diffaug_fwd", x, table, y, workspace, B, C, H, W, table_rows, colour, fill, stream);
}

extern "C" int ngan_diffaug_bwd(const float* gy, const void* table, float* gx, void* workspace, int B, int C, int H, int W,
                                int table_rows, int colour, void* stream) {
    return run<true>("ngan_diffaug_bwd", gy, table, gx, workspace, B, C, H, W, table_rows, colour, 0.f, stream);
}
