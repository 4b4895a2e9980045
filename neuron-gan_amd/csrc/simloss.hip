// Pairwise similarity loss of the generator: the kernels behind ops.SimilarityLoss (include/nganx.h has the formulas; the per-pair
// arithmetic is simloss_bits.h, which the host compiles too).
//   gram_kernel    A VALU / LDS design, not the f64 MFMA: the job is bound by its B N 4 bytes of loads (2 B^2 N flops against them:
//                  32 flops per byte at B = 64, 8 at the flagship's B = 16, far under the chip's fp64 VALU ratio), so the matrix
//                  core buys nothing here, while a plain fma chain has an operation order that tests/simloss_cases.py can restate
//                  line by line.  A workgroup of 256 threads owns one slab of `chunk` pixels (simloss::gram_plan: a function of
//                  (B, N) alone).  It stages a tile of pixels through LDS as tile[row][p] with an odd pitch (no bank conflict on the
//                  stores or on the reads), 16-byte loads from global memory, rows beyond B and pixels beyond N as zeros.  The
//                  threads form `groups` groups of lanes x lanes; thread
//                  (ti, tj) of a group holds the 4 x 4 block G[4 ti .. ][4 tj .. ] in fp64 and the group takes the pixels
//                  p = g, g + groups, ... of every tile, ascending: acc = fma(x_i, x_j, acc), the product exact in fp64.  The
//                  threads with tj = 0 add the row sums the same way.  The groups' accumulators meet in LDS, ascending g, and the
//                  slab's partials are written element-major, partials[e][slab].
//   gram_reduce    a wave per output element: lane l adds the slabs l, l + 64, ... ascending, the lanes meet in a fixed butterfly.
//   head_kernel    ONE workgroup of 16 waves; wave w takes rows w, w + 16, ..., lane j the pair (i, j): simloss::pair_terms in fp64,
//                  the row sums of d^2, A S and M m through a fixed butterfly (lanes beyond B add zeros), thread 0 the rows' sums of
//                  d^2, ascending.  lambda is read from device memory.
//   mix_kernel     a thread owns V consecutive pixels of all B rows in registers, M and r sit in LDS:
//                  grad[i][p] = addend + upstream * (fma chain over j ascending - r_i).
// No atomics, no state between calls, no inline assembly; contraction is off in the fp32 chain.
#include "ngan_common.h"
#include "simloss_bits.h"
#include "../../include/nganx.h"
#include <cstdint>

namespace {

constexpr int NT = 256;
constexpr int HT = 1024, HW = HT / 64;

// grid (slabs); LDS: the tile (4 lanes x (tile + 1) floats, at most 16.3 KB) and the groups' accumulators (256 x 20 doubles = 40 KB)
template <int LANES>
__global__ __launch_bounds__(NT) void gram_kernel(const float* __restrict__ x, double* __restrict__ partials, int B, long N, long chunk) {
    constexpr int BP = 4 * LANES, GROUPS = NT / (LANES * LANES), TILE = GROUPS > 64 ? 256 : 64, PITCH = TILE + 1;
    __shared__ float tile[BP * PITCH];
    __shared__ double meet[NT * 20];
    const int tid = threadIdx.x;
    const int g = tid / (LANES * LANES), t = tid - g * (LANES * LANES), ti = t / LANES, tj = t - ti * LANES;
    const long p_begin = (long)blockIdx.x * chunk;
    const long p_end = p_begin + chunk < N ? p_begin + chunk : N;
    double acc[4][4], sum[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        sum[a] = 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
    }
    for (long p0 = p_begin; p0 < p_end; p0 += TILE) {
        __syncthreads();                                       // the previous tile has been read
        for (int e = tid; e < BP * (TILE / 4); e += NT) {      // one 16-byte load: row i, pixels p0 + 4 q ..
            const int i = e / (TILE / 4), q = e - i * (TILE / 4);
            const long p = p0 + 4 * q;
            float4 v = f4zero();
            if (i < B && p < p_end) v = ld4(x + (long)i * N + p);      // N % 4 == 0 and p_end <= N: whole or not at all
            float* dst = tile + i * PITCH + 4 * q;
            dst[0] = v.x;
            dst[1] = v.y;
            dst[2] = v.z;
            dst[3] = v.w;
        }
        __syncthreads();
        for (int p = g; p < TILE; p += GROUPS) {
            const float* ra = tile + 4 * ti * PITCH + p;
            const float* rb = tile + 4 * tj * PITCH + p;
            const double a[4] = {(double)ra[0], (double)ra[PITCH], (double)ra[2 * PITCH], (double)ra[3 * PITCH]};
            const double b[4] = {(double)rb[0], (double)rb[PITCH], (double)rb[2 * PITCH], (double)rb[3 * PITCH]};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
            }
            if (tj == 0) {
#pragma unroll
                for (int u = 0; u < 4; ++u) sum[u] += a[u];
            }
        }
    }
    double* mine = meet + tid * 20;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int v = 0; v < 4; ++v) mine[4 * u + v] = acc[u][v];
        mine[16 + u] = sum[u];
    }
    __syncthreads();
    double* out = partials + blockIdx.x;                      // element-major: partials[e * slabs + slab]
    const long slabs = gridDim.x;
    // element (i, j) lives in thread (i / 4, j / 4) of every group, slot 4 (i % 4) + (j % 4); the groups add ascending
    for (int e = tid; e < B * B; e += NT) {
        const int i = e / B, j = e - i * B;
        const int at = ((i >> 2) * LANES + (j >> 2)) * 20 + 4 * (i & 3) + (j & 3);
        double s = meet[at];
        for (int k = 1; k < GROUPS; ++k) s += meet[k * (LANES * LANES) * 20 + at];
        out[e * slabs] = s;
    }
    for (int i = tid; i < B; i += NT) {
        const int at = ((i >> 2) * LANES) * 20 + 16 + (i & 3);
        double s = meet[at];
        for (int k = 1; k < GROUPS; ++k) s += meet[k * (LANES * LANES) * 20 + at];
        out[(long)(B * B + i) * slabs] = s;
    }
}

__device__ __forceinline__ double lane_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);       // a fixed butterfly: every lane ends with the same sum
    return v;
}

// grid (ceil(M / 4)), a wave per element e (whole waves enter or leave): lane l adds partials[e][l], [l + 64], ... ascending, then the
// butterfly; the first B * B elements go to gram, the rest to sums
__global__ __launch_bounds__(NT) void gram_reduce_kernel(const double* __restrict__ partials, int slabs, int B, double* __restrict__ gram,
                                                         double* __restrict__ sums) {
    const int M = B * B + B;
    const int e = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= M) return;
    const double* row = partials + (long)e * slabs;
    double s = 0.0;
    for (int k = lane; k < slabs; k += 64) s += row[k];
    s = lane_sum(s);
    if (lane == 0) {
        if (e < B * B) gram[e] = s;
        else sums[e - B * B] = s;
    }
}

// grid (1)
__global__ __launch_bounds__(HT) void head_kernel(const double* __restrict__ gx, const double* __restrict__ sx, const double* __restrict__ gz,
                                                  const float* __restrict__ lambda, int B, long N, int center, float* __restrict__ loss,
                                                  double* __restrict__ sim, float* __restrict__ mix, float* __restrict__ shift) {
    __shared__ double mean[simloss::B_MAX], gxd[simloss::B_MAX], gzd[simloss::B_MAX], rowl[simloss::B_MAX];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < B) {
        const double m = simloss::row_mean(center ? sx[tid] : 0.0, N, center);
        mean[tid] = m;
        gxd[tid] = simloss::centred(gx[tid * B + tid], N, m, m);
        gzd[tid] = gz[tid * B + tid];
    }
    __syncthreads();
    const double lam = (double)*lambda;
    const double w = simloss::pair_weight(lam, B);
    for (int i = wave; i < B; i += HW) {                       // a whole wave enters or none: the shuffles see all 64 lanes
        const int j = lane;
        const bool live = j < B;
        simloss::Pair p = {0.0, 0.0, 0.0, 0.0, 0.0};
        if (live) p = simloss::pair_terms(simloss::centred(gx[i * B + j], N, mean[i], mean[j]), gxd[i], gxd[j], gz[i * B + j], gzd[i], gzd[j], w, i == j);
        const double row_c = lane_sum(live ? p.c : 0.0);
        const double row_d2 = lane_sum(live ? p.d * p.d : 0.0);
        const double m = (i == j) ? simloss::mix_diagonal(row_c, gxd[i]) : p.m_off;
        const double row_r = lane_sum(live ? m * mean[j] : 0.0);
        if (live) {
            sim[i * B + j] = p.s;
            mix[i * B + j] = (float)m;
        }
        if (lane == 0) {
            shift[i] = (float)row_r;
            rowl[i] = row_d2;
        }
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int i = 0; i < B; ++i) total += rowl[i];
        *loss = (float)(w * total);
    }
}

template <int V> struct Vec;
template <> struct Vec<4> { typedef float4 type; };
template <> struct Vec<1> { typedef float type; };

// grid (ceil(N / V / NT)); BMAX bounds the registers: x[BMAX][V]
template <int BMAX, int V>
__global__ __launch_bounds__(NT) void mix_kernel(const float* __restrict__ x, const float* __restrict__ mix, const float* __restrict__ shift,
                                                 const float* __restrict__ upstream, const float* addend, float* grad, int B, long N) {
#pragma clang fp contract(off)
    __shared__ float m[BMAX * BMAX], r[BMAX];
    const int tid = threadIdx.x;
    for (int e = tid; e < B * B; e += NT) m[e] = mix[e];
    for (int e = tid; e < B; e += NT) r[e] = shift[e];
    __syncthreads();
    const long p = ((long)blockIdx.x * NT + tid) * V;
    if (p >= N) return;                                        // N % V == 0: a thread's V pixels are all inside or all outside
    const float up = *upstream;
    float xv[BMAX][V];
#pragma unroll
    for (int j = 0; j < BMAX; ++j) {
        if (j < B) {
            if constexpr (V == 4) {
                const float4 v = ld4(x + (long)j * N + p);
                xv[j][0] = v.x; xv[j][1] = v.y; xv[j][2] = v.z; xv[j][3] = v.w;
            } else {
                xv[j][0] = x[(long)j * N + p];
            }
        } else {
#pragma unroll
            for (int c = 0; c < V; ++c) xv[j][c] = 0.f;
        }
    }
    for (int i = 0; i < B; ++i) {
        float acc[V];
#pragma unroll
        for (int c = 0; c < V; ++c) acc[c] = 0.f;
#pragma unroll
        for (int j = 0; j < BMAX; ++j) {
            if (j < B) {
                const float mij = m[i * B + j];
#pragma unroll
                for (int c = 0; c < V; ++c) acc[c] = fmaf(mij, xv[j][c], acc[c]);
            }
        }
        const float ri = r[i];
        const long at = (long)i * N + p;
        float o[V];
#pragma unroll
        for (int c = 0; c < V; ++c) {
            const float centred = acc[c] - ri;
            o[c] = up * centred;
        }
        if constexpr (V == 4) {
            if (addend) {
                const float4 q = ld4(addend + at);
                o[0] = q.x + o[0]; o[1] = q.y + o[1]; o[2] = q.z + o[2]; o[3] = q.w + o[3];
            }
            st4(grad + at, make_float4(o[0], o[1], o[2], o[3]));
        } else {
            if (addend) o[0] = addend[at] + o[0];
            grad[at] = o[0];
        }
    }
}

bool shape_ok(const char* who, int B, long N) {
    if (B < simloss::B_MIN || B > simloss::B_MAX) {
        ngan::set_error("%s: B=%d unsupported (%d .. %d rows: a pair needs two, the head is one workgroup of 64 lanes a row)", who, B,
                        simloss::B_MIN, simloss::B_MAX);
        return false;
    }
    if (N < simloss::N_MIN || N >= simloss::N_LIMIT || N % 4 != 0) {
        ngan::set_error("%s: N=%ld unsupported (a multiple of 4, %ld <= N < 2^31)", who, N, simloss::N_MIN);
        return false;
    }
    return true;
}

template <int LANES>
void launch_gram(const float* rows, double* partials, int B, long N, const simloss::GramPlan& plan, hipStream_t s) {
    hipLaunchKernelGGL(gram_kernel<LANES>, dim3(plan.slabs), dim3(NT), 0, s, rows, partials, B, N, plan.chunk);
}

template <int BMAX, int V>
void launch_mix(const float* rows, const float* mix, const float* shift, const float* upstream, const float* addend, float* grad, int B,
                long N, hipStream_t s) {
    const long threads = N / V;
    hipLaunchKernelGGL((mix_kernel<BMAX, V>), dim3((unsigned)((threads + NT - 1) / NT)), dim3(NT), 0, s, rows, mix, shift, upstream, addend,
                       grad, B, N);
}

}  // namespace

extern "C" size_t nganx_pair_gram_workspace_bytes(int B, long N) {
    if (!simloss::shape_ok(B, N)) return 0;
    return (size_t)simloss::gram_plan(B, N).slabs * simloss::gram_elements(B) * sizeof(double);
}

extern "C" int nganx_pair_gram(const float* rows, double* gram, double* sums, void* workspace, int B, long N, void* stream) {
    NGAN_REQUIRE(rows, NGAN_ERR_ARG, "pair_gram: rows is a null pointer");
    NGAN_REQUIRE(gram, NGAN_ERR_ARG, "pair_gram: gram is a null pointer");
    NGAN_REQUIRE(sums, NGAN_ERR_ARG, "pair_gram: sums is a null pointer");
    NGAN_REQUIRE(workspace, NGAN_ERR_ARG, "pair_gram: workspace is a null pointer (nganx_pair_gram_workspace_bytes names its size)");
    if (!shape_ok("pair_gram", B, N)) return NGAN_ERR_SHAPE;
    NGAN_REQUIRE((uintptr_t)rows % 16 == 0, NGAN_ERR_ARG, "pair_gram: rows must start on a 16-byte boundary");
    NGAN_REQUIRE((uintptr_t)workspace % 16 == 0, NGAN_ERR_ARG, "pair_gram: workspace must start on a 16-byte boundary");
    NGAN_REQUIRE(((uintptr_t)gram | (uintptr_t)sums) % 8 == 0, NGAN_ERR_ARG, "pair_gram: gram and sums must start on an 8-byte boundary");
    const simloss::GramPlan plan = simloss::gram_plan(B, N);
    hipStream_t s = (hipStream_t)stream;
    double* partials = reinterpret_cast<double*>(workspace);
    switch (plan.lanes) {
        case 1: launch_gram<1>(rows, partials, B, N, plan, s); break;
        case 2: launch_gram<2>(rows, partials, B, N, plan, s); break;
        case 4: launch_gram<4>(rows, partials, B, N, plan, s); break;
        case 8: launch_gram<8>(rows, partials, B, N, plan, s); break;
        default: launch_gram<16>(rows, partials, B, N, plan, s); break;
    }
    const int M = (int)simloss::gram_elements(B);
    hipLaunchKernelGGL(gram_reduce_kernel, dim3((M + NT / 64 - 1) / (NT / 64)), dim3(NT), 0, s, partials, plan.slabs, B, gram, sums);
    return ngan::launch_status("nganx_pair_gram");
}

extern "C" int nganx_simloss_head(const double* gram_x, const double* sums_x, const double* gram_z, const float* lambda, int B, long N,
                                  int center, float* loss, double* sim, float* mix, float* shift, void* stream) {
    NGAN_REQUIRE(gram_x, NGAN_ERR_ARG, "simloss_head: gram_x is a null pointer");
    NGAN_REQUIRE(sums_x, NGAN_ERR_ARG, "simloss_head: sums_x is a null pointer");
    NGAN_REQUIRE(gram_z, NGAN_ERR_ARG, "simloss_head: gram_z is a null pointer");
    NGAN_REQUIRE(lambda, NGAN_ERR_ARG, "simloss_head: lambda is a null pointer (a device fp32 scalar)");
    NGAN_REQUIRE(loss && sim && mix && shift, NGAN_ERR_ARG, "simloss_head: an output (loss, sim, mix, shift) is a null pointer");
    if (!shape_ok("simloss_head", B, N)) return NGAN_ERR_SHAPE;
    NGAN_REQUIRE(((uintptr_t)gram_x | (uintptr_t)sums_x | (uintptr_t)gram_z | (uintptr_t)sim) % 8 == 0, NGAN_ERR_ARG,
                 "simloss_head: gram_x, sums_x, gram_z and sim must start on an 8-byte boundary");
    NGAN_REQUIRE(((uintptr_t)lambda | (uintptr_t)loss | (uintptr_t)mix | (uintptr_t)shift) % 4 == 0, NGAN_ERR_ARG,
                 "simloss_head: lambda, loss, mix and shift must start on a 4-byte boundary");
    hipLaunchKernelGGL(head_kernel, dim3(1), dim3(HT), 0, (hipStream_t)stream, gram_x, sums_x, gram_z, lambda, B, N, center != 0, loss, sim,
                       mix, shift);
    return ngan::launch_status("nganx_simloss_head");
}

extern "C" int nganx_pair_mix(const float* rows, const float* mix, const float* shift, const float* upstream, const float* addend_or_null,
                              float* grad, int B, long N, void* stream) {
    NGAN_REQUIRE(rows, NGAN_ERR_ARG, "pair_mix: rows is a null pointer");
    NGAN_REQUIRE(mix && shift, NGAN_ERR_ARG, "pair_mix: mix or shift is a null pointer");
    NGAN_REQUIRE(upstream, NGAN_ERR_ARG, "pair_mix: upstream is a null pointer (a device fp32 scalar)");
    NGAN_REQUIRE(grad, NGAN_ERR_ARG, "pair_mix: grad is a null pointer");
    if (!shape_ok("pair_mix", B, N)) return NGAN_ERR_SHAPE;
    NGAN_REQUIRE((uintptr_t)rows % 16 == 0, NGAN_ERR_ARG, "pair_mix: rows must start on a 16-byte boundary");
    NGAN_REQUIRE((uintptr_t)grad % 16 == 0, NGAN_ERR_ARG, "pair_mix: grad must start on a 16-byte boundary");
    NGAN_REQUIRE((uintptr_t)addend_or_null % 16 == 0, NGAN_ERR_ARG, "pair_mix: addend must start on a 16-byte boundary");
    NGAN_REQUIRE(((uintptr_t)mix | (uintptr_t)shift | (uintptr_t)upstream) % 4 == 0, NGAN_ERR_ARG,
                 "pair_mix: mix, shift and upstream must start on a 4-byte boundary");
    hipStream_t s = (hipStream_t)stream;
    if (B <= 4) launch_mix<4, 4>(rows, mix, shift, upstream, addend_or_null, grad, B, N, s);
    else if (B <= 8) launch_mix<8, 4>(rows, mix, shift, upstream, addend_or_null, grad, B, N, s);
    else if (B <= 16) launch_mix<16, 4>(rows, mix, shift, upstream, addend_or_null, grad, B, N, s);
    else if (B <= 32) launch_mix<32, 1>(rows, mix, shift, upstream, addend_or_null, grad, B, N, s);
    else launch_mix<64, 1>(rows, mix, shift, upstream, addend_or_null, grad, B, N, s);
    return ngan::launch_status("nganx_pair_mix");
}
