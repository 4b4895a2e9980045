// Geometric differentiable augmentation of the critic's inputs: mirror, quarter turns, isotropic scale and rotation as one bilinear
// resampling per sample, and its adjoint for the generator step (Karras et al. 2020, "Training generative adversarial networks with
// limited data": the pixel-blitting and geometric groups, at a fixed probability).  include/ngan_geoaug.h and DESIGN.md section 7 hold
// the definition; tests/diffgeo_cases.py restates it in fp64; the per-pixel arithmetic is csrc/diffgeo_bits.h.
//   ngan_diffgeo_params  params_kernel: one thread per sample maps eight uniforms to the sample's affine row (formed in double).
//   ngan_diffgeo_fwd     fwd_kernel: a thread owns four consecutive output pixels of a row: four source cells, sixteen cached gathers,
//                        one float4 store.
//   ngan_diffgeo_bwd     bwd_kernel: a thread owns one INPUT pixel, derives the window of output pixels that can read it, visits them
//                        in row-major order and adds where the recomputed cell touches its pixel.  No atomics: bit-reproducible, a
//                        sample's values do not depend on the rest of the batch, and the weights are the forward pass's own.
// Values are fp32 in memory; coordinates, fractions, weights and sums are double, rounded to fp32 once per element (an fp32 coordinate
// would put up to 2^-24 |s| of a pixel into every fraction: more than the whole blend's rounding).  Contraction is off: the fused
// operations are the explicit fma of the two coordinates.
#include <cstdint>
#include "ngan_common.h"
#include "../../include/ngan_geoaug.h"
#include "../../include/ngada.h"

#pragma clang fp contract(off)
#include "diffgeo_bits.h"

namespace {

constexpr int FWD_TILE = 1024;             // elements per workgroup of the forward pass: 256 threads x 1 float4
constexpr int BWD_TILE = 256;              // elements per workgroup of the adjoint: one per thread

// LIVE: the probability is the device scalar p_live[0] (include/ngada.h), read by every thread; otherwise the argument p_value
template <bool LIVE>
__global__ __launch_bounds__(256) void params_kernel(const float* __restrict__ u, geo::Row* __restrict__ rows, int B, int R, int policy,
                                                     float p_value, const float* __restrict__ p_live) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= B) return;
    rows[n] = geo::geo_params(u + (long)n * 8, R, policy, LIVE ? p_live[0] : p_value);
}

__global__ __launch_bounds__(256) void fwd_kernel(const float* __restrict__ x, const geo::Row* __restrict__ rows, float* __restrict__ y,
                                                  int N, int R, float fill) {
    const int n = blockIdx.y;
    const long el = (long)blockIdx.x * FWD_TILE + threadIdx.x * 4;            // N is a multiple of 16: a float4 is inside or outside
    if (el >= N) return;
    const int e = (int)el;
    const geo::Row r = rows[n];
    const int row = e / R, j = e - row * R, i = row % R;                    // (channel * R + i, j): R % 4 == 0, so one row per float4
    const float* plane = x + (long)n * N + (long)(row - i) * R;
    float w[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) w[a] = geo::geo_forward(plane, r, R, i, j + a, fill);
    st4(y + (long)n * N + e, make_float4(w[0], w[1], w[2], w[3]));
}

__global__ __launch_bounds__(256) void bwd_kernel(const float* __restrict__ gy, const geo::Row* __restrict__ rows, float* __restrict__ gx,
                                                  int N, int R) {
    const int n = blockIdx.y;
    const long el = (long)blockIdx.x * BWD_TILE + threadIdx.x;
    if (el >= N) return;
    const int e = (int)el;
    const geo::Row r = rows[n];
    const int row = e / R, j = e - row * R, i = row % R;
    gx[(long)n * N + e] = geo::geo_adjoint(gy + (long)n * N + (long)(row - i) * R, r, R, i, j);
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

int check_images(const char* what, const float* in, const void* table, float* out, int B, int C, int H, int W, int table_rows) {
    NGAN_REQUIRE(in && table && out, NGAN_ERR_ARG, "%s: null pointer", what);
    if (int st = check_shape(what, B, C, H, W, table_rows)) return st;
    NGAN_REQUIRE(aligned16(in) && aligned16(out) && aligned16(table), NGAN_ERR_ARG,
                 "%s: images and the table must start on a 16-byte boundary", what);
    return NGAN_OK;
}

}  // namespace

extern "C" int ngan_diffgeo_params(const float* uniforms, void* table, int B, int H, int W, int table_rows, int policy, float p,
                                   void* stream) {
    NGAN_REQUIRE(uniforms && table, NGAN_ERR_ARG, "diffgeo_params: null pointer");
    if (int st = check_shape("diffgeo_params", B, 1, H, W, table_rows)) return st;
    NGAN_REQUIRE(aligned16(table), NGAN_ERR_ARG, "diffgeo_params: the table must start on a 16-byte boundary");
    NGAN_REQUIRE(policy >= 0 && policy < 4, NGAN_ERR_ARG, "diffgeo_params: policy mask %d (bits 1 blit, 2 geometry)", policy);
    NGAN_REQUIRE(p >= 0.f && p <= 1.f, NGAN_ERR_ARG, "diffgeo_params: p=%g must lie in [0, 1]", (double)p);
    hipLaunchKernelGGL(params_kernel<false>, dim3(ngan::ceil_div(B, 256)), dim3(256), 0, (hipStream_t)stream, uniforms,
                       reinterpret_cast<geo::Row*>(table), B, H, policy, p, (const float*)nullptr);
    return ngan::launch_status("ngan_diffgeo_params");
}

// the same mapping with the probability in device memory (include/ngada.h): no range check, the host does not know the value
extern "C" int ngada_diffgeo_params(const float* uniforms, void* table, int B, int H, int W, int table_rows, int policy, const float* p,
                                    void* stream) {
    NGAN_REQUIRE(uniforms && table, NGAN_ERR_ARG, "ngada_diffgeo_params: null pointer");
    NGAN_REQUIRE(p, NGAN_ERR_ARG, "ngada_diffgeo_params: p is a null pointer");
    if (int st = check_shape("ngada_diffgeo_params", B, 1, H, W, table_rows)) return st;
    NGAN_REQUIRE(aligned16(table), NGAN_ERR_ARG, "ngada_diffgeo_params: the table must start on a 16-byte boundary");
    NGAN_REQUIRE(policy >= 0 && policy < 4, NGAN_ERR_ARG, "ngada_diffgeo_params: policy mask %d (bits 1 blit, 2 geometry)", policy);
    hipLaunchKernelGGL(params_kernel<true>, dim3(ngan::ceil_div(B, 256)), dim3(256), 0, (hipStream_t)stream, uniforms,
                       reinterpret_cast<geo::Row*>(table), B, H, policy, 0.f, p);
    return ngan::launch_status("ngada_diffgeo_params");
}

extern "C" int ngan_diffgeo_fwd(const float* x, const void* table, float* y, int B, int C, int H, int W, int table_rows, float fill,
                                void* stream) {
    if (int st = check_images("ngan_diffgeo_fwd", x, table, y, B, C, H, W, table_rows)) return st;
    NGAN_REQUIRE(fill == fill && fill - fill == 0.f, NGAN_ERR_ARG, "ngan_diffgeo_fwd: fill=%g must be finite", (double)fill);
    const int N = C * H * H;
    hipLaunchKernelGGL(fwd_kernel, dim3(ngan::ceil_div(N, FWD_TILE), B), dim3(256), 0, (hipStream_t)stream, x,
                       reinterpret_cast<const geo::Row*>(table), y, N, H, fill);
    return ngan::launch_status("ngan_diffgeo_fwd");
}

extern "C" int ngan_diffgeo_bwd(const float* gy, const void* table, float* gx, int B, int C, int H, int W, int table_rows, void* stream) {
    if (int st = check_images("ngan_diffgeo_bwd", gy, table, gx, B, C, H, W, table_rows)) return st;
    const int N = C * H * H;
    hipLaunchKernelGGL(bwd_kernel, dim3(ngan::ceil_div(N, BWD_TILE), B), dim3(256), 0, (hipStream_t)stream, gy,
                       reinterpret_cast<const geo::Row*>(table), gx, N, H);
    return ngan::launch_status("ngan_diffgeo_bwd");
}
