// Multi-scale structural similarity (Wang, Simoncelli and Bovik 2003) between pairs of images: the kernels behind metrics.msssim.
//   ngan_msssim_scale   scale_kernel: one workgroup per 32 x 32 tile of the valid (H - 10)^2 map of one pair.  Per colour channel the
//                       42 x 42 input tiles of both images (the tile and its 10-pixel halo; zeros past the image, which only masked
//                       outputs read) are staged in LDS, filtered along the rows with the 11-tap window for the five moments
//                       (a, b, a a, b b, a b) into LDS, then along the columns in registers; cs and ssim are formed per pixel in fp32
//                       and summed in fp64 per thread, per workgroup (block_sum256) and, in mean_kernel, per pair over the tiles in
//                       a fixed order.  No moment or map goes to HBM, no floating-point atomic: results are bit-reproducible, and a
//                       pair's values do not depend on which other pairs share the launch.
//   ngan_msssim_pool2   pool2_kernel: the 2 x 2 average of both images (the next scale), summed in fp64 and rounded once.
// Summation order (tests/msssim_cases.py emulates it): every 11-tap sum is acc = 0, then acc = fmaf(g[k], x[k], acc) for
// k = 0 .. 10, first along the row (k = column offset), then along the column (k = row offset); the products a a, b b, a b are
// rounded to fp32 before the row pass.  Variances and the covariance are one fused multiply-add each, fmaf(-mu_a, mu_b, E[a b]):
// the difference of the two rounded moments is itself rounded once.  Every fused multiply-add is an explicit fmaf and contraction
// is switched off for this file, so the plain operators round one by one and the order is the source's (left to the compiler,
// mu_a^2 + mu_b^2 became fma(mu_a, mu_a, mu_b^2), which is not symmetric in the two images; the __f*_rn functions do not help:
// they are plain operators of a header compiled with contraction on).  The fp32 division is the correctly rounded one.
#include <cmath>
#include "ngan_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int WIN = 11;                    // window taps
constexpr int HALO = WIN - 1;
constexpr int TO = 32;                     // output tile edge
constexpr int TI = TO + HALO;              // input tile edge: 42
constexpr int TP = TI + 1;                 // pitch of the input tiles: the row pass reads 8 rows x 4 strips per half wave, 43 r + 8 s
                                           // (r < 8, s < 4) are 32 different banks
constexpr int HP = TO + 1;                 // pitch of the row-filtered moments: the row pass stores at 33 r + 8 s + o, r + 8 s distinct
constexpr int STRIP = 8;                   // outputs per thread of the row pass
constexpr int VROWS = 4;                   // outputs per thread of the column pass (one column, four consecutive rows)

struct Window { float g[WIN]; };

// sum over the workgroup's 256 threads in a fixed order: butterfly inside each wave, then the four waves in order; thread 0 holds it
__device__ __forceinline__ double block_sum256(double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

template <int C>
__global__ __launch_bounds__(256) void scale_kernel(const float* __restrict__ a, const float* __restrict__ b, double* __restrict__ partials,
                                                    int H, int tiles, Window win, float C1, float C2) {
    __shared__ float ta[TI * TP], tb[TI * TP];
    __shared__ float hm[5][TI * HP];
    __shared__ double red[4];
    const int V = H - HALO;                                   // valid outputs per axis
    const int ty = blockIdx.x / tiles, tx = blockIdx.x - ty * tiles;
    const int oy0 = ty * TO, ox0 = tx * TO;
    const long img = (long)blockIdx.y * H * H * C;
    const int tid = threadIdx.x;
    const int vx = tid & (TO - 1), vy0 = (tid >> 5) * VROWS;  // column pass: this thread's column and first row
    double sum_cs = 0.0, sum_ssim = 0.0;
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        {                                                     // seven rounds of 256 tile entries: every load is issued before the
            constexpr int ROUNDS = (TI * TI + 255) / 256;     // first is stored (an entry past the image reads the pair's first
            float ra[ROUNDS], rb[ROUNDS];                     // value instead and stores zero)
#pragma unroll
            for (int i = 0; i < ROUNDS; ++i) {
                const int e = tid + i * 256, r = e / TI, x = e - r * TI;
                const int gy = oy0 + r, gx = ox0 + x;
                const long at = img + (gy < H && gx < H ? ((long)gy * H + gx) * C + c : 0);
                ra[i] = a[at];
                rb[i] = b[at];
            }
#pragma unroll
            for (int i = 0; i < ROUNDS; ++i) {
                const int e = tid + i * 256, r = e / TI, x = e - r * TI;
                const bool inside = oy0 + r < H && ox0 + x < H;
                if (e < TI * TI) {
                    ta[r * TP + x] = inside ? ra[i] : 0.0f;
                    tb[r * TP + x] = inside ? rb[i] : 0.0f;
                }
            }
        }
        __syncthreads();                                      // (also: every thread has left the previous channel's column pass)
        if (tid < TI * (TO / STRIP)) {                        // row pass: 42 rows x 4 strips of 8 outputs
            const int r = tid >> 2, s = tid & 3;
            const float* pa = ta + r * TP + s * STRIP;
            const float* pb = tb + r * TP + s * STRIP;
            float acc[5][STRIP];
#pragma unroll
            for (int m = 0; m < 5; ++m)
#pragma unroll
                for (int o = 0; o < STRIP; ++o) acc[m][o] = 0.0f;
#pragma unroll
            for (int k = 0; k < STRIP + HALO; ++k) {          // input k feeds output o with tap k - o: ascending taps per output
                const float x = pa[k], y = pb[k];
                const float xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
                for (int o = 0; o < STRIP; ++o) {
                    if (k - o >= 0 && k - o < WIN) {
                        const float g = win.g[k - o];
                        acc[0][o] = fmaf(g, x, acc[0][o]);
                        acc[1][o] = fmaf(g, y, acc[1][o]);
                        acc[2][o] = fmaf(g, xx, acc[2][o]);
                        acc[3][o] = fmaf(g, yy, acc[3][o]);
                        acc[4][o] = fmaf(g, xy, acc[4][o]);
                    }
                }
            }
#pragma unroll
            for (int m = 0; m < 5; ++m)
#pragma unroll
                for (int o = 0; o < STRIP; ++o) hm[m][r * HP + s * STRIP + o] = acc[m][o];
        }
        __syncthreads();
        {                                                     // column pass: 4 outputs of one column per thread
            float acc[5][VROWS];
#pragma unroll
            for (int m = 0; m < 5; ++m)
#pragma unroll
                for (int o = 0; o < VROWS; ++o) acc[m][o] = 0.0f;
#pragma unroll
            for (int k = 0; k < VROWS + HALO; ++k) {
                float v[5];
#pragma unroll
                for (int m = 0; m < 5; ++m) v[m] = hm[m][(vy0 + k) * HP + vx];
#pragma unroll
                for (int o = 0; o < VROWS; ++o) {
                    if (k - o >= 0 && k - o < WIN) {
                        const float g = win.g[k - o];
#pragma unroll
                        for (int m = 0; m < 5; ++m) acc[m][o] = fmaf(g, v[m], acc[m][o]);
                    }
                }
            }
#pragma unroll
            for (int o = 0; o < VROWS; ++o) {
                const float mu_a = acc[0][o], mu_b = acc[1][o];
                const float var_a = fmaf(-mu_a, mu_a, acc[2][o]);
                const float var_b = fmaf(-mu_b, mu_b, acc[3][o]);
                const float cov = fmaf(-mu_a, mu_b, acc[4][o]);
                const float cs = fmaf(2.0f, cov, C2) / ((var_a + var_b) + C2);
                const float l = fmaf(2.0f, mu_a * mu_b, C1) / ((mu_a * mu_a + mu_b * mu_b) + C1);
                const float ssim = l * cs;
                if (oy0 + vy0 + o < V && ox0 + vx < V) {      // rows ascending, channels ascending: this thread's fixed order
                    sum_cs += (double)cs;
                    sum_ssim += (double)ssim;
                }
            }
        }
    }
    const double t_cs = block_sum256(sum_cs, red);
    const double t_ssim = block_sum256(sum_ssim, red);
    if (tid == 0) {
        double* out = partials + ((long)blockIdx.y * gridDim.x + blockIdx.x) * 2;
        out[0] = t_cs;
        out[1] = t_ssim;
    }
}

// out[p] = {mean cs, mean ssim} of pair p: the pair's tiles summed in a fixed order, one workgroup per pair
__global__ __launch_bounds__(256) void mean_kernel(const double* __restrict__ partials, int ntiles, double count, double* __restrict__ out) {
    __shared__ double red[4];
    const double* p = partials + (long)blockIdx.x * ntiles * 2;
    for (int i = 0; i < 2; ++i) {
        double v = 0.0;
        for (int j = threadIdx.x; j < ntiles; j += 256) v += p[2 * j + i];
        const double t = block_sum256(v, red);
        if (threadIdx.x == 0) out[(long)blockIdx.x * 2 + i] = t / count;       // (a division: a map of ones has mean 1 exactly)
    }
}

// one thread per pooled value of both images; the four fp32 values are summed in fp64 (exact up to 29 binades of spread), one rounding
__global__ __launch_bounds__(256) void pool2_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ ao,
                                                    float* __restrict__ bo, int Ho, int C, long total) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const long rowlen = (long)Ho * C;                         // values per pooled row
    const long q = t % rowlen;                                // (x, c) inside the row
    const long pr = t / rowlen;                               // pair * Ho + pooled row
    const int x = (int)(q / C), c = (int)(q - (long)x * C);
    const long W = 2L * rowlen;                               // values per input row
    const long base = 2 * pr * W + (long)(2 * x) * C + c;     // (pair * 2 Ho + 2 y) input rows in
    const double sa = ((double)a[base] + (double)a[base + C]) + ((double)a[base + W] + (double)a[base + W + C]);
    const double sb = ((double)b[base] + (double)b[base + C]) + ((double)b[base + W] + (double)b[base + W + C]);
    ao[t] = (float)(0.25 * sa);
    bo[t] = (float)(0.25 * sb);
}

bool pow2(long v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace

extern "C" int ngan_msssim_window(float* window11) {
    NGAN_REQUIRE(window11, NGAN_ERR_ARG, "msssim_window: null pointer");
    double g[WIN], sum = 0.0;
    for (int i = 0; i < WIN; ++i) {
        g[i] = std::exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        sum += g[i];
    }
    for (int i = 0; i < WIN; ++i) window11[i] = (float)(g[i] / sum);
    return NGAN_OK;
}

extern "C" size_t ngan_msssim_workspace_bytes(int P, int H) {
    if (P <= 0 || H < 16 || !pow2(H)) return 0;
    const size_t tiles = (size_t)ngan::ceil_div(H - HALO, TO);
    return (size_t)P * tiles * tiles * 2 * sizeof(double);
}

extern "C" int ngan_msssim_scale(const float* a, const float* b, double* out, void* workspace, int P, int H, int C, double data_range,
                                 void* stream) {
    NGAN_REQUIRE(a && b && out && workspace, NGAN_ERR_ARG, "msssim_scale: null pointer");
    NGAN_REQUIRE(C == 1 || C == 3, NGAN_ERR_SHAPE, "msssim_scale: C=%d unsupported (1 or 3 colour channels)", C);
    NGAN_REQUIRE(H >= 16 && H <= 32768 && pow2(H), NGAN_ERR_SHAPE,
                 "msssim_scale: H=%d unsupported (a power of two, 16 .. 32768: the 11 x 11 window needs a valid map)", H);
    NGAN_REQUIRE(P > 0 && P < 65536, NGAN_ERR_SHAPE, "msssim_scale: P=%d unsupported (1 .. 65535 pairs per call)", P);
    NGAN_REQUIRE(data_range > 0.0 && std::isfinite(data_range), NGAN_ERR_ARG, "msssim_scale: data_range=%g must be positive", data_range);
    Window win;
    ngan_msssim_window(win.g);
    const float C1 = (float)((0.01 * data_range) * (0.01 * data_range)), C2 = (float)((0.03 * data_range) * (0.03 * data_range));
    const int V = H - HALO, tiles = ngan::ceil_div(V, TO);
    hipStream_t s = (hipStream_t)stream;
    double* partials = reinterpret_cast<double*>(workspace);
    const dim3 grid(tiles * tiles, P);
    if (C == 1) hipLaunchKernelGGL(scale_kernel<1>, grid, dim3(256), 0, s, a, b, partials, H, tiles, win, C1, C2);
    else hipLaunchKernelGGL(scale_kernel<3>, grid, dim3(256), 0, s, a, b, partials, H, tiles, win, C1, C2);
    hipLaunchKernelGGL(mean_kernel, dim3(P), dim3(256), 0, s, partials, tiles * tiles, (double)V * (double)V * (double)C, out);
    return ngan::launch_status("ngan_msssim_scale");
}

extern "C" int ngan_msssim_pool2(const float* a, const float* b, float* a_out, float* b_out, int P, int H, int C, void* stream) {
    NGAN_REQUIRE(a && b && a_out && b_out, NGAN_ERR_ARG, "msssim_pool2: null pointer");
    NGAN_REQUIRE(C == 1 || C == 3, NGAN_ERR_SHAPE, "msssim_pool2: C=%d unsupported (1 or 3 colour channels)", C);
    NGAN_REQUIRE(H >= 2 && H <= 32768 && pow2(H), NGAN_ERR_SHAPE, "msssim_pool2: H=%d unsupported (a power of two, 2 .. 32768)", H);
    NGAN_REQUIRE(P > 0, NGAN_ERR_SHAPE, "msssim_pool2: P=%d must be positive", P);
    const int Ho = H / 2;
    const long total = (long)P * Ho * Ho * C;
    NGAN_REQUIRE((total + 255) / 256 < (1L << 31), NGAN_ERR_SHAPE, "msssim_pool2: %ld pooled values in one call", total);
    hipLaunchKernelGGL(pool2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, a_out, b_out, Ho, C,
                       total);
    return ngan::launch_status("ngan_msssim_pool2");
}
