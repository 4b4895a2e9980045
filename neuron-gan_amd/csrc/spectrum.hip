// Radial power spectrum of images (Durall et al. 2020): the kernels behind metrics.radial_spectrum.  A batched two-dimensional real
// transform in LDS, |F|^2 binned into integer rings in fp64; no vendor FFT library, no atomics, no workspace state between calls.
//   row_kernel   one workgroup per ROWS consecutive rows of one image and colour channel (ROWS = 16 from R = 128 on; 32 at R = 32
//                and 64; 16 at R = 16).  float4 loads along the rows (for C = 3 the other two channels' lanes are skipped), the Hann
//                window applied on load (w = h[y] h[x] one product, x w one product), rows 2t and 2t+1 packed as re + i im of one
//                complex length-R transform (real-input symmetry), transformed in LDS, split by A[v] = (Z[v] + conj Z[R-v]) / 2,
//                B[v] = (Z[v] - conj Z[R-v]) / 2i, and the Hermitian half v = 0 .. R/2 written transposed, G[b][c][v][y]: a run of
//                ROWS float2 per v, 128 bytes and more.
//   col_kernel   one workgroup per COLS = ROWS / 2 consecutive columns v of one image and channel: a contiguous block of G, float4
//                loads (columns past R/2 in the last workgroup are zero fill and take part in nothing), the transform along y in
//                LDS, then |F|^2 = re re + im im in fp32 and the ring sums in fp64.  Thread k owns bin k (and k + 256, k + 512): for
//                every column of the tile, ascending, it finds the interval of |u| whose d = u^2 + v^2 falls in ring k in integers
//                ((2k-1)^2 <= 4d < (2k+1)^2) and adds the negative frequencies, ascending, then the positive ones, with Hermitian
//                weight 2 for 0 < v < R/2 and 1 for v = 0 and v = R/2.  One thread per bin and one fixed order: the workgroup's
//                partial needs no combination across threads; it goes to the workspace.  With `power` the tile is also stored as
//                P = |F|^2 / norm, (B, C, R, R/2 + 1) fp32, divided in fp64 and rounded once.
//   fold_kernel  radial[b][k] = (sum over channels, then column groups, ascending, of the partials) / (C n_k norm); n_k is counted
//                from the same interval function.
// The transform is Stockham's autosort form, radix 4 with one radix-2 stage at the end for odd log2 R; every butterfly reads its
// inputs, waits at a barrier and writes in place, so one buffer of COLS x (R + 2) float2 serves (the pad keeps the split step's and
// the power store's column-strided reads on different banks).  Twiddles: a table exp(-2 pi i k / R), k < R, built in LDS at kernel
// start from sincospi in double and rounded once (exact on the axes); the window taps are built the same way, 0.5 - 0.5 cospi(2 i / R)
// in double, rounded once.  Contraction is switched off for this file (`#pragma clang fp contract(off)`) and there is no fmaf: every
// fp32 product, sum and difference rounds on its own, in the source's order -- a complex product is (wr tr - wi ti, wr ti + wi tr)
// -- and tests/spectrum_cases.py emulates exactly that.  Only plain C++: no inline assembly.
#include <cmath>
#include <cstdint>
#include "ngan_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                                        // threads per workgroup

constexpr int rows_of(int R) { return R >= 128 ? 16 : (R >= 32 ? 32 : 16); }
constexpr int pitch_of(int R) { return R + 2; }                // float2 per transform in LDS

// floor(sqrt(n)), n < 2^24: the float estimate settled in integers
__host__ __device__ inline int isqrt_floor(int n) {
    int r = (int)sqrtf((float)n);
    while (r * r > n) --r;
    while ((r + 1) * (r + 1) <= n) ++r;
    return r;
}

// the |u| of ring k in column v: lo <= |u| <= hi are those with (2k-1)^2 <= 4 (u^2 + v^2) < (2k+1)^2 (k = 0: d = 0 alone), cut to R/2;
// false if there is none
__host__ __device__ inline bool ring_interval(int k, int v, int half, int& lo, int& hi) {
    const int v4 = 4 * v * v;
    const int upper = (2 * k + 1) * (2 * k + 1) - v4;          // 4 u^2 < upper
    if (upper <= 0) return false;
    hi = isqrt_floor((upper - 1) / 4);
    if (hi > half) hi = half;
    const int lower = (k == 0 ? 0 : (2 * k - 1) * (2 * k - 1)) - v4;   // 4 u^2 >= lower
    if (lower <= 0) lo = 0;
    else {
        const int q = (lower + 3) / 4;                         // u^2 >= q
        lo = isqrt_floor(q);
        if (lo * lo < q) ++lo;
    }
    return lo <= hi;
}

// frequencies of ring k in the full plane u, v in [-half, half): what the half plane's weights add up to
__host__ __device__ inline int ring_count(int k, int half) {
    int n = 0;
    for (int v = 0; v <= half; ++v) {
        int lo, hi;
        if (!ring_interval(k, v, half, lo, hi)) continue;
        const int neg = hi - (lo > 1 ? lo : 1) + 1;            // u = -hi .. -max(lo, 1)
        const int top = hi < half - 1 ? hi : half - 1;         // u = lo .. min(hi, half - 1)
        const int cnt = (neg > 0 ? neg : 0) + (top >= lo ? top - lo + 1 : 0);
        n += (v == 0 || v == half) ? cnt : 2 * cnt;
    }
    return n;
}

__device__ __forceinline__ float2 cmul(float2 w, float2 t) { return make_float2(w.x * t.x - w.y * t.y, w.x * t.y + w.y * t.x); }

// tw[k] = exp(-2 pi i k / R), k < R
template <int R>
__device__ __forceinline__ void build_twiddles(float2* tw) {
    for (int k = threadIdx.x; k < R; k += NT) {
        double s, c;
        sincospi(2.0 * (double)k / (double)R, &s, &c);
        tw[k] = make_float2((float)c, (float)(-s));
    }
}

// T transforms of length R in place, transform t at buf + t * pitch_of(R); the caller has synchronised the workgroup after filling
// buf and tw, and finds it synchronised on return
template <int R, int T>
__device__ __forceinline__ void fft_lds(float2* buf, const float2* tw) {
    constexpr int P = pitch_of(R);
    constexpr int BF4 = T * R / 4;                             // radix-4 butterflies per stage
    constexpr int NB4 = (BF4 + NT - 1) / NT;
    const int tid = threadIdx.x;
    int n = R, s = 1;
#pragma unroll
    for (; n >= 4; n >>= 2, s <<= 2) {
        float2 a[NB4], b[NB4], c[NB4], d[NB4];
#pragma unroll
        for (int i = 0; i < NB4; ++i) {
            const int e = tid + i * NT;
            if (e < BF4) {
                const int t = e / (R / 4), j = e % (R / 4);    // x[q + s (p + m n1)] = x[j + m R/4]
                const float2* x = buf + t * P + j;
                a[i] = x[0];
                b[i] = x[R / 4];
                c[i] = x[R / 2];
                d[i] = x[3 * R / 4];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NB4; ++i) {
            const int e = tid + i * NT;
            if (e < BF4) {
                const int t = e / (R / 4), j = e % (R / 4);
                const int p = j / s, q = j - p * s;
                const float2 apc = make_float2(a[i].x + c[i].x, a[i].y + c[i].y);
                const float2 amc = make_float2(a[i].x - c[i].x, a[i].y - c[i].y);
                const float2 bpd = make_float2(b[i].x + d[i].x, b[i].y + d[i].y);
                const float2 jbmd = make_float2(-(b[i].y - d[i].y), b[i].x - d[i].x);
                float2* y = buf + t * P + q + s * 4 * p;
                y[0] = make_float2(apc.x + bpd.x, apc.y + bpd.y);
                y[s] = cmul(tw[p * s], make_float2(amc.x - jbmd.x, amc.y - jbmd.y));
                y[2 * s] = cmul(tw[2 * p * s], make_float2(apc.x - bpd.x, apc.y - bpd.y));
                y[3 * s] = cmul(tw[3 * p * s], make_float2(amc.x + jbmd.x, amc.y + jbmd.y));
            }
        }
        __syncthreads();
    }
    if (n == 2) {                                              // s = R / 2: y[q] = x[q] + x[q + s], y[q + s] = x[q] - x[q + s]
        constexpr int BF2 = T * R / 2;
        constexpr int NB2 = (BF2 + NT - 1) / NT;
        float2 a[NB2], b[NB2];
#pragma unroll
        for (int i = 0; i < NB2; ++i) {
            const int e = tid + i * NT;
            if (e < BF2) {
                const float2* x = buf + (e / (R / 2)) * P + e % (R / 2);
                a[i] = x[0];
                b[i] = x[R / 2];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NB2; ++i) {
            const int e = tid + i * NT;
            if (e < BF2) {
                float2* y = buf + (e / (R / 2)) * P + e % (R / 2);
                y[0] = make_float2(a[i].x + b[i].x, a[i].y + b[i].y);
                y[R / 2] = make_float2(a[i].x - b[i].x, a[i].y - b[i].y);
            }
        }
        __syncthreads();
    }
}

// grid (R / ROWS, C, B)
template <int R, int C>
__global__ __launch_bounds__(NT) void row_kernel(const float* __restrict__ images, float2* __restrict__ G, int window) {
    constexpr int ROWS = rows_of(R), T = ROWS / 2, P = pitch_of(R), K = R / 2 + 1;
    __shared__ __attribute__((aligned(16))) float2 buf[T * P];
    __shared__ float2 tw[R];
    __shared__ float h[R];
    const int tid = threadIdx.x;
    const int y0 = blockIdx.x * ROWS, c = blockIdx.y;
    const long b = blockIdx.z;
    build_twiddles<R>(tw);
    if (window) {
        for (int i = tid; i < R; i += NT) h[i] = (float)(0.5 - 0.5 * cospi(2.0 * (double)i / (double)R));
        __syncthreads();
    }
    {                                                          // ROWS consecutive rows are one contiguous block of ROWS R C floats
        const float* src = images + (b * R + y0) * (long)R * C;
        float* flat = reinterpret_cast<float*>(buf);
        for (int e4 = tid; e4 < ROWS * R * C / 4; e4 += NT) {
            const float4 v4 = ld4(src + 4 * e4);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int f = 4 * e4 + m, pix = f / C;
                if (C == 1 || f - pix * C == c) {
                    const int r = pix / R, x = pix - r * R;    // row r of the group: transform r / 2, part r & 1
                    float val = v[m];
                    if (window) {
                        const float w = h[y0 + r] * h[x];
                        val = val * w;
                    }
                    flat[2 * ((r >> 1) * P + x) + (r & 1)] = val;
                }
            }
        }
    }
    __syncthreads();
    fft_lds<R, T>(buf, tw);
    float2* out = G + ((b * C + c) * K) * (long)R + y0;        // G[b][c][v][y0 + r]
    for (int e = tid; e < K * ROWS; e += NT) {
        const int v = e / ROWS, r = e - v * ROWS;
        const float2 z = buf[(r >> 1) * P + v], w = buf[(r >> 1) * P + ((R - v) & (R - 1))];
        const float2 g = (r & 1) ? make_float2((z.y + w.y) * 0.5f, (w.x - z.x) * 0.5f) : make_float2((z.x + w.x) * 0.5f, (z.y - w.y) * 0.5f);
        out[(long)v * R + r] = g;
    }
}

// grid (ceil(K / COLS), C, B)
template <int R>
__global__ __launch_bounds__(NT) void col_kernel(const float2* __restrict__ G, double* __restrict__ partials, float* __restrict__ power,
                                                 double norm) {
    constexpr int T = rows_of(R) / 2, P = pitch_of(R), K = R / 2 + 1, HALF = R / 2;
    __shared__ __attribute__((aligned(16))) float2 buf[T * P];
    __shared__ float2 tw[R];
    const int tid = threadIdx.x;
    const int v0 = blockIdx.x * T;
    const int valid = K - v0 < T ? K - v0 : T;                 // columns of this tile that exist
    const long plane = (long)blockIdx.z * gridDim.y + blockIdx.y;
    build_twiddles<R>(tw);
    {
        const float2* src = G + (plane * K + v0) * (long)R;    // columns v0 .. v0 + valid: one contiguous block
        for (int e2 = tid; e2 < T * R / 2; e2 += NT) {         // two complex values per load
            const int t = (2 * e2) / R, y = 2 * e2 - t * R;
            float4 v = f4zero();
            if (t < valid) v = ld4(reinterpret_cast<const float*>(src + 2 * e2));
            *reinterpret_cast<float4*>(buf + t * P + y) = v;
        }
    }
    __syncthreads();
    fft_lds<R, T>(buf, tw);
    double* part = partials + (plane * gridDim.x + blockIdx.x) * (long)K;
    for (int k = tid; k < K; k += NT) {
        double acc = 0.0;
        for (int t = 0; t < valid; ++t) {
            const int v = v0 + t;
            int lo, hi;
            if (!ring_interval(k, v, HALF, lo, hi)) continue;
            const float2* col = buf + t * P;
            double sum = 0.0;
            for (int u = -hi; u <= -(lo > 1 ? lo : 1); ++u) {
                const float2 z = col[u + R];
                const float m = z.x * z.x + z.y * z.y;
                sum += (double)m;
            }
            const int top = hi < HALF - 1 ? hi : HALF - 1;
            for (int u = lo; u <= top; ++u) {
                const float2 z = col[u];
                const float m = z.x * z.x + z.y * z.y;
                sum += (double)m;
            }
            acc += (v == 0 || v == HALF) ? sum : 2.0 * sum;
        }
        part[k] = acc;
    }
    if (power) {
        float* out = power + plane * (long)R * K;              // [fy][fx]
        for (int e = tid; e < R * T; e += NT) {
            const int fy = e / T, t = e - fy * T;
            if (t < valid) {
                const float2 z = buf[t * P + fy];
                const float m = z.x * z.x + z.y * z.y;
                out[(long)fy * K + v0 + t] = (float)((double)m / norm);
            }
        }
    }
}

// grid (B): radial[b][k]
__global__ __launch_bounds__(NT) void fold_kernel(const double* __restrict__ partials, double* __restrict__ radial, int R, int C, int groups,
                                                  double norm) {
    const int K = R / 2 + 1;
    const double* p = partials + (long)blockIdx.x * C * groups * K;
    for (int k = threadIdx.x; k < K; k += NT) {
        double acc = 0.0;
        for (int j = 0; j < C * groups; ++j) acc += p[(long)j * K + k];
        radial[(long)blockIdx.x * K + k] = acc / ((double)(C * ring_count(k, R / 2)) * norm);
    }
}

bool supported(int R) { return R >= 16 && R <= 1024 && (R & (R - 1)) == 0; }
int col_groups(int R) { return ngan::ceil_div(R / 2 + 1, rows_of(R) / 2); }
size_t half_plane_bytes(int B, int R, int C) { return (size_t)B * C * (R / 2 + 1) * R * sizeof(float2); }

template <int R>
void launch(const float* images, double* radial, float* power, void* workspace, int B, int C, int window, double norm, hipStream_t s) {
    float2* G = reinterpret_cast<float2*>(workspace);
    double* partials = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + half_plane_bytes(B, R, C));
    const dim3 rows(R / rows_of(R), C, B), cols(col_groups(R), C, B);
    if (C == 1) hipLaunchKernelGGL((row_kernel<R, 1>), rows, dim3(NT), 0, s, images, G, window);
    else hipLaunchKernelGGL((row_kernel<R, 3>), rows, dim3(NT), 0, s, images, G, window);
    hipLaunchKernelGGL(col_kernel<R>, cols, dim3(NT), 0, s, G, partials, power, norm);
    hipLaunchKernelGGL(fold_kernel, dim3(B), dim3(NT), 0, s, partials, radial, R, C, col_groups(R), norm);
}

}  // namespace

extern "C" int ngan_spectrum_window(float* taps, int R) {
    NGAN_REQUIRE(taps, NGAN_ERR_ARG, "spectrum_window: null pointer");
    NGAN_REQUIRE(supported(R), NGAN_ERR_SHAPE, "spectrum_window: R=%d unsupported (a power of two, 16 .. 1024)", R);
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < R; ++i) taps[i] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)i / (double)R));
    return NGAN_OK;
}

extern "C" int ngan_spectrum_ring_counts(int* counts, int R) {
    NGAN_REQUIRE(counts, NGAN_ERR_ARG, "spectrum_ring_counts: null pointer");
    NGAN_REQUIRE(supported(R), NGAN_ERR_SHAPE, "spectrum_ring_counts: R=%d unsupported (a power of two, 16 .. 1024)", R);
    const int half = R / 2;
    for (int k = 0; k <= half; ++k) counts[k] = 0;
    for (int u = -half; u < half; ++u)                         // the definition itself, over the whole plane
        for (int v = -half; v < half; ++v) {
            const long d4 = 4L * (u * u + v * v);
            long k = (long)std::floor(std::sqrt((double)(u * u + v * v)) + 0.5);
            while (k > 0 && (2 * k - 1) * (2 * k - 1) > d4) --k;
            while ((2 * k + 1) * (2 * k + 1) <= d4) ++k;
            if (k <= half) ++counts[k];
        }
    return NGAN_OK;
}

extern "C" size_t ngan_spectrum_workspace_bytes(int B, int R, int C) {
    if (B <= 0 || B > 65535 || !supported(R) || (C != 1 && C != 3)) return 0;
    return half_plane_bytes(B, R, C) + (size_t)B * C * col_groups(R) * (R / 2 + 1) * sizeof(double);
}

extern "C" int ngan_spectrum_radial(const float* images, double* radial, float* power_or_null, void* workspace, int B, int R, int C,
                                    int window, void* stream) {
    NGAN_REQUIRE(images && radial, NGAN_ERR_ARG, "spectrum_radial: null pointer");
    NGAN_REQUIRE(workspace, NGAN_ERR_ARG, "spectrum_radial: null workspace (ngan_spectrum_workspace_bytes names its size)");
    NGAN_REQUIRE(supported(R), NGAN_ERR_SHAPE, "spectrum_radial: R=%d unsupported (a power of two, 16 .. 1024)", R);
    NGAN_REQUIRE(C == 1 || C == 3, NGAN_ERR_SHAPE, "spectrum_radial: C=%d unsupported (1 or 3 colour channels)", C);
    NGAN_REQUIRE(B > 0 && B < 65536, NGAN_ERR_SHAPE, "spectrum_radial: B=%d unsupported (1 .. 65535 images per call)", B);
    NGAN_REQUIRE(((uintptr_t)images | (uintptr_t)workspace | (uintptr_t)power_or_null) % 16 == 0 && (uintptr_t)radial % 8 == 0,
                 NGAN_ERR_ARG, "spectrum_radial: images, power and workspace must start on a 16-byte boundary, radial on an 8-byte one");
    double norm = (double)R * (double)R;
    if (window) {
        float taps[1024];
        ngan_spectrum_window(taps, R);
        double s = 0.0;
        for (int i = 0; i < R; ++i) s += (double)taps[i] * (double)taps[i];
        norm = s * s;
    }
    hipStream_t s = (hipStream_t)stream;
    switch (R) {
        case 16: launch<16>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
        case 32: launch<32>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
        case 64: launch<64>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
        case 128: launch<128>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
        case 256: launch<256>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
        case 512: launch<512>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
        default: launch<1024>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
    }
    return ngan::launch_status("ngan_spectrum_radial");
}
