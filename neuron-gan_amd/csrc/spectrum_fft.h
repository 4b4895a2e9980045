// The batched transform in LDS and the three kernels of the radial power spectrum, shared by csrc/spectrum.hip (the metric) and
// csrc/specloss.hip (the generator's spectral loss); the description of the kernels and of the arithmetic is at the top of
// csrc/spectrum.hip.  Contraction is off from here to the end of the including file: every fp32 operation rounds on its own.
#pragma once
#include <cmath>
#include <cstdint>
#include "ngan_common.h"
#include "spectrum_ring.h"

#pragma clang fp contract(off)

namespace {

constexpr int NT = 256;                                        // threads per workgroup

constexpr int rows_of(int R) { return R >= 128 ? 16 : (R >= 32 ? 32 : 16); }
constexpr int pitch_of(int R) { return R + 2; }                // float2 per transform in LDS

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

// grid (ceil(K / COLS), C, B); keep (or null): the half-plane transform itself, laid out as G is, F[b][c][v][fy]
template <int R>
__global__ __launch_bounds__(NT) void col_kernel(const float2* __restrict__ G, double* __restrict__ partials, float* __restrict__ power,
                                                 float2* __restrict__ keep, double norm) {
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
    if (keep) {
        float2* dst = keep + (plane * K + v0) * (long)R;
        for (int e2 = tid; e2 < T * R / 2; e2 += NT) {
            const int t = (2 * e2) / R, y = 2 * e2 - t * R;
            if (t < valid) st4(reinterpret_cast<float*>(dst + 2 * e2), *reinterpret_cast<const float4*>(buf + t * P + y));
        }
    }
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

// grid (B): radial[b][k]; ring_norm (or null): the divisor of every bin, C n_k norm, written once (by the first image's workgroup)
__global__ __launch_bounds__(NT) void fold_kernel(const double* __restrict__ partials, double* __restrict__ radial,
                                                  double* __restrict__ ring_norm, int R, int C, int groups, double norm) {
    const int K = R / 2 + 1;
    const double* p = partials + (long)blockIdx.x * C * groups * K;
    for (int k = threadIdx.x; k < K; k += NT) {
        double acc = 0.0;
        for (int j = 0; j < C * groups; ++j) acc += p[(long)j * K + k];
        const double den = (double)(C * ring_count(k, R / 2)) * norm;
        radial[(long)blockIdx.x * K + k] = acc / den;
        if (ring_norm && blockIdx.x == 0) ring_norm[k] = den;
    }
}

bool supported(int R) { return R >= 16 && R <= 1024 && (R & (R - 1)) == 0; }
int col_groups(int R) { return ngan::ceil_div(R / 2 + 1, rows_of(R) / 2); }
size_t half_plane_bytes(int B, int R, int C) { return (size_t)B * C * (R / 2 + 1) * R * sizeof(float2); }

// norm = sum w^2 as the library forms it: (sum h^2)^2 of the fp32 taps in fp64; R^2 with the window off
double spectrum_norm(int R, int window) {
    if (!window) return (double)R * (double)R;
    const double pi = 3.14159265358979323846;
    double s = 0.0;
    for (int i = 0; i < R; ++i) {
        const float h = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)i / (double)R));
        s += (double)h * (double)h;
    }
    return s * s;
}

}  // namespace
