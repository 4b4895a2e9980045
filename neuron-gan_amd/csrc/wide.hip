// Channel counts the lane-group kernels of pixelnorm.hip / pointwise.hip do not take -- more than 256, or C / 4 not a power of two:
// the reference's constructors accept any widths and its presets 0004 - 0008 have 512- and 1024-channel blocks on 4x4 .. 32x32
// images (configs/config.py:87-98).  Same operators (formulas: include/ngan.h), one THREAD per pixel walking the channels for the
// per-pixel operators, one thread per channel walking the pixels for the parameter gradients.  A compatibility path for small
// images: no lane-group reductions, no workspaces, fixed summation order (bit-reproducible).
// Every kernel is a template over the activation storage type T (ngan_common.h): float, or __bf16 for the bf16 mode (precision code 5),
// which reads bf16, computes in fp32 and rounds once, on the store.  Images, norms and parameter gradients are fp32 in both.
#include "ngan_common.h"

namespace {

__device__ __forceinline__ float lmask(float y, float slope) { return y > 0.f ? 1.f : slope; }

template <typename T>
__global__ __launch_bounds__(256) void wide_pn_fwd_kernel(const T* __restrict__ c, const float* __restrict__ bias, T* __restrict__ y,
                                                          float* __restrict__ rn, long npix, int C, float slope, float eps) {
    const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= npix) return;
    const T* src = c + pix * C;
    float ss = 0.f;
    for (int k = 0; k < C; k += 4) {
        float4 v = lda4(src + k);
        if (bias) v = f4add(v, ld4(bias + k));
        v.x = v.x > 0.f ? v.x : slope * v.x; v.y = v.y > 0.f ? v.y : slope * v.y;
        v.z = v.z > 0.f ? v.z : slope * v.z; v.w = v.w > 0.f ? v.w : slope * v.w;
        ss += f4dot(v, v);
    }
    const float r = sqrtf(ss / (float)C + eps), inv = 1.0f / r;
    T* dst = y + pix * C;
    for (int k = 0; k < C; k += 4) {                       // (src may be dst: element k is read before it is written)
        float4 v = lda4(src + k);
        if (bias) v = f4add(v, ld4(bias + k));
        v.x = v.x > 0.f ? v.x : slope * v.x; v.y = v.y > 0.f ? v.y : slope * v.y;
        v.z = v.z > 0.f ? v.z : slope * v.z; v.w = v.w > 0.f ? v.w : slope * v.w;
        sta4(dst + k, f4scale(v, inv));
    }
    rn[pix] = r;
}

template <typename T>
__global__ __launch_bounds__(256) void wide_pn_bwd_kernel(const T* __restrict__ gy, const T* __restrict__ gy2, const float* __restrict__ gr,
                                                          const T* __restrict__ y, const float* __restrict__ rn, T* __restrict__ gc,
                                                          long npix, int C, float slope) {
    const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= npix) return;
    const long o = pix * C;
    float s = 0.f;
    for (int k = 0; k < C; k += 4) {
        float4 g = lda4(gy + o + k);
        if (gy2) g = f4add(g, lda4(gy2 + o + k));
        s += f4dot(g, lda4(y + o + k));
    }
    const float inv_c = 1.0f / (float)C, inv_r = 1.0f / rn[pix];
    s *= inv_c;
    const float kk = gr ? gr[pix] * inv_c : 0.f;
    for (int k = 0; k < C; k += 4) {                       // (gy may be gc)
        float4 g = lda4(gy + o + k);
        if (gy2) g = f4add(g, lda4(gy2 + o + k));
        const float4 yy = lda4(y + o + k);
        sta4(gc + o + k, make_float4(((g.x - yy.x * s) * inv_r + kk * yy.x) * lmask(yy.x, slope), ((g.y - yy.y * s) * inv_r + kk * yy.y) * lmask(yy.y, slope),
                                    ((g.z - yy.z * s) * inv_r + kk * yy.z) * lmask(yy.z, slope), ((g.w - yy.w * s) * inv_r + kk * yy.w) * lmask(yy.w, slope)));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void wide_pn_bwdbwd_kernel(const T* __restrict__ h, const T* __restrict__ gy, const T* __restrict__ y,
                                                             const float* __restrict__ rn, T* __restrict__ ggy, T* __restrict__ gy_out,
                                                             float* __restrict__ gr_out, long npix, int C, float slope) {
    const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= npix) return;
    const long o = pix * C;
    float s = 0.f, t = 0.f, u = 0.f;
    for (int k = 0; k < C; k += 4) {
        const float4 g = lda4(gy + o + k), yy = lda4(y + o + k);
        float4 hp = lda4(h + o + k);
        hp.x *= lmask(yy.x, slope); hp.y *= lmask(yy.y, slope); hp.z *= lmask(yy.z, slope); hp.w *= lmask(yy.w, slope);
        s += f4dot(g, yy); t += f4dot(hp, yy); u += f4dot(hp, g);
    }
    const float inv_c = 1.0f / (float)C, inv_r = 1.0f / rn[pix];
    s *= inv_c; t *= inv_c; u *= inv_c;
    for (int k = 0; k < C; k += 4) {
        const float4 g = lda4(gy + o + k), yy = lda4(y + o + k);
        float4 hp = lda4(h + o + k);
        hp.x *= lmask(yy.x, slope); hp.y *= lmask(yy.y, slope); hp.z *= lmask(yy.z, slope); hp.w *= lmask(yy.w, slope);
        sta4(ggy + o + k, make_float4((hp.x - yy.x * t) * inv_r, (hp.y - yy.y * t) * inv_r, (hp.z - yy.z * t) * inv_r, (hp.w - yy.w * t) * inv_r));
        sta4(gy_out + o + k, make_float4(-(s * hp.x + t * g.x) * inv_r, -(s * hp.y + t * g.y) * inv_r, -(s * hp.z + t * g.z) * inv_r, -(s * hp.w + t * g.w) * inv_r));
    }
    gr_out[pix] = -(float)C * (u - s * t) * inv_r * inv_r;
}

// A thread's sum over the pixels, in three levels: runs of 1024 pixels, runs of 1024 such runs, and the rest.  One sequential fp32
// accumulator over n terms is off by ~ 2^-24 sqrt(n) of the terms' magnitude, 1.4e-4 of the result at 4.5e7 pixels (measured:
// tests/test_gpu_large_offsets.py); in levels the longest run is 1024 terms whatever n is.  Up to 1024 pixels there is one run and
// the order, and with it every bit, is the single accumulator's.  add(p, acc) returns acc with pixel p's term added.
constexpr long kSumRun = 1024;
template <typename F>
__device__ __forceinline__ float wide_pixel_sum(long npix, F add) {
    float s2 = 0.f;
    for (long p2 = 0; p2 < npix; p2 += kSumRun * kSumRun) {
        const long e2 = p2 + kSumRun * kSumRun < npix ? p2 + kSumRun * kSumRun : npix;
        float s1 = 0.f;
        for (long p1 = p2; p1 < e2; p1 += kSumRun) {
            const long e1 = p1 + kSumRun < e2 ? p1 + kSumRun : e2;
            float s0 = 0.f;
            for (long p = p1; p < e1; ++p) s0 = add(p, s0);
            s1 += s0;
        }
        s2 += s1;
    }
    return s2;
}

template <typename T>
__global__ __launch_bounds__(256) void wide_channel_sum_kernel(const T* __restrict__ g, float* __restrict__ out, long npix, int C, float scale) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float s = wide_pixel_sum(npix, [&](long p, float acc) { return acc + lda1(g + p * C + c); });
    out[c] = s * scale;
}

template <typename T>
__global__ __launch_bounds__(256) void wide_to_image_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, float* __restrict__ t,
                                                                long npix, int C, int Ncol) {
    const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= npix) return;
    for (int k = 0; k < Ncol; ++k) {
        float s = 0.f;
        for (int c = 0; c < C; c += 4) s += f4dot(lda4(x + pix * C + c), ld4(w + k * C + c));
        t[pix * Ncol + k] = tanhf(s);
    }
}

// gx (optionally followed by the LeakyReLU -> PixelNorm backward of the layer that produced x: rn != nullptr)
template <typename T>
__global__ __launch_bounds__(256) void wide_to_image_dx_kernel(const float* __restrict__ g, const float* __restrict__ t, const T* __restrict__ x,
                                                               const float* __restrict__ w, T* __restrict__ gx, long npix, int C, int Ncol,
                                                               const float* __restrict__ rn, float slope) {
    const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= npix) return;
    float qv[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < Ncol; ++k) { const float tv = t[pix * Ncol + k]; qv[k] = g[pix * Ncol + k] * (1.0f - tv * tv); }
    float sdot = 0.f;
    if (rn) {
        for (int c = 0; c < C; c += 4) {
            float4 o = f4zero();
            for (int k = 0; k < Ncol; ++k) o = f4fma(ld4(w + k * C + c), qv[k], o);
            sdot += f4dot(o, lda4(x + pix * C + c));
        }
        sdot *= 1.0f / (float)C;
    }
    const float inv_r = rn ? 1.0f / rn[pix] : 1.f;
    for (int c = 0; c < C; c += 4) {
        float4 o = f4zero();
        for (int k = 0; k < Ncol; ++k) o = f4fma(ld4(w + k * C + c), qv[k], o);
        if (rn) {
            const float4 yy = lda4(x + pix * C + c);
            o = make_float4((o.x - yy.x * sdot) * inv_r * lmask(yy.x, slope), (o.y - yy.y * sdot) * inv_r * lmask(yy.y, slope),
                            (o.z - yy.z * sdot) * inv_r * lmask(yy.z, slope), (o.w - yy.w * sdot) * inv_r * lmask(yy.w, slope));
        }
        sta4(gx + pix * C + c, o);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void wide_to_image_dw_kernel(const float* __restrict__ g, const float* __restrict__ t, const T* __restrict__ x,
                                                               float* __restrict__ gw, long npix, int C, int Ncol) {
    const int i = blockIdx.x * 256 + threadIdx.x;          // (k, c)
    if (i >= Ncol * C) return;
    const int k = i / C, c = i - k * C;
    gw[i] = wide_pixel_sum(npix, [&](long p, float acc) {
        const float tv = t[p * Ncol + k];
        return fmaf(lda1(x + p * C + c), g[p * Ncol + k] * (1.0f - tv * tv), acc);
    });
}

__device__ __forceinline__ float wide_img(const float* __restrict__ x, int b, int yy, int xx, int k, int H, int W, int Ncol, int pool) {
    if (!pool) return x[(((long)b * H + yy) * W + xx) * Ncol + k];
    const long W2 = 2L * W;
    const float* p = x + (((long)b * 2 * H + 2 * yy) * W2 + 2 * xx) * Ncol + k;
    return 0.25f * ((p[0] + p[Ncol]) + (p[W2 * Ncol] + p[W2 * Ncol + Ncol]));
}

template <typename T>
__global__ __launch_bounds__(256) void wide_from_image_dx_kernel(const T* __restrict__ g, const float* __restrict__ w, float* __restrict__ gx,
                                                                 int B, int H, int W, int Ncol, int C, int pool) {
    const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (long)B * H * W) return;
    const int xx = (int)(pix % W), yy = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
    for (int k = 0; k < Ncol; ++k) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = fmaf(lda1(g + pix * C + c), w[c * Ncol + k], s);
        if (!pool) gx[pix * Ncol + k] = s;
        else {
            const long W2 = 2L * W;
            float* p = gx + (((long)b * 2 * H + 2 * yy) * W2 + 2 * xx) * Ncol + k;
            const float q4 = 0.25f * s;
            p[0] = q4; p[Ncol] = q4; p[W2 * Ncol] = q4; p[W2 * Ncol + Ncol] = q4;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void wide_from_image_dw_kernel(const float* __restrict__ x, const T* __restrict__ g, float* __restrict__ gw,
                                                                 float* __restrict__ gb, int B, int H, int W, int Ncol, int C, int pool) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    // the pixels in their order (b, yy, xx), each of the Ncol + 1 sums in the levels of wide_pixel_sum
    const long npix = (long)B * H * W;
    auto pixel = [&](long p, int& b, int& yy, int& xx) { xx = (int)(p % W); const long r = p / W; yy = (int)(r % H); b = (int)(r / H); };
    if (gb)
        gb[c] = wide_pixel_sum(npix, [&](long p, float acc) { return acc + lda1(g + p * C + c); });
    for (int k = 0; k < Ncol; ++k)
        gw[c * Ncol + k] = wide_pixel_sum(npix, [&](long p, float acc) {
            int b, yy, xx;
            pixel(p, b, yy, xx);
            return fmaf(lda1(g + p * C + c), wide_img(x, b, yy, xx, k, H, W, Ncol, pool), acc);
        });
}

// bilinear x2 adjoint followed by the LeakyReLU -> PixelNorm backward of the layer that produced the low-resolution input (gr = 0),
// fused: one thread per low-resolution pixel; the adjoint is formed in fp32 twice (once for the per-pixel sum, once for the store), so
// the intermediate never passes through the storage type.  Taps and weights: up2_adjoint_vec_kernel (pointwise.hip).
__device__ __forceinline__ float wide_up2_adj_w(int i, int R, int n) {
    if (R < 0 || R > 2 * n - 1) return 0.f;
    const int d = R - 2 * i;
    if (d == -1 || d == 2) return 0.25f;
    if (d == 0) return i == 0 ? 1.0f : 0.75f;
    return i == n - 1 ? 1.0f : 0.75f;
}
template <typename T>
__device__ __forceinline__ float4 wide_up2_adj4(const T* __restrict__ base, int X, int Y, int h, int w, int C) {
    float4 s = f4zero();
    for (int dy = -1; dy <= 2; ++dy) {
        const int RY = 2 * Y + dy;
        const float wy = wide_up2_adj_w(Y, RY, h);
        if (wy == 0.f) continue;
        float4 rowsum = f4zero();
        for (int dx = -1; dx <= 2; ++dx) {
            const int RX = 2 * X + dx;
            const float wx = wide_up2_adj_w(X, RX, w);
            if (wx != 0.f) rowsum = f4fma(lda4(base + ((long)RY * (2 * w) + RX) * C), wx, rowsum);
        }
        s = f4fma(rowsum, wy, s);
    }
    return s;
}
template <typename T>
__global__ __launch_bounds__(256) void wide_up2_adjoint_pnbwd_kernel(const T* __restrict__ g, const T* __restrict__ y, const float* __restrict__ rn,
                                                                     T* __restrict__ o, int B, int h, int w, int C, float slope) {
    const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (long)B * h * w) return;
    const int X = (int)(pix % w), Y = (int)((pix / w) % h), b = (int)(pix / ((long)w * h));
    const T* base = g + (long)b * 4 * h * w * C;
    const long off = pix * C;
    float s = 0.f;
    for (int k = 0; k < C; k += 4) s += f4dot(wide_up2_adj4(base + k, X, Y, h, w, C), lda4(y + off + k));
    s *= 1.0f / (float)C;
    const float inv_r = 1.0f / rn[pix];
    for (int k = 0; k < C; k += 4) {                       // (y may be o: element k is read before it is written)
        const float4 a = wide_up2_adj4(base + k, X, Y, h, w, C), yy = lda4(y + off + k);
        sta4(o + off + k, make_float4((a.x - yy.x * s) * inv_r * lmask(yy.x, slope), (a.y - yy.y * s) * inv_r * lmask(yy.y, slope),
                                      (a.z - yy.z * s) * inv_r * lmask(yy.z, slope), (a.w - yy.w * s) * inv_r * lmask(yy.w, slope)));
    }
}

}  // namespace

namespace ngan {

// (called by the C ABI entry points of pixelnorm.hip / pointwise.hip when C is outside their lane-group kernels' range; C % 4 == 0;
// T = float: the fp32 contract, T = __bf16: the bf16-storage entry points)
template <typename T>
int wide_pn_fwd(const T* c, const float* bias, T* y, float* rn, long npix, int C, float slope, float eps, hipStream_t s) {
    NGAN_REQUIRE_THREADS("lrelu_pixelnorm_fwd(wide)", npix);
    hipLaunchKernelGGL(wide_pn_fwd_kernel<T>, dim3(ceil_div(npix, 256)), dim3(256), 0, s, c, bias, y, rn, npix, C, slope, eps);
    return launch_status("ngan_lrelu_pixelnorm_fwd(wide)");
}
template <typename T>
int wide_pn_bwd(const T* gy, const T* gy2, const float* gr, const T* y, const float* rn, T* gc, long npix, int C, float slope, hipStream_t s) {
    NGAN_REQUIRE_THREADS("lrelu_pixelnorm_bwd(wide)", npix);
    hipLaunchKernelGGL(wide_pn_bwd_kernel<T>, dim3(ceil_div(npix, 256)), dim3(256), 0, s, gy, gy2, gr, y, rn, gc, npix, C, slope);
    return launch_status("ngan_lrelu_pixelnorm_bwd(wide)");
}
template <typename T>
int wide_pn_bwdbwd(const T* h, const T* gy, const T* y, const float* rn, T* ggy, T* gy_out, float* gr_out, long npix, int C, float slope,
                   hipStream_t s) {
    NGAN_REQUIRE_THREADS("lrelu_pixelnorm_bwdbwd(wide)", npix);
    hipLaunchKernelGGL(wide_pn_bwdbwd_kernel<T>, dim3(ceil_div(npix, 256)), dim3(256), 0, s, h, gy, y, rn, ggy, gy_out, gr_out, npix, C, slope);
    return launch_status("ngan_lrelu_pixelnorm_bwdbwd(wide)");
}
template <typename T>
int wide_channel_sum(const T* g, float* out, long npix, int C, float scale, hipStream_t s) {
    hipLaunchKernelGGL(wide_channel_sum_kernel<T>, dim3(ceil_div(C, 256)), dim3(256), 0, s, g, out, npix, C, scale);
    return launch_status("ngan_channel_sum(wide)");
}
template <typename T>
int wide_to_image_fwd(const T* x, const float* w, float* t, long npix, int C, int Ncol, hipStream_t s) {
    NGAN_REQUIRE_THREADS("to_image_fwd(wide)", npix);
    hipLaunchKernelGGL(wide_to_image_fwd_kernel<T>, dim3(ceil_div(npix, 256)), dim3(256), 0, s, x, w, t, npix, C, Ncol);
    return launch_status("ngan_to_image_fwd(wide)");
}
template <typename T>
int wide_to_image_bwd(const float* g, const float* t, const T* x, const float* w, T* gx, float* gw, long npix, int C, int Ncol, const float* rn,
                      float slope, hipStream_t s) {
    NGAN_REQUIRE_THREADS("to_image_bwd(wide)", npix);
    hipLaunchKernelGGL(wide_to_image_dw_kernel<T>, dim3(ceil_div((long)Ncol * C, 256)), dim3(256), 0, s, g, t, x, gw, npix, C, Ncol);
    hipLaunchKernelGGL(wide_to_image_dx_kernel<T>, dim3(ceil_div(npix, 256)), dim3(256), 0, s, g, t, x, w, gx, npix, C, Ncol, rn, slope);
    return launch_status("ngan_to_image_bwd(wide)");
}
template <typename T>
int wide_from_image_dx(const T* g, const float* w, float* gx, int B, int H, int W, int Ncol, int C, int pool, hipStream_t s) {
    NGAN_REQUIRE_THREADS("from_image_dx(wide)", (long)B * H * W);
    hipLaunchKernelGGL(wide_from_image_dx_kernel<T>, dim3(ceil_div((long)B * H * W, 256)), dim3(256), 0, s, g, w, gx, B, H, W, Ncol, C, pool);
    return launch_status("ngan_from_image_dx(wide)");
}
template <typename T>
int wide_from_image_dw(const float* x, const T* g, float* gw, float* gb, int B, int H, int W, int Ncol, int C, int pool, hipStream_t s) {
    hipLaunchKernelGGL(wide_from_image_dw_kernel<T>, dim3(ceil_div(C, 256)), dim3(256), 0, s, x, g, gw, gb, B, H, W, Ncol, C, pool);
    return launch_status("ngan_from_image_dw(wide)");
}
template <typename T>
int wide_up2_adjoint_pnbwd(const T* g, const T* yprev, const float* rn, T* o, int B, int h, int w, int C, float slope, hipStream_t s) {
    NGAN_REQUIRE_THREADS("up2_adjoint_pnbwd(wide)", (long)B * h * w);
    hipLaunchKernelGGL(wide_up2_adjoint_pnbwd_kernel<T>, dim3(ceil_div((long)B * h * w, 256)), dim3(256), 0, s, g, yprev, rn, o, B, h, w, C, slope);
    return launch_status("ngan_bf16_up2_adjoint_pnbwd(wide)");
}

#define WIDE_INSTANTIATE(T)                                                                                                                   \
    template int wide_pn_fwd<T>(const T*, const float*, T*, float*, long, int, float, float, hipStream_t);                                    \
    template int wide_pn_bwd<T>(const T*, const T*, const float*, const T*, const float*, T*, long, int, float, hipStream_t);                 \
    template int wide_pn_bwdbwd<T>(const T*, const T*, const T*, const float*, T*, T*, float*, long, int, float, hipStream_t);                 \
    template int wide_channel_sum<T>(const T*, float*, long, int, float, hipStream_t);                                                       \
    template int wide_to_image_fwd<T>(const T*, const float*, float*, long, int, int, hipStream_t);                                          \
    template int wide_to_image_bwd<T>(const float*, const float*, const T*, const float*, T*, float*, long, int, int, const float*, float,     \
                                      hipStream_t);                                                                                           \
    template int wide_from_image_dx<T>(const T*, const float*, float*, int, int, int, int, int, int, hipStream_t);                            \
    template int wide_from_image_dw<T>(const float*, const T*, float*, float*, int, int, int, int, int, int, hipStream_t);
WIDE_INSTANTIATE(float)
WIDE_INSTANTIATE(__bf16)
#undef WIDE_INSTANTIATE
template int wide_up2_adjoint_pnbwd<__bf16>(const __bf16*, const __bf16*, const float*, __bf16*, int, int, int, int, float, hipStream_t);

}  // namespace ngan
