// Per-feature arithmetic of the minibatch standard-deviation layer (mbstd.hip; Karras et al. 2018, section 3), written so that the
// same text runs in a kernel and, serially, in a plain host program (tools/mbstd_host_check.cpp compares it with a long double loop).
//
// One feature j of one group of G samples, values x_0 .. x_{G-1}:
//     mu = mean_n x_n        d_n = x_n - mu        sigma = sqrt(mean_n d_n^2 + eps)        (biased variance, eps = 1e-8)
// The statistic s of the group is the mean of sigma over the J features.  With gs the sum of the group's cotangents of s and
// coef = gs / (G J):
//     backward               gx_n = coef d_n / sigma
//     backward of backward   (cotangent h on gx)   hbar = mean_n h_n      hd = sum_n h_n d_n
//                            d/d gs  = sum_j hd / (G J sigma)
//                            d/d x_m = coef ((h_m - hbar) / sigma - d_m hd / (G sigma^3))
// Every product that feeds a sum is an explicit fma, so host and device round alike whatever the compiler contracts.
// The sum of the group is taken in pairs, (x_0 + x_1) + (x_2 + x_3) ...: for G = 2 and G = 4 equal values it is exact, so a group of
// identical samples has d = 0 exactly (a sequential sum of four equal floats need not round back to 4 x).
//
// The statistic enters the head's 3x3 convolution as a constant plane; through zero padding that is scale * s * T with
//     T(y, x) = sum of the taps (ky, kx) of the channel's 3x3 weights whose source pixel (y + ky - 1, x + kx - 1) is inside the image.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define MBSTD_HD __host__ __device__ inline
#else
#define MBSTD_HD inline
#endif

namespace mbstd {

constexpr float EPS = 1e-8f;

template <typename T> MBSTD_HD T pair_step(T acc, T a, T b) { return acc + (a + b); }
template <typename T> MBSTD_HD T mean_of(T sum, int G) { return sum / (T)G; }
template <typename T> MBSTD_HD T sq_step(T q, T v, T mu) {
    const T d = v - mu;
    return std::fma(d, d, q);
}
template <typename T> MBSTD_HD T sigma_of(T q, int G, T eps) { return std::sqrt(q / (T)G + eps); }
template <typename T> MBSTD_HD T coef_of(T gs, int G, long J) { return gs / ((T)G * (T)J); }
template <typename T> MBSTD_HD T gx_of(T coef, T v, T mu, T sigma) { return coef * (v - mu) / sigma; }
template <typename T> MBSTD_HD T hd_step(T hd, T h, T v, T mu) { return std::fma(h, v - mu, hd); }
// hd / (G sigma^3), once per feature
template <typename T> MBSTD_HD T curv_of(T hd, int G, T sigma) { return hd / ((T)G * (sigma * sigma * sigma)); }
template <typename T> MBSTD_HD T dx_of(T coef, T h, T hbar, T v, T mu, T sigma, T curv) {
    const T a = (h - hbar) / sigma;
    return coef * std::fma(-(v - mu), curv, a);
}

// sum over p[0], p[stride], .. of G values, in pairs
template <typename T> MBSTD_HD T group_sum(const T* p, long stride, int G) {
    T s = 0;
    int n = 0;
    for (; n + 1 < G; n += 2) s = pair_step(s, p[n * stride], p[(n + 1) * stride]);
    if (n < G) s = s + p[n * stride];
    return s;
}

// mu and sigma of one feature: x[0], x[stride], ..
template <typename T> MBSTD_HD void feature_stat(const T* x, long stride, int G, T eps, T& mu, T& sigma) {
    mu = mean_of(group_sum(x, stride, G), G);
    T q = 0;
    for (int n = 0; n < G; ++n) q = sq_step(q, x[n * stride], mu);
    sigma = sigma_of(q, G, eps);
}

// the feature's term of d/d gs (before the division by G J) and its G values of d/d x
template <typename T> MBSTD_HD T feature_bwdbwd(const T* x, const T* h, long stride, int G, T eps, T coef, T* dx) {
    T mu, sigma;
    feature_stat(x, stride, G, eps, mu, sigma);
    const T hbar = mean_of(group_sum(h, stride, G), G);
    T hd = 0;
    for (int n = 0; n < G; ++n) hd = hd_step(hd, h[n * stride], x[n * stride], mu);
    const T curv = curv_of(hd, G, sigma);
    for (int n = 0; n < G; ++n) dx[n * stride] = dx_of(coef, h[n * stride], hbar, x[n * stride], mu, sigma, curv);
    return hd / sigma;
}

// T(y, x) of one output channel: w9 holds its 3x3 taps, row-major; H = W = 1 leaves the centre tap alone
template <typename T> MBSTD_HD T field_taps(const T* w9, int y, int x, int H, int W) {
    T t = 0;
    for (int ky = 0; ky < 3; ++ky) {
        const int yy = y + ky - 1;
        if (yy < 0 || yy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int xx = x + kx - 1;
            if (xx < 0 || xx >= W) continue;
            t = t + w9[ky * 3 + kx];
        }
    }
    return t;
}
// c + (scale s) T
template <typename T> MBSTD_HD T field_add(T c, T k, T t) { return std::fma(k, t, c); }
// is tap index k (0 .. 2) along one axis inside an extent n at position p
MBSTD_HD bool tap_inside(int k, int p, int n) { return p + k - 1 >= 0 && p + k - 1 < n; }

}  // namespace mbstd
