// The integer ring rule of the radial power spectrum, shared by csrc/spectrum.hip, csrc/specloss.hip and the host check
// (tools/specloss_host_check.cpp, a plain C++ build: no HIP header is needed to include this file).  Signed frequencies u, v in
// [-R/2, R/2), d = u^2 + v^2 < 2^24; ring k is the integer with (2k-1)^2 <= 4d < (2k+1)^2 (k = 0 for d = 0), i.e.
// floor(sqrt(d) + 1/2) decided in integers.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NGAN_HD __host__ __device__
#else
#define NGAN_HD
#endif

namespace {

// floor(sqrt(n)), n < 2^24: the float estimate settled in integers
NGAN_HD inline int isqrt_floor(int n) {
    int r = (int)sqrtf((float)n);
    while (r * r > n) --r;
    while ((r + 1) * (r + 1) <= n) ++r;
    return r;
}

// the |u| of ring k in column v: lo <= |u| <= hi are those with (2k-1)^2 <= 4 (u^2 + v^2) < (2k+1)^2 (k = 0: d = 0 alone), cut to R/2;
// false if there is none
NGAN_HD inline bool ring_interval(int k, int v, int half, int& lo, int& hi) {
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
NGAN_HD inline int ring_count(int k, int half) {
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

// the ring of the signed frequency pair (u, v): with k0 = floor(sqrt(d)), k0^2 <= d < (k0 + 1)^2, the ring is k0 + 1 where
// (2 k0 + 1)^2 <= 4d and k0 elsewhere.  Rings beyond R/2 (the corners) are returned as they are: the caller drops them.
NGAN_HD inline int ring_of_pair(int u, int v) {
    const int d = u * u + v * v;
    const int k0 = isqrt_floor(d);
    return (2 * k0 + 1) * (2 * k0 + 1) <= 4 * d ? k0 + 1 : k0;
}

}  // namespace
