// Host check of csrc/spectrum_ring.h, the integer ring rule shared by the radial spectrum (csrc/spectrum.hip) and the adjoint of the
// generator's spectral loss (csrc/specloss.hip), built for the CPU under the address and undefined-behaviour sanitizers:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/specloss_host_check.cpp -o specloss_host_check
// For every R = 16 .. 1024 it checks
//   the rule      ring_of_pair(u, v) against the definition as ngan_spectrum_ring_counts states it (floor(sqrt(d) + 1/2), settled in
//                 integers by (2k-1)^2 <= 4d < (2k+1)^2), for every signed pair u, v in [-R/2, R/2);
//   the tallies   the number of pairs ring_of_pair sends to ring k equals ring_count(k, R/2), k = 0 .. R/2, and the corners (k > R/2)
//                 take the rest of the R^2 pairs;
//   the intervals for every column v = 0 .. R/2 and ring k, the |u| that ring_interval names are exactly those ring_of_pair sends to k;
//   the half plane  the adjoint's indexing: element (v, fy) of the half-plane transform, v = 0 .. R/2, fy in DFT order, has the signed
//                 frequencies (fy < R/2 ? fy : fy - R, v); with the Hermitian weights (1 for v = 0 and v = R/2, 2 between) the
//                 half plane's tallies are ring_count again.
// Tables are exact-size heap buffers: a stray index is the sanitizer's to report.  The record is profiles/specloss_host_check.txt.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../neuron-gan_amd/csrc/spectrum_ring.h"

namespace {

long g_checks = 0, g_failures = 0;

void expect(bool ok, const char* what, int R, int a, int b) {
    ++g_checks;
    if (!ok && ++g_failures <= 20) std::printf("FAIL %s (R=%d, %d, %d)\n", what, R, a, b);
}

// the definition, as ngan_spectrum_ring_counts states it
long ring_by_definition(int u, int v) {
    const long d4 = 4L * (u * u + v * v);
    long k = (long)std::floor(std::sqrt((double)(u * u + v * v)) + 0.5);
    while (k > 0 && (2 * k - 1) * (2 * k - 1) > d4) --k;
    while ((2 * k + 1) * (2 * k + 1) <= d4) ++k;
    return k;
}

void check_size(int R) {
    const int half = R / 2, K = half + 1;
    std::vector<long> full(K, 0), halfplane(K, 0);
    long corners = 0;
    for (int u = -half; u < half; ++u)
        for (int v = -half; v < half; ++v) {
            const int k = ring_of_pair(u, v);
            expect(k == ring_by_definition(u, v), "ring_of_pair against the definition", R, u, v);
            if (k <= half) ++full[k];
            else ++corners;
        }
    long kept = 0;
    for (int k = 0; k < K; ++k) {
        expect(full[k] == ring_count(k, half), "tally against ring_count", R, k, (int)full[k]);
        kept += full[k];
    }
    expect(kept + corners == (long)R * R && corners > 0, "kept + corners = R^2", R, (int)kept, (int)corners);
    for (int v = 0; v <= half; ++v) {
        std::vector<char> named(half + 1, 0);                  // |u| -> the ring an interval named it for, + 1
        for (int k = 0; k < K; ++k) {
            int lo, hi;
            if (!ring_interval(k, v, half, lo, hi)) continue;
            expect(lo >= 0 && hi <= half, "interval inside the plane", R, v, k);
            for (int a = lo; a <= hi; ++a) {
                expect(named[a] == 0, "intervals of two rings overlap", R, v, a);
                named[a] = 1;
                expect(ring_of_pair(a, v) == k && ring_of_pair(-a, v) == k, "interval member in another ring", R, v, a);
            }
        }
        for (int a = 0; a <= half; ++a) expect((named[a] != 0) == (ring_of_pair(a, v) <= half), "interval cover", R, v, a);
    }
    for (int v = 0; v <= half; ++v)
        for (int fy = 0; fy < R; ++fy) {
            const int u = fy < half ? fy : fy - R;
            const int k = ring_of_pair(u, v);
            expect(k == ring_by_definition(u, v == half ? -half : v), "half-plane element against the definition", R, fy, v);
            if (k <= half) halfplane[k] += (v == 0 || v == half) ? 1 : 2;
        }
    for (int k = 0; k < K; ++k) expect(halfplane[k] == ring_count(k, half), "half-plane tally against ring_count", R, k, (int)halfplane[k]);
}

}  // namespace

int main() {
    int sizes = 0;
    for (int R = 16; R <= 1024; R *= 2, ++sizes) check_size(R);
    std::printf("specloss_host_check: %d sizes R = 16 .. 1024, %ld checks, %ld failures\n", sizes, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
