// Host check of csrc/ada_bits.h, the per-element arithmetic of the adaptive augmentation controller (csrc/ada.hip), built for the CPU
// under the address and undefined-behaviour sanitizers:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/ada_host_check.cpp -o ada_host_check
// It runs the counting and the update rule through the shared functions -- side, midpoint, update -- against a straightforward
// restatement in long double and 128-bit integers, over a grid of cases:
//   counting   score vectors of 1 .. 4099 values with ties, NaN and +-inf, thresholds finite, NaN and +-inf, and the midpoint of two
//              batch means: ada::side summed into 64-bit counters that start near 2^40, against a plain loop that classifies each
//              score with the comparison operators on long double and counts in __int128; pos + neg + (ties and NaN) = n;
//   the sign   of (pos - neg) - target n against the exact sign from 128-bit integer arithmetic on the target's mantissa, for counts
//              up to 2^40, n = 0 and d = 0.  (The rule forms the product target n in fp64.  It is exact when the target's
//              significant bits plus n's fit 53: every target of the grid with n < 2^29, and the targets of at most 12 bits with any
//              n of the grid.  Only those pairs are compared; the others are counted as skipped.)
//   the step   p' against the same expression written out independently in volatile doubles (bit for bit), against the long double
//              value of min(p_max, max(0, p + s n / span)) (within one fp32 rounding plus one fp64 one), inside [0, p_max] always,
//              a NaN p giving 0, and last_r = fp32((pos - neg) / n), kept for n = 0.
// Tables are exact-size heap buffers: a stray index is the sanitizer's to report.  The record is profiles/ada_host_check.txt.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../neuron-gan_amd/csrc/ada_bits.h"

namespace {

long g_cases = 0, g_checks = 0, g_failures = 0, g_skipped = 0;

void expect(bool ok, const char* what, double a, double b, double c) {
    ++g_checks;
    if (!ok && ++g_failures <= 20) std::printf("FAIL %s (%.17g, %.17g, %.17g)\n", what, a, b, c);
}

uint32_t bits_of(float v) {
    uint32_t u;
    std::memcpy(&u, &v, sizeof u);
    return u;
}

// ---- counting ---------------------------------------------------------------------------------------------------------------------
void check_counting(const std::vector<float>& real, double t, long start) {
    ++g_cases;
    long counters[3] = {start, start + 1, start + 2};
    __int128 pos = 0, neg = 0, neither = 0;
    for (size_t i = 0; i < real.size(); ++i) {
        const int s = ada::side(real[i], t);
        counters[0] += s > 0;
        counters[1] += s < 0;
        const long double v = (long double)real[i], tl = (long double)t;
        if (v > tl) ++pos;
        else if (v < tl) ++neg;
        else ++neither;                                           // a tie, or a NaN on either side
        expect(s == (v > tl) - (v < tl), "side", (double)real[i], t, s);
    }
    counters[2] += (long)real.size();
    expect((__int128)counters[0] == (__int128)start + pos, "pos", (double)counters[0], (double)pos, t);
    expect((__int128)counters[1] == (__int128)start + 1 + neg, "neg", (double)counters[1], (double)neg, t);
    expect(pos + neg + neither == (__int128)real.size(), "pos + neg + neither = n", (double)pos, (double)neg, (double)neither);
    if (std::isnan(t)) expect(pos == 0 && neg == 0, "a NaN threshold counts in n alone", (double)pos, (double)neg, t);
}

void counting_grid() {
    std::mt19937_64 rng(17);
    std::normal_distribution<float> normal(0.2f, 1.5f);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const long start = (1L << 40) - 7;
    for (int n : {1, 2, 5, 8, 63, 64, 65, 257, 4099}) {
        std::vector<float> real((size_t)n), fake((size_t)(n / 2 + 1));
        for (auto& v : real) v = std::round(normal(rng) * 8.f) / 8.f;            // multiples of 1/8: ties are common
        for (auto& v : fake) v = std::round(normal(rng) * 8.f) / 8.f;
        std::vector<float> special = real;
        special[0] = nan;
        if (n > 2) special[1] = inf, special[2] = -inf;
        for (double t : {0.0, 0.5, -0.125, (double)real[(size_t)n / 2], (double)nan, (double)inf, -(double)inf}) {
            check_counting(real, t, start);
            check_counting(special, t, start);
        }
        // the midpoint of the two batch means, from sums added up in index order (any order gives these bits: multiples of 1/8)
        double sr = 0.0, sf = 0.0;
        for (float v : real) sr += (double)v;
        for (float v : fake) sf += (double)v;
        const double mid = ada::midpoint(sr, n, sf, (int)fake.size());
        const long double want = 0.5L * ((long double)sr / n + (long double)sf / (long double)fake.size());
        expect(std::fabs((double)((long double)mid - want)) <= 4e-16 * (1.0 + std::fabs((double)want)), "midpoint", mid, (double)want, n);
        check_counting(real, mid, start);
        double bad = 0.0;
        for (float v : special) bad += (double)v;                                // NaN (n > 2: inf - inf as well)
        check_counting(special, ada::midpoint(bad, n, sf, (int)fake.size()), start);
    }
}

// ---- the update rule ----------------------------------------------------------------------------------------------------------------
// sign of (pos - neg) - target * n, exactly: target = m 2^e with an integer m of at most 24 bits
int exact_sign(long pos, long neg, long n, float target) {
    int e;
    const double fr = std::frexp((double)target, &e);                          // target = fr 2^e, 0.5 <= |fr| < 1 (or 0)
    const __int128 m = (__int128)std::llround(std::ldexp(fr, 24));              // target = m 2^(e - 24)
    const int shift = 24 - e;                                                   // d 2^shift = (pos - neg) 2^shift - m n
    if (shift < 0 || shift > 60) return 2;                                      // (outside the grid)
    const __int128 d = (__int128)(pos - neg) * ((__int128)1 << shift) - m * (__int128)n;
    return (d > 0) - (d < 0);
}

bool product_exact(long n, float target) {
    const long double p = (long double)target * (long double)n;                // 24 + 41 bits > 64: test through the fp64 rounding
    const double r = (double)target * (double)n;
    int bits_t = 0;
    for (uint32_t m = bits_of(target) & 0x7fffffu; m; m <<= 1, m &= 0x7fffffu) ++bits_t;   // significant bits below the leading one
    int bits_n = 0;
    for (unsigned long v = (unsigned long)n; v; v >>= 1) ++bits_n;
    return bits_t + 1 + bits_n <= 53 && (long double)r == p;
}

void check_update(long pos, long neg, long n, float p, float last_r, float target, double span, float p_max) {
    ++g_cases;
    const ada::Step st = ada::update(pos, neg, n, p, last_r, target, span, p_max);
    expect(st.p >= 0.f && st.p <= p_max, "p inside [0, p_max]", st.p, p_max, p);
    if (n == 0) {
        expect(bits_of(st.r) == bits_of(last_r), "n = 0 keeps last_r", st.r, last_r, 0);
        expect(std::isnan(p) ? st.p == 0.f : bits_of(st.p) == bits_of(p < 0.f ? 0.f : (p > p_max ? p_max : p)), "n = 0 keeps p", st.p, p, p_max);
        return;
    }
    const long double r = (long double)(pos - neg) / (long double)n;          // (rounded through fp64 by the rule: half an fp32 ulp and a bit)
    expect(std::fabs((double)((long double)st.r - r)) <= 5.97e-8 * std::fabs((double)r) + 1e-40 && st.r >= -1.f && st.r <= 1.f, "last_r", st.r,
           (double)r, (double)n);
    if (!product_exact(n, target)) {
        ++g_skipped;
        return;
    }
    const int s = exact_sign(pos, neg, n, target);
    if (s == 2) {
        ++g_skipped;
        return;
    }
    // the same expression, independently, in volatile doubles: bit for bit
    volatile double move = (double)s * (double)n;
    move = move / span;
    volatile double q = (std::isnan(p) ? std::numeric_limits<double>::quiet_NaN() : (double)p) + move;
    q = q > 0.0 ? q : 0.0;
    q = q < (double)p_max ? q : (double)p_max;
    expect(bits_of(st.p) == bits_of((float)q), "p' bit for bit", st.p, (float)q, s);
    // and the long double value of the rule
    long double w = std::isnan(p) ? 0.0L : (long double)p + (long double)s * (long double)n / (long double)span;
    if (std::isnan(p)) w = 0.0L;
    w = w > 0.0L ? w : 0.0L;
    w = w < (long double)p_max ? w : (long double)p_max;
    expect(std::fabs((double)((long double)st.p - w)) <= 6.1e-8 * (double)(w > 0.25L ? w : 0.25L) + 1e-16, "p' against long double", st.p, (double)w, s);
    if (std::isnan(p)) expect(st.p == 0.f, "a NaN p becomes 0", st.p, 0, 0);
    if (s != 0 && !std::isnan(p) && w > 0.0L && w < (long double)p_max)
        expect((st.p > p) == (s > 0) || st.p == p, "moves towards the target", st.p, p, s);
}

void update_grid() {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const long ns[] = {0, 1, 8, 16, 4096, (1L << 28) + 3, (1L << 31) + 7, (1L << 33) + 5, (1L << 40) - 3, 1L << 40};
    const float targets[] = {0.f, 0.25f, 0.5f, 0.6f, 0.599853515625f, 0.75f, 0.99f, -0.5f};
    const float ps[] = {0.f, 1e-9f, 0.125f, 0.3f, 0.5f, 0.999999f, 1.f, nan};
    const double spans[] = {3.0, 8.0, 64.0, 1000.0, 500000.0, 68719476736.0, 1e12};
    const float p_maxs[] = {1.f, 0.3f, 0.f};
    for (long n : ns)
        for (float target : targets) {
            // pos - neg around target n: below, on (where an integer), above; and the extremes
            const long on = (long)std::floor((double)target * (double)n);
            for (long diff : {-n, on - 1, on, on + 1, n}) {
                if (diff < -n || diff > n || ((n - diff) & 1)) continue;       // pos + neg = n here, so n - diff is even
                const long pos = (n + diff) / 2, neg = (n - diff) / 2;
                for (float p : ps)
                    for (double span : spans)
                        for (float p_max : p_maxs) check_update(pos, neg, n, p > p_max ? p_max : p, -0.375f, target, span, p_max);
            }
            // with ties / NaN scores among the n: pos + neg < n
            if (n >= 8) check_update(n / 2, n / 8, n, 0.5f, 0.f, target, 1000.0, 1.f);
        }
    check_update(3, 1, 4, 0.9f, 0.f, 0.6f, 64.0, 0.3f);                        // p above p_max (a resumed run under a lower clamp)
}

}  // namespace

int main() {
    counting_grid();
    const long counting_cases = g_cases;
    update_grid();
    std::printf("ada_host_check: %ld cases (%ld counting, %ld update; %ld update cases skipped the exact-sign comparison: the product "
                "target n is not exact in fp64 there), %ld checks, %ld failures\n",
                g_cases, counting_cases, g_cases - counting_cases, g_skipped, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
