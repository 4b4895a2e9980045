// Runs the per-feature arithmetic of neuron-gan_amd/csrc/mbstd_bits.h -- the text the minibatch standard-deviation kernels execute -- in
// fp32 on the host over the test families (random, unit-RMS rows, values of 1e3, groups of identical samples) and the group sizes
// 1, 2, 3, 4 and 8, and compares every output with a long double loop written from the definitions in include/ngan_mbstd.h: the
// statistic, its backward, its backward-of-backward (both outputs), and the tap sums of the field for every pixel of 1 x 1 .. 5 x 5
// images.  Bound per element, as tests/mbstd_cases.py derives it: n 2^-23 |ref| + 8 2^-24 absref.  The groups of identical samples
// must give d = 0 exactly for G = 2 and G = 4 (pair sums).  The sanitizers see every index formed.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/mbstd_host_check.cpp -o mbstd_host_check
//     ./mbstd_host_check > profiles/mbstd_host_check.txt
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../neuron-gan_amd/csrc/mbstd_bits.h"

typedef long double ld;
static const ld EPS = 1e-8L;

static ld bound(ld ref, ld absref, int n) { return n * ldexpl(1.0L, -23) * fabsl(ref) + 8 * ldexpl(1.0L, -24) * absref + 1e-300L; }

struct Worst {
    double s = 0, gx = 0, dgs = 0, dx = 0;
};

// one group of G samples with J features each (x[n * J + j]), cotangents gs (G values) and h
static Worst check_group(const std::vector<float>& x, const std::vector<float>& h, const std::vector<float>& gs, int G, int J, bool constant,
                         int& failures) {
    Worst w;
    float gsum = mbstd::group_sum(gs.data(), 1L, G);
    const float coef = mbstd::coef_of(gsum, G, (long)J);
    ld gsl = 0, gsa = 0;
    for (int n = 0; n < G; ++n) gsl += gs[n], gsa += fabsl((ld)gs[n]);
    const ld coefl = gsl / ((ld)G * J), cs = gsa / ((ld)G * J);
    ld s_ref = 0, s_abs = 0, dgs_ref = 0, dgs_abs = 0;
    double s_got = 0, dgs_got = 0;
    std::vector<float> dx(x.size());
    for (int j = 0; j < J; ++j) {
        float mu, sigma;
        mbstd::feature_stat(x.data() + j, (long)J, G, mbstd::EPS, mu, sigma);
        s_got += (double)sigma;
        dgs_got += (double)mbstd::feature_bwdbwd(x.data() + j, h.data() + j, (long)J, G, mbstd::EPS, coef, dx.data() + j);
        // the definitions
        ld m = 0, A = 0, hb = 0, ha = 0;
        for (int n = 0; n < G; ++n) m += x[n * J + j], A += fabsl((ld)x[n * J + j]), hb += h[n * J + j], ha += fabsl((ld)h[n * J + j]);
        m /= G, A /= G, hb /= G, ha /= G;
        ld q = 0, hd = 0, HD = 0;
        for (int n = 0; n < G; ++n) {
            const ld d = x[n * J + j] - m;
            q += d * d, hd += h[n * J + j] * d, HD += fabsl((ld)h[n * J + j]) * (fabsl(d) + A);
        }
        const ld sg = sqrtl(q / G + EPS), k1 = A / sg;
        s_ref += sg, s_abs += sg + A;
        dgs_ref += hd / sg, dgs_abs += (1 + k1) * HD / sg;
        for (int n = 0; n < G; ++n) {
            const ld d = x[n * J + j] - m;
            const float gx = mbstd::gx_of(coef, x[n * J + j], mu, sigma);
            const ld gx_ref = coefl * d / sg;
            w.gx = std::max(w.gx, (double)(fabsl(gx - gx_ref) / bound(gx_ref, cs * (fabsl(d) + A) / sg + fabsl(gx_ref) * k1, 4)));
            const ld dx_ref = coefl * ((h[n * J + j] - hb) / sg - d * hd / (G * sg * sg * sg));
            const ld dx_abs = cs * ((fabsl((ld)h[n * J + j]) + ha) / sg * (1 + k1) + (fabsl(d) + A) * HD / (G * sg * sg * sg) * (1 + 3 * k1));
            w.dx = std::max(w.dx, (double)(fabsl(dx[n * J + j] - dx_ref) / bound(dx_ref, dx_abs, 3)));
            if (!std::isfinite(gx) || !std::isfinite(dx[n * J + j])) ++failures;
            if (constant && (G == 2 || G == 4) && (x[n * J + j] - mu != 0.0f || gx != 0.0f)) ++failures;      // d = 0 exactly
        }
    }
    const float s = (float)(s_got / J), dgs = (float)(dgs_got / ((double)G * J));
    w.s = (double)(fabsl(s - s_ref / J) / bound(s_ref / J, s_abs / J, 1));
    w.dgs = (double)(fabsl(dgs - dgs_ref / ((ld)G * J)) / bound(dgs_ref / ((ld)G * J), dgs_abs / ((ld)G * J), 1));
    return w;
}

int main() {
    std::mt19937 rng(12345);
    std::normal_distribution<float> normal(0.f, 1.f);
    int cases = 0, failures = 0;
    const char* families[] = {"random", "pixelnormed", "large", "constant_group"};
    for (int G : {1, 2, 3, 4, 8})
        for (int J : {4, 20, 64, 1152})
            for (int f = 0; f < 4; ++f) {
                std::vector<float> x((size_t)G * J), h((size_t)G * J), gs(G);
                for (auto& v : x) v = normal(rng);
                for (auto& v : h) v = normal(rng);
                for (auto& v : gs) v = normal(rng);
                if (f == 1)             // rows of 4 features with unit RMS
                    for (size_t i = 0; i + 3 < x.size(); i += 4) {
                        const float r = std::sqrt((x[i] * x[i] + x[i + 1] * x[i + 1] + x[i + 2] * x[i + 2] + x[i + 3] * x[i + 3]) / 4);
                        for (int k = 0; k < 4; ++k) x[i + k] /= r;
                    }
                if (f == 2)
                    for (auto& v : x) v *= 1e3f;
                if (f == 3)
                    for (int n = 1; n < G; ++n) std::copy(x.begin(), x.begin() + J, x.begin() + (size_t)n * J);
                const Worst w = check_group(x, h, gs, G, J, f == 3, failures);
                const bool ok = w.s <= 1 && w.gx <= 1 && w.dgs <= 1 && w.dx <= 1;
                failures += !ok;
                ++cases;
                std::printf("G=%d J=%-5d %-15s err / bound: s %.3f  gx %.3f  dgs %.3f  dx %.3f   %s\n", G, J, families[f], w.s, w.gx, w.dgs, w.dx,
                            ok ? "within the bound of the long double loop" : "OUTSIDE THE BOUND");
            }
    // the field's tap sums: every pixel of H x W images against a loop over the zero-padded plane
    for (int H = 1; H <= 5; ++H)
        for (int W = 1; W <= 5; ++W) {
            float w9[9];
            for (auto& v : w9) v = normal(rng);
            double worst = 0;
            int classes[10] = {0};
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    std::vector<ld> plane((size_t)(H + 2) * (W + 2), 0.0L);          // 1 inside, 0 on the padding ring
                    for (int yy = 0; yy < H; ++yy)
                        for (int xx = 0; xx < W; ++xx) plane[(size_t)(yy + 1) * (W + 2) + xx + 1] = 1.0L;
                    ld ref = 0, a = 0;
                    int n = 0;
                    for (int ky = 0; ky < 3; ++ky)
                        for (int kx = 0; kx < 3; ++kx) {
                            const ld inside = plane[(size_t)(y + ky) * (W + 2) + x + kx];
                            ref += inside * w9[ky * 3 + kx], a += inside * fabsl((ld)w9[ky * 3 + kx]), n += inside != 0;
                            if ((inside != 0) != (mbstd::tap_inside(ky, y, H) && mbstd::tap_inside(kx, x, W))) ++failures;
                        }
                    ++classes[n];
                    worst = std::max(worst, (double)(fabsl(mbstd::field_taps(w9, y, x, H, W) - ref) / bound(ref, a, 1)));
                }
            const bool ok = worst <= 1;
            failures += !ok;
            ++cases;
            std::printf("field taps %d x %d: pixels with 1/2/3/4/6/9 taps inside %d/%d/%d/%d/%d/%d  err / bound %.3f   %s\n", H, W, classes[1],
                        classes[2], classes[3], classes[4], classes[6], classes[9], worst,
                        ok ? "equal to the zero-padded plane within the bound" : "OUTSIDE THE BOUND");
        }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures != 0;
}
