// Host check of csrc/diffgeo_bits.h, the per-pixel arithmetic of the geometric augmentation (csrc/diffgeo.hip), built for the CPU under
// the address and undefined-behaviour sanitizers:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/diffgeo_host_check.cpp -o diffgeo_host_check
// At R in {4, 8, 16, 32} it runs the forward and the adjoint of every pixel on exact-size heap buffers (a stray index is the
// sanitizer's to report) over the eight blits, theta on a grid that holds +-pi/4, +-pi/2 and +-pi, s at both ends of the scale range and
// at 1, and checks
//   the window    brute force over all pairs: every output pixel whose cell touches an input pixel lies inside that pixel's window;
//   the transpose <T x - T 0, g> = <x, T^T g> to double rounding, and the blits copy bit for bit both ways;
//   the clamps    no window index and no tap that is read leaves the image, also for rows outside the supported range (a zero matrix,
//                 entries of 1e6, infinities and NaN, offsets far off the image).
// The record is profiles/diffgeo_host_check.txt.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#pragma clang fp contract(off)
#include "../neuron-gan_amd/csrc/diffgeo_bits.h"

namespace {

long g_checks = 0, g_failures = 0;

void expect(bool ok, const char* what, int R, int a, int b) {
    ++g_checks;
    if (!ok && ++g_failures <= 20) std::printf("FAIL %s (R=%d, %d, %d)\n", what, R, a, b);
}

geo::Row make_row(int R, bool flip, int k, double s, bool rotate, double theta) {
    // through geo_params' own arithmetic: uniforms that open the wanted gates would quantise s and theta, so restate the composition
    double b00 = 1, b01 = 0, b10 = 0, b11 = 1;
    for (int t = 0; t < k; ++t) {
        const double n00 = -b01, n01 = b00, n10 = -b11, n11 = b10;
        b00 = n00; b01 = n01; b10 = n10; b11 = n11;
    }
    if (flip) { b10 = -b10; b11 = -b11; }
    const double inv = 1.0 / s, co = rotate ? std::cos(theta) : 1.0, sn = rotate ? std::sin(theta) : 0.0;
    double g00 = inv * co, g01 = -(inv * sn), g10 = inv * sn, g11 = inv * co;
    if (sn == 0.0) { g01 = 0.0; g10 = 0.0; }
    const double a00 = b00 * g00 + b01 * g10 + 0.0, a01 = b00 * g01 + b01 * g11 + 0.0;
    const double a10 = b10 * g00 + b11 * g10 + 0.0, a11 = b10 * g01 + b11 * g11 + 0.0;
    const double c = 0.5 * (R - 1);
    return geo::Row{(float)a00, (float)a01, (float)(c - (a00 + a01) * c), (float)a10, (float)a11, (float)(c - (a10 + a11) * c), 0.f, 0.f};
}

// forward and adjoint of a whole plane on exact-size heap buffers
void run_plane(const geo::Row& r, int R, const std::vector<float>& x, const std::vector<float>& g, float fill, std::vector<float>& y,
               std::vector<float>& gx) {
    y.assign((size_t)R * R, 0.f);
    gx.assign((size_t)R * R, 0.f);
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < R; ++j) {
            y[(size_t)i * R + j] = geo::geo_forward(x.data(), r, R, i, j, fill);
            gx[(size_t)i * R + j] = geo::geo_adjoint(g.data(), r, R, i, j);
        }
}

void check_window_holds_every_reader(const geo::Row& r, int R) {
    for (int qi = 0; qi < R; ++qi)
        for (int qj = 0; qj < R; ++qj) {
            const geo::Window w = geo::geo_window(r, R, qi, qj);
            expect(w.ilo > w.ihi || (w.ilo >= 0 && w.ihi < R && w.jlo >= 0 && w.jhi < R), "window leaves the image", R, qi, qj);
            for (int i = 0; i < R; ++i)
                for (int j = 0; j < R; ++j) {
                    const geo::Cell c = geo::geo_cell(r, R, i, j);
                    if (!c.near) continue;
                    const int di = qi - c.i0, dj = qj - c.j0;
                    if (di < 0 || di > 1 || dj < 0 || dj > 1) continue;
                    expect(i >= w.ilo && i <= w.ihi && j >= w.jlo && j <= w.jhi, "a reader outside the window", R, qi * R + qj, i * R + j);
                }
        }
}

void check_regular_row(const geo::Row& r, int R, bool blit, unsigned seed) {
    std::vector<float> x((size_t)R * R), g((size_t)R * R), zero((size_t)R * R, 0.f), y, gx, y0, gx0;
    std::srand(seed);
    for (auto& v : x) v = (float)(std::rand() % 2001 - 1000) / 1000.f;
    for (auto& v : g) v = (float)(std::rand() % 2001 - 1000) / 500.f;
    x[1] = -0.0f;
    g[2] = -0.0f;
    check_window_holds_every_reader(r, R);
    run_plane(r, R, x, g, -1.f, y, gx);
    run_plane(r, R, zero, g, -1.f, y0, gx0);
    double lhs = 0, rhs = 0, scale = 0;
    for (size_t e = 0; e < x.size(); ++e) {
        lhs += ((double)y[e] - (double)y0[e]) * g[e];
        rhs += (double)x[e] * gx[e];
        scale += std::fabs((double)x[e] * gx[e]) + std::fabs((double)y[e] * g[e]) + std::fabs((double)y0[e] * g[e]);
    }
    expect(std::fabs(lhs - rhs) <= 16 * std::ldexp(1.0, -24) * scale, "the adjoint is not the transpose", R, 0, 0);
    if (blit) {                            // a permutation: every value appears once, bit for bit, both ways
        for (int i = 0; i < R; ++i)
            for (int j = 0; j < R; ++j) {
                const geo::Cell c = geo::geo_cell(r, R, i, j);
                expect(c.near && c.ti == 0.0 && c.tj == 0.0 && geo::geo_inside(c.i0, c.j0, R), "a blit with a fraction", R, i, j);
                const size_t p = (size_t)i * R + j, q = (size_t)c.i0 * R + c.j0;
                expect(std::memcmp(&y[p], &x[q], 4) == 0 && std::memcmp(&gx[q], &g[p], 4) == 0, "a blit changed a bit", R, i, j);
            }
    }
}

void check_degenerate_row(const geo::Row& r, int R) {
    std::vector<float> x((size_t)R * R, 0.5f), y, gx;
    run_plane(r, R, x, x, -1.f, y, gx);                                    // the sanitizer watches the exact-size buffers
    for (size_t e = 0; e < y.size(); ++e) expect(std::isfinite(y[e]) && std::isfinite(gx[e]), "a value that is not finite", R, (int)e, 0);
    for (int qi = 0; qi < R; ++qi)
        for (int qj = 0; qj < R; ++qj) {
            const geo::Window w = geo::geo_window(r, R, qi, qj);
            expect(w.ilo > w.ihi || w.jlo > w.jhi || (w.ilo >= 0 && w.ihi < R && w.jlo >= 0 && w.jhi < R), "window leaves the image", R, qi, qj);
            expect((long)(w.ihi - w.ilo + 1) * (w.jhi - w.jlo + 1) <= 64 || w.ilo > w.ihi, "window larger than 8 x 8", R, qi, qj);
            const geo::Cell c = geo::geo_cell(r, R, qi, qj);
            expect(!c.near || (c.i0 >= -1 && c.i0 <= R - 1 && c.j0 >= -1 && c.j0 <= R - 1), "cell off the image", R, qi, qj);
        }
}

}  // namespace

int main() {
    const double pi = 3.14159265358979323846, lo = std::exp2(-0.35), hi = std::exp2(0.35);
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), big = 1e6f;
    int rows = 0;
    for (int R : {4, 8, 16, 32}) {
        for (int f = 0; f < 2; ++f)
            for (int k = 0; k < 4; ++k, ++rows) check_regular_row(make_row(R, f, k, 1.0, false, 0.0), R, true, 17u * R + rows);
        for (double s : {lo, 1.0, hi})
            for (int t = -8; t <= 8; ++t, ++rows)                           // theta = t pi / 8: +-pi/4, +-pi/2, +-pi among them
                check_regular_row(make_row(R, (t & 1) != 0, (t + 8) % 4, s, true, t * pi / 8), R, false, 31u * R + rows);
        for (double th : {1e-3, 2.0, -0.7}) check_regular_row(make_row(R, true, 1, 1.1, true, th), R, false, 5u * R + ++rows);
        // the edge of the supported range: singular values 1/2 and 2
        check_regular_row(make_row(R, false, 0, 2.0, true, pi / 4), R, false, 3u);
        check_regular_row(make_row(R, false, 0, 0.5, true, pi / 4), R, false, 4u);
        const float c = 0.5f * (R - 1);
        const geo::Row degenerate[] = {
            {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, c, 0, 0, c, 0, 0}, {big, big, big, big, big, big, 0, 0}, {big, 0, -big, 0, 1e-6f, c, 0, 0},
            {big, -big, c, big, big, c, 0, 0}, {1, 0, 3e9f, 0, 1, -3e9f, 0, 0}, {inf, 0, 0, 0, 1, 0, 0, 0}, {1, 0, nan, 0, 1, 0, 0, 0},
            {nan, nan, nan, nan, nan, nan, 0, 0}, {1, 0, inf, 0, 1, -inf, 0, 0}, {1e-3f, 0, c, 0, 1e-3f, c, 0, 0}, {3e38f, 3e38f, 0, 3e38f, -3e38f, 0, 0, 0},
            {0.26f, 0, c, 0, 0.26f, c, 0, 0}, {3.9f, 0, -c, 0, 3.9f, -c, 0, 0},
        };
        for (const geo::Row& r : degenerate) {
            check_degenerate_row(r, R);
            ++rows;
        }
        // geo_params: gates closed is the identity, blit-only entries are exact
        for (int u3 = 0; u3 < 4; ++u3)
            for (int fl = 0; fl < 2; ++fl) {
                const float u[8] = {0.f, fl ? 0.25f : 0.75f, 0.f, 0.25f * u3 + 0.1f, 0.9f, 0.3f, 0.9f, 0.3f};
                const geo::Row a = geo::geo_params(u, R, 3, 0.5f), b = make_row(R, fl, u3, 1.0, false, 0.0);
                expect(std::memcmp(&a, &b, sizeof a) == 0, "geo_params blit row", R, u3, fl);
            }
        const float open[8] = {0.9f, 0.f, 0.9f, 0.f, 0.1f, 1.f - 0x1p-24f, 0.1f, 1.f - 0x1p-24f};
        const geo::Row z = geo::geo_params(open, R, 3, 0.5f);
        expect(std::fabs(z.a00 + (float)lo) < 1e-6f && std::fabs(z.a01) < 1e-6f, "geo_params at u = 1 - 2^-24", R, 0, 0);
        const geo::Row id = geo::geo_params(open, R, 3, 0.f), want = make_row(R, false, 0, 1.0, false, 0.0);
        expect(std::memcmp(&id, &want, sizeof id) == 0, "geo_params at p = 0", R, 0, 0);
    }
    std::printf("diffgeo_host_check: %d rows at R in {4, 8, 16, 32}, %ld checks, %ld failures\n", rows, g_checks, g_failures);
    return g_failures ? 1 : 0;
}
