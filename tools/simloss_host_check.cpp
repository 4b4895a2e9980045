// Host check of csrc/simloss_bits.h, the per-pair arithmetic of the pairwise similarity loss (csrc/simloss.hip) and its slab plan,
// built for the CPU under the address and undefined-behaviour sanitizers:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/simloss_host_check.cpp -o simloss_host_check
// For B = 2 .. 64 (every size up to 9, then 16, 33, 64) and several row lengths, raw and centred, it runs the head's arithmetic
// through the shared functions -- row_mean, centred, pair_terms, mix_diagonal, pair_weight -- on a Gram matrix added up by a plain
// double loop, and checks
//   the plan      gram_plan(B, N): lanes x lanes threads cover B rows, the groups fill a workgroup of 256, the tile is a multiple of
//                 the groups, chunk a multiple of the tile, slabs * chunk covers N with no empty slab, slabs <= 1024; shape_ok at the
//                 domain's edges;
//   the loss      L from pair_terms' d against a plain double loop over the rows divided by their norms (the reference's expression);
//   the gradient  sum_j M_ij x_j - r_i against a central difference of that loop, for a handful of elements;
//   symmetry      A_ij = A_ji bit for bit, a zero diagonal, and sum_j M_ij (x_j - m_j) orthogonal to the constant (centred).
// Tables are exact-size heap buffers: a stray index is the sanitizer's to report.  The record is profiles/simloss_host_check.txt.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../neuron-gan_amd/csrc/simloss_bits.h"

namespace {

long g_checks = 0, g_failures = 0;

void expect(bool ok, const char* what, int B, long N, double a, double b) {
    ++g_checks;
    if (!ok && ++g_failures <= 20) std::printf("FAIL %s (B=%d, N=%ld: %.17g, %.17g)\n", what, B, N, a, b);
}

// the reference's expression by a plain double loop: rows (less their means) divided by their norms, the two cosine matrices, the
// squared difference off the diagonal
double loss_plain(const std::vector<double>& x, const std::vector<double>& z, int B, long N, long K, double lambda, bool center) {
    std::vector<double> xn((size_t)B * N), zn((size_t)B * K);
    for (int i = 0; i < B; ++i) {
        double m = 0.0, q = 0.0;
        if (center) {
            for (long p = 0; p < N; ++p) m += x[i * N + p];
            m /= (double)N;
        }
        for (long p = 0; p < N; ++p) q += (x[i * N + p] - m) * (x[i * N + p] - m);
        for (long p = 0; p < N; ++p) xn[i * N + p] = (x[i * N + p] - m) / std::sqrt(q);
        q = 0.0;
        for (long p = 0; p < K; ++p) q += z[i * K + p] * z[i * K + p];
        for (long p = 0; p < K; ++p) zn[i * K + p] = z[i * K + p] / std::sqrt(q);
    }
    double total = 0.0;
    for (int i = 0; i < B; ++i)
        for (int j = 0; j < B; ++j) {
            if (i == j) continue;
            double s = 0.0, t = 0.0;
            for (long p = 0; p < N; ++p) s += xn[i * N + p] * xn[j * N + p];
            for (long p = 0; p < K; ++p) t += zn[i * K + p] * zn[j * K + p];
            total += (t - s) * (t - s);
        }
    return lambda * total / ((double)B * (double)(B - 1));
}

void gram_plain(const std::vector<double>& x, int B, long N, std::vector<double>& g, std::vector<double>& s) {
    g.assign((size_t)B * B, 0.0);
    s.assign((size_t)B, 0.0);
    for (int i = 0; i < B; ++i) {
        for (long p = 0; p < N; ++p) s[i] += x[i * N + p];
        for (int j = 0; j < B; ++j)
            for (long p = 0; p < N; ++p) g[i * B + j] += x[i * N + p] * x[j * N + p];
    }
}

void check_plan(int B, long N) {
    expect(simloss::shape_ok(B, N), "shape_ok refuses a shape of the domain", B, N, 0, 0);
    const simloss::GramPlan p = simloss::gram_plan(B, N);
    expect(4 * p.lanes >= B && (p.lanes == 1 || 2 * p.lanes < B), "lanes cover B, tightly", B, N, p.lanes, 0);
    expect(p.groups * p.lanes * p.lanes == 256, "groups fill the workgroup", B, N, p.groups, p.lanes);
    expect(p.tile % p.groups == 0 && p.tile % 4 == 0, "tile is a multiple of the groups and of 4", B, N, p.tile, p.groups);
    expect(p.chunk % p.tile == 0 && p.chunk >= 256, "chunk is a multiple of the tile", B, N, (double)p.chunk, p.tile);
    expect((long)p.slabs * p.chunk >= N && (long)(p.slabs - 1) * p.chunk < N, "slabs cover N, none empty", B, N, p.slabs, (double)p.chunk);
    expect(p.slabs >= 1 && p.slabs <= 1024, "at most 1024 slabs", B, N, p.slabs, 0);
    expect((p.tile + 1) * 4 * p.lanes * 4 <= 16640, "the tile (pitch tile + 1) and the 40 KB of accumulators fit 64 KB of LDS", B, N, p.tile, p.lanes);
}

void check_case(int B, long N, long K, bool center, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> uni(-1.f, 1.f);
    std::vector<double> x((size_t)B * N), z((size_t)B * K);
    for (auto& v : x) v = (double)uni(rng) + (center ? 0.5 : 0.0);      // fp32 values, as the kernels read them
    for (auto& v : z) v = (double)uni(rng);
    const double lambda = 0.7;
    std::vector<double> gx, sx, gz, sz;
    gram_plain(x, B, N, gx, sx);
    gram_plain(z, B, K, gz, sz);
    std::vector<double> mean(B), dx(B), M((size_t)B * B), A((size_t)B * B), r(B);
    for (int i = 0; i < B; ++i) {
        mean[i] = simloss::row_mean(sx[i], N, center);
        dx[i] = simloss::centred(gx[i * B + i], N, mean[i], mean[i]);
    }
    const double w = simloss::pair_weight(lambda, B);
    double total = 0.0;
    for (int i = 0; i < B; ++i) {
        double row_c = 0.0, row_d2 = 0.0;
        for (int j = 0; j < B; ++j) {
            const simloss::Pair p = simloss::pair_terms(simloss::centred(gx[i * B + j], N, mean[i], mean[j]), dx[i], dx[j], gz[i * B + j],
                                                        gz[i * B + i], gz[j * B + j], w, i == j);
            A[i * B + j] = p.a;
            M[i * B + j] = p.m_off;
            row_c += p.c;
            row_d2 += p.d * p.d;
            if (i == j) expect(p.d == 0.0 && p.a == 0.0, "the diagonal is excluded exactly", B, N, p.d, p.a);
        }
        M[i * B + i] = simloss::mix_diagonal(row_c, dx[i]);
        total += row_d2;
    }
    for (int i = 0; i < B; ++i) {
        r[i] = 0.0;
        for (int j = 0; j < B; ++j) {
            r[i] += M[i * B + j] * mean[j];
            expect(A[i * B + j] == A[j * B + i], "A is symmetric bit for bit", B, N, A[i * B + j], A[j * B + i]);
        }
    }
    const double L = w * total, ref = loss_plain(x, z, B, N, K, lambda, center);
    expect(std::fabs(L - ref) <= 1e-11 * std::fabs(ref) * (center ? 100 : 1), "L against the plain loop", B, N, L, ref);
    for (int probe = 0; probe < 6; ++probe) {
        const int i = probe % B;
        const long p = (long)((probe * 7919L + 13) % N);
        double g = -r[i], ortho = 0.0;
        for (int j = 0; j < B; ++j) g += M[i * B + j] * x[j * N + p];
        if (center) {
            for (long q = 0; q < N; ++q) {
                double v = 0.0;
                for (int j = 0; j < B; ++j) v += M[i * B + j] * (x[j * N + q] - mean[j]);
                ortho += v;
            }
            expect(std::fabs(ortho) <= 1e-9 * (std::fabs(g) * N + 1e-12), "the gradient row sums to zero (centred)", B, N, ortho, g);
        }
        const double h = 1e-4, keep = x[i * N + p];
        x[i * N + p] = keep + h;
        const double up = loss_plain(x, z, B, N, K, lambda, center);
        x[i * N + p] = keep - h;
        const double down = loss_plain(x, z, B, N, K, lambda, center);
        x[i * N + p] = keep;
        const double fd = (up - down) / (2 * h);
        expect(std::fabs(g - fd) <= 1e-5 * std::fabs(fd) + 1e-10, "gradient element against a central difference", B, N, g, fd);
    }
}

}  // namespace

int main() {
    const int batches[] = {2, 3, 4, 5, 6, 7, 8, 9, 16, 33, 64};
    const long lengths[] = {16, 64, 256, 1024, 4100, 16388, 262144, 1048576, (1L << 31) - 4};
    int cases = 0;
    for (int B : batches)
        for (long N : lengths) check_plan(B, N);
    expect(!simloss::shape_ok(1, 64) && !simloss::shape_ok(65, 64) && !simloss::shape_ok(2, 18) && !simloss::shape_ok(2, 12) &&
               !simloss::shape_ok(2, 1L << 31),
           "shape_ok at the edges", 0, 0, 0, 0);
    for (int B : batches)
        for (long N : {16L, 64L, 260L})
            for (int center = 0; center < 2; ++center, ++cases) check_case(B, N, 32, center != 0, 17u * B + (unsigned)N + center);
    std::printf("simloss_host_check: %d cases (B = 2 .. 64, N = 16, 64, 260, raw and centred), %ld checks, %ld failures\n", cases, g_checks,
                g_failures);
    return g_failures ? 1 : 0;
}
