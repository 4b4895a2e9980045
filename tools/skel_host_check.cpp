// Runs the bit-sliced functions of neuron-gan_amd/csrc/skel_bits.h -- the text the skeleton kernel executes -- serially on the host:
// the mask is packed into 32-bit row words as the kernel packs it, thinned word by word (all deletions of a sub-iteration decided
// before any is applied) and counted, and skeleton, pass count and the six counts are compared with a per-pixel loop written from
// the definitions in include/ngan.h; the counts are also compared on the unthinned mask.  The sanitizers see every index formed.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/skel_host_check.cpp -o skel_host_check
//     ./skel_host_check > profiles/skel_host_check.txt
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../neuron-gan_amd/csrc/skel_bits.h"

using skel::u32;
typedef std::vector<unsigned char> Mask;
typedef std::array<int, 6> Counts;

// ---- the definitions, pixel by pixel ---------------------------------------------------------------------------------------------------
static int at(const Mask& m, int R, int y, int x) { return y >= 0 && y < R && x >= 0 && x < R && m[y * R + x] ? 1 : 0; }

static void ring_of(const Mask& m, int R, int y, int x, int P[10]) {
    static const int dy[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, dx[8] = {0, 1, 1, 1, 0, -1, -1, -1};
    for (int k = 0; k < 8; ++k) P[2 + k] = at(m, R, y + dy[k], x + dx[k]);
}

static int thin_pixels(Mask& m, int R) {
    int passes = 0;
    for (;;) {
        bool changed = false;
        for (int sub = 0; sub < 2; ++sub) {
            Mask next = m;
            for (int y = 0; y < R; ++y)
                for (int x = 0; x < R; ++x) {
                    if (!m[y * R + x]) continue;
                    int P[10];
                    ring_of(m, R, y, x, P);
                    const int C = (!P[2] && (P[3] || P[4])) + (!P[4] && (P[5] || P[6])) + (!P[6] && (P[7] || P[8])) + (!P[8] && (P[9] || P[2]));
                    const int N1 = (P[9] || P[2]) + (P[3] || P[4]) + (P[5] || P[6]) + (P[7] || P[8]);
                    const int N2 = (P[2] || P[3]) + (P[4] || P[5]) + (P[6] || P[7]) + (P[8] || P[9]);
                    const int N = N1 < N2 ? N1 : N2;
                    const int side = sub == 0 ? ((P[2] || P[3] || !P[5]) && P[4]) : ((P[6] || P[7] || !P[9]) && P[8]);
                    if (C == 1 && N >= 2 && N <= 3 && !side) {
                        next[y * R + x] = 0;
                        changed = true;
                    }
                }
            m = next;
            ++passes;
        }
        if (!changed) return passes;
    }
}

static Counts count_pixels(const Mask& m, int R) {
    Counts c{};
    for (int y = 0; y < R; ++y)
        for (int x = 0; x < R; ++x) {
            if (!m[y * R + x]) continue;
            int P[10];
            ring_of(m, R, y, x, P);
            int B = 0, X = 0;
            for (int k = 2; k < 10; ++k) {
                B += P[k];
                X += !P[k] && P[k == 9 ? 2 : k + 1];
            }
            c[0] += 1;
            c[1] += X == 1 && B <= 2;
            c[2] += X >= 3;
            c[3] += B == 0;
            c[4] += P[4] + P[6];
            c[5] += (P[5] && !P[4] && !P[6]) + (P[7] && !P[8] && !P[6]);
        }
    return c;
}

// ---- the header, word by word ----------------------------------------------------------------------------------------------------------
static std::vector<u32> pack(const Mask& m, int R, int wpr) {
    std::vector<u32> bits(R * wpr, 0u);
    for (int i = 0; i < R * wpr; ++i) {
        const int pieces = R >= 32 ? 2 : 1;
        for (int h = 0; h < pieces; ++h) {
            u32 w[4];
            for (int q = 0; q < 4; ++q) {
                w[q] = 0;
                for (int k = 0; k < 4; ++k) w[q] |= (u32)m[(R >= 32 ? 32 * i : 16 * i) + 16 * h + 4 * q + k] << (8 * k);
            }
            bits[i] |= skel::nonzero_bits16(w) << (16 * h);
        }
    }
    return bits;
}

static Mask unpack(const std::vector<u32>& bits, int R, int wpr) {
    Mask m(R * R, 0);
    for (int i = 0; i < R * wpr; ++i) {
        const int pieces = R >= 32 ? 2 : 1;
        for (int h = 0; h < pieces; ++h)
            for (int q = 0; q < 4; ++q) {
                const u32 bytes = skel::bytes_of_nibble((bits[i] >> (16 * h + 4 * q)) & 15u);
                for (int k = 0; k < 4; ++k) m[(R >= 32 ? 32 * i : 16 * i) + 16 * h + 4 * q + k] = (bytes >> (8 * k)) & 255u;
            }
    }
    return m;
}

static int thin_words(std::vector<u32>& bits, int R, int wpr) {
    int passes = 0;
    std::vector<u32> del(bits.size());
    for (;;) {
        bool changed = false;
        for (int sub = 0; sub < 2; ++sub) {
            for (int i = 0; i < R * wpr; ++i) del[i] = bits[i] ? skel::deletable(skel::planes_at(bits.data(), R, wpr, i / wpr, i % wpr), sub) : 0u;
            for (int i = 0; i < R * wpr; ++i) {
                changed |= del[i] != 0u;
                bits[i] &= ~del[i];
            }
            ++passes;
        }
        if (!changed) return passes;
    }
}

static Counts count_words(const std::vector<u32>& bits, int R, int wpr) {
    int c[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < R * wpr; ++i) skel::count_word(skel::planes_at(bits.data(), R, wpr, i / wpr, i % wpr), c);
    return Counts{c[0], c[1], c[2], c[3], c[4], c[5]};
}

// ---- families --------------------------------------------------------------------------------------------------------------------------
static Mask filled(int R, int (*f)(int, int, int)) {
    Mask m(R * R);
    for (int y = 0; y < R; ++y)
        for (int x = 0; x < R; ++x) m[y * R + x] = f(R, y, x) ? 255 - (x + y) % 3 : 0;   // any non-zero byte is foreground
    return m;
}

static int bars(int R, int y, int x) {
    const int c = R / 2;
    bool in = false;
    for (int b = 32; b <= 64; b += 32) {
        if (b == 64 && R < 128) break;
        in |= y >= 1 && y < c - 1 && x >= b - 2 && x <= b;
        in |= y >= c + 1 && y < R - 1 && x >= b - 1 && x <= b + 1;
    }
    return in;
}

static Mask random_mask(int R, double density, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    Mask m(R * R);
    for (auto& v : m) v = u(rng) < density;
    return m;
}

static Mask walk(int R, unsigned seed) {                  // random walks from the centre, dilated by a 3 x 3 square
    std::mt19937 rng(seed);
    Mask m(R * R, 0), out(R * R, 0);
    for (int w = 0; w < 8 + R / 4; ++w) {
        int y = R / 2, x = R / 2;
        for (int s = 0; s < R; ++s) {
            m[y * R + x] = 1;
            y += (int)(rng() % 3) - 1;
            x += (int)(rng() % 3) - 1;
            if (y < 1 || y >= R - 1 || x < 1 || x >= R - 1) break;
        }
    }
    for (int y = 0; y < R; ++y)
        for (int x = 0; x < R; ++x)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) out[y * R + x] |= at(m, R, y + dy, x + dx);
    return out;
}

int main() {
    int cases = 0, failures = 0;
    for (int R : {16, 32, 64, 128}) {
        const int wpr = R >= 32 ? R / 32 : 1;
        std::vector<std::pair<std::string, Mask>> fams = {
            {"empty", Mask(R * R, 0)},
            {"full", Mask(R * R, 1)},
            {"checkerboard", filled(R, [](int, int y, int x) { return (x + y) % 2 == 0 ? 1 : 0; })},
            {"diagonal", filled(R, [](int, int y, int x) { return y == x ? 1 : 0; })},
            {"cross_x", filled(R, [](int R, int y, int x) { return y == x || y + x == R - 1 ? 1 : 0; })},
            {"snake", filled(R, [](int R, int y, int x) { return y % 2 == 0 || (y < R - 1 && x == (y % 4 == 1 ? R - 1 : 0)) ? 1 : 0; })},
            {"rings", filled(R, [](int R, int y, int x) { return std::min(std::min(y, x), std::min(R - 1 - y, R - 1 - x)) % 2 == 0 ? 1 : 0; })},
            {"gaps", filled(R, [](int, int, int x) { return x % 64 != 0 ? 1 : 0; })},
            {"bars_v", filled(R, bars)},
            {"bars_h", filled(R, [](int R, int y, int x) { return bars(R, x, y); })},
            {"frame", filled(R, [](int R, int y, int x) { return y < 3 || x < 3 || y >= R - 3 || x >= R - 3 ? 1 : 0; })},
            {"block2", filled(R, [](int R, int y, int x) { return (y == R / 2 || y == R / 2 - 1) && (x == R / 2 || x == R / 2 - 1) ? 1 : 0; })},
            {"plus3", filled(R, [](int R, int y, int x) {
                 const bool a = std::abs(y - R / 2) <= 1 && x >= 2 && x < R - 2, b = std::abs(x - R / 2) <= 1 && y >= 2 && y < R - 2;
                 return a || b ? 1 : 0; })},
            {"disc", filled(R, [](int R, int y, int x) { return std::hypot(y - 0.5 * (R - 1), x - 0.5 * (R - 1)) <= 0.4 * R ? 1 : 0; })},
            {"walk1", walk(R, 1)}, {"walk2", walk(R, 2)}, {"walk3", walk(R, 3)},
            {"random0.20", random_mask(R, 0.2, 1)}, {"random0.41", random_mask(R, 0.41, 2)}, {"random0.60", random_mask(R, 0.6, 3)},
            {"random0.80", random_mask(R, 0.8, 4)}, {"random0.95", random_mask(R, 0.95, 5)}};
        for (auto& f : fams) {
            const Counts raw_want = count_pixels(f.second, R);
            Mask want = f.second;
            const int passes_want = thin_pixels(want, R);
            const Counts thin_want = count_pixels(want, R);
            std::vector<u32> bits = pack(f.second, R, wpr);
            const Counts raw_got = count_words(bits, R, wpr);
            const int passes_got = thin_words(bits, R, wpr);
            const Counts thin_got = count_words(bits, R, wpr);
            Mask got = unpack(bits, R, wpr);
            bool same = true;
            for (int p = 0; p < R * R; ++p) same &= got[p] == (want[p] ? 1 : 0);
            const bool ok = same && passes_got == passes_want && raw_got == raw_want && thin_got == thin_want;
            ++cases;
            failures += !ok;
            std::printf("R=%-4d %-13s area=%-6d passes=%-4d pixels=%-5d tips=%-4d junctions=%-4d isolated=%-4d orth=%-5d diag=%-5d  %s\n", R,
                        f.first.c_str(), raw_want[0], passes_got, thin_got[0], thin_got[1], thin_got[2], thin_got[3], thin_got[4], thin_got[5],
                        ok ? "equal to the per-pixel loop" : "DIFFERENT");
        }
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
