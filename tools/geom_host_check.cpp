// Runs the integer functions of neuron-gan_amd/csrc/geom_bits.h -- the text the arbor-geometry kernels execute -- serially on the host:
// the column distances are formed by two scans as the kernel forms them, every row goes through geom::row_min, and the squared
// distances are compared with a brute-force search over all background pixels, those of the one-pixel ring outside the image included;
// the soma is compared with a scan for the largest value and smallest index.  The Sholl crossings of the mask taken as a skeleton, about
// the soma and about both far corners, formed pixel by pixel with geom::edges_from, geom::ring_index and geom::crossing_bin, are
// compared with a loop over all pairs of neighbouring pixels written from the definitions in include/ngan.h, the ring index found by
// counting up.  The sanitizers see every index formed.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/geom_host_check.cpp -o geom_host_check
//     ./geom_host_check > profiles/geom_host_check.txt
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../neuron-gan_amd/csrc/geom_bits.h"

typedef std::vector<unsigned char> Mask;
typedef std::array<int, geom::SHOLL_BINS> Bins;

static int at(const Mask& m, int R, int y, int x) { return y >= 0 && y < R && x >= 0 && x < R && m[y * R + x] ? 1 : 0; }

// ---- the definitions, pixel by pixel ---------------------------------------------------------------------------------------------------
static std::vector<int> edt_brute(const Mask& m, int R) {
    std::vector<int> out(R * R, 0);
    for (int y = 0; y < R; ++y)
        for (int x = 0; x < R; ++x) {
            if (!m[y * R + x]) continue;
            int best = 1 << 30;
            for (int qy = -1; qy <= R; ++qy)
                for (int qx = -1; qx <= R; ++qx)
                    if (!at(m, R, qy, qx)) best = std::min(best, (y - qy) * (y - qy) + (x - qx) * (x - qx));
            out[y * R + x] = best;
        }
    return out;
}

static int ring_brute(int d2, int s) {
    int k = 0;
    while ((k + 1) * s * (k + 1) * s <= d2) ++k;
    return k;
}

static Bins crossings_brute(const Mask& m, int R, int cy, int cx) {
    Bins bins{};
    const int s = R / 64 > 2 ? R / 64 : 2;
    auto ring = [&](int y, int x) { return ring_brute((y - cy) * (y - cy) + (x - cx) * (x - cx), s); };
    for (int y = 0; y < R; ++y)
        for (int x = 0; x < R; ++x) {
            if (!at(m, R, y, x)) continue;
            static const int dy[4] = {0, 1, 1, 1}, dx[4] = {1, 0, 1, -1};
            for (int n = 0; n < 4; ++n) {
                const int qy = y + dy[n], qx = x + dx[n];
                if (!at(m, R, qy, qx)) continue;
                if (n >= 2 && (at(m, R, y, qx) || at(m, R, qy, x))) continue;      // a diagonal pair with a common 4-neighbour set
                const int a = ring(y, x), b = ring(qy, qx);
                if (a != b) bins[std::max(a, b)] += 1;
            }
        }
    return bins;
}

// ---- the header ------------------------------------------------------------------------------------------------------------------------
static std::vector<int> edt_header(const Mask& m, int R) {
    std::vector<int> g2(R * R), out(R * R);
    for (int x = 0; x < R; ++x) {
        int d = 0;
        for (int y = 0; y < R; ++y) g2[y * R + x] = d = m[y * R + x] ? d + 1 : 0;
        int u = 0;
        for (int y = R - 1; y >= 0; --y) {
            u = g2[y * R + x] ? u + 1 : 0;
            g2[y * R + x] = std::min(g2[y * R + x], u);
        }
    }
    for (auto& v : g2) v *= v;
    for (int y = 0; y < R; ++y)
        for (int x = 0; x < R; ++x) out[y * R + x] = geom::row_min(g2.data() + y * R, R, x);
    return out;
}

static Bins crossings_header(const Mask& m, int R, int cy, int cx) {
    Bins bins{};
    const int s = geom::sholl_step(R);
    for (int y = 0; y < R; ++y)
        for (int x = 0; x < R; ++x) {
            if (!m[y * R + x]) continue;
            const int edges = geom::edges_from(at(m, R, y, x + 1), at(m, R, y, x - 1), at(m, R, y + 1, x), at(m, R, y + 1, x + 1), at(m, R, y + 1, x - 1));
            const int dy = y - cy, dx = x - cx, k = geom::ring_index(dy * dy + dx * dx, s);
            const int qy[4] = {dy, dy + 1, dy + 1, dy + 1}, qx[4] = {dx + 1, dx, dx + 1, dx - 1};
            for (int n = 0; n < 4; ++n) {
                if (!(edges & (1 << n))) continue;
                const int bin = geom::crossing_bin(k, geom::ring_index(qy[n] * qy[n] + qx[n] * qx[n], s));
                if (bin >= 0) bins.at(bin) += 1;
            }
        }
    return bins;
}

// ---- families --------------------------------------------------------------------------------------------------------------------------
static Mask filled(int R, int (*f)(int, int, int)) {
    Mask m(R * R);
    for (int y = 0; y < R; ++y)
        for (int x = 0; x < R; ++x) m[y * R + x] = f(R, y, x) ? 255 - (x + y) % 3 : 0;   // any non-zero byte is foreground
    return m;
}

static int disc_at(int R, int y, int x, int cy, int cx) { return (y - cy) * (y - cy) + (x - cx) * (x - cx) <= (R / 8) * (R / 8); }

static Mask random_mask(int R, double density, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    Mask m(R * R);
    for (auto& v : m) v = u(rng) < density;
    return m;
}

static Mask walk(int R, unsigned seed, bool soma) {       // random walks from the centre, dilated by a 3 x 3 square
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
        for (int x = 0; x < R; ++x) {
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) out[y * R + x] |= at(m, R, y + dy, x + dx);
            if (soma && disc_at(R, y, x, R / 2, R / 2)) out[y * R + x] = 1;
        }
    return out;
}

int main() {
    int cases = 0, failures = 0;
    for (int R : {16, 32, 64}) {
        std::vector<std::pair<std::string, Mask>> fams = {
            {"empty", Mask(R * R, 0)},
            {"full", Mask(R * R, 1)},
            {"single", filled(R, [](int R, int y, int x) { return y == R - 1 && x == R - 1 ? 1 : 0; })},
            {"hole", filled(R, [](int R, int y, int x) { return y == R / 4 && x == 3 * R / 8 + 1 ? 0 : 1; })},
            {"wedge", filled(R, [](int, int y, int x) { return x > y ? 1 : 0; })},
            {"two_discs", filled(R, [](int R, int y, int x) { return disc_at(R, y, x, R / 4, R / 4) || disc_at(R, y, x, 3 * R / 4, 3 * R / 4) ? 1 : 0; })},
            {"checkerboard", filled(R, [](int, int y, int x) { return (x + y) % 2 == 0 ? 1 : 0; })},
            {"diagonal", filled(R, [](int, int y, int x) { return y == x ? 1 : 0; })},
            {"cross_x", filled(R, [](int R, int y, int x) { return y == x || y + x == R - 1 ? 1 : 0; })},
            {"plus", filled(R, [](int R, int y, int x) { return (y == R / 2 && x >= 2 && x < R - 2) || (x == R / 2 && y >= 2 && y < R - 2) ? 1 : 0; })},
            {"snake", filled(R, [](int R, int y, int x) { return y % 2 == 0 || (y < R - 1 && x == (y % 4 == 1 ? R - 1 : 0)) ? 1 : 0; })},
            {"rings", filled(R, [](int R, int y, int x) { return std::min(std::min(y, x), std::min(R - 1 - y, R - 1 - x)) % 2 == 0 ? 1 : 0; })},
            {"gaps", filled(R, [](int, int, int x) { return x % 64 != 0 ? 1 : 0; })},
            {"frame", filled(R, [](int R, int y, int x) { return y < 3 || x < 3 || y >= R - 3 || x >= R - 3 ? 1 : 0; })},
            {"block2", filled(R, [](int R, int y, int x) { return (y == R / 2 || y == R / 2 - 1) && (x == R / 2 || x == R / 2 - 1) ? 1 : 0; })},
            {"disc", filled(R, [](int R, int y, int x) { return std::hypot(y - 0.5 * (R - 1), x - 0.5 * (R - 1)) <= 0.4 * R ? 1 : 0; })},
            {"walk1", walk(R, 1, false)}, {"walk2", walk(R, 2, false)}, {"soma_walk", walk(R, 3, true)},
            {"random0.20", random_mask(R, 0.2, 1)}, {"random0.41", random_mask(R, 0.41, 2)}, {"random0.60", random_mask(R, 0.6, 3)},
            {"random0.80", random_mask(R, 0.8, 4)}, {"random0.95", random_mask(R, 0.95, 5)}, {"random0.995", random_mask(R, 0.995, 6)}};
        for (auto& f : fams) {
            const Mask& m = f.second;
            const std::vector<int> want = edt_brute(m, R), got = edt_header(m, R);
            int sy = -1, sx = -1, sd = 0;
            for (int p = 0; p < R * R; ++p)
                if (want[p] > sd) sd = want[p], sy = p / R, sx = p % R;
            bool ok = want == got;
            int edges = 0, last = 0;
            const int centres[3][2] = {{sy < 0 ? R / 2 : sy, sy < 0 ? R / 2 : sx}, {0, 0}, {R - 1, R - 1}};
            for (auto& c : centres) {
                const Bins a = crossings_brute(m, R, c[0], c[1]), b = crossings_header(m, R, c[0], c[1]);
                ok &= a == b && a[0] == 0;
                if (&c == &centres[0])
                    for (int k = 0; k < geom::SHOLL_BINS; ++k) {
                        edges += a[k];
                        if (a[k]) last = k;
                    }
            }
            for (int d2 = 0; d2 < 2 * R * R; ++d2) ok &= geom::ring_index(d2, geom::sholl_step(R)) == ring_brute(d2, geom::sholl_step(R));
            ++cases;
            failures += !ok;
            std::printf("R=%-3d %-12s soma=(%d, %d) dist2=%-5d crossings about the soma=%-5d last ring=%-3d %s\n", R, f.first.c_str(), sy, sx, sd,
                        edges, last, ok ? "equal to the brute-force search and the per-edge loop" : "DIFFERENT");
        }
    }
    for (int s : {2, 4, 8, 16}) {                           // the ring index over the whole range the kernels form, for every ring step
        bool ok = true;
        for (int d2 = 0; d2 <= 2 * 1023 * 1023; ++d2) {
            const int k = geom::ring_index(d2, s);
            ok &= (k * s) * (k * s) <= d2 && (k + 1) * s * (k + 1) * s > d2;
        }
        ++cases;
        failures += !ok;
        std::printf("ring index, step %-2d, every squared distance up to 2 * 1023^2: largest %d  %s\n", s, geom::ring_index(2 * 1023 * 1023, s),
                    ok ? "the largest k with (k s)^2 <= d2" : "DIFFERENT");
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
