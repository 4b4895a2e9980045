// Runs the union-find functions of neuron-gan_amd/csrc/morph_uf.h -- the text the labelling kernels execute -- serially on the host, in
// the kernels' three phases (tile labelling from row masks, border merge, flatten), with the pixels of each phase taken in forward,
// reversed and shuffled order, on the snake, checkerboard, corner, gap and random families, for tiles of 8, 16 and 64, and compares the
// labels with a flood fill's canonical ones.  Every loop of the header therefore ends on these inputs in every order tried, and the
// sanitizers see every index it forms.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/morph_host_check.cpp -o morph_host_check
//     ./morph_host_check > profiles/morph_host_check.txt
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../neuron-gan_amd/csrc/morph_uf.h"

using morph::u64;
typedef std::vector<unsigned char> Mask;

static Mask snake(int R) {
    Mask m(R * R, 0);
    for (int y = 0; y < R; ++y) {
        if (y % 2 == 0) std::fill(m.begin() + y * R, m.begin() + (y + 1) * R, 1);
        else m[y * R + (y % 4 == 1 ? R - 1 : 0)] = 1;
    }
    return m;
}

static Mask checkerboard(int R) {
    Mask m(R * R, 0);
    for (int y = 0; y < R; ++y)
        for (int x = 0; x < R; ++x) m[y * R + x] = (x + y) % 2 == 0;
    return m;
}

static Mask corners(int R) {
    Mask m(R * R, 0);
    for (int my = 8; my < R; my += 8)
        for (int mx = 8; mx < R; mx += 8) {
            if (((my + mx) / 8) % 2 == 0) m[(my - 1) * R + mx - 1] = m[my * R + mx] = 1;
            else m[(my - 1) * R + mx] = m[my * R + mx - 1] = 1;
        }
    return m;
}

// every row full except the first column of every 64-pixel tile: a run that ends in bit 63 of a row mask and starts in bit 1
static Mask gaps(int R) {
    Mask m(R * R, 1);
    for (int y = 0; y < R; ++y)
        for (int x = 0; x < R; x += 64) m[y * R + x] = 0;
    return m;
}

static Mask random_mask(int R, double density, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    Mask m(R * R);
    for (auto& v : m) v = u(rng) < density;
    return m;
}

static std::vector<int> flood_fill(const Mask& m, int R) {
    std::vector<int> lab(R * R, -1), stack;
    for (int s = 0; s < R * R; ++s) {
        if (!m[s] || lab[s] >= 0) continue;               // s is the smallest index of its component: the scan is ascending
        lab[s] = s;
        stack.assign(1, s);
        while (!stack.empty()) {
            const int p = stack.back(), y = p / R, x = p % R;
            stack.pop_back();
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int yy = y + dy, xx = x + dx;
                    if (yy < 0 || yy >= R || xx < 0 || xx >= R) continue;
                    const int q = yy * R + xx;
                    if (m[q] && lab[q] < 0) { lab[q] = s; stack.push_back(q); }
                }
        }
    }
    return lab;
}

static std::vector<int> order_of(int n, int mode, unsigned seed) {
    std::vector<int> o(n);
    std::iota(o.begin(), o.end(), 0);
    if (mode == 1) std::reverse(o.begin(), o.end());
    if (mode == 2) std::shuffle(o.begin(), o.end(), std::mt19937(seed));
    return o;
}

// the kernels' phases, serially; tw is the tile (the kernel uses min(R, 64))
static std::vector<int> label(const Mask& m, int R, int tw, int mode, long& invariant_breaks) {
    std::vector<int> labels(R * R, -1);
    const int tiles = R / tw;
    for (int ty = 0; ty < tiles; ++ty)
        for (int tx = 0; tx < tiles; ++tx) {
            std::vector<u64> rows(tw, 0);
            std::vector<int> parent(tw * tw, -1);
            for (int ly = 0; ly < tw; ++ly)
                for (int lx = 0; lx < tw; ++lx)
                    if (m[(ty * tw + ly) * R + tx * tw + lx]) rows[ly] |= 1ull << lx;
            for (int p : order_of(tw * tw, mode, 11)) {
                const int ly = p / tw, lx = p % tw;
                if ((rows[ly] >> lx) & 1ull) parent[p] = ly * tw + morph::uf_run_start(rows[ly], lx);
            }
            for (int p : order_of(tw * tw, mode, 12)) {
                const int ly = p / tw, lx = p % tw;
                if (ly > 0 && ((rows[ly] >> lx) & 1ull)) morph::uf_merge_up(parent.data(), tw, ly, lx, rows[ly], rows[ly - 1]);
            }
            for (int p = 0; p < tw * tw; ++p) {
                if (parent[p] > p) ++invariant_breaks;
                if (parent[p] < 0) continue;
                const int r = morph::uf_find(parent.data(), p);
                labels[(ty * tw + p / tw) * R + tx * tw + p % tw] = (ty * tw + r / tw) * R + tx * tw + r % tw;
            }
        }
    if (tiles > 1) {
        const int half = (tiles - 1) * R;
        for (int i : order_of(2 * half, mode, 13)) {
            if (i < half) morph::uf_merge_border_up(labels.data(), R, tw, (i / R + 1) * tw, i % R);
            else morph::uf_merge_border_left(labels.data(), R, tw, (i - half) % R, ((i - half) / R + 1) * tw);
        }
    }
    for (int p = 0; p < R * R; ++p)
        if (labels[p] > p) ++invariant_breaks;
    for (int p : order_of(R * R, mode, 14))
        if (labels[p] >= 0) labels[p] = morph::uf_find(labels.data(), p);
    return labels;
}

int main() {
    const char* modes[3] = {"forward", "reversed", "shuffled"};
    int failures = 0, cases = 0;
    {                                                     // uf_run_start against the definition: every bit of dense random masks
        std::mt19937_64 rng(5);
        long checked = 0, wrong = 0;
        for (int t = 0; t < 20000; ++t) {
            const u64 m = t < 4 ? (t == 0 ? ~0ull : t == 1 ? ~1ull : t == 2 ? 1ull << 63 : ~(1ull << 62)) : (rng() | rng() | (t % 2 ? rng() : 0));
            for (int x = 0; x < 64; ++x) {
                if (!((m >> x) & 1ull)) continue;
                int s = x;
                while (s > 0 && ((m >> (s - 1)) & 1ull)) --s;
                ++checked;
                wrong += morph::uf_run_start(m, x) != s;
            }
        }
        std::printf("uf_run_start: %ld bits checked, %ld wrong\n", checked, wrong);
        failures += wrong != 0;
    }
    for (int R : {16, 32, 64, 128, 256}) {
        std::vector<std::pair<std::string, Mask>> fams = {{"snake", snake(R)}, {"checkerboard", checkerboard(R)}, {"corners", corners(R)}, {"gaps", gaps(R)},
                                                           {"random0.20", random_mask(R, 0.2, 1)}, {"random0.41", random_mask(R, 0.41, 2)},
                                                           {"random0.60", random_mask(R, 0.6, 3)}};
        for (auto& f : fams) {
            const std::vector<int> want = flood_fill(f.second, R);
            int comps = 0;
            for (int p = 0; p < R * R; ++p) comps += want[p] == p;
            for (int tw : {8, 16, 64}) {
                if (tw > R) continue;
                for (int mode = 0; mode < 3; ++mode) {
                    long breaks = 0;
                    const std::vector<int> got = label(f.second, R, tw, mode, breaks);
                    const bool ok = got == want && breaks == 0;
                    ++cases;
                    failures += !ok;
                    std::printf("R=%-4d %-13s tile=%-3d %-9s components=%-6d parent[i]<=i breaks=%ld  %s\n", R, f.first.c_str(), tw,
                                modes[mode], comps, breaks, ok ? "equal to the flood fill" : "DIFFERENT");
                }
            }
        }
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
