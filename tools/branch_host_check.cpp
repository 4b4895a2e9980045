// Runs the integer text of neuron-gan_amd/csrc/branch_bits.h and the union-find of morph_uf.h -- what the arbor-branch kernels execute --
// serially on the host, the five passes of branch.hip one after the other with the pixels taken in forward, reversed and shuffled order
// (the order in which a kernel's threads happen to run), and compares labels, stats and hist with a plain version written from the
// definitions in include/ngan.h: degrees from a loop over all pairs of neighbouring pixels, nodes and branches by flood fill over the
// classified edges, records by a loop over the edges.  isqrt is compared with a search by multiplication.  The sanitizers see every
// index formed.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/branch_host_check.cpp -o branch_host_check
//     ./branch_host_check > profiles/branch_host_check.txt
#include <algorithm>
#include <array>
#include <cstdio>
#include <numeric>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../neuron-gan_amd/csrc/branch_bits.h"
#include "../neuron-gan_amd/csrc/morph_uf.h"

typedef std::vector<unsigned char> Mask;
typedef unsigned long long u64;

struct Result {
    std::vector<int> labels;
    std::array<int, branch::STATS> stats{};
    std::array<int, branch::BINS> hist{};
    bool operator==(const Result& o) const { return labels == o.labels && stats == o.stats && hist == o.hist; }
};

static int at(const Mask& m, int R, int y, int x) { return y >= 0 && y < R && x >= 0 && x < R && m[y * R + x] ? 1 : 0; }

// ---- the definitions ---------------------------------------------------------------------------------------------------------------------
struct Edge {
    int p, q, diag;
};

static std::vector<Edge> edges_of(const Mask& m, int R) {
    std::vector<Edge> out;
    static const int dy[4] = {0, 1, 1, 1}, dx[4] = {1, 0, 1, -1};
    for (int y = 0; y < R; ++y)
        for (int x = 0; x < R; ++x) {
            if (!at(m, R, y, x)) continue;
            for (int n = 0; n < 4; ++n) {
                const int qy = y + dy[n], qx = x + dx[n];
                if (!at(m, R, qy, qx)) continue;
                if (n >= 2 && (at(m, R, y, qx) || at(m, R, qy, x))) continue;      // a diagonal pair with a common 4-neighbour set
                out.push_back({y * R + x, qy * R + qx, n >= 2});
            }
        }
    return out;
}

static Result plain(const Mask& m, int R, int spur) {
    const int P = R * R;
    const std::vector<Edge> edges = edges_of(m, R);
    std::vector<int> deg(P, 0);
    for (const Edge& e : edges) ++deg[e.p], ++deg[e.q];
    auto node = [&](int p) { return deg[p] >= 3; };
    std::vector<std::vector<int>> same(P);                  // neighbours along node edges and branch edges
    for (const Edge& e : edges)
        if (node(e.p) == node(e.q)) same[e.p].push_back(e.q), same[e.q].push_back(e.p);
    std::vector<int> root(P, -1);
    for (int p = 0; p < P; ++p) {                           // flood fill in index order: the seed is the smallest index of its component
        if (!m[p] || root[p] >= 0) continue;
        std::vector<int> stack{p};
        root[p] = p;
        while (!stack.empty()) {
            const int v = stack.back();
            stack.pop_back();
            for (int w : same[v])
                if (root[w] < 0) root[w] = p, stack.push_back(w);
        }
    }
    Result r;
    r.labels.assign(P, -1);
    std::vector<int> n(P, 0), o(P, 0), d(P, 0), a(P, 0), strong(P, 0);
    for (int p = 0; p < P; ++p) {
        if (!m[p]) continue;
        r.labels[p] = node(p) ? -2 - root[p] : root[p];
        ++r.stats[branch::S_PIXELS];
        if (node(p)) ++r.stats[branch::S_NODE_PIXELS];
        else ++n[root[p]];
    }
    for (const Edge& e : edges) {
        if (node(e.p) && node(e.q)) {
            ++r.stats[e.diag ? branch::S_NODE_DIAG : branch::S_NODE_ORTH];
            continue;
        }
        const int b = root[node(e.p) ? e.q : e.p];
        ++(e.diag ? d : o)[b];
        if (node(e.p) || node(e.q)) ++a[b];
    }
    auto spur_branch = [&](int b) { return a[b] == 1 && n[b] < spur; };
    for (const Edge& e : edges)
        if (node(e.p) != node(e.q) && !spur_branch(root[node(e.p) ? e.q : e.p])) ++strong[root[node(e.p) ? e.p : e.q]];
    for (int p = 0; p < P; ++p) {
        if (!m[p] || root[p] != p) continue;
        if (node(p)) {
            ++r.stats[branch::S_NODES];
            if (strong[p] >= 3) ++r.stats[branch::S_FORKS];
            continue;
        }
        ++r.stats[branch::S_BRANCHES];
        u64 lo = 0;                                         // floor(sqrt(2 d^2)) by counting up
        while ((lo + 1) * (lo + 1) <= 2ull * d[p] * d[p]) ++lo;
        const int L = o[p] + (int)lo, w = std::max(1, R / 128);
        if (a[p] == 0) {
            ++r.stats[branch::S_FREE], r.stats[branch::S_FREE_ORTH] += o[p], r.stats[branch::S_FREE_DIAG] += d[p];
        } else if (a[p] == 2) {
            ++r.stats[branch::S_LINKS], r.stats[branch::S_LINK_ORTH] += o[p], r.stats[branch::S_LINK_DIAG] += d[p];
        } else if (n[p] < spur) {
            ++r.stats[branch::S_SPURS], r.stats[branch::S_SPUR_ORTH] += o[p], r.stats[branch::S_SPUR_DIAG] += d[p];
            continue;
        } else {
            ++r.stats[branch::S_TERMINAL], r.stats[branch::S_TERM_ORTH] += o[p], r.stats[branch::S_TERM_DIAG] += d[p];
        }
        r.stats[branch::S_LONGEST] = std::max(r.stats[branch::S_LONGEST], L);
        if (a[p]) ++r.hist[std::min(branch::BINS - 1, L / w)];
    }
    return r;
}

// ---- the kernels' passes, serially, pixel i of the pass being order[i] -------------------------------------------------------------------
static int step(int R, int i, int k) { return i + branch::dir_dy(k) * R + branch::dir_dx(k); }

static unsigned node_neighbours(const std::vector<unsigned char>& em, int R, int i, unsigned edges) {
    unsigned nb = 0;
    for (int k = 0; k < 8; ++k)
        if (((edges >> k) & 1u) && branch::is_node(em.at(step(R, i, k)))) nb |= 1u << k;
    return nb;
}

static Result header(const Mask& m, int R, int spur, const std::vector<int>& order, bool& bounded) {
    const int P = R * R;
    std::vector<int> parent(P);
    std::vector<u64> rec(P, 0);
    std::vector<unsigned char> em(P);
    Result r;
    for (int i : order) {                                   // branch_edges
        unsigned edges = 0;
        if (m[i]) {
            unsigned char nb[8];
            for (int k = 0; k < 8; ++k) nb[k] = (unsigned char)at(m, R, i / R + branch::dir_dy(k), i % R + branch::dir_dx(k));
            edges = branch::edge_mask(nb);
        }
        parent[i] = m[i] ? i : -1;
        em[i] = (unsigned char)edges;
    }
    for (int i : order) {                                   // branch_merge
        const unsigned edges = em[i];
        const bool node = branch::is_node(edges);
        for (int k = 4; k < 8; ++k) {
            if (!((edges >> k) & 1u)) continue;
            const int q = step(R, i, k);
            if (branch::is_node(em.at(q)) == node) morph::uf_union(parent.data(), i, q);
        }
    }
    for (int p = 0; p < P; ++p) bounded &= m[p] ? parent[p] >= 0 && parent[p] <= p : parent[p] == -1;         // the invariant of morph_uf.h
    for (int i : order) {                                   // branch_flatten
        if (parent[i] < 0) continue;
        const int root = morph::uf_find(parent.data(), i);
        parent[i] = root;
        const unsigned edges = em[i], nb = node_neighbours(em, R, i, edges);
        ++r.stats[branch::S_PIXELS];
        if (branch::is_node(edges)) {
            ++r.stats[branch::S_NODE_PIXELS];
            r.stats[branch::S_NODE_ORTH] += __builtin_popcount(nb & 0x5u);
            r.stats[branch::S_NODE_DIAG] += __builtin_popcount(nb & 0xau);
        } else {
            rec.at(root) += branch::pixel_record(edges, nb);
        }
    }
    for (int i : order) {                                   // branch_strong
        const unsigned edges = em[i];
        if (!edges || branch::is_node(edges)) continue;
        const unsigned nb = node_neighbours(em, R, i, edges);
        if (!nb) continue;
        const u64 mine = rec.at(parent[i]);
        if (branch::branch_class(branch::record_a(mine), branch::record_n(mine), spur) == branch::SPUR) continue;
        for (int k = 0; k < 8; ++k)
            if ((nb >> k) & 1u) rec.at(parent.at(step(R, i, k))) += 1ull;
    }
    r.labels.assign(P, -1);
    for (int i : order) {                                   // branch_reduce
        const int p = parent[i];
        const bool node = p >= 0 && branch::is_node(em[i]);
        r.labels[i] = p < 0 ? -1 : node ? -2 - p : p;
        if (p != i) continue;
        if (node) branch::add_node(rec[i], r.stats.data());
        else branch::add_branch(rec[i], spur, R, r.stats.data(), r.hist.data());
    }
    return r;
}

// ---- masks ---------------------------------------------------------------------------------------------------------------------------------
template <typename F>
static Mask filled(int R, F f) {
    Mask m(R * R);
    for (int y = 0; y < R; ++y)
        for (int x = 0; x < R; ++x) m[y * R + x] = (unsigned char)f(R, y, x);
    return m;
}

static Mask random_mask(int R, double fill, unsigned seed) {
    std::mt19937 rng(seed * 7919u + (unsigned)R);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    Mask m(R * R);
    for (auto& v : m) v = u(rng) < fill ? 255 : 0;
    return m;
}

// a tree of thin random walks that start on the tree
static Mask walk(int R, unsigned seed) {
    std::mt19937 rng(seed * 104729u + (unsigned)R);
    Mask m(R * R, 0);
    std::vector<int> on{R / 2 * R + R / 2};
    m[on[0]] = 1;
    for (int b = 0; b < R / 2; ++b) {
        int p = on[rng() % on.size()], dy = (int)(rng() % 3) - 1, dx = (int)(rng() % 3) - 1;
        for (int s = 0; s < R / 2; ++s) {
            if (rng() % 4 == 0) dy = (int)(rng() % 3) - 1, dx = (int)(rng() % 3) - 1;
            const int y = p / R + dy, x = p % R + dx;
            if (y < 1 || y >= R - 1 || x < 1 || x >= R - 1) break;
            p = y * R + x;
            if (!m[p]) m[p] = 1, on.push_back(p);
        }
    }
    return m;
}

int main() {
    int cases = 0, failures = 0;
    for (int R : {16, 32, 64}) {
        std::vector<std::pair<std::string, Mask>> fams = {
            {"empty", Mask(R * R, 0)}, {"full", Mask(R * R, 1)},
            {"single", filled(R, [](int R, int y, int x) { return y == R / 2 && x == R / 2 ? 7 : 0; })},
            {"row", filled(R, [](int R, int y, int) { return y == R / 2 ? 1 : 0; })},
            {"column", filled(R, [](int R, int, int x) { return x == R - 1 ? 1 : 0; })},
            {"diagonal", filled(R, [](int, int y, int x) { return y == x ? 1 : 0; })},
            {"cross_x", filled(R, [](int R, int y, int x) { return y == x || y + x == R - 1 ? 1 : 0; })},
            {"plus", filled(R, [](int R, int y, int x) { return (y == R / 2 && x >= 2 && x < R - 2) || (x == R / 2 && y >= 2 && y < R - 2) ? 1 : 0; })},
            {"plus3", filled(R, [](int R, int y, int x) { return (std::abs(y - R / 2) <= 1 && x >= 2 && x < R - 2) || (std::abs(x - R / 2) <= 1 && y >= 2 && y < R - 2) ? 1 : 0; })},
            {"tee", filled(R, [](int R, int y, int x) { return (y == 4 && x >= 2 && x < R - 2) || (x == R / 2 && y >= 4 && y < R - 2) ? 1 : 0; })},
            {"double_t", filled(R, [](int R, int y, int x) { return ((y == 4 || y == 7) && x >= 2 && x < R - 2) || (x == R / 2 && y >= 4 && y <= 7) ? 1 : 0; })},
            {"loop", filled(R, [](int R, int y, int x) {
                 const int a = R / 4, b = 3 * R / 4 - 1;
                 return ((y == a || y == b) && x >= a && x <= b) || ((x == a || x == b) && y >= a && y <= b) || (y == b && x >= b && x < R - 2) ? 1 : 0; })},
            {"burrs", filled(R, [](int R, int y, int x) {
                 const int c = R / 2;
                          if ((y == c && x >= 2 && x < R - 2) || (x == c && y >= 2 && y < R - 2)) return 1;
                 if (x % 5 == 4 && std::abs(x - c) >= 3 && x < R - 4 && y < c && y >= c - 1 - (x / 5) % 3) return 1;      // stubs up from the row
                 return 0; })},
            {"block2", filled(R, [](int R, int y, int x) { return (y == R / 2 || y == R / 2 - 1) && (x == R / 2 || x == R / 2 - 1) ? 1 : 0; })},
            {"blocks", filled(R, [](int, int y, int x) { return y % 4 < 2 && x % 4 < 2 ? 1 : 0; })},
            {"frame", filled(R, [](int R, int y, int x) { return y < 3 || x < 3 || y >= R - 3 || x >= R - 3 ? 1 : 0; })},
            {"checkerboard", filled(R, [](int, int y, int x) { return (x + y) % 2 == 0 ? 1 : 0; })},
            {"rings", filled(R, [](int R, int y, int x) { return std::min(std::min(y, x), std::min(R - 1 - y, R - 1 - x)) % 2 == 0 ? 1 : 0; })},
            {"snake", filled(R, [](int R, int y, int x) { return y % 2 == 0 || (y < R - 1 && x == (y % 4 == 1 ? R - 1 : 0)) ? 1 : 0; })},
            {"comb", filled(R, [](int R, int y, int x) { return y == R - 1 || x % 2 == 0 ? 1 : 0; })},
            {"walk1", walk(R, 1)}, {"walk2", walk(R, 2)}, {"walk3", walk(R, 3)},
            {"random0.05", random_mask(R, 0.05, 1)}, {"random0.20", random_mask(R, 0.2, 2)}, {"random0.41", random_mask(R, 0.41, 3)},
            {"random0.60", random_mask(R, 0.6, 4)}, {"random0.80", random_mask(R, 0.8, 5)}, {"random0.95", random_mask(R, 0.95, 6)}};
        std::vector<int> forward(R * R), reversed, shuffled;
        std::iota(forward.begin(), forward.end(), 0);
        reversed.assign(forward.rbegin(), forward.rend());
        shuffled = forward;
        std::shuffle(shuffled.begin(), shuffled.end(), std::mt19937(12345u + (unsigned)R));
        for (auto& f : fams)
            for (int spur : {1, 2, 4}) {
                const Result want = plain(f.second, R, spur);
                bool ok = true, bounded = true;
                for (const std::vector<int>* order : {&forward, &reversed, &shuffled}) ok &= header(f.second, R, spur, *order, bounded) == want;
                const auto& s = want.stats;
                ok &= s[branch::S_BRANCHES] == s[branch::S_TERMINAL] + s[branch::S_LINKS] + s[branch::S_FREE] + s[branch::S_SPURS];
                ++cases;
                failures += !(ok && bounded);
                std::printf("R=%-3d %-12s spur=%d pixels=%-5d nodes=%-4d forks=%-4d terminal=%-4d links=%-4d free=%-4d spurs=%-4d longest=%-4d %s\n", R,
                            f.first.c_str(), spur, s[branch::S_PIXELS], s[branch::S_NODES], s[branch::S_FORKS], s[branch::S_TERMINAL],
                            s[branch::S_LINKS], s[branch::S_FREE], s[branch::S_SPURS], s[branch::S_LONGEST],
                            !bounded ? "parent[i] <= i BROKEN" : ok ? "equal to the flood fill in forward, reversed and shuffled order" : "DIFFERENT");
            }
    }
    {                                                       // isqrt(2 d^2) for every d a branch can have, and at the ends of the range
        bool ok = true;
        for (u64 d = 0; d <= (1ull << 18); ++d) {
            const u64 v = 2 * d * d, r = branch::isqrt(v);
            ok &= r * r <= v && (r + 1) * (r + 1) > v;
        }
        for (u64 v : {0ull, 1ull, 2ull, 3ull, 4ull, (1ull << 32) - 1, 1ull << 32, (1ull << 62) - 1, 1ull << 62, ~0ull}) {
            const u64 r = branch::isqrt(v);
            ok &= r * r <= v && (r >= 0xffffffffull || (r + 1) * (r + 1) > v);
        }
        ++cases;
        failures += !ok;
        std::printf("isqrt(2 d^2), d up to 2^18, and the ends of the 64-bit range: %s\n", ok ? "the largest r with r^2 <= v" : "DIFFERENT");
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
