// Runs the integer text of neuron-gan_amd/csrc/tree_bits.h and the union-find of morph_uf.h -- what the arbor-tree kernels execute --
// serially on the host, the passes of tree.hip one after the other with the pixels taken in forward, reversed and shuffled order (the
// order in which a kernel's threads happen to run: the relaxation then reads a mixture of this sweep's and the last sweep's values, as
// the kernel does), and compares cost, parent, order and the twelve statistics with a plain version written from the definition in
// include/ngtree.h: components by flood fill, roots by a loop, costs by a priority-queue Dijkstra, parents and orders from the costs.
// The sanitizers see every index formed.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/tree_host_check.cpp -o tree_host_check
//     ./tree_host_check > profiles/tree_host_check.txt
#include <algorithm>
#include <array>
#include <cstdio>
#include <functional>
#include <numeric>
#include <queue>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../neuron-gan_amd/csrc/morph_uf.h"
#include "../neuron-gan_amd/csrc/tree_bits.h"

typedef std::vector<unsigned char> Mask;
typedef unsigned long long u64;

struct Result {
    std::vector<int> cost, parent, order;
    std::array<int, tree::STATS> stats{};
    u64 tip_cost = 0;
    int sweeps = 0;
    bool operator==(const Result& o) const {
        return cost == o.cost && parent == o.parent && order == o.order && stats == o.stats && tip_cost == o.tip_cost;
    }
};

static int at(const Mask& m, int R, int y, int x) { return y >= 0 && y < R && x >= 0 && x < R && m[y * R + x] ? 1 : 0; }

// ---- the definition ----------------------------------------------------------------------------------------------------------------------
struct Edge {
    int p, q, w;
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
                out.push_back({y * R + x, qy * R + qx, n >= 2 ? 577 : 408});
            }
        }
    return out;
}

static Result plain(const Mask& m, int R, int cy, int cx) {
    const int P = R * R;
    Result r;
    r.cost.assign(P, -1), r.parent.assign(P, -2), r.order.assign(P, -1);
    r.stats[tree::S_MAIN_ROOT] = -1;
    if (cy < 0 || cy >= R || cx < 0 || cx >= R) return r;
    const std::vector<Edge> edges = edges_of(m, R);
    std::vector<std::vector<std::pair<int, int>>> adj(P);
    for (const Edge& e : edges) adj[e.p].push_back({e.q, e.w}), adj[e.q].push_back({e.p, e.w});
    auto key = [&](int p) { return std::make_pair((p / R - cy) * (p / R - cy) + (p % R - cx) * (p % R - cx), p); };
    std::vector<int> comp(P, -1), root_of_comp;
    for (int p = 0; p < P; ++p) {                           // 8-connected flood fill: the components of the mask
        if (!m[p] || comp[p] >= 0) continue;
        const int c = (int)root_of_comp.size();
        int best = p;
        std::vector<int> stack{p};
        comp[p] = c;
        while (!stack.empty()) {
            const int v = stack.back();
            stack.pop_back();
            if (key(v) < key(best)) best = v;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int y = v / R + dy, x = v % R + dx;
                    if (at(m, R, y, x) && comp[y * R + x] < 0) comp[y * R + x] = c, stack.push_back(y * R + x);
                }
        }
        root_of_comp.push_back(best);
    }
    typedef std::pair<int, int> Item;
    std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
    std::vector<int> cost(P, tree::INF);
    for (int p : root_of_comp) cost[p] = 0, heap.push({0, p});
    while (!heap.empty()) {
        const Item it = heap.top();
        heap.pop();
        if (it.first > cost[it.second]) continue;
        for (auto& e : adj[it.second])
            if (it.first + e.second < cost[e.first]) cost[e.first] = it.first + e.second, heap.push({cost[e.first], e.first});
    }
    std::vector<int> kids(P, 0), by_cost;
    int main_root = -1;
    for (int p = 0; p < P; ++p) {
        if (!m[p]) continue;
        by_cost.push_back(p);
        r.cost[p] = cost[p];
        r.parent[p] = -1;
        if (cost[p] == 0) {
            if (main_root < 0 || key(p) < key(main_root)) main_root = p;
            continue;
        }
        int best = P;
        for (auto& e : adj[p])
            if (cost[e.first] + e.second == cost[p]) best = std::min(best, e.first);
        r.parent[p] = best;
        ++kids[best];
    }
    std::sort(by_cost.begin(), by_cost.end(), [&](int a, int b) { return std::make_pair(cost[a], a) < std::make_pair(cost[b], b); });
    for (int p : by_cost) r.order[p] = r.parent[p] < 0 ? 0 : r.order[r.parent[p]] + (kids[r.parent[p]] >= 2);
    auto& s = r.stats;
    for (const Edge& e : edges) ++s[e.w == 577 ? tree::S_DIAG : tree::S_ORTH];
    for (int p : by_cost) {
        ++s[tree::S_PIXELS];
        s[tree::S_TREES] += r.parent[p] == -1;
        s[tree::S_LEAVES] += kids[p] == 0;
        const bool tip = kids[p] == 0 && adj[p].size() <= 1;
        s[tree::S_TIPS] += tip;
        s[tree::S_FORKS] += kids[p] >= 2;
        s[tree::S_PATH_MAX] = std::max(s[tree::S_PATH_MAX], cost[p]);
        s[tree::S_MAX_ORDER] = std::max(s[tree::S_MAX_ORDER], r.order[p]);
        s[tree::S_MAIN_PIXELS] += comp[p] == comp[main_root];
        if (tip) r.tip_cost += (u64)cost[p];
    }
    s[tree::S_CYCLES] = s[tree::S_ORTH] + s[tree::S_DIAG] - s[tree::S_PIXELS] + s[tree::S_TREES];
    s[tree::S_MAIN_ROOT] = main_root;
    return r;
}

// ---- the kernels' passes, serially, pixel i of a pass being order[i] ---------------------------------------------------------------------
static Result header(const Mask& m, int R, int cy, int cx, const std::vector<int>& seq, bool& bounded) {
    const int P = R * R;
    Result r;
    r.cost.assign(P, -1), r.parent.assign(P, -2), r.order.assign(P, -1);
    r.stats[tree::S_MAIN_ROOT] = -1;
    if (cy < 0 || cy >= R || cx < 0 || cx >= R) return r;
    std::vector<int> label(P, -1);
    std::vector<u64> keys(P, tree::NO_KEY);
    std::vector<unsigned char> em(P);
    for (int i : seq) {                                     // tree_edges
        unsigned edges = 0;
        if (m[i]) {
            unsigned char nb[8];
            for (int k = 0; k < 8; ++k) nb[k] = (unsigned char)at(m, R, i / R + branch::dir_dy(k), i % R + branch::dir_dx(k));
            edges = branch::edge_mask(nb);
            label[i] = i;
        }
        em[i] = (unsigned char)edges;
    }
    for (int i : seq)                                       // tree_merge
        for (int k = 4; k < 8; ++k)
            if ((em[i] >> k) & 1u) morph::uf_union(label.data(), i, i + tree::step(k, R));
    for (int p = 0; p < P; ++p) bounded &= m[p] ? label[p] >= 0 && label[p] <= p : label[p] == -1;            // the invariant of morph_uf.h
    for (int i : seq) {                                     // tree_roots
        if (!m[i]) continue;
        const int root = morph::uf_find(label.data(), i);
        label[i] = root;
        keys.at(root) = std::min(keys.at(root), tree::root_key(i / R, i % R, cy, cx, i));
    }
    std::vector<int> root(P, -1);
    for (int i : seq) {                                     // tree_trace: init
        if (!m[i]) continue;
        root[i] = (int)(unsigned)keys.at(label[i]);
        r.cost[i] = root[i] == i ? 0 : tree::INF;
        r.parent[i] = -1;
        r.order[i] = 0;
    }
    for (bool changed = true; changed; ++r.sweeps) {        // relax
        changed = false;
        for (int i : seq)
            if (em[i]) changed |= tree::relax(r.cost.data(), i, em[i], R);
    }
    for (int i : seq)                                       // parents
        if (em[i] && r.cost[i] != 0) r.parent[i] = tree::settle_parent(r.cost.data(), i, em[i], R);
    for (int i : seq)                                       // order
        if (em[i] && r.cost[i] != 0)
            r.order[i] = tree::order_unknown(tree::children(r.parent.data(), r.parent.at(i), em.at(r.parent.at(i)), R) >= 2);
    for (bool changed = true; changed;) {
        changed = false;
        for (int i : seq)
            if (em[i]) changed |= tree::settle_order(r.order.data(), r.parent.data(), i);
    }
    auto& s = r.stats;
    u64 main_key = tree::NO_KEY;
    for (int i : seq) {                                     // counts
        if (!m[i]) continue;
        const int kids = tree::children(r.parent.data(), i, em[i], R);
        const bool tip = kids == 0 && branch::degree(em[i]) <= 1;
        ++s[tree::S_PIXELS];
        s[tree::S_TREES] += r.parent[i] == -1;
        s[tree::S_ORTH] += __builtin_popcount(em[i] & 0x5u);
        s[tree::S_DIAG] += __builtin_popcount(em[i] & 0xau);
        s[tree::S_LEAVES] += kids == 0;
        s[tree::S_TIPS] += tip;
        s[tree::S_FORKS] += kids >= 2;
        s[tree::S_PATH_MAX] = std::max(s[tree::S_PATH_MAX], r.cost[i]);
        s[tree::S_MAX_ORDER] = std::max(s[tree::S_MAX_ORDER], r.order[i]);
        main_key = std::min(main_key, tree::root_key(i / R, i % R, cy, cx, i));
        if (tip && r.cost[i] > 0) {
            r.tip_cost += (u64)r.cost[i];
            const double t = tree::contraction_term(i, root[i], r.cost[i], R);
            bounded &= t > 0.0 && t <= 1.0 + 2e-6;         // a path is no shorter than the straight line, up to 577 / 408 against sqrt 2
        }
    }
    const int main_root = main_key == tree::NO_KEY ? -1 : (int)(unsigned)main_key;
    for (int i : seq) s[tree::S_MAIN_PIXELS] += m[i] && root[i] == main_root;
    s[tree::S_CYCLES] = s[tree::S_ORTH] + s[tree::S_DIAG] - s[tree::S_PIXELS] + s[tree::S_TREES];
    s[tree::S_MAIN_ROOT] = main_root;
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
            {"diagonal", filled(R, [](int, int y, int x) { return y == x ? 1 : 0; })},
            {"cross_x", filled(R, [](int R, int y, int x) { return y == x || y + x == R - 1 ? 1 : 0; })},
            {"plus", filled(R, [](int R, int y, int x) { return (y == R / 2 && x >= 2 && x < R - 2) || (x == R / 2 && y >= 2 && y < R - 2) ? 1 : 0; })},
            {"tee", filled(R, [](int R, int y, int x) { return (y == 4 && x >= 2 && x < R - 2) || (x == R / 2 && y >= 4 && y < R - 2) ? 1 : 0; })},
            {"loop", filled(R, [](int R, int y, int x) {
                 const int a = R / 4, b = 3 * R / 4 - 1;
                 return ((y == a || y == b) && x >= a && x <= b) || ((x == a || x == b) && y >= a && y <= b) || (y == b && x >= b && x < R - 2) ? 1 : 0; })},
            {"ring_tie", filled(R, [](int R, int y, int x) {
                 const int a = R / 4, b = 3 * R / 4;
                 return ((y == a || y == b) && x >= a && x <= b) || ((x == a || x == b) && y >= a && y <= b) ? 1 : 0; })},
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
        const std::vector<std::array<int, 2>> centres = {{R / 2, R / 2}, {R / 4, R / 2}, {R - 1, 0}, {0, R - 1}, {-1, -1}};
        for (auto& f : fams)
            for (auto& c : centres) {
                const Result want = plain(f.second, R, c[0], c[1]);
                bool ok = true, bounded = true;
                int sweeps[3], n = 0;
                for (const std::vector<int>* seq : {&forward, &reversed, &shuffled}) {
                    const Result got = header(f.second, R, c[0], c[1], *seq, bounded);
                    ok &= got == want;
                    sweeps[n++] = got.sweeps;
                }
                const auto& s = want.stats;
                ok &= s[tree::S_CYCLES] >= 0 && s[tree::S_TIPS] <= s[tree::S_LEAVES];
                ++cases;
                failures += !(ok && bounded);
                std::printf("R=%-3d %-12s centre=(%2d,%2d) pixels=%-5d trees=%-4d cycles=%-4d leaves=%-4d tips=%-4d forks=%-4d path_max=%-7d "
                            "order=%-3d main=%-5d sweeps=%d/%d/%d %s\n",
                            R, f.first.c_str(), c[0], c[1], s[tree::S_PIXELS], s[tree::S_TREES], s[tree::S_CYCLES], s[tree::S_LEAVES], s[tree::S_TIPS],
                            s[tree::S_FORKS], s[tree::S_PATH_MAX], s[tree::S_MAX_ORDER], s[tree::S_MAIN_ROOT], sweeps[0], sweeps[1], sweeps[2],
                            !bounded ? "an invariant BROKEN" : ok ? "equal to Dijkstra in forward, reversed and shuffled order" : "DIFFERENT");
            }
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
