// Integer pieces of the rooted arbor trees (tree.hip), written so that the same text runs in a kernel and, serially, in a plain host
// program (tools/tree_host_check.cpp runs the relaxation in forward, reversed and shuffled pixel order against a priority-queue
// Dijkstra).  include/ngtree.h has the definition.
//
// Graph.  That of branch_bits.h: a pixel's edges are one byte, bit k for the neighbour in direction k, clockwise from east: 0 E, 1 SE,
// 2 S, 3 SW, 4 W, 5 NW, 6 N, 7 NE; even directions are orth and weigh 408, odd ones diag and weigh 577.
// Relaxation.  cost[p] is 0 on a root, INF on every other set pixel at the start, and only ever replaced by the smaller
// min(cost[q] + w) over p's neighbours.  Every value a pixel ever holds is the length of some path from its root, so the costs are
// bounded below by the shortest paths; they only fall; and a sweep over all pixels that changes nothing has read only final values and
// so stands at the one fixed point, the shortest paths.  The order in which pixels are visited, and whether a neighbour's value is this
// sweep's or the last one's, decides the number of sweeps alone.
#pragma once

#include "branch_bits.h"

#if defined(__HIPCC__)
#define TREE_HD __host__ __device__ inline
#else
#define TREE_HD inline
#endif

namespace tree {

typedef unsigned long long u64;

constexpr int ORTH = 408, DIAG = 577;        // 577 / 408 = sqrt 2 (1 + 1.5e-6); 577 (512^2 - 1) < 2^31
constexpr int INF = 0x7fffffff;              // the cost of a set pixel no front has reached yet
constexpr int STATS = 12;
enum { S_PIXELS, S_TREES, S_ORTH, S_DIAG, S_CYCLES, S_LEAVES, S_TIPS, S_FORKS, S_PATH_MAX, S_MAX_ORDER, S_MAIN_ROOT, S_MAIN_PIXELS };
constexpr u64 NO_KEY = ~0ull;                // the root key of a component before any of its pixels has offered its own

TREE_HD int weight(int k) { return (k & 1) ? DIAG : ORTH; }
TREE_HD int step(int k, int R) { return branch::dir_dy(k) * R + branch::dir_dx(k); }

// the eight directions in the order of the neighbour's linear index: NW N NE W E SW S SE
TREE_HD int by_index(int n) { return (int)((0x56740321u >> (4 * (7 - n))) & 15u); }

// what pixel (y, x) = index offers as its component's root: the squared distance to the centre, then the index
TREE_HD u64 root_key(int y, int x, int cy, int cx, int index) {
    const int dy = y - cy, dx = x - cx;
    return ((u64)(unsigned)(dy * dy + dx * dx) << 32) | (u64)(unsigned)index;
}

// Loads and stores of values that other threads of the workgroup replace meanwhile: whole words, never torn
TREE_HD int ld(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    return *p;
#endif
}
TREE_HD void st(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#else
    *p = v;
#endif
}

// One pull at pixel p, whose edges are `edges`: cost[p] = min(cost[p], cost[q] + w) over its neighbours; true if it fell.  Every
// edge of a pixel leads to a pixel inside the image.
TREE_HD bool relax(int* cost, int p, unsigned edges, int R) {
    const int mine = ld(cost + p);
    int best = mine;
    for (int k = 0; k < 8; ++k) {
        if (!((edges >> k) & 1u)) continue;
        const int c = ld(cost + p + step(k, R));
        if (c != INF && c + weight(k) < best) best = c + weight(k);
    }
    if (best < mine) st(cost + p, best);
    return best < mine;
}

// The parent of a pixel that is no root, from the converged costs: the smallest linear index among the neighbours q with
// cost[q] + w == cost[p]; -1 if there is none (a root).
TREE_HD int settle_parent(const int* cost, int p, unsigned edges, int R) {
    const int mine = cost[p];
    for (int n = 0; n < 8; ++n) {
        const int k = by_index(n);
        if (!((edges >> k) & 1u)) continue;
        const int q = p + step(k, R), c = cost[q];
        if (c != INF && c + weight(k) == mine) return q;
    }
    return -1;
}

// children(p): the neighbours whose parent is p
TREE_HD int children(const int* parent, int p, unsigned edges, int R) {
    int n = 0;
    for (int k = 0; k < 8; ++k)
        if (((edges >> k) & 1u) && parent[p + step(k, R)] == p) ++n;
    return n;
}

// Branch order.  Before the sweeps a root holds 0 and every other set pixel -2 - (children(parent) >= 2), "not known yet" with its own
// increment; a pull replaces that by order[parent] + increment once the parent's is known (>= 0).  True if it became known.
TREE_HD int order_unknown(bool parent_forks) { return parent_forks ? -3 : -2; }
TREE_HD bool settle_order(int* order, const int* parent, int p) {
    const int mine = ld(order + p);
    if (mine > -2) return false;
    const int q = parent[p];
    if (q < 0) return false;                 // (no pixel that is "not known yet" is a root)
    const int up = ld(order + q);
    if (up < 0) return false;
    st(order + p, up + (-2 - mine));
    return true;
}

// a tip's term of the contraction: its Euclidean distance from its root over its path length in pixels (cost > 0)
TREE_HD double contraction_term(int p, int root, int cost, int R) {
    const int lr_mask = R - 1;
    int shift = 0;
    while ((1 << shift) < R) ++shift;
    const int dy = (p >> shift) - (root >> shift), dx = (p & lr_mask) - (root & lr_mask);
    return __builtin_sqrt((double)(dy * dy + dx * dx)) / ((double)cost / 408.0);
}

}  // namespace tree
