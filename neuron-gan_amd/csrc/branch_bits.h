// Integer pieces of the arbor branch graph (branch.hip), written so that the same text runs in a kernel and, serially, in a plain host
// program (tools/branch_host_check.cpp compares them with a flood fill over the classified edges).
//
// Graph.  The vertices are the set pixels; the edges are those ngan_skel_counts counts: horizontal and vertical neighbours (orth), and
// diagonal neighbours neither of whose two common 4-neighbours is set (diag).  A pixel's edges are held as one byte, bit k for the
// neighbour in direction k, clockwise from east: 0 E, 1 SE, 2 S, 3 SW, 4 W, 5 NW, 6 N, 7 NE.  Even directions are orth, odd ones diag;
// the directions 0 .. 3 lead to a larger linear index ("forward": an edge is named once, at its smaller end), k ^ 4 is the way back.
// deg is the number of set bits.  A pixel of deg >= 3 is a node pixel, one of deg <= 2 a branch pixel; an edge is a node edge, a branch
// edge or an attachment as its ends are two node pixels, two branch pixels or one of each.
// Records.  A branch's record is one 64-bit word that only ever receives integer adds: pixels n, orth edges o, diag edges d (20 bits
// each: n <= 2^18 and o + d <= n + 1 for a path or a cycle) and attachments a (a <= 2: a branch pixel has at most two edges, and in a
// path of two or more only the two ends have one to spare).  A node's record is its count of attachments whose branch is no spur.
#pragma once

#if defined(__HIPCC__)
#define BRANCH_HD __host__ __device__ inline
#else
#define BRANCH_HD inline
#endif

namespace branch {

typedef unsigned long long u64;

constexpr int STATS = 20, BINS = 64;
enum { S_PIXELS, S_NODE_PIXELS, S_NODES, S_BRANCHES, S_TERMINAL, S_LINKS, S_FREE, S_SPURS, S_TERM_ORTH, S_TERM_DIAG, S_LINK_ORTH,
       S_LINK_DIAG, S_FREE_ORTH, S_FREE_DIAG, S_SPUR_ORTH, S_SPUR_DIAG, S_NODE_ORTH, S_NODE_DIAG, S_LONGEST, S_FORKS };
enum { FREE = 0, SPUR = 1, TERMINAL = 2, LINK = 3 };

BRANCH_HD int dir_dy(int k) { return k >= 1 && k <= 3 ? 1 : (k >= 5 ? -1 : 0); }
BRANCH_HD int dir_dx(int k) { return k == 0 || k == 1 || k == 7 ? 1 : (k >= 3 && k <= 5 ? -1 : 0); }

// the edges of a set pixel from its eight neighbours (non-zero: set), in the order of the directions
BRANCH_HD unsigned edge_mask(const unsigned char nb[8]) {
    unsigned m = 0;
    for (int k = 0; k < 8; k += 2)
        if (nb[k]) m |= 1u << k;
    for (int k = 1; k < 8; k += 2)
        if (nb[k] && !nb[k - 1] && !nb[(k + 1) & 7]) m |= 1u << k;
    return m;
}

BRANCH_HD int degree(unsigned edges) {
    int n = 0;
    for (unsigned e = edges & 255u; e; e &= e - 1) ++n;
    return n;
}

BRANCH_HD bool is_node(unsigned edges) { return degree(edges) >= 3; }

// floor(sqrt(v)), exact for every 64-bit v: one bit of the root per step, from the top
BRANCH_HD u64 isqrt(u64 v) {
    u64 r = 0;
    for (u64 bit = 1ull << 62; bit; bit >>= 2) {
        if (v >= r + bit) {
            v -= r + bit;
            r = (r >> 1) + bit;
        } else {
            r >>= 1;
        }
    }
    return r;
}

// the floor length of o orth and d diag edges: o + floor(d sqrt 2)
BRANCH_HD int floor_length(int o, int d) { return o + (int)isqrt(2ull * (u64)d * (u64)d); }

BRANCH_HD int branch_class(int a, int n, int spur) { return a == 0 ? FREE : a >= 2 ? LINK : n < spur ? SPUR : TERMINAL; }

// the histogram bin of a branch of floor length L in an R x R image
BRANCH_HD int length_bin(int L, int R) {
    const int w = R / 128 > 1 ? R / 128 : 1, b = L / w;
    return b < BINS - 1 ? b : BINS - 1;
}

// what one branch pixel adds to its branch's record
BRANCH_HD u64 record(int n, int o, int d, int a) { return (u64)n | ((u64)o << 20) | ((u64)d << 40) | ((u64)a << 60); }
BRANCH_HD int record_n(u64 r) { return (int)(r & 0xfffffull); }
BRANCH_HD int record_o(u64 r) { return (int)((r >> 20) & 0xfffffull); }
BRANCH_HD int record_d(u64 r) { return (int)((r >> 40) & 0xfffffull); }
BRANCH_HD int record_a(u64 r) { return (int)(r >> 60); }

// A branch pixel's share of its branch's record, from its own edges and, in nb_node, the directions whose neighbour is a node pixel:
// itself, every attachment, and every branch edge it names (the forward ones).
BRANCH_HD u64 pixel_record(unsigned edges, unsigned nb_node) {
    int o = 0, d = 0, a = 0;
    for (int k = 0; k < 8; ++k) {
        if (!((edges >> k) & 1u)) continue;
        const bool attach = (nb_node >> k) & 1u;
        if (!attach && k >= 4) continue;
        if (k & 1) ++d; else ++o;
        if (attach) ++a;
    }
    return record(1, o, d, a);
}

// *p += v and *p = max(*p, v) on counters that many threads of a kernel share
BRANCH_HD void acc_add(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}
BRANCH_HD void acc_max(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}

// adds what a branch root's finished record says to the counters stats[20] and hist[64]
BRANCH_HD void add_branch(u64 rec, int spur, int R, int* stats, int* hist) {
    const int n = record_n(rec), o = record_o(rec), d = record_d(rec), cls = branch_class(record_a(rec), n, spur);
    const int count[4] = {S_FREE, S_SPURS, S_TERMINAL, S_LINKS}, orth[4] = {S_FREE_ORTH, S_SPUR_ORTH, S_TERM_ORTH, S_LINK_ORTH};
    acc_add(stats + S_BRANCHES, 1);
    acc_add(stats + count[cls], 1);
    if (o) acc_add(stats + orth[cls], o);
    if (d) acc_add(stats + orth[cls] + 1, d);
    if (cls != SPUR) {
        const int L = floor_length(o, d);
        if (L) acc_max(stats + S_LONGEST, L);
        if (cls != FREE) acc_add(hist + length_bin(L, R), 1);
    }
}

// adds a node root's finished record, its count of attachments whose branch is no spur
BRANCH_HD void add_node(u64 strong, int* stats) {
    acc_add(stats + S_NODES, 1);
    if (strong >= 3) acc_add(stats + S_FORKS, 1);
}

}  // namespace branch
