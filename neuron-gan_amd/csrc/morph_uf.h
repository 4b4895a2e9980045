// Union-find pieces of the connected-component labelling (morph.hip), written so that the same text runs in a kernel and, serially,
// in a plain host program (tools/morph_host_check.cpp compares them with a flood fill in forward, reversed and shuffled pixel order).
//
// One array of parents per image, indexed by the linear pixel index; parent[i] == i marks a root, background pixels hold -1 and are
// never entered.  The invariant that bounds every loop here: 0 <= parent[i] <= i for every foreground pixel, at all times.  It holds
// after initialisation (a pixel points at the first pixel of its row run), and the only later writes are min(parent[a], b) with
// b < a, which can only lower an entry.  Labels therefore end as the smallest linear index of the component.
#pragma once

#if defined(__HIPCC__)
#define MORPH_HD __host__ __device__
#else
#define MORPH_HD
#endif

namespace morph {

typedef unsigned long long u64;

MORPH_HD inline int uf_load(const int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return *p;
#endif
}

// *p = min(*p, v); returns the value found
MORPH_HD inline int uf_min(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicMin(p, v);
#else
    const int old = *p;
    if (v < old) *p = v;
    return old;
#endif
}

// the root of i's tree
MORPH_HD inline int uf_find(const int* parent, int i) {
    // Bounded: the loop goes on only with 0 <= p < i, so i strictly decreases and stays a valid index; at most i + 1 steps, whatever
    // other threads write meanwhile (an entry that breaks the invariant ends the walk instead of leaving the array).
    for (;;) {
        const int p = uf_load(parent + i);
        if (p >= i || p < 0) return i;
        i = p;
    }
}

// join the trees of a and b, the larger root under the smaller
MORPH_HD inline void uf_union(int* parent, int a, int b) {
    // Bounded: an iteration either returns or replaces a, the larger of the two roots, by a value found below it (old < a, then its
    // root <= old), while b < a stays: max(a, b) strictly decreases and is >= 0.  Lock-free: no thread waits for another; a thread
    // whose atomicMin lost only goes on with the smaller index it found there.
    // A negative index (a background entry reached through an entry that broke the invariant) ends the union: no index below 0 is
    // ever formed.
    for (;;) {
        if (a < 0 || b < 0) return;
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = uf_min(parent + a, b);         // a was a root: parent[a] == a unless someone was faster
        if (old == a) return;                          // linked a under b
        a = old;                                       // parent[a] is now min(old, b): what is left is to join old and b
    }
}

// first pixel of the run of ones that bit x of the row mask m belongs to (bit x must be set)
MORPH_HD inline int uf_run_start(u64 m, int x) {
    const u64 upto = x == 63 ? ~0ull : (1ull << (x + 1)) - 1ull;       // bits 0 .. x
    const u64 zeros_below = ~m & upto;
    if (zeros_below == 0) return 0;
    return 64 - __builtin_clzll(zeros_below);          // one past the highest zero below x
}

// Inside a tile of row pitch tw: join foreground pixel (ly, lx), ly >= 1, with the row above, given the row masks cur and up.  A run
// of the row above is reached through its pixel straight above where there is one, else through the diagonal ones, and only by the
// first pixel of an overlap: the others are already joined with that pixel through their own row run.
MORPH_HD inline void uf_merge_up(int* parent, int tw, int ly, int lx, u64 cur, u64 up) {
    const int p = ly * tw + lx, q = p - tw;
    const bool cl = lx > 0 && ((cur >> (lx - 1)) & 1ull), cr = lx < 63 && ((cur >> (lx + 1)) & 1ull);
    const bool ul = lx > 0 && ((up >> (lx - 1)) & 1ull), uc = (up >> lx) & 1ull, ur = lx < 63 && ((up >> (lx + 1)) & 1ull);
    if (uc) {
        if (!(cl && ul)) uf_union(parent, p, q);
    } else {
        if (ul && !cl) uf_union(parent, p, q - 1);
        if (ur && !cr) uf_union(parent, p, q + 1);
    }
}

// Across tile borders, on the image's parent array (R x R, tiles of tw x th).  uf_merge_border_up joins foreground pixel (y, x) on the
// first row of a tile with all three neighbours beyond the upper border; uf_merge_border_left joins a pixel on the first column of a
// tile with all three beyond the left border.  Every 8-connected pair of pixels in different tiles is met this way: a pair across a
// vertical border by its right pixel, a pair across a horizontal border alone by its lower pixel.  The two diagonal pairs across a
// tile corner are met by both (the corner pixel's upper-left neighbour, and the pair (y - 1, x), (y, x - 1) from either side): a
// second union of a joined pair finds equal roots and writes nothing.
MORPH_HD inline void uf_merge_border_up(int* parent, int R, int th, int y, int x) {
    const int p = y * R + x;
    if (y <= 0 || y % th != 0 || uf_load(parent + p) < 0) return;
    for (int dx = -1; dx <= 1; ++dx) {
        const int xx = x + dx;
        if (xx < 0 || xx >= R) continue;
        const int q = (y - 1) * R + xx;
        if (uf_load(parent + q) >= 0) uf_union(parent, p, q);
    }
}

MORPH_HD inline void uf_merge_border_left(int* parent, int R, int tw, int y, int x) {
    const int p = y * R + x;
    if (x <= 0 || x % tw != 0 || uf_load(parent + p) < 0) return;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= R) continue;
        const int q = yy * R + x - 1;
        if (uf_load(parent + q) >= 0) uf_union(parent, p, q);
    }
}

}  // namespace morph
