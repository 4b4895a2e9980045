// Integer pieces of the arbor geometry (sholl.hip), written so that the same text runs in a kernel and, serially, in a plain host
// program (tools/geom_host_check.cpp compares them with a brute-force distance search and a per-edge loop).
//
// Distance transform.  g(y, x) is the distance from pixel (y, x) to the nearest background pixel of its own column, the rows -1 and R
// counting as background (0 on the background, at most R / 2 elsewhere).  The squared Euclidean distance to the nearest background
// pixel is then min over x' in -1 .. R of g(y, x')^2 + (x - x')^2 with g = 0 in the columns -1 and R.
// Sholl rings.  With the ring step s, the ring index of a pixel at squared distance d2 from the centre is the largest k with
// (k s)^2 <= d2.
// Skeleton edges.  Those ngan_skel_counts counts: horizontal and vertical neighbours, and diagonal neighbours neither of whose two
// common 4-neighbours is set.  Every edge is named at its upper (for a horizontal one: left) pixel.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define GEOM_HD __host__ __device__ inline
#else
#define GEOM_HD inline
#endif

namespace geom {

constexpr int SHOLL_BINS = 91;          // k <= 90 for every R in 16 .. 1024 and every centre inside the image

// the ring step of an R x R image
GEOM_HD int sholl_step(int R) { return R / 64 > 2 ? R / 64 : 2; }

// min over x' of g2[x'] + (x - x')^2 for one row of squared column distances g2[0 .. R), zero outside: walk d = 1, 2, ... outwards while
// d^2 is below the best so far (nothing further away can improve it).  0 where g2[x] is 0; at most R / 2 steps.
GEOM_HD int row_min(const int* g2, int R, int x) {
    int best = g2[x];
    for (int d = 1; d * d < best; ++d) {
        const int l = x - d >= 0 ? g2[x - d] : 0, r = x + d < R ? g2[x + d] : 0;
        const int c = d * d + (l < r ? l : r);
        best = c < best ? c : best;
    }
    return best;
}

// the largest k with (k s)^2 <= d2, for 0 <= d2 < 2^22 and s >= 1: a float square root seeds it, integer comparisons settle it
GEOM_HD int ring_index(int d2, int s) {
    int k = (int)(sqrtf((float)d2) / (float)s);
    while (k > 0 && (k * s) * (k * s) > d2) --k;
    while ((k + 1) * s * ((k + 1) * s) <= d2) ++k;
    return k;
}

// the edges that start at a set pixel, from its neighbours east, west, south, south-east and south-west (non-zero: set):
// bit 0 east, bit 1 south, bit 2 south-east, bit 3 south-west
enum { EDGE_E = 1, EDGE_S = 2, EDGE_SE = 4, EDGE_SW = 8 };
GEOM_HD int edges_from(int e, int w, int s, int se, int sw) {
    return (e ? EDGE_E : 0) | (s ? EDGE_S : 0) | (se && !e && !s ? EDGE_SE : 0) | (sw && !w && !s ? EDGE_SW : 0);
}

// crossing bin of an edge between pixels of ring index ka and kb: the larger index when they differ, -1 otherwise
GEOM_HD int crossing_bin(int ka, int kb) { return ka == kb ? -1 : (ka > kb ? ka : kb); }

}  // namespace geom
