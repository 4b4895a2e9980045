/* ngtree.h -- arbor skeletons traced into rooted trees: entry points of libngan_hip.so under the prefix ngtree_.  None of ngan.h,
 * nganx.h and ngada.h includes this file: those three headers are frozen.  Same library, same conventions as ngada.h: the entry point
 * returns a status (NGAN_OK or an NGAN_ERR_* of ngan.h, the message in ngan_last_error), the trailing void* is the hipStream_t, device
 * pointers, no state inside the library, and nothing is launched and nothing is written when a status other than NGAN_OK is returned.
 * Python binding: _C.TREE_SIGNATURES and _C.TREE_NON_STATUS; kernels: csrc/tree.hip; per-pixel integer text: csrc/tree_bits.h (which
 * tools/tree_host_check.cpp runs serially on the host); tests/tree_cases.py restates the definition in plain Python; DESIGN.md
 * section 7 has it too.
 *
 * Definition.  It leaves no freedom in any integer output.
 *   input     skeleton (B, R, R) bytes, any mask, non-zero: set.  centre (B, 3) int32 of which {y, x} are read: the layout of
 *             ngan_geom_edt's soma.  R a power of two in 16 .. 512 (the thinning's range), 1 <= B <= 65535.
 *   graph     exactly the one of the branch section of ngan.h: the vertices are the set pixels, the edges the orth pairs (horizontal
 *             or vertical neighbours) and the diag pairs (diagonal neighbours neither of whose two common 4-neighbours is set) that
 *             ngan_skel_counts counts.  Its connected components are the 8-connected components of the mask.  An orth edge weighs 408,
 *             a diag edge 577: 577 / 408 is sqrt 2 to 1.5e-6, and 577 (R^2 - 1) < 2^31 for R <= 512.
 *   roots     in every component the pixel that minimises ((y - cy)^2 + (x - cx)^2, y R + x) lexicographically.  The component whose
 *             root has the smallest such key of the image is the main tree.  An image whose centre lies outside the image -- y < 0 is
 *             the soma of an empty mask, {-1, -1, 0} -- has no root: its pixels get the background values, its statistics are zero
 *             but main_root, which is -1, and its sums are zero.
 *   cost      (B, R, R) int32: -1 on the background; on a set pixel the minimum over the paths from its component's root of
 *             408 (orth edges) + 577 (diag edges).  A path length in pixels is cost / 408.
 *   parent    (B, R, R) int32: -2 on the background, -1 on a root; otherwise the smallest linear index among the graph neighbours q
 *             with cost[q] + w(q, p) == cost[p].  The parent pointers form a spanning forest: every cycle of the graph is broken where
 *             two fronts meet.
 *   order     (B, R, R) int32, or a null pointer (the other outputs are the same bits without it): -1 on the background, 0 on a root;
 *             otherwise order[parent] + (children(parent) >= 2), the centrifugal branch order; children(q) is the number of pixels
 *             whose parent is q.
 *   stats     (B, 12) int32, overwritten:
 *               0 pixels       1 trees: the components     2 orth, 3 diag: the edge counts of ngan_skel_counts
 *               4 cycles: orth + diag - pixels + trees, the cycle rank of the graph
 *               5 leaves: pixels without a child that are no roots, and isolated roots
 *               6 tips: leaves of graph degree <= 1 (the two fronts that meet in a ring are leaves but no tips)
 *               7 forks: pixels with two or more children          8 path_max: the largest cost       9 max_order
 *               10 main_root: a linear index, or -1 without a root  11 main_pixels: the pixels of the main tree
 *   sums      (B, 2) fp64, overwritten: {tip_cost, contraction}.  tip_cost is the sum of cost over the tips, an integer below 2^53 and
 *             so exact in any order.  contraction is the sum over the tips with cost > 0 of
 *                 sqrt((double)|tip - its root|^2) / ((double)cost / 408.0)
 *             every thread adding its tips in ascending pixel order and the partial sums added by a fixed tree, as `roots` in
 *             ngan_geom_sholl: bit-reproducible from call to call.
 * Integers and integer atomics only, except for contraction; no workgroup waits on another; an image's values do not depend on the
 * rest of the batch.  The cost relaxation runs one workgroup per image and as many sweeps as the longest path has edges: R^2 / 2 on a
 * serpentine that fills the image, a few hundred on a neuron's skeleton. */
#ifndef NGTREE_H
#define NGTREE_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace ngtree_trace needs for B images of R x R (17 per pixel), or 0 for a shape outside its domain. */
size_t ngtree_workspace_bytes(int B, int R);

/* Trace B skeletons.  NGAN_ERR_SHAPE for R or B outside the domain above; NGAN_ERR_ARG for a null pointer (order_or_null may be one) and
 * for a pointer off its boundary: 16 bytes for skeleton, cost, parent, order_or_null and workspace, 8 for sums, 4 for centre and
 * stats.  The workspace holds nothing between calls. */
int ngtree_trace(const unsigned char* skeleton, const int* centre, int* cost, int* parent, int* order_or_null, int* stats, double* sums,
                 void* workspace, int B, int R, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NGTREE_H */
