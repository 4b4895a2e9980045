// Arbor skeletons traced into rooted trees: the kernels behind metrics.arbor_tree.  The skeleton graph of branch.hip gets a root per
// component -- the pixel nearest the soma --, every pixel its shortest-path cost from that root, its parent on such a path, and its
// centrifugal branch order; the image gets the counts of include/ngtree.h (which has the definition; tree_bits.h has every piece of
// per-pixel integer text, which tools/tree_host_check.cpp runs serially on the host).  Integers and integer atomics only (minima,
// adds and maxima, order-independent), but for `contraction`, which is summed in fp64 in a fixed order: every output is
// bit-reproducible, an image's values never depend on the rest of the batch, and no workgroup waits on another.  Four launches:
//   tree_edges    one thread per pixel, grid (R^2 / 256, B): the edge byte from the 3 x 3 bytes; on a set pixel label[i] = i and an
//                 empty root key
//   tree_merge    the same grid: a pixel joins its tree with the neighbour's along every backward edge (morph_uf.h: lock-free,
//                 label[i] <= i throughout, so every walk is bounded whatever other threads write)
//   tree_roots    the same grid: every set pixel takes its label, the smallest index of its component, and offers its own key
//                 (d2 << 32) | index to the label's entry, a 64-bit atomicMin: the minimum is the component's root
//   tree_trace    one workgroup per image, min(1024, R^2 / 16) threads.
//                 init      cost 0 on roots, INF on other set pixels, the background values elsewhere; every pixel replaces its
//                           label by its root; the pixels with an edge go into a list in LDS, (index | edges << 18), 12288 at most:
//                           skeletons are sparse.  A mask with more (`full`, `checkerboard`) is walked pixel by pixel instead.
//                 relax     sweeps of tree::relax over the list, a barrier after each, until a sweep changes nothing: as many sweeps
//                           as the longest path has edges, plus one.  A pixel writes its own entry alone.
//                 parents   tree::settle_parent from the converged costs
//                 order     every pixel takes its increment, children(parent) >= 2, then sweeps of tree::settle_order until nothing
//                           changes: the depth of the forest in edges, plus one
//                 counts    one pass in ascending pixel order per thread: integer counters in LDS, the contraction terms into a
//                           per-thread fp64 sum, these added by a fixed shuffle tree and then wave by wave
//                 The two sweep counts are left in the first two int32 of the image's slice of the workspace, for tools/tree_time.py.
// Only plain C++: no inline assembly.
#include <cstdint>
#include "ngan_common.h"
#include "../../include/ngtree.h"
#include "morph_uf.h"

#pragma clang fp contract(off)
#include "tree_bits.h"

namespace {

using tree::u64;

constexpr int NT = 256;                 // threads per workgroup of the per-pixel launches
constexpr int TRACE_NT = 1024;          // threads of a tree_trace workgroup at most
constexpr int CAP = 12288;              // entries of the LDS list: 48 KiB
constexpr int R_MIN = 16, R_MAX = 512;  // the thinning's range

bool supported(int R) { return R >= R_MIN && R <= R_MAX && (R & (R - 1)) == 0; }
bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
int log2_of(int R) {
    int l = 0;
    while ((1 << l) < R) ++l;
    return l;
}

__device__ __forceinline__ bool centre_inside(const int* __restrict__ centre, int b, int R, int& cy, int& cx) {
    cy = centre[3L * b];
    cx = centre[3L * b + 1];
    return cy >= 0 && cy < R && cx >= 0 && cx < R;
}

__global__ __launch_bounds__(NT) void tree_edges(const unsigned char* __restrict__ skeleton, int* __restrict__ label,
                                                 u64* __restrict__ keys, unsigned char* __restrict__ em, int R, int lr) {
    const int i = blockIdx.x * NT + threadIdx.x, y = i >> lr, x = i & (R - 1);
    const long image = (long)blockIdx.y << (2 * lr);
    const unsigned char* sk = skeleton + image;
    const bool set = sk[i] != 0;
    unsigned edges = 0;
    if (set) {
        unsigned char nb[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int yy = y + branch::dir_dy(k), xx = x + branch::dir_dx(k);
            nb[k] = yy >= 0 && yy < R && xx >= 0 && xx < R ? sk[(yy << lr) + xx] : 0;
        }
        edges = branch::edge_mask(nb);
    }
    em[image + i] = (unsigned char)edges;
    if (set) {                                                         // background entries of label and keys are never read
        label[image + i] = i;
        keys[image + i] = tree::NO_KEY;
    }
}

__global__ __launch_bounds__(NT) void tree_merge(int* __restrict__ labels, const unsigned char* __restrict__ ems, int R, int lr) {
    const int i = blockIdx.x * NT + threadIdx.x;
    const long image = (long)blockIdx.y << (2 * lr);
    const unsigned edges = ems[image + i];
#pragma unroll
    for (int k = 4; k < 8; ++k)
        if ((edges >> k) & 1u) morph::uf_union(labels + image, i, i + tree::step(k, R));
}

__global__ __launch_bounds__(NT) void tree_roots(const unsigned char* __restrict__ skeleton, const int* __restrict__ centre,
                                                 int* __restrict__ labels, u64* __restrict__ keys, int R, int lr) {
    const int i = blockIdx.x * NT + threadIdx.x;
    const long image = (long)blockIdx.y << (2 * lr);
    int cy, cx;
    if (!centre_inside(centre, blockIdx.y, R, cy, cx) || !skeleton[image + i]) return;
    int* label = labels + image;
    const int root = morph::uf_find(label, i);
    __hip_atomic_store(label + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);               // root <= the entry it replaces
    atomicMin(keys + image + root, tree::root_key(i >> lr, i & (R - 1), cy, cx, i));
}

// f(p, edges) at every pixel of the image that has an edge: from the LDS list, or pixel by pixel where the list did not hold them all
template <typename F>
__device__ __forceinline__ void each_edge_pixel(bool dense, int n, const unsigned* list, const unsigned char* __restrict__ em, int npix,
                                                F f) {
    if (!dense) {
        for (int e = threadIdx.x; e < n; e += blockDim.x) {
            const unsigned w = list[e];
            f((int)(w & 0x3ffffu), w >> 18);
        }
    } else {
        for (int i = threadIdx.x; i < npix; i += blockDim.x) {
            const unsigned m = em[i];
            if (m) f(i, m);
        }
    }
}

// grid (B), threads min(1024, R^2 / 16) (a multiple of 64).  `order` is the caller's array or, without one, a plane of the workspace.
__global__ __launch_bounds__(TRACE_NT) void tree_trace(const unsigned char* __restrict__ skeleton, const int* __restrict__ centre,
                                                       int* costs, int* parents, int* orders, int* __restrict__ stats,
                                                       double* __restrict__ sums, u64* keys_all, int* roots, const unsigned char* __restrict__ ems,
                                                       int R, int lr) {
    __shared__ unsigned list[CAP];
    __shared__ int s_stats[tree::STATS];
    __shared__ int s_count, s_epoch;
    __shared__ u64 s_main, s_tip;
    __shared__ double part[TRACE_NT / 64];
    const int tid = threadIdx.x, nt = blockDim.x, npix = R * R;
    const long image = (long)blockIdx.x << (2 * lr);
    const unsigned char* sk = skeleton + image;
    const unsigned char* em = ems + image;
    int* cost = costs + image;
    int* parent = parents + image;
    int* order = orders + image;
    int* root = roots + image;
    u64* keys = keys_all + image;
    int cy, cx;
    const bool valid = centre_inside(centre, blockIdx.x, R, cy, cx);   // (uniform over the workgroup)
    if (tid < tree::STATS) s_stats[tid] = 0;
    if (tid == 0) {
        s_count = 0;
        s_epoch = -1;
        s_main = tree::NO_KEY;
        s_tip = 0ull;
    }
    __syncthreads();
    for (int i = tid; i < npix; i += nt) {
        if (!valid || !sk[i]) {
            cost[i] = -1;
            parent[i] = -2;
            order[i] = -1;
            continue;
        }
        const int r = (int)(unsigned)keys[root[i]];                    // the low word of the component's smallest key: its root
        root[i] = r;
        cost[i] = r == i ? 0 : tree::INF;
        parent[i] = -1;                                                // stays on the roots
        order[i] = 0;
        const unsigned m = em[i];
        if (m) {
            const int at = atomicAdd(&s_count, 1);
            if (at < CAP) list[at] = (unsigned)i | (m << 18);
        }
    }
    __syncthreads();
    if (!valid) {
        if (tid < tree::STATS) stats[(long)blockIdx.x * tree::STATS + tid] = tid == tree::S_MAIN_ROOT ? -1 : 0;
        if (tid < 2) sums[2L * blockIdx.x + tid] = 0.0;
        return;
    }
    const int n = s_count;
    const bool dense = n > CAP;
    int sweep = 0, relax_sweeps = 0, order_sweeps = 0;

    // A sweep that changed something stores its number; every thread goes on while the number it reads after the barrier is at least
    // the sweep's (a thread that is already in the next sweep can only have raised it).
    for (;; ++sweep) {
        bool changed = false;
        each_edge_pixel(dense, n, list, em, npix, [&](int p, unsigned m) { changed |= tree::relax(cost, p, m, R); });
        if (changed) tree::st(&s_epoch, sweep);
        ++relax_sweeps;
        __syncthreads();
        if (tree::ld(&s_epoch) < sweep) break;
    }
    each_edge_pixel(dense, n, list, em, npix, [&](int p, unsigned m) {
        if (cost[p] != 0) parent[p] = tree::settle_parent(cost, p, m, R);
    });
    __syncthreads();
    each_edge_pixel(dense, n, list, em, npix, [&](int p, unsigned) {
        if (cost[p] == 0) return;
        const int q = parent[p];
        if (q < 0) return;                                             // (converged costs leave no such pixel)
        order[p] = tree::order_unknown(tree::children(parent, q, em[q], R) >= 2);
    });
    __syncthreads();
    for (++sweep;; ++sweep) {
        bool changed = false;
        each_edge_pixel(dense, n, list, em, npix, [&](int p, unsigned) { changed |= tree::settle_order(order, parent, p); });
        if (changed) tree::st(&s_epoch, sweep);
        ++order_sweeps;
        __syncthreads();
        if (tree::ld(&s_epoch) < sweep) break;
    }

    double sum = 0.0;
    for (int i = tid; i < npix; i += nt) {                             // ascending pixel order in every thread
        if (!sk[i]) continue;
        const unsigned m = em[i];
        const int c = cost[i], kids = tree::children(parent, i, m, R), deg = branch::degree(m);
        const bool tip = kids == 0 && deg <= 1;
        atomicAdd(&s_stats[tree::S_PIXELS], 1);
        if (parent[i] == -1) atomicAdd(&s_stats[tree::S_TREES], 1);
        if (m & 0x5u) atomicAdd(&s_stats[tree::S_ORTH], __popc(m & 0x5u));         // the forward edges: E and S,
        if (m & 0xau) atomicAdd(&s_stats[tree::S_DIAG], __popc(m & 0xau));         // SE and SW
        if (kids == 0) atomicAdd(&s_stats[tree::S_LEAVES], 1);                     // (a root without a child is an isolated pixel)
        if (tip) atomicAdd(&s_stats[tree::S_TIPS], 1);
        if (kids >= 2) atomicAdd(&s_stats[tree::S_FORKS], 1);
        atomicMax(&s_stats[tree::S_PATH_MAX], c);
        atomicMax(&s_stats[tree::S_MAX_ORDER], order[i]);
        atomicMin(&s_main, tree::root_key(i >> lr, i & (R - 1), cy, cx, i));
        if (tip && c > 0) {
            atomicAdd(&s_tip, (u64)c);
            sum += tree::contraction_term(i, root[i], c, R);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = sum;
    __syncthreads();
    const int main_root = s_main == tree::NO_KEY ? -1 : (int)(unsigned)s_main;
    int mine = 0;
    for (int i = tid; i < npix; i += nt) mine += sk[i] && root[i] == main_root;
    if (mine) atomicAdd(&s_stats[tree::S_MAIN_PIXELS], mine);
    __syncthreads();
    if (tid < tree::STATS) {
        int v = s_stats[tid];
        if (tid == tree::S_CYCLES) v = s_stats[tree::S_ORTH] + s_stats[tree::S_DIAG] - s_stats[tree::S_PIXELS] + s_stats[tree::S_TREES];
        if (tid == tree::S_MAIN_ROOT) v = main_root;
        stats[(long)blockIdx.x * tree::STATS + tid] = v;
    }
    if (tid == 0) {
        double total = 0.0;
        for (int w = 0; w < nt / 64; ++w) total += part[w];
        sums[2L * blockIdx.x] = (double)s_tip;
        sums[2L * blockIdx.x + 1] = total;
        int* note = reinterpret_cast<int*>(keys);                      // the keys are spent: the sweep counts, for the timing tool
        note[0] = relax_sweeps;
        note[1] = order_sweeps;
    }
}

}  // namespace

extern "C" size_t ngtree_workspace_bytes(int B, int R) {
    if (!supported(R) || B <= 0 || B >= 65536) return 0;
    return (size_t)B * R * R * (sizeof(u64) + 2 * sizeof(int) + 1);    // per pixel: the root key, the label, the order and the edge byte
}

extern "C" int ngtree_trace(const unsigned char* skeleton, const int* centre, int* cost, int* parent, int* order_or_null, int* stats,
                            double* sums, void* workspace, int B, int R, void* stream) {
    NGAN_REQUIRE(skeleton && centre && cost && parent && stats && sums, NGAN_ERR_ARG, "ngtree_trace: null pointer");
    NGAN_REQUIRE(workspace, NGAN_ERR_ARG, "ngtree_trace: null workspace (ngtree_workspace_bytes names its size)");
    NGAN_REQUIRE(supported(R), NGAN_ERR_SHAPE, "ngtree_trace: R=%d unsupported (a power of two, 16 .. 512)", R);
    NGAN_REQUIRE(B > 0 && B < 65536, NGAN_ERR_SHAPE, "ngtree_trace: B=%d unsupported (1 .. 65535 images per call)", B);
    NGAN_REQUIRE(aligned(skeleton, 16) && aligned(cost, 16) && aligned(parent, 16) && aligned(order_or_null, 16) && aligned(workspace, 16) &&
                     aligned(sums, 8) && aligned(centre, 4) && aligned(stats, 4),
                 NGAN_ERR_ARG,
                 "ngtree_trace: skeleton, cost, parent, order and workspace must start on a 16-byte boundary, sums on an 8-byte one, centre "
                 "and stats on a 4-byte one");
    hipStream_t s = (hipStream_t)stream;
    const int lr = log2_of(R);
    const size_t all = (size_t)B * R * R;
    u64* keys = static_cast<u64*>(workspace);
    int* label = reinterpret_cast<int*>(keys + all);
    int* order = reinterpret_cast<int*>(label + all);
    unsigned char* em = reinterpret_cast<unsigned char*>(order + all);
    const dim3 grid(R * R / NT, B), block(NT);
    hipLaunchKernelGGL(tree_edges, grid, block, 0, s, skeleton, label, keys, em, R, lr);
    hipLaunchKernelGGL(tree_merge, grid, block, 0, s, label, em, R, lr);
    hipLaunchKernelGGL(tree_roots, grid, block, 0, s, skeleton, centre, label, keys, R, lr);
    const int chunks = (R * R) >> 4;
    const int nt = chunks < 64 ? 64 : chunks > TRACE_NT ? TRACE_NT : chunks;
    hipLaunchKernelGGL(tree_trace, dim3(B), dim3(nt), 0, s, skeleton, centre, cost, parent, order_or_null ? order_or_null : order, stats, sums,
                       keys, label, em, R, lr);
    return ngan::launch_status("ngtree_trace");
}
