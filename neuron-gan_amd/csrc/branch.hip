// Arbor branch graph of skeletons: the kernels behind metrics.branch_graph.  The skeleton's pixels are cut into nodes (components of
// pixels where three or more edges meet) and branches (paths and cycles of the others), branches are classed as free, spur, terminal
// or link, and nodes that keep three or more branches after spur pruning are counted as forks (include/ngan.h, last section;
// branch_bits.h has the definitions and every piece of integer text, which tools/branch_host_check.cpp runs serially on the host).
// Integers and integer atomics only (adds and maxima, order-independent): every output is bit-reproducible, an image's values never
// depend on the rest of the batch, and no workgroup waits on another.  Five launches, each one thread per pixel, grid (R^2 / 256, B):
//   branch_edges     the edge byte of every pixel from its 3 x 3 bytes; on a set pixel parent[i] = i and a cleared record (the
//                    background's entries are never written or read: a later pass asks the skeleton byte or the edge byte); stats and
//                    hist cleared
//   branch_merge     a pixel joins its tree with the neighbour's along every backward edge that is a node edge or a branch edge
//                    (morph_uf.h: lock-free, parent[i] <= i throughout, so every walk is bounded whatever other threads write)
//   branch_flatten   every pixel takes its root; a branch pixel adds {1, its orth, its diag, its attachments} to the record at its root,
//                    one 64-bit add; pixels, node pixels and node edges go to stats, one add per wave that has any
//   branch_strong    a branch pixel with an attachment reads its branch's finished record and, unless the branch is a spur, adds one to
//                    the record of the node at the other end (a launch of its own: it needs the finished n)
//   branch_reduce    a root adds its branch or node to per-workgroup counters in LDS, which go to stats and hist by one add per
//                    non-zero counter; labels are written here when they are wanted
// Skeletons are sparse: most threads find a background pixel and leave at once, so all five are bound by their one coalesced pass.
// Only plain C++: no inline assembly.
#include <cstdint>
#include "ngan_common.h"
#include "morph_uf.h"
#include "branch_bits.h"

namespace {

using branch::u64;

constexpr int NT = 256;                 // threads per workgroup
constexpr int R_MIN = 16, R_MAX = 512;  // the thinning's range

bool supported(int R) { return R >= R_MIN && R <= R_MAX && (R & (R - 1)) == 0; }
bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
int log2_of(int R) {
    int l = 0;
    while ((1 << l) < R) ++l;
    return l;
}

// the directions of `edges` whose neighbour is a node pixel; every edge of a pixel leads to a pixel inside the image
__device__ __forceinline__ unsigned node_neighbours(const unsigned char* __restrict__ em, int i, int R, unsigned edges) {
    unsigned nb = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if ((edges >> k) & 1u)
            if (branch::is_node(em[i + branch::dir_dy(k) * R + branch::dir_dx(k)])) nb |= 1u << k;
    return nb;
}

__global__ __launch_bounds__(NT) void branch_edges(const unsigned char* __restrict__ skeleton, int* __restrict__ parent,
                                                   u64* __restrict__ rec, unsigned char* __restrict__ em, int* __restrict__ stats,
                                                   int* __restrict__ hist, int R, int lr) {
    const int tid = threadIdx.x, i = blockIdx.x * NT + tid, y = i >> lr, x = i & (R - 1);
    const long image = (long)blockIdx.y << (2 * lr);
    const unsigned char* sk = skeleton + image;
    if (blockIdx.x == 0) {
        if (tid < branch::STATS) stats[(long)blockIdx.y * branch::STATS + tid] = 0;
        if (tid < branch::BINS) hist[(long)blockIdx.y * branch::BINS + tid] = 0;
    }
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
    if (set) {                                                         // background entries of parent and rec are never read
        parent[image + i] = i;
        rec[image + i] = 0ull;
    }
}

__global__ __launch_bounds__(NT) void branch_merge(int* __restrict__ parents, const unsigned char* __restrict__ ems, int R, int lr) {
    const int i = blockIdx.x * NT + threadIdx.x;
    const long image = (long)blockIdx.y << (2 * lr);
    int* parent = parents + image;
    const unsigned char* em = ems + image;
    const unsigned edges = em[i];
    if (!(edges >> 4)) return;                                         // no backward edge (a background pixel has none at all)
    const bool node = branch::is_node(edges);
#pragma unroll
    for (int k = 4; k < 8; ++k) {
        if (!((edges >> k) & 1u)) continue;
        const int q = i + branch::dir_dy(k) * R + branch::dir_dx(k);
        if (branch::is_node(em[q]) == node) morph::uf_union(parent, i, q);
    }
}

__global__ __launch_bounds__(NT) void branch_flatten(const unsigned char* __restrict__ skeleton, int* __restrict__ parents,
                                                     u64* __restrict__ recs, const unsigned char* __restrict__ ems,
                                                     int* __restrict__ stats, int R, int lr) {
    const int i = blockIdx.x * NT + threadIdx.x;
    const long image = (long)blockIdx.y << (2 * lr);
    int* parent = parents + image;
    const unsigned char* em = ems + image;
    int pixels = 0, node_pixels = 0, node_orth = 0, node_diag = 0;
    if (skeleton[image + i]) {
        const int root = morph::uf_find(parent, i);
        __hip_atomic_store(parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // root <= the entry it replaces
        const unsigned edges = em[i], nb = node_neighbours(em, i, R, edges);
        pixels = 1;
        if (branch::is_node(edges)) {
            node_pixels = 1;
            node_orth = __popc(nb & 0x5u);                             // the forward node edges: E and S,
            node_diag = __popc(nb & 0xau);                             // SE and SW
        } else {
            atomicAdd(recs + image + root, branch::pixel_record(edges, nb));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        pixels += __shfl_xor(pixels, o, 64);
        node_pixels += __shfl_xor(node_pixels, o, 64);
        node_orth += __shfl_xor(node_orth, o, 64);
        node_diag += __shfl_xor(node_diag, o, 64);
    }
    if ((threadIdx.x & 63) == 0 && pixels) {
        int* out = stats + (long)blockIdx.y * branch::STATS;
        atomicAdd(out + branch::S_PIXELS, pixels);
        if (node_pixels) atomicAdd(out + branch::S_NODE_PIXELS, node_pixels);
        if (node_orth) atomicAdd(out + branch::S_NODE_ORTH, node_orth);
        if (node_diag) atomicAdd(out + branch::S_NODE_DIAG, node_diag);
    }
}

__global__ __launch_bounds__(NT) void branch_strong(const int* __restrict__ parents, u64* __restrict__ recs,
                                                    const unsigned char* __restrict__ ems, int R, int lr, int spur) {
    const int i = blockIdx.x * NT + threadIdx.x;
    const long image = (long)blockIdx.y << (2 * lr);
    const int* parent = parents + image;
    const unsigned char* em = ems + image;
    u64* rec = recs + image;
    const unsigned edges = em[i];
    if (!edges || branch::is_node(edges)) return;
    const unsigned nb = node_neighbours(em, i, R, edges);
    if (!nb) return;
    const u64 mine = rec[parent[i]];                                   // the flattened entry: the branch's root, whose record is finished
    if (branch::branch_class(branch::record_a(mine), branch::record_n(mine), spur) == branch::SPUR) return;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if ((nb >> k) & 1u) atomicAdd(rec + parent[i + branch::dir_dy(k) * R + branch::dir_dx(k)], 1ull);
}

__global__ __launch_bounds__(NT) void branch_reduce(const unsigned char* __restrict__ skeleton, const int* __restrict__ parents,
                                                    const u64* __restrict__ recs,
                                                    const unsigned char* __restrict__ ems, int* __restrict__ labels,
                                                    int* __restrict__ stats, int* __restrict__ hist, int R, int lr, int spur) {
    __shared__ int s_stats[branch::STATS];
    __shared__ int s_hist[branch::BINS];
    const int tid = threadIdx.x, i = blockIdx.x * NT + tid;
    const long image = (long)blockIdx.y << (2 * lr);
    if (tid < branch::STATS) s_stats[tid] = 0;
    if (tid < branch::BINS) s_hist[tid] = 0;
    __syncthreads();
    const int p = skeleton[image + i] ? parents[image + i] : -1;
    const bool node = branch::is_node(ems[image + i]);                 // (the edge byte of a background pixel is 0)
    if (labels) labels[image + i] = p < 0 ? -1 : node ? -2 - p : p;
    if (p == i) {
        const u64 r = recs[image + i];
        if (node) branch::add_node(r, s_stats);
        else branch::add_branch(r, spur, R, s_stats, s_hist);
    }
    __syncthreads();
    if (tid < branch::STATS && s_stats[tid]) {
        int* out = stats + (long)blockIdx.y * branch::STATS + tid;
        if (tid == branch::S_LONGEST) atomicMax(out, s_stats[tid]);
        else atomicAdd(out, s_stats[tid]);
    }
    if (tid < branch::BINS && s_hist[tid]) atomicAdd(hist + (long)blockIdx.y * branch::BINS + tid, s_hist[tid]);
}

}  // namespace

extern "C" size_t ngan_branch_workspace_bytes(int B, int R) {
    if (!supported(R) || B <= 0 || B >= 65536) return 0;
    return (size_t)B * R * R * (sizeof(u64) + sizeof(int) + 1);        // per pixel: the record, the parent and the edge byte
}

extern "C" int ngan_branch_graph(const unsigned char* skeleton, int* labels_or_null, int* stats, int* hist, void* workspace, int B, int R,
                                 int spur, void* stream) {
    NGAN_REQUIRE(skeleton && stats && hist, NGAN_ERR_ARG, "branch_graph: null pointer");
    NGAN_REQUIRE(workspace, NGAN_ERR_ARG, "branch_graph: null workspace (ngan_branch_workspace_bytes names its size)");
    NGAN_REQUIRE(supported(R), NGAN_ERR_SHAPE, "branch_graph: R=%d unsupported (a power of two, 16 .. 512)", R);
    NGAN_REQUIRE(B > 0 && B < 65536, NGAN_ERR_SHAPE, "branch_graph: B=%d unsupported (1 .. 65535 images per call)", B);
    NGAN_REQUIRE(spur >= 1, NGAN_ERR_ARG, "branch_graph: spur=%d must be at least 1", spur);
    NGAN_REQUIRE(aligned(skeleton, 16) && aligned(labels_or_null, 16) && aligned(workspace, 16) && aligned(stats, 4) && aligned(hist, 4),
                 NGAN_ERR_ARG, "branch_graph: skeleton, labels and workspace must start on a 16-byte boundary, stats and hist on a 4-byte one");
    hipStream_t s = (hipStream_t)stream;
    const int lr = log2_of(R);
    const size_t all = (size_t)B * R * R;
    u64* rec = static_cast<u64*>(workspace);
    int* parent = reinterpret_cast<int*>(rec + all);
    unsigned char* em = reinterpret_cast<unsigned char*>(parent + all);
    const dim3 grid(R * R / NT, B), block(NT);
    hipLaunchKernelGGL(branch_edges, grid, block, 0, s, skeleton, parent, rec, em, stats, hist, R, lr);
    hipLaunchKernelGGL(branch_merge, grid, block, 0, s, parent, em, R, lr);
    hipLaunchKernelGGL(branch_flatten, grid, block, 0, s, skeleton, parent, rec, em, stats, R, lr);
    hipLaunchKernelGGL(branch_strong, grid, block, 0, s, parent, rec, em, R, lr, spur);
    hipLaunchKernelGGL(branch_reduce, grid, block, 0, s, skeleton, parent, rec, em, labels_or_null, stats, hist, R, lr, spur);
    return ngan::launch_status("ngan_branch_graph");
}
