// Arbor morphology of images: the kernels behind metrics.arbor_statistics.  Every result is an integer; the only atomics are integer
// ones (order-independent), so every output is bit-reproducible and an image's values never depend on the rest of the batch.
//   ngan_morph_levels    levels_kernel: 16-byte loads (four pixels per thread and pass), the 8-bit level by one explicit fmaf, four
//                        levels per 4-byte store; per-wave sub-histograms in LDS, one global add per level and workgroup
//   ngan_morph_mask      mask_kernel: level > cut[b], 16 pixels per thread
//   ngan_morph_label     8-connected components with canonical labels (the smallest linear index of the component), union-find
//                        with the invariant parent[i] <= i (morph_uf.h, which also runs serially on the host):
//                          label_tile_kernel     phase 1: a tile of min(R, 64)^2 pixels in LDS.  Row bit masks are built from 16-byte
//                                                loads; a pixel starts at the first pixel of its row run (bit operations on the
//                                                mask), rows are joined by uf_merge_up, the tile is flattened and written out with
//                                                image-wide indices (the order of indices inside a tile is the image's order).
//                          label_border_kernel   phase 2: one thread per pixel on a tile's first row (uf_merge_border_up) or column (_left), on
//                                                the image's label array (lock-free atomicMin union towards the smaller index)
//                          label_flatten_kernel  phase 3: every pixel takes its root; sizes go to the roots, one integer add per
//                                                stretch of equal roots in a wave
//                          label_stats_kernel    phase 3, second launch (it needs the finished sizes; there is no waiting between
//                                                workgroups anywhere): area, counted components, the largest, the kept area, and
//                                                the mask of the counted components
//   ngan_morph_boxcount  box_tile_kernel: a tile of min(R, 128)^2 pixels as 128-bit row masks; per level the rows are OR-ed in
//                        pairs (ping-pong in LDS) and folded sideways with shifts, boxes are popcounts under a stride mask; one
//                        integer add per level and workgroup.  Levels above the tile (R >= 256): every occupied tile sets the bit of
//                        its box in the level's slot of `counts` (at most 16 boxes there), and a second small launch,
//                        box_finish_kernel, replaces each such slot by its popcount.
// Only plain C++: no inline assembly.
#include <cstdint>
#include "ngan_common.h"
#include "morph_uf.h"

#pragma clang fp contract(off)

namespace {

using morph::u64;

constexpr int NT = 256;                 // threads per workgroup
constexpr int TILE = 64;                // labelling tile: one 64-bit mask per row
constexpr int BOX_TILE = 128;           // box-count tile: two 64-bit masks per row
constexpr int LEVELS_MAX_BLOCKS = 32;   // workgroups per image of the level pass at most

bool supported(int R) { return R >= 16 && R <= 1024 && (R & (R - 1)) == 0; }
int log2_of(int R) { int l = 0; while ((1 << l) < R) ++l; return l; }

// bit j = byte j of the 16 bytes is non-zero
__device__ __forceinline__ unsigned nonzero_bits16(uint4 v) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((w[i] >> (8 * k)) & 255u) bits |= 1u << (4 * i + k);
    return bits;
}

__device__ __forceinline__ unsigned level_of(float g) {
    return (unsigned)(int)fminf(fmaxf(fmaf(g, 127.5f, 128.0f), 0.0f), 255.0f);
}

// grid (blocks, B); pixels = R * R, a multiple of 256
template <int C>
__global__ __launch_bounds__(NT) void levels_kernel(const float* __restrict__ images, unsigned char* __restrict__ levels,
                                                    unsigned* __restrict__ hist, int pixels) {
    __shared__ unsigned counts[4 * 256];            // one sub-histogram per wave
    const int tid = threadIdx.x;
    for (int i = tid; i < 4 * 256; i += NT) counts[i] = 0;
    __syncthreads();
    unsigned* sub = counts + (tid >> 6) * 256;
    const long base = (long)blockIdx.y * pixels;
    const int groups = pixels / 4;
    for (int g = blockIdx.x * NT + tid; g < groups; g += gridDim.x * NT) {
        const float* src = images + (base + 4L * g) * C;
        float v[4];
        if (C == 1) {
            const float4 a = ld4(src);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        } else {
            const float4 a = ld4(src), b = ld4(src + 4), c = ld4(src + 8);
            v[0] = (a.x + a.y + a.z) * (1.0f / 3.0f);
            v[1] = (a.w + b.x + b.y) * (1.0f / 3.0f);
            v[2] = (b.z + b.w + c.x) * (1.0f / 3.0f);
            v[3] = (c.y + c.z + c.w) * (1.0f / 3.0f);
        }
        unsigned packed = 0, cur = level_of(v[0]), run = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const unsigned level = level_of(v[m]);
            packed |= level << (8 * m);
            if (level != cur) {                     // equal neighbours share one LDS add
                atomicAdd(sub + cur, run);
                cur = level;
                run = 0;
            }
            ++run;
        }
        atomicAdd(sub + cur, run);
        reinterpret_cast<unsigned*>(levels + base)[g] = packed;
    }
    __syncthreads();
    const unsigned total = counts[tid] + counts[256 + tid] + counts[512 + tid] + counts[768 + tid];
    if (total) atomicAdd(hist + (long)blockIdx.y * 256 + tid, total);
}

// grid (ceil(vecs / NT), B); vecs = R * R / 16
__global__ __launch_bounds__(NT) void mask_kernel(const unsigned char* __restrict__ levels, const int* __restrict__ cut,
                                                  unsigned char* __restrict__ mask, int vecs) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= vecs) return;
    const long at = (long)blockIdx.y * vecs + i;
    const int c = cut[blockIdx.y];
    const uint4 v = reinterpret_cast<const uint4*>(levels)[at];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    unsigned o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o[j] = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((int)((w[j] >> (8 * k)) & 255u) > c) o[j] |= 1u << (8 * k);
    }
    reinterpret_cast<uint4*>(mask)[at] = make_uint4(o[0], o[1], o[2], o[3]);
}

// ---- labelling ----------------------------------------------------------------------------------------------------------------------
// phase 1.  grid (R / tw, R / tw, B), tw = min(R, 64)
__global__ __launch_bounds__(NT) void label_tile_kernel(const unsigned char* __restrict__ mask, int* __restrict__ labels,
                                                        int* __restrict__ sizes, int* __restrict__ stats, int R, int tw) {
    __shared__ u64 rows[TILE];
    __shared__ int parent[TILE * TILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * tw, y0 = blockIdx.y * tw;
    const long image = (long)blockIdx.z * R * R;
    if (tid < TILE) rows[tid] = 0;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid < 4) stats[(long)blockIdx.z * 4 + tid] = 0;
    __syncthreads();
    {
        const int per_row = tw / 16, r = tid / per_row, piece = tid - r * per_row;
        if (r < tw) {
            const uint4 v = *reinterpret_cast<const uint4*>(mask + image + (long)(y0 + r) * R + x0 + 16 * piece);
            reinterpret_cast<unsigned short*>(rows)[4 * r + piece] = (unsigned short)nonzero_bits16(v);
        }
    }
    __syncthreads();
    for (int ly = wave; ly < tw; ly += 4) {
        const u64 m = rows[ly];
        if (lane < tw) parent[ly * tw + lane] = ((m >> lane) & 1ull) ? ly * tw + morph::uf_run_start(m, lane) : -1;
    }
    __syncthreads();
    for (int ly = wave; ly < tw; ly += 4) {
        if (ly > 0 && lane < tw) {
            const u64 cur = rows[ly];
            if ((cur >> lane) & 1ull) morph::uf_merge_up(parent, tw, ly, lane, cur, rows[ly - 1]);
        }
    }
    __syncthreads();
    for (int ly = wave; ly < tw; ly += 4) {
        if (lane < tw) {
            const int p = ly * tw + lane;
            int out = -1;
            if ((rows[ly] >> lane) & 1ull) {
                const int r = morph::uf_find(parent, p);
                out = (y0 + r / tw) * R + x0 + r % tw;
            }
            const long g = image + (long)(y0 + ly) * R + x0 + lane;
            labels[g] = out;
            sizes[g] = 0;
        }
    }
}

// phase 2.  grid (ceil(2 * borders * R / NT), B), borders = R / tw - 1 >= 1
__global__ __launch_bounds__(NT) void label_border_kernel(int* __restrict__ labels, int R, int tw, int borders) {
    const int i = blockIdx.x * NT + threadIdx.x, half = borders * R;
    if (i >= 2 * half) return;
    int* parent = labels + (long)blockIdx.y * R * R;
    if (i < half)                                    // the first row of every tile row but the top one: upwards
        morph::uf_merge_border_up(parent, R, tw, (i / R + 1) * tw, i % R);
    else                                             // the first column of every tile column but the left one: leftwards
        morph::uf_merge_border_left(parent, R, tw, (i - half) % R, ((i - half) / R + 1) * tw);
}

// phase 3.  grid (pixels / NT, B)
__global__ __launch_bounds__(NT) void label_flatten_kernel(int* __restrict__ labels, int* __restrict__ sizes, int pixels) {
    const int i = blockIdx.x * NT + threadIdx.x, lane = threadIdx.x & 63;
    int* parent = labels + (long)blockIdx.y * pixels;
    int* sz = sizes + (long)blockIdx.y * pixels;
    int root = -1;
    if (morph::uf_load(parent + i) >= 0) {
        root = morph::uf_find(parent, i);
        __hip_atomic_store(parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // root <= the entry it replaces
    }
    const int prev = __shfl_up(root, 1, 64);
    const bool head = lane == 0 || prev != root;
    const u64 heads = __ballot(head);
    if (head && root >= 0) {
        const u64 above = lane == 63 ? 0ull : heads >> (lane + 1);
        atomicAdd(sz + root, above ? __ffsll((unsigned long long)above) : 64 - lane);
    }
}

// phase 3, second launch.  grid (ceil(pixels / 4 / NT), B)
__global__ __launch_bounds__(NT) void label_stats_kernel(const int* __restrict__ labels, const int* __restrict__ sizes,
                                                         int* __restrict__ stats, unsigned char* __restrict__ kept, int pixels,
                                                         int min_size) {
    __shared__ int part[4][4];
    const int tid = threadIdx.x, g = blockIdx.x * NT + tid;
    const long base = (long)blockIdx.y * pixels;
    int area = 0, comps = 0, kept_area = 0, largest = 0;
    if (g < pixels / 4) {
        const int4 l4 = reinterpret_cast<const int4*>(labels + base)[g];
        const int l[4] = {l4.x, l4.y, l4.z, l4.w};
        unsigned packed = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            if (l[m] < 0 || l[m] >= pixels) continue;
            ++area;
            const int s = sizes[base + l[m]];
            if (l[m] == 4 * g + m) {
                largest = max(largest, s);
                if (s >= min_size) { ++comps; kept_area += s; }
            }
            if (s >= min_size) packed |= 1u << (8 * m);
        }
        if (kept) reinterpret_cast<unsigned*>(kept + base)[g] = packed;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        area += __shfl_xor(area, o, 64);
        comps += __shfl_xor(comps, o, 64);
        kept_area += __shfl_xor(kept_area, o, 64);
        largest = max(largest, __shfl_xor(largest, o, 64));
    }
    if ((tid & 63) == 0) {
        part[tid >> 6][0] = area; part[tid >> 6][1] = comps; part[tid >> 6][2] = largest; part[tid >> 6][3] = kept_area;
    }
    __syncthreads();
    if (tid < 4) {
        const int a = part[0][tid], b = part[1][tid], c = part[2][tid], d = part[3][tid];
        int* out = stats + (long)blockIdx.y * 4 + tid;
        if (tid == 2) {
            const int v = max(max(a, b), max(c, d));
            if (v) atomicMax(out, v);
        } else {
            const int v = a + b + c + d;
            if (v) atomicAdd(out, v);
        }
    }
}

// ---- box counts -----------------------------------------------------------------------------------------------------------------------
// boxes of side 2^k holding a pixel in one 128-bit row mask that is already the OR of 2^k rows
__device__ __forceinline__ int boxes_in_row(u64 lo, u64 hi, int k) {
    if (k >= 7) return (lo | hi) != 0ull;
    const u64 stride[7] = {~0ull, 0x5555555555555555ull, 0x1111111111111111ull, 0x0101010101010101ull, 0x0001000100010001ull,
                           0x0000000100000001ull, 1ull};
    for (int j = 0; j < k; ++j) {                    // bit p becomes the OR of bits p .. p + 2^k - 1
        lo |= lo >> (1 << j);
        hi |= hi >> (1 << j);
    }
    return __popcll(lo & stride[k]) + __popcll(hi & stride[k]);
}

// grid (R / tw, R / tw, B), tw = min(R, 128), lt = log2 tw, L = log2 R; counts zeroed beforehand
__global__ __launch_bounds__(NT) void box_tile_kernel(const unsigned char* __restrict__ mask, int* __restrict__ counts, int R, int tw,
                                                      int lt, int L) {
    __shared__ u64 buf[2][BOX_TILE][2];
    __shared__ int cnt[8];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * tw, y0 = blockIdx.y * tw;
    const long image = (long)blockIdx.z * R * R;
    if (tid < BOX_TILE) buf[0][tid][0] = buf[0][tid][1] = 0;
    if (tid < 8) cnt[tid] = 0;
    __syncthreads();
    {
        const int per_row = tw / 16;
        unsigned short* pieces = reinterpret_cast<unsigned short*>(&buf[0][0][0]);
        for (int e = tid; e < tw * per_row; e += NT) {
            const int r = e / per_row, piece = e - r * per_row;
            const uint4 v = *reinterpret_cast<const uint4*>(mask + image + (long)(y0 + r) * R + x0 + 16 * piece);
            pieces[8 * r + piece] = (unsigned short)nonzero_bits16(v);
        }
    }
    __syncthreads();
    for (int k = 0; k <= lt; ++k) {
        const int n = tw >> k;                       // rows at this level
        u64 (*src)[2] = buf[k & 1], (*dst)[2] = buf[(k + 1) & 1];
        if (tid < n) {
            const int c = boxes_in_row(src[tid][0], src[tid][1], k);
            if (c) atomicAdd(&cnt[k], c);
        }
        if (tid < n / 2) {
            dst[tid][0] = src[2 * tid][0] | src[2 * tid + 1][0];
            dst[tid][1] = src[2 * tid][1] | src[2 * tid + 1][1];
        }
        __syncthreads();
    }
    int* out = counts + (long)blockIdx.z * (L + 1);
    if (tid <= lt) {
        if (cnt[tid]) atomicAdd(out + tid, cnt[tid]);
    } else if (tid <= L && cnt[lt]) {                // above the tile (lt = 7): this tile's box at level tid, (R >> tid)^2 <= 16 boxes
        const int up = tid - lt;
        atomicOr(out + tid, 1 << ((blockIdx.y >> up) * (R >> tid) + (blockIdx.x >> up)));
    }
}

// grid (B): the levels above the tile hold box bit maps; they become counts
__global__ void box_finish_kernel(int* __restrict__ counts, int lt, int L) {
    const int k = lt + 1 + threadIdx.x;
    if (k <= L) {
        int* at = counts + (long)blockIdx.x * (L + 1) + k;
        *at = __popc((unsigned)*at);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

#define MORPH_SHAPE(name, B, R)                                                                                                        \
    NGAN_REQUIRE(supported(R), NGAN_ERR_SHAPE, name ": R=%d unsupported (a power of two, 16 .. 1024)", R);                             \
    NGAN_REQUIRE((B) > 0 && (B) < 65536, NGAN_ERR_SHAPE, name ": B=%d unsupported (1 .. 65535 images per call)", B)

extern "C" int ngan_morph_levels(const float* images, unsigned char* levels, unsigned int* hist, int B, int R, int C, void* stream) {
    NGAN_REQUIRE(images && levels && hist, NGAN_ERR_ARG, "morph_levels: null pointer");
    MORPH_SHAPE("morph_levels", B, R);
    NGAN_REQUIRE(C == 1 || C == 3, NGAN_ERR_SHAPE, "morph_levels: C=%d unsupported (1 or 3 colour channels)", C);
    NGAN_REQUIRE(aligned16(images) && aligned16(levels) && ((uintptr_t)hist & 3) == 0, NGAN_ERR_ARG,
                 "morph_levels: images and levels must start on a 16-byte boundary, hist on a 4-byte one");
    hipStream_t s = (hipStream_t)stream;
    const int pixels = R * R;
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)B * 256 * sizeof(unsigned), s);
    NGAN_REQUIRE(e == hipSuccess, (int)e, "morph_levels: clearing hist failed: %s", hipGetErrorString(e));
    int blocks = ngan::ceil_div(pixels / 4, NT * 4);
    if (blocks > LEVELS_MAX_BLOCKS) blocks = LEVELS_MAX_BLOCKS;
    if (C == 1) hipLaunchKernelGGL(levels_kernel<1>, dim3(blocks, B), dim3(NT), 0, s, images, levels, hist, pixels);
    else hipLaunchKernelGGL(levels_kernel<3>, dim3(blocks, B), dim3(NT), 0, s, images, levels, hist, pixels);
    return ngan::launch_status("ngan_morph_levels");
}

extern "C" int ngan_morph_mask(const unsigned char* levels, const int* cut, unsigned char* mask, int B, int R, void* stream) {
    NGAN_REQUIRE(levels && cut && mask, NGAN_ERR_ARG, "morph_mask: null pointer");
    MORPH_SHAPE("morph_mask", B, R);
    NGAN_REQUIRE(aligned16(levels) && aligned16(mask) && ((uintptr_t)cut & 3) == 0, NGAN_ERR_ARG,
                 "morph_mask: levels and mask must start on a 16-byte boundary, cut on a 4-byte one");
    const int vecs = R * R / 16;
    hipLaunchKernelGGL(mask_kernel, dim3(ngan::ceil_div(vecs, NT), B), dim3(NT), 0, (hipStream_t)stream, levels, cut, mask, vecs);
    return ngan::launch_status("ngan_morph_mask");
}

extern "C" size_t ngan_morph_workspace_bytes(int B, int R) {
    if (B <= 0 || B > 65535 || !supported(R)) return 0;
    return (size_t)B * R * R * sizeof(int);          // one size per pixel; only roots are read
}

extern "C" int ngan_morph_label(const unsigned char* mask, int* labels, int* stats, unsigned char* kept_or_null, void* workspace, int B,
                                int R, int min_size, void* stream) {
    NGAN_REQUIRE(mask && labels && stats, NGAN_ERR_ARG, "morph_label: null pointer");
    NGAN_REQUIRE(workspace, NGAN_ERR_ARG, "morph_label: null workspace (ngan_morph_workspace_bytes names its size)");
    MORPH_SHAPE("morph_label", B, R);
    NGAN_REQUIRE(min_size >= 1, NGAN_ERR_ARG, "morph_label: min_size=%d must be at least 1", min_size);
    NGAN_REQUIRE(aligned16(mask) && aligned16(labels) && aligned16(workspace) && aligned16(kept_or_null) && ((uintptr_t)stats & 3) == 0,
                 NGAN_ERR_ARG, "morph_label: mask, labels, kept and workspace must start on a 16-byte boundary, stats on a 4-byte one");
    hipStream_t s = (hipStream_t)stream;
    int* sizes = reinterpret_cast<int*>(workspace);
    const int tw = R < TILE ? R : TILE, tiles = R / tw, pixels = R * R;
    hipLaunchKernelGGL(label_tile_kernel, dim3(tiles, tiles, B), dim3(NT), 0, s, mask, labels, sizes, stats, R, tw);
    if (tiles > 1)
        hipLaunchKernelGGL(label_border_kernel, dim3(ngan::ceil_div(2L * (tiles - 1) * R, NT), B), dim3(NT), 0, s, labels, R, tw, tiles - 1);
    hipLaunchKernelGGL(label_flatten_kernel, dim3(pixels / NT, B), dim3(NT), 0, s, labels, sizes, pixels);
    hipLaunchKernelGGL(label_stats_kernel, dim3(ngan::ceil_div(pixels / 4, NT), B), dim3(NT), 0, s, labels, sizes, stats, kept_or_null,
                       pixels, min_size);
    return ngan::launch_status("ngan_morph_label");
}

extern "C" int ngan_morph_boxcount(const unsigned char* mask, int* counts, int B, int R, void* stream) {
    NGAN_REQUIRE(mask && counts, NGAN_ERR_ARG, "morph_boxcount: null pointer");
    MORPH_SHAPE("morph_boxcount", B, R);
    NGAN_REQUIRE(aligned16(mask) && ((uintptr_t)counts & 3) == 0, NGAN_ERR_ARG,
                 "morph_boxcount: mask must start on a 16-byte boundary, counts on a 4-byte one");
    hipStream_t s = (hipStream_t)stream;
    const int L = log2_of(R), tw = R < BOX_TILE ? R : BOX_TILE, lt = log2_of(tw), tiles = R / tw;
    hipError_t e = hipMemsetAsync(counts, 0, (size_t)B * (L + 1) * sizeof(int), s);
    NGAN_REQUIRE(e == hipSuccess, (int)e, "morph_boxcount: clearing counts failed: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(box_tile_kernel, dim3(tiles, tiles, B), dim3(NT), 0, s, mask, counts, R, tw, lt, L);
    if (L > lt) hipLaunchKernelGGL(box_finish_kernel, dim3(B), dim3(64), 0, s, counts, lt, L);
    return ngan::launch_status("ngan_morph_boxcount");
}
