// Arbor geometry of masks: the kernels behind metrics.distance_transform and metrics.sholl_crossings.  Integers and integer atomics
// only, but for `roots`, which is summed in fp64 in a fixed order: every output is bit-reproducible, an image's values never depend on
// the rest of the batch, and no workgroup waits on another.
//   ngan_geom_edt     three launches
//       columns   one thread per column of the batch (consecutive threads read consecutive bytes): a scan down writes the distance to
//                 the nearest background pixel above, the row -1 included, as uint16 into the workspace; a scan up takes the minimum
//                 with the distance to the nearest one below, the row R included.  The thread of column 0 clears its image's soma key.
//       rows      a workgroup holds max(256 / R, 1) rows of squared column distances in LDS (4 KiB at most); the thread of pixel x walks
//                 d = 1, 2, ... outwards while d^2 is below its best (geom::row_min, which also runs serially on the host) and writes
//                 dist2.  The soma is the maximum of the 64-bit key (dist2 << 32) | ~index over the foreground: a wave maximum by
//                 shuffles, then one atomicMax per wave that holds foreground.  A workgroup never spans two images.
//       soma      one thread per image unpacks the key: {y, x, dist2}, or {-1, -1, 0} when no pixel was foreground.
//   ngan_geom_sholl   one workgroup per image, min(1024, R^2 / 16) threads, one launch.  The image goes by in slabs of 16 pixels per
//                 thread: a thread turns its 16 bytes into a bit mask, a scan of the popcounts over the workgroup gives every thread the
//                 place of its set pixels in an LDS list (pixel order, so the list does not depend on timing), and the list is then
//                 shared out evenly: skeletons are sparse, and a thread that walked its own 16 pixels would leave most lanes idle at
//                 every one.  At a set pixel a thread adds sqrt(dist2) to its fp64 partial sum and names the edges that start there
//                 (geom::edges_from); an edge whose ends lie in different rings (geom::ring_index) increments the larger ring's bin,
//                 an LDS integer atomic.  The partial sums are added by a fixed shuffle tree and then wave by wave.
// Only plain C++: no inline assembly.
#include <cstdint>
#include "ngan_common.h"
#include "geom_bits.h"

namespace {

typedef unsigned short u16;
typedef unsigned long long u64;

constexpr int R_MIN = 16, R_MAX = 1024;
constexpr int ROW_NT = 256;             // threads of a row-pass workgroup when R <= 256 (R above)
constexpr int SHOLL_NT = 1024;          // threads of a Sholl workgroup at most

bool supported(int R) { return R >= R_MIN && R <= R_MAX && (R & (R - 1)) == 0; }
bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
int log2_of(int R) {
    int l = 0;
    while ((1 << l) < R) ++l;
    return l;
}
size_t key_bytes(int B) { return ((size_t)B * sizeof(u64) + 15) & ~(size_t)15; }

// grid ceil(B R / 64) x 64 threads: column c of the batch is column c % R of image c / R
__global__ __launch_bounds__(64) void geom_columns(const unsigned char* __restrict__ mask, u16* __restrict__ g, u64* __restrict__ keys,
                                                   int columns, int R, int lr) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= columns) return;
    const int b = c >> lr, x = c & (R - 1);
    if (x == 0) keys[b] = 0ull;
    const long base = ((long)b << (2 * lr)) + x;
    const unsigned char* m = mask + base;
    u16* o = g + base;
    int d = 0;
#pragma unroll 8
    for (int y = 0; y < R; ++y) {
        d = m[(long)y << lr] ? d + 1 : 0;
        o[(long)y << lr] = (u16)d;
    }
    int u = 0;
#pragma unroll 8
    for (int y = R - 1; y >= 0; --y) {
        const int v = o[(long)y << lr];
        u = v ? u + 1 : 0;
        o[(long)y << lr] = (u16)(v < u ? v : u);
    }
}

// grid B R / rows_per_block, max(R, 256) threads, dynamic LDS 4 * threads bytes
__global__ __launch_bounds__(R_MAX) void geom_rows(const u16* __restrict__ g, int* __restrict__ dist2, u64* __restrict__ keys, int R, int lr) {
    extern __shared__ int g2[];
    const int tid = threadIdx.x, x = tid & (R - 1);
    const long row = (long)blockIdx.x * (blockDim.x >> lr) + (tid >> lr);     // row of the batch: image row >> lr, line row & (R - 1)
    const long at = (row << lr) + x;
    const int v = g[at];
    g2[tid] = v * v;
    __syncthreads();
    const int best = geom::row_min(g2 + (tid - x), R, x);
    dist2[at] = best;
    const unsigned index = (unsigned)(at & (((long)1 << (2 * lr)) - 1));
    u64 key = best ? ((u64)(unsigned)best << 32) | (u64)(0xffffffffu - index) : 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned hi = __shfl_xor((unsigned)(key >> 32), o, 64), lo = __shfl_xor((unsigned)key, o, 64);
        const u64 other = ((u64)hi << 32) | lo;
        key = other > key ? other : key;
    }
    if ((tid & 63) == 0 && key) atomicMax(&keys[row >> lr], key);
}

// grid ceil(B / 64) x 64 threads
__global__ __launch_bounds__(64) void geom_soma(const u64* __restrict__ keys, int* __restrict__ soma, int B, int R, int lr) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const u64 key = keys[b];
    int* out = soma + 3L * b;
    if (!key) {
        out[0] = -1;
        out[1] = -1;
        out[2] = 0;
    } else {
        const unsigned index = 0xffffffffu - (unsigned)key;
        out[0] = (int)(index >> lr);
        out[1] = (int)(index & (unsigned)(R - 1));
        out[2] = (int)(key >> 32);
    }
}

// grid (B), threads min(1024, R^2 / 16) (a multiple of 64)
__global__ __launch_bounds__(SHOLL_NT) void geom_sholl(const unsigned char* __restrict__ skeleton, const int* __restrict__ dist2,
                                                       const int* __restrict__ centre, int* __restrict__ crossings,
                                                       double* __restrict__ roots, int R, int lr) {
    __shared__ int bins[geom::SHOLL_BINS];
    __shared__ double part[SHOLL_NT / 64];
    __shared__ int wave_total[SHOLL_NT / 64];
    __shared__ u16 list[SHOLL_NT * 16];                 // the set pixels of a slab of 16 * threads pixels, in pixel order
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const long image = (long)blockIdx.x << (2 * lr);
    const int cy = centre[3L * blockIdx.x], cx = centre[3L * blockIdx.x + 1];
    const bool valid = cy >= 0 && cy < R && cx >= 0 && cx < R;         // (uniform over the workgroup)
    for (int t = tid; t < geom::SHOLL_BINS; t += nt) bins[t] = 0;
    __syncthreads();
    double sum = 0.0;
    if (valid) {
        const unsigned char* sk = skeleton + image;
        const int step = geom::sholl_step(R), chunks = (R * R) >> 4;
        for (int first = 0; first < chunks; first += nt) {             // slab by slab; chunks is 16 or a multiple of nt
            const int i = first + tid;
            unsigned set = 0;                                          // bit t: pixel 16 i + t is set
            if (i < chunks) {
                const uint4 v = *reinterpret_cast<const uint4*>(sk + 16L * i);
                const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int t = 0; t < 16; ++t) set |= ((w[t >> 2] >> (8 * (t & 3))) & 255u) ? 1u << t : 0u;
            }
            const int mine = __popc(set);
            int before = mine;                                         // inclusive scan over the wave, then over the waves
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(before, o, 64);
                if (lane >= o) before += up;
            }
            if (lane == 63) wave_total[wave] = before;
            __syncthreads();
            int offset = before - mine, total = 0;
            for (int w = 0; w < nt / 64; ++w) {
                const int n = wave_total[w];
                offset += w < wave ? n : 0;
                total += n;
            }
            while (set) {
                const int t = __ffs(set) - 1;
                set &= set - 1;
                list[offset++] = (u16)(16 * tid + t);
            }
            __syncthreads();
            for (int e = tid; e < total; e += nt) {
                const long p = 16L * first + list[e];
                const int y = (int)(p >> lr), x = (int)(p & (R - 1));
                sum += sqrt((double)dist2[image + p]);
                const bool down = y + 1 < R, left = x > 0, right = x + 1 < R;
                const int e_ = right ? sk[p + 1] : 0, w_ = left ? sk[p - 1] : 0, s_ = down ? sk[p + R] : 0;
                const int se = down && right ? sk[p + R + 1] : 0, sw = down && left ? sk[p + R - 1] : 0;
                const int edges = geom::edges_from(e_, w_, s_, se, sw);
                if (!edges) continue;
                const int dy = y - cy, dx = x - cx;
                const int k = geom::ring_index(dy * dy + dx * dx, step);
                const int qy[4] = {dy, dy + 1, dy + 1, dy + 1}, qx[4] = {dx + 1, dx, dx + 1, dx - 1};
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    if (!(edges & (1 << n))) continue;
                    const int bin = geom::crossing_bin(k, geom::ring_index(qy[n] * qy[n] + qx[n] * qx[n], step));
                    if (bin >= 0 && bin < geom::SHOLL_BINS) atomicAdd(&bins[bin], 1);
                }
            }
            __syncthreads();                                           // the list is read before the next slab overwrites it
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    for (int t = tid; t < geom::SHOLL_BINS; t += nt) crossings[(long)blockIdx.x * geom::SHOLL_BINS + t] = bins[t];
    if (tid == 0) {
        double total = 0.0;
        for (int w = 0; w < nt / 64; ++w) total += part[w];
        roots[blockIdx.x] = total;
    }
}

}  // namespace

#define GEOM_SHAPE(name, B, R)                                                                                        \
    NGAN_REQUIRE(supported(R), NGAN_ERR_SHAPE, name ": R=%d unsupported (a power of two, 16 .. 1024)", R);            \
    NGAN_REQUIRE((B) > 0 && (B) < 65536, NGAN_ERR_SHAPE, name ": B=%d unsupported (1 .. 65535 images per call)", B)

extern "C" size_t ngan_geom_workspace_bytes(int B, int R) {
    if (!supported(R) || B <= 0 || B >= 65536) return 0;
    return key_bytes(B) + (size_t)B * R * R * sizeof(u16);
}

extern "C" int ngan_geom_edt(const unsigned char* mask, int* dist2, int* soma, void* workspace, int B, int R, void* stream) {
    NGAN_REQUIRE(mask && dist2 && soma && workspace, NGAN_ERR_ARG, "geom_edt: null pointer");
    GEOM_SHAPE("geom_edt", B, R);
    NGAN_REQUIRE(aligned(mask, 16) && aligned(dist2, 16) && aligned(workspace, 16) && aligned(soma, 4), NGAN_ERR_ARG,
                 "geom_edt: mask, dist2 and workspace must start on a 16-byte boundary, soma on a 4-byte one");
    const int lr = log2_of(R);
    u64* keys = static_cast<u64*>(workspace);
    u16* g = reinterpret_cast<u16*>(static_cast<char*>(workspace) + key_bytes(B));
    const int columns = B * R;
    hipLaunchKernelGGL(geom_columns, dim3((columns + 63) / 64), dim3(64), 0, (hipStream_t)stream, mask, g, keys, columns, R, lr);
    int status = ngan::launch_status("ngan_geom_edt (columns)");
    if (status != NGAN_OK) return status;
    const int nt = R > ROW_NT ? R : ROW_NT;
    hipLaunchKernelGGL(geom_rows, dim3((unsigned)(((long)B * R) / (nt >> lr))), dim3(nt), (size_t)nt * sizeof(int), (hipStream_t)stream, g,
                       dist2, keys, R, lr);
    status = ngan::launch_status("ngan_geom_edt (rows)");
    if (status != NGAN_OK) return status;
    hipLaunchKernelGGL(geom_soma, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, keys, soma, B, R, lr);
    return ngan::launch_status("ngan_geom_edt (soma)");
}

extern "C" int ngan_geom_sholl(const unsigned char* skeleton, const int* dist2, const int* centre, int* crossings, double* roots, int B,
                               int R, void* stream) {
    NGAN_REQUIRE(skeleton && dist2 && centre && crossings && roots, NGAN_ERR_ARG, "geom_sholl: null pointer");
    GEOM_SHAPE("geom_sholl", B, R);
    NGAN_REQUIRE(aligned(skeleton, 16) && aligned(dist2, 16) && aligned(centre, 4) && aligned(crossings, 4) && aligned(roots, 8),
                 NGAN_ERR_ARG,
                 "geom_sholl: skeleton and dist2 must start on a 16-byte boundary, centre and crossings on a 4-byte one, roots on an "
                 "8-byte one");
    const int lr = log2_of(R);
    const int chunks = (R * R) >> 4;
    const int nt = chunks < 64 ? 64 : chunks > SHOLL_NT ? SHOLL_NT : chunks;
    hipLaunchKernelGGL(geom_sholl, dim3(B), dim3(nt), 0, (hipStream_t)stream, skeleton, dist2, centre, crossings, roots, R, lr);
    return ngan::launch_status("ngan_geom_sholl");
}
