// Arbor skeleton of masks: the kernel behind metrics.thin and metrics.skeleton_counts.  Every result is an integer and there is no
// atomic: every output is bit-reproducible and an image's values never depend on the rest of the batch.
//   ngan_skel_thin / ngan_skel_counts   skel_kernel, one workgroup per image, min(1024, max(64, words)) threads:
//       pack     the mask becomes bit rows in LDS (32-bit words, R / 32 per row, one half-used word per row for R = 16; at most 32 KiB)
//                from 16-byte loads; the input area is the popcount of the words
//       thin     Guo-Hall A1 (skel_bits.h, which also runs serially on the host).  A thread owns the words tid, tid + threads, ... (at
//                most 8; neighbouring lanes read neighbouring LDS words), forms the eight neighbour planes of each from the 3 x 3 words
//                around it and keeps the bits to delete in registers; the workgroup-wide OR of "deleted something" is the barrier
//                after which the bits are cleared in place, and a second barrier ends the sub-iteration: one LDS buffer.  A word
//                without a set pixel is skipped: nothing can be deleted from it, so the results are the same.  The loop ends after
//                the first pair of sub-iterations that deleted nothing.
//       count    pixels, tips, junctions, isolated, orth, diag of the final bit rows (skel::count_word), summed by wave shuffles and
//                one pass over the waves' partial sums in LDS; the skeleton, when asked for, is written as bytes 0 / 1 with 16-byte
//                stores
// Only plain C++: no inline assembly.
#include <cstdint>
#include "ngan_common.h"
#include "skel_bits.h"

namespace {

using skel::u32;

constexpr int NT_MAX = 1024;            // threads per workgroup at most
constexpr int KMAX = 8;                 // words per thread at most: 512 * 16 words over 1024 threads
constexpr int R_MAX = 512;              // 512 rows of 16 words: 32 KiB of LDS

bool supported(int R) { return R >= 16 && R <= R_MAX && (R & (R - 1)) == 0; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__device__ __forceinline__ u32 bits_of(uint4 v) {
    const u32 w[4] = {v.x, v.y, v.z, v.w};
    return skel::nonzero_bits16(w);
}

__device__ __forceinline__ uint4 bytes_of(u32 bits16) {
    return make_uint4(skel::bytes_of_nibble(bits16 & 15u), skel::bytes_of_nibble((bits16 >> 4) & 15u),
                      skel::bytes_of_nibble((bits16 >> 8) & 15u), skel::bytes_of_nibble((bits16 >> 12) & 15u));
}

// grid (B), threads a multiple of 64, dynamic LDS 4 * words bytes; words = R * wpr, wpr = max(R / 32, 1) = 1 << lw
__global__ __launch_bounds__(NT_MAX) void skel_kernel(const unsigned char* __restrict__ mask, unsigned char* __restrict__ skeleton,
                                                      int* __restrict__ stats, int R, int lw, int do_thin) {
    extern __shared__ u32 bits[];
    __shared__ int part[NT_MAX / 64][8];
    const int tid = threadIdx.x, nt = blockDim.x, wpr = 1 << lw, words = R << lw;
    const int k = (words + nt - 1) / nt;             // words per thread, <= KMAX
    const long image = (long)blockIdx.x * R * R;
    int area = 0;
#pragma unroll
    for (int j = 0; j < KMAX; ++j) {
        const int i = tid + j * nt;
        if (j < k && i < words) {
            u32 w;
            if (R >= 32) {
                const uint4* src = reinterpret_cast<const uint4*>(mask + image + 32L * i);
                w = bits_of(src[0]) | (bits_of(src[1]) << 16);
            } else {
                w = bits_of(*reinterpret_cast<const uint4*>(mask + image + 16L * i));
            }
            bits[i] = w;
            area += skel::popc(w);
        }
    }
    __syncthreads();
    int passes = 0;
    if (do_thin) {
        for (;;) {
            int pair = 0;
            for (int sub = 0; sub < 2; ++sub) {
                u32 del[KMAX], mine = 0;
#pragma unroll
                for (int j = 0; j < KMAX; ++j) {
                    const int i = tid + j * nt;
                    del[j] = 0;
                    if (j < k && i < words && bits[i] != 0u) {
                        del[j] = skel::deletable(skel::planes_at(bits, R, wpr, i >> lw, i & (wpr - 1)), sub);
                        mine |= del[j];
                    }
                }
                const int any = __syncthreads_or(mine != 0u);    // every read of this sub-iteration is done
                if (any) {                                       // (uniform over the workgroup)
#pragma unroll
                    for (int j = 0; j < KMAX; ++j)
                        if (del[j]) bits[tid + j * nt] &= ~del[j];
                    __syncthreads();
                }
                pair |= any;
            }
            passes += 2;
            if (!pair) break;
        }
    }
    int v[8] = {0, 0, 0, 0, 0, 0, 0, area};
#pragma unroll 1
    for (int j = 0; j < k; ++j) {
        const int i = tid + j * nt;
        if (i < words) {
            const u32 w = bits[i];
            skel::count_word(skel::planes_at(bits, R, wpr, i >> lw, i & (wpr - 1)), v);
            if (skeleton) {
                if (R >= 32) {
                    uint4* dst = reinterpret_cast<uint4*>(skeleton + image + 32L * i);
                    dst[0] = bytes_of(w & 0xffffu);
                    dst[1] = bytes_of(w >> 16);
                } else {
                    *reinterpret_cast<uint4*>(skeleton + image + 16L * i) = bytes_of(w & 0xffffu);
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[m] += __shfl_xor(v[m], o, 64);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int m = 0; m < 8; ++m) part[tid >> 6][m] = v[m];
    }
    __syncthreads();
    if (tid < 8) {
        int sum = 0;
        for (int w = 0; w < nt / 64; ++w) sum += part[w][tid];
        stats[(long)blockIdx.x * 8 + tid] = tid == 6 ? passes : sum;
    }
}

int launch(const char* name, const unsigned char* mask, unsigned char* skeleton, int* stats, int B, int R, int do_thin, void* stream) {
    int lw = 0;
    while ((32 << lw) < R) ++lw;
    const int words = R << lw;
    const int nt = words < 64 ? 64 : words > NT_MAX ? NT_MAX : words;
    hipLaunchKernelGGL(skel_kernel, dim3(B), dim3(nt), (size_t)words * sizeof(u32), (hipStream_t)stream, mask, skeleton, stats, R, lw, do_thin);
    return ngan::launch_status(name);
}

}  // namespace

#define SKEL_SHAPE(name, B, R)                                                                                                         \
    NGAN_REQUIRE(supported(R), NGAN_ERR_SHAPE,                                                                                         \
                 name ": R=%d unsupported (a power of two, 16 .. 512: the bit rows of an image stay in one workgroup's LDS)", R);       \
    NGAN_REQUIRE((B) > 0 && (B) < 65536, NGAN_ERR_SHAPE, name ": B=%d unsupported (1 .. 65535 images per call)", B)

extern "C" int ngan_skel_thin(const unsigned char* mask, unsigned char* skeleton_or_null, int* stats, int B, int R, void* stream) {
    NGAN_REQUIRE(mask && stats, NGAN_ERR_ARG, "skel_thin: null pointer");
    SKEL_SHAPE("skel_thin", B, R);
    NGAN_REQUIRE(aligned16(mask) && aligned16(skeleton_or_null) && ((uintptr_t)stats & 3) == 0, NGAN_ERR_ARG,
                 "skel_thin: mask and skeleton must start on a 16-byte boundary, stats on a 4-byte one");
    return launch("ngan_skel_thin", mask, skeleton_or_null, stats, B, R, 1, stream);
}

extern "C" int ngan_skel_counts(const unsigned char* mask, int* stats, int B, int R, void* stream) {
    NGAN_REQUIRE(mask && stats, NGAN_ERR_ARG, "skel_counts: null pointer");
    SKEL_SHAPE("skel_counts", B, R);
    NGAN_REQUIRE(aligned16(mask) && ((uintptr_t)stats & 3) == 0, NGAN_ERR_ARG,
                 "skel_counts: mask must start on a 16-byte boundary, stats on a 4-byte one");
    return launch("ngan_skel_counts", mask, nullptr, stats, B, R, 0, stream);
}
