// Loading a folder of 8-bit greyscale micrographs (reference data/NeuronDataset.py:84-107) on the device: per image a 256-bin
// histogram, the 4-class multi-Otsu thresholds (what skimage.filters.threshold_multiotsu(img, classes=4) searches for), the mean and
// standard deviation of the camera's noise floor (pixels strictly between 0 and the lowest threshold), and the pad by R // 4 with
// every zero pixel replaced by Gaussian noise of those statistics -- a handful of launches for the whole folder instead of a Python
// loop over images.  Decoding the files stays on the host (data.py).  Integer atomics only: every result is order-independent.
//   ngan_u8_histogram            u8_histogram_kernel: 16-byte loads, run-length merged LDS atomics into 16 sub-histograms
//   ngan_multiotsu4_noise_stats  multiotsu4_search_kernel (OTSU_SPLIT workgroups per image, each its best (score, triplet)) and
//                                multiotsu4_finish_kernel (the winner in lexicographic order, then the noise record)
//   ngan_u8_pad_noise_fill       u8_pad_noise_fill_kernel
#include "ngan_common.h"

namespace {

constexpr int HIST_SUB = 16;            // sub-histograms per workgroup (lane & 15 picks one): an all-one-level image spreads its
                                        // LDS atomics over 16 addresses on 16 banks instead of serialising on one
constexpr int HIST_MAX_BLOCKS = 32;     // workgroups per image at most
constexpr int HIST_VEC_PER_THREAD = 8;  // 16-byte loads per thread a workgroup is sized for
constexpr int OTSU_SPLIT = 32;          // workgroups (and workspace slots) per image of the threshold search
constexpr long MAX_PIXELS = 1L << 23;   // n * S2 and S1^2 of the variance stay below 2^63

// counts[sub][bin] with a row pitch of 257 words: the 16 copies of one bin sit on 16 different banks
constexpr int HIST_PITCH = 257;

__device__ __forceinline__ void hist_add(unsigned* sub, unsigned level, unsigned n) { atomicAdd(sub + level, n); }

// the 16 bytes of one load, equal neighbours merged: the zero background costs one LDS atomic per load, not sixteen
__device__ __forceinline__ void hist_add16(unsigned* sub, uint4 v) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    unsigned cur = w[0] & 255u, run = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned level = (w[i] >> (8 * k)) & 255u;
            if (level != cur) {
                hist_add(sub, cur, run);
                cur = level;
                run = 0;
            }
            ++run;
        }
    }
    hist_add(sub, cur, run);
}

__global__ __launch_bounds__(256) void u8_histogram_kernel(const unsigned char* __restrict__ images, unsigned* __restrict__ hist,
                                                           long pixels) {
    __shared__ unsigned counts[HIST_SUB * HIST_PITCH];
    const int tid = threadIdx.x;
    for (int i = tid; i < HIST_SUB * HIST_PITCH; i += 256) counts[i] = 0;
    __syncthreads();
    const unsigned char* im = images + (long)blockIdx.y * pixels;
    unsigned* sub = counts + (tid & (HIST_SUB - 1)) * HIST_PITCH;
    // [0, head) scalar up to the first 16-byte boundary, nvec 16-byte loads, then a scalar tail: pixels is any number
    long head = (long)((16 - (reinterpret_cast<size_t>(im) & 15)) & 15);
    if (head > pixels) head = pixels;
    const long nvec = (pixels - head) >> 4;
    const uint4* body = reinterpret_cast<const uint4*>(im + head);
    for (long i = (long)blockIdx.x * 256 + tid; i < nvec; i += (long)gridDim.x * 256) hist_add16(sub, body[i]);
    if (blockIdx.x == 0) {
        const long tail0 = head + (nvec << 4);
        if (tid < head) hist_add(sub, im[tid], 1);
        if (tail0 + tid < pixels && tid < 16) hist_add(sub, im[tail0 + tid], 1);
    }
    __syncthreads();
    unsigned total = 0;
#pragma unroll
    for (int s = 0; s < HIST_SUB; ++s) total += counts[s * HIST_PITCH + tid];
    if (total) atomicAdd(hist + (long)blockIdx.y * 256 + tid, total);
}

// ---- multi-Otsu, four classes -------------------------------------------------------------------------------------------------
// Candidates are the level triplets lo <= t0 < t1 < t2 <= hi - 1 (lo, hi: lowest / highest occupied level); the score of one is the
// sum over its classes lo..t0, t0+1..t1, t1+1..t2, t2+1..hi of S^2 / P (S = sum v h[v], P = sum h[v], exact 64-bit integers from
// prefix sums; P = 0 contributes 0), each term a fixed fp64 formula of the integers, added as ((c0 + c1) + c2) + c3: triplets that cut
// the occupied levels into the same four sets score bit-identically, and the answer is the lexicographically smallest triplet of the
// largest score (skimage's loop order with its strict `>`).
struct OtsuBest { double score; unsigned triplet, pad; };      // triplet = t0 << 16 | t1 << 8 | t2; one workspace slot

__device__ __forceinline__ bool otsu_better(double s, unsigned t, double s0, unsigned t0) { return s > s0 || (s == s0 && t < t0); }

// inclusive-prefix tables over the 256 levels, shifted by one: pp[v] = sum h[0..v-1], sp[v] = sum u h[u] over the same range
__device__ __forceinline__ void otsu_prefix(const unsigned* __restrict__ h, long long* pp, long long* sp, int tid) {
    long long p = h[tid], s = (long long)tid * p;
    pp[tid + 1] = p;
    sp[tid + 1] = s;
    if (tid == 0) pp[0] = sp[0] = 0;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                        // Hillis-Steele: integer sums, any order gives the same result
        long long ap = 0, as = 0;
        if (tid >= o) { ap = pp[tid + 1 - o]; as = sp[tid + 1 - o]; }
        __syncthreads();
        if (tid >= o) { pp[tid + 1] += ap; sp[tid + 1] += as; }
        __syncthreads();
    }
}

__device__ __forceinline__ double otsu_class(const long long* pp, const long long* sp, int a, int b) {   // levels a..b inclusive
    const long long p = pp[b + 1] - pp[a];
    if (p == 0) return 0.0;
    const double s = (double)(sp[b + 1] - sp[a]);
    return s * s / (double)p;
}

// lowest / highest occupied level and whether at least four levels are occupied (every thread gets the same answer)
__device__ __forceinline__ bool otsu_range(const long long* pp, int tid, int* red, int& lo, int& hi) {
    const bool occ = pp[tid + 1] != pp[tid];
    if (tid == 0) { red[0] = 256; red[1] = -1; red[2] = 0; }
    __syncthreads();
    if (occ) { atomicMin(&red[0], tid); atomicMax(&red[1], tid); atomicAdd(&red[2], 1); }
    __syncthreads();
    lo = red[0];
    hi = red[1];
    return red[2] >= 4;
}

__global__ __launch_bounds__(256) void multiotsu4_search_kernel(const unsigned* __restrict__ hist, OtsuBest* __restrict__ slots) {
    __shared__ long long pp[257], sp[257];
    __shared__ double head[256], tail[256];     // class lo..t0 by t0; class t2+1..hi by t2
    __shared__ double best_s[4];
    __shared__ unsigned best_t[4];
    __shared__ int red[3];
    const int tid = threadIdx.x, n = blockIdx.y;
    otsu_prefix(hist + (long)n * 256, pp, sp, tid);
    int lo, hi;
    const bool ok = otsu_range(pp, tid, red, lo, hi);
    double bs = -1.0;                           // every real score is >= 0
    unsigned bt = 0xffffffffu;
    if (ok) {
        head[tid] = (tid >= lo && tid < hi) ? otsu_class(pp, sp, lo, tid) : 0.0;
        tail[tid] = (tid >= lo && tid < hi) ? otsu_class(pp, sp, tid + 1, hi) : 0.0;
        __syncthreads();
        // this workgroup's share: t0 = lo + blockIdx.x, + OTSU_SPLIT, ...; a thread takes t1 = t0 + 1 + tid and walks t2 upwards, so
        // its own candidates come in lexicographic order and a strict `>` keeps the smallest triplet of its best score
        for (int t0 = lo + blockIdx.x; t0 <= hi - 3; t0 += OTSU_SPLIT) {
            const int t1 = t0 + 1 + tid;
            if (t1 > hi - 2) continue;
            const double c01 = head[t0] + otsu_class(pp, sp, t0 + 1, t1);
            const long long p1 = pp[t1 + 1], s1 = sp[t1 + 1];
            for (int t2 = t1 + 1; t2 <= hi - 1; ++t2) {
                const long long p = pp[t2 + 1] - p1;
                double c2 = 0.0;
                if (p != 0) {
                    const double s = (double)(sp[t2 + 1] - s1);
                    c2 = s * s / (double)p;
                }
                const double score = (c01 + c2) + tail[t2];
                if (score > bs) { bs = score; bt = (unsigned)t0 << 16 | (unsigned)t1 << 8 | (unsigned)t2; }
            }
        }
    }
    // best of the wave, then of the workgroup
    for (int o = 32; o > 0; o >>= 1) {
        const double os = __shfl_xor(bs, o, 64);
        const unsigned ot = __shfl_xor(bt, o, 64);
        if (otsu_better(os, ot, bs, bt)) { bs = os; bt = ot; }
    }
    if ((tid & 63) == 0) { best_s[tid >> 6] = bs; best_t[tid >> 6] = bt; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (otsu_better(best_s[w], best_t[w], bs, bt)) { bs = best_s[w]; bt = best_t[w]; }
        slots[(long)n * OTSU_SPLIT + blockIdx.x] = OtsuBest{bs, bt, 0u};
    }
}

// one workgroup per image: the winner over the OTSU_SPLIT slots, then count / mean / population standard deviation of the levels
// 0 < v < t0 straight from the histogram: mean = S1 / n, var = (n S2 - S1^2) / n^2 with an exact integer numerator
__global__ __launch_bounds__(256) void multiotsu4_finish_kernel(const unsigned* __restrict__ hist, const OtsuBest* __restrict__ slots,
                                                                int* __restrict__ thresholds, double* __restrict__ record,
                                                                int* __restrict__ status) {
    __shared__ long long pp[257], sp[257];
    __shared__ int red[3];
    const int tid = threadIdx.x, n = blockIdx.x;
    const unsigned* h = hist + (long)n * 256;
    otsu_prefix(h, pp, sp, tid);
    int lo, hi;
    const bool ok = otsu_range(pp, tid, red, lo, hi);
    if (tid != 0) return;
    int st = 1, t[3] = {0, 0, 0};
    double rec[3] = {0.0, 0.0, 0.0};
    if (ok) {
        double bs = -1.0;
        unsigned bt = 0xffffffffu;
        for (int i = 0; i < OTSU_SPLIT; ++i) {
            const OtsuBest b = slots[(long)n * OTSU_SPLIT + i];
            if (otsu_better(b.score, b.triplet, bs, bt)) { bs = b.score; bt = b.triplet; }
        }
        const int t0 = (int)(bt >> 16) & 255;
        const long long cnt = t0 >= 1 ? pp[t0] - pp[1] : 0;     // levels 1 .. t0 - 1
        st = 2;
        if (cnt > 0) {
            const long long s1 = sp[t0] - sp[1];
            long long s2 = 0;
            for (int v = 1; v < t0; ++v) s2 += (long long)v * v * (long long)h[v];
            const double dn = (double)cnt;
            st = 0;
            t[0] = t0;
            t[1] = (int)(bt >> 8) & 255;
            t[2] = (int)bt & 255;
            rec[0] = dn;
            rec[1] = (double)s1 / dn;
            rec[2] = sqrt((double)(cnt * s2 - s1 * s1) / (dn * dn));
        }
    }
    for (int i = 0; i < 3; ++i) {
        thresholds[n * 3 + i] = t[i];
        record[n * 3 + i] = rec[i];
    }
    status[n] = st;
}

// ---- pad by R // 4 and replace every zero pixel by noise (NeuronDataset.py:13-19, 70-71, 100-107) ---------------------------------
__device__ __forceinline__ float fill_pixel(const unsigned char* __restrict__ images, float draw, const double* __restrict__ record,
                                            long e, int R, int pad, int P) {
    const long pp2 = (long)P * P;
    const long n = e / pp2;
    const int r = (int)(e - n * pp2);
    const int y = r / P - pad, x = r % P - pad;
    int level = 0;
    if (y >= 0 && y < R && x >= 0 && x < R) level = images[(n * R + y) * R + x];
    if (level == 0) {
        // mean + std * draw as a product and a sum, each rounded (numpy's `noise_std * randn + noise_mean`), clamped where the
        // reference's uint8 assignment wraps, truncated toward zero as that assignment does
        const double v = __dadd_rn(__dmul_rn(record[n * 3 + 2], (double)draw), record[n * 3 + 1]);
        level = (int)fmin(fmax(v, 0.0), 255.0);
    }
    return (float)level / 255.0f;               // ToTensor: a true division
}

__global__ __launch_bounds__(256) void u8_pad_noise_fill_kernel(const unsigned char* __restrict__ images,
                                                                const float* __restrict__ normals, const double* __restrict__ record,
                                                                float* __restrict__ canvases, long total, int R, int pad, int P) {
    const long e = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (e + 4 <= total) {
        const float4 d = ld4(normals + e);
        float4 o;
        o.x = fill_pixel(images, d.x, record, e, R, pad, P);
        o.y = fill_pixel(images, d.y, record, e + 1, R, pad, P);
        o.z = fill_pixel(images, d.z, record, e + 2, R, pad, P);
        o.w = fill_pixel(images, d.w, record, e + 3, R, pad, P);
        st4(canvases + e, o);
    } else {
        for (long i = e; i < total; ++i) canvases[i] = fill_pixel(images, normals[i], record, i, R, pad, P);
    }
}

}  // namespace

extern "C" size_t ngan_multiotsu_workspace_bytes(int n_images) {
    if (n_images <= 0) return 0;
    return (size_t)n_images * OTSU_SPLIT * sizeof(OtsuBest);
}

extern "C" int ngan_u8_histogram(const unsigned char* images, unsigned int* hist, int n_images, long pixels, void* stream) {
    NGAN_REQUIRE(images && hist, NGAN_ERR_ARG, "u8_histogram: null pointer");
    NGAN_REQUIRE(n_images > 0 && pixels > 0, NGAN_ERR_ARG, "u8_histogram: n_images=%d pixels=%ld must be positive", n_images, pixels);
    NGAN_REQUIRE(n_images < 65536 && pixels <= MAX_PIXELS, NGAN_ERR_SHAPE,
                 "u8_histogram: n_images=%d pixels=%ld unsupported (at most 65535 images of 2^23 pixels)", n_images, pixels);
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)n_images * 256 * sizeof(unsigned), s);    // overwritten, not accumulated
    if (e != hipSuccess) {
        ngan::set_error("ngan_u8_histogram: clearing the counts failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    int blocks = ngan::ceil_div(pixels >> 4, 256L * HIST_VEC_PER_THREAD);
    blocks = blocks < 1 ? 1 : (blocks > HIST_MAX_BLOCKS ? HIST_MAX_BLOCKS : blocks);
    hipLaunchKernelGGL(u8_histogram_kernel, dim3(blocks, n_images), dim3(256), 0, s, images, hist, pixels);
    return ngan::launch_status("ngan_u8_histogram");
}

extern "C" int ngan_multiotsu4_noise_stats(const unsigned int* hist, void* workspace, int* thresholds, double* record, int* status,
                                           int n_images, void* stream) {
    NGAN_REQUIRE(hist && workspace && thresholds && record && status, NGAN_ERR_ARG, "multiotsu4_noise_stats: null pointer");
    NGAN_REQUIRE(n_images > 0, NGAN_ERR_ARG, "multiotsu4_noise_stats: n_images=%d must be positive", n_images);
    NGAN_REQUIRE(n_images < 65536, NGAN_ERR_SHAPE, "multiotsu4_noise_stats: n_images=%d unsupported (at most 65535)", n_images);
    hipStream_t s = (hipStream_t)stream;
    OtsuBest* slots = reinterpret_cast<OtsuBest*>(workspace);
    hipLaunchKernelGGL(multiotsu4_search_kernel, dim3(OTSU_SPLIT, n_images), dim3(256), 0, s, hist, slots);
    hipLaunchKernelGGL(multiotsu4_finish_kernel, dim3(n_images), dim3(256), 0, s, hist, slots, thresholds, record, status);
    return ngan::launch_status("ngan_multiotsu4_noise_stats");
}

extern "C" int ngan_u8_pad_noise_fill(const unsigned char* images, const float* normals, const double* record, float* canvases,
                                      int n_images, int R, void* stream) {
    NGAN_REQUIRE(images && normals && record && canvases, NGAN_ERR_ARG, "u8_pad_noise_fill: null pointer");
    NGAN_REQUIRE(n_images > 0 && R > 0, NGAN_ERR_ARG, "u8_pad_noise_fill: n_images=%d R=%d must be positive", n_images, R);
    NGAN_REQUIRE(n_images < 65536 && (long)R * R <= MAX_PIXELS, NGAN_ERR_SHAPE,
                 "u8_pad_noise_fill: n_images=%d R=%d unsupported (at most 65535 images of 2^23 pixels)", n_images, R);
    NGAN_REQUIRE((reinterpret_cast<size_t>(canvases) & 15) == 0 && (reinterpret_cast<size_t>(normals) & 15) == 0, NGAN_ERR_ARG,
                 "u8_pad_noise_fill: normals and canvases must be 16-byte aligned (16-byte loads and stores)");
    const int pad = R / 4, P = R + 2 * pad;
    const long total = (long)n_images * P * P;
    const long groups = (total + 3) / 4;
    NGAN_REQUIRE((groups + 255) / 256 < (1L << 31), NGAN_ERR_SHAPE, "u8_pad_noise_fill: %ld canvas pixels in one call", total);
    hipLaunchKernelGGL(u8_pad_noise_fill_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream, images,
                       normals, record, canvases, total, R, pad, P);
    return ngan::launch_status("ngan_u8_pad_noise_fill");
}
