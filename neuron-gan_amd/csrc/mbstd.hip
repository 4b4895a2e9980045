// Minibatch standard deviation of the PG critic's head (include/ngan_mbstd.h): the statistic, its backward and backward-of-backward,
// and the bilinear field family that feeds the statistic into the head's 3x3 convolution as a constant plane.
//
// Layout of the work.  A thread owns four consecutive features (one 16-byte access per sample) of one group and walks the group's
// G samples; everything per feature is local to those G values and fp32 (mbstd_bits.h).  The only reduction across threads is the sum
// over features: each thread's term goes to fp64 at once, a block sums its 256 terms by a wave butterfly and four LDS slots, and a
// second, tiny launch adds the blocks' partial sums in index order.  No atomics, no hand-off between workgroups inside a launch.
// The tensors are small (at most 32 x 16 x 16 x 128 floats): these launches are bound by latency, so a sample is simply read again for
// each pass over the group (the second and third reads hit the L2) instead of being held in registers for a compile-time G.
#include "ngan_common.h"
#include "mbstd_bits.h"

namespace {

constexpr int TPB = 256;
constexpr long FEATURES_PER_BLOCK = 4L * TPB;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the block's 256 threads, in every thread; sh: 4 doubles that nothing else uses
__device__ __forceinline__ double block_sum_d(double v, double* sh) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

#define F4_EACH(expr_x, expr_y, expr_z, expr_w) make_float4(expr_x, expr_y, expr_z, expr_w)

// sum over the group of the float4 at p, p + J, ..: pairs, as mbstd::group_sum
__device__ __forceinline__ float4 group_sum4(const float* p, long J, int G) {
    float4 s = f4zero();
    int n = 0;
    for (; n + 1 < G; n += 2) {
        const float4 a = ld4(p + n * J), b = ld4(p + (n + 1) * J);
        s = F4_EACH(mbstd::pair_step(s.x, a.x, b.x), mbstd::pair_step(s.y, a.y, b.y), mbstd::pair_step(s.z, a.z, b.z),
                    mbstd::pair_step(s.w, a.w, b.w));
    }
    if (n < G) s = f4add(s, ld4(p + n * J));
    return s;
}

__device__ __forceinline__ void stat4(const float* p, long J, int G, float4& mu, float4& sg) {
    const float4 s = group_sum4(p, J, G);
    mu = F4_EACH(mbstd::mean_of(s.x, G), mbstd::mean_of(s.y, G), mbstd::mean_of(s.z, G), mbstd::mean_of(s.w, G));
    float4 q = f4zero();
    for (int n = 0; n < G; ++n) {
        const float4 v = ld4(p + n * J);
        q = F4_EACH(mbstd::sq_step(q.x, v.x, mu.x), mbstd::sq_step(q.y, v.y, mu.y), mbstd::sq_step(q.z, v.z, mu.z),
                    mbstd::sq_step(q.w, v.w, mu.w));
    }
    sg = F4_EACH(mbstd::sigma_of(q.x, G, mbstd::EPS), mbstd::sigma_of(q.y, G, mbstd::EPS), mbstd::sigma_of(q.z, G, mbstd::EPS),
                 mbstd::sigma_of(q.w, G, mbstd::EPS));
}

__device__ __forceinline__ double f4sum_d(float4 v) { return ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w); }

// grid (blocks of 1024 features, groups): part[group][block] = sum of sigma over the block's features
__global__ __launch_bounds__(TPB) void k_mbstd_fwd(const float* __restrict__ x, double* __restrict__ part, long J, int G) {
    __shared__ double sh[4];
    const long j4 = (long)blockIdx.x * TPB + threadIdx.x;
    double t = 0.0;
    if (j4 < (J >> 2)) {
        float4 mu, sg;
        stat4(x + (long)blockIdx.y * G * J + 4 * j4, J, G, mu, sg);
        t = f4sum_d(sg);
    }
    t = block_sum_d(t, sh);
    if (threadIdx.x == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// one wave per group: out[n] = (sum of the group's partial sums) / divisor for the group's G samples
__global__ __launch_bounds__(64) void k_mbstd_finish(const double* __restrict__ part, int nblk, double divisor, float* __restrict__ out,
                                                     int G) {
    const long g = blockIdx.x;
    double a = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) a += part[g * nblk + i];
    a = wave_sum_d(a);
    const float v = (float)(a / divisor);
    for (int n = threadIdx.x; n < G; n += 64) out[g * G + n] = v;
}

__global__ __launch_bounds__(TPB) void k_mbstd_bwd(const float* __restrict__ gs, const float* __restrict__ x, float* __restrict__ gx, long J,
                                                   int G) {
    const long j4 = (long)blockIdx.x * TPB + threadIdx.x;
    if (j4 >= (J >> 2)) return;
    const long base = (long)blockIdx.y * G * J + 4 * j4;
    const float coef = mbstd::coef_of(mbstd::group_sum(gs + (long)blockIdx.y * G, 1L, G), G, J);
    float4 mu, sg;
    stat4(x + base, J, G, mu, sg);
    for (int n = 0; n < G; ++n) {
        const float4 v = ld4(x + base + n * J);
        st4(gx + base + n * J, F4_EACH(mbstd::gx_of(coef, v.x, mu.x, sg.x), mbstd::gx_of(coef, v.y, mu.y, sg.y),
                                       mbstd::gx_of(coef, v.z, mu.z, sg.z), mbstd::gx_of(coef, v.w, mu.w, sg.w)));
    }
}

// part[group][block] = sum over the block's features of hd / sigma; dx complete
__global__ __launch_bounds__(TPB) void k_mbstd_bwdbwd(const float* __restrict__ h, const float* __restrict__ gs, const float* __restrict__ x,
                                                      double* __restrict__ part, float* __restrict__ dx, long J, int G) {
    __shared__ double sh[4];
    const long j4 = (long)blockIdx.x * TPB + threadIdx.x;
    double t = 0.0;
    if (j4 < (J >> 2)) {
        const long base = (long)blockIdx.y * G * J + 4 * j4;
        const float coef = mbstd::coef_of(mbstd::group_sum(gs + (long)blockIdx.y * G, 1L, G), G, J);
        float4 mu, sg;
        stat4(x + base, J, G, mu, sg);
        const float4 hs = group_sum4(h + base, J, G);
        const float4 hbar = F4_EACH(mbstd::mean_of(hs.x, G), mbstd::mean_of(hs.y, G), mbstd::mean_of(hs.z, G), mbstd::mean_of(hs.w, G));
        float4 hd = f4zero();
        for (int n = 0; n < G; ++n) {
            const float4 v = ld4(x + base + n * J), hv = ld4(h + base + n * J);
            hd = F4_EACH(mbstd::hd_step(hd.x, hv.x, v.x, mu.x), mbstd::hd_step(hd.y, hv.y, v.y, mu.y), mbstd::hd_step(hd.z, hv.z, v.z, mu.z),
                         mbstd::hd_step(hd.w, hv.w, v.w, mu.w));
        }
        const float4 cv = F4_EACH(mbstd::curv_of(hd.x, G, sg.x), mbstd::curv_of(hd.y, G, sg.y), mbstd::curv_of(hd.z, G, sg.z),
                                  mbstd::curv_of(hd.w, G, sg.w));
        for (int n = 0; n < G; ++n) {
            const float4 v = ld4(x + base + n * J), hv = ld4(h + base + n * J);
            st4(dx + base + n * J,
                F4_EACH(mbstd::dx_of(coef, hv.x, hbar.x, v.x, mu.x, sg.x, cv.x), mbstd::dx_of(coef, hv.y, hbar.y, v.y, mu.y, sg.y, cv.y),
                        mbstd::dx_of(coef, hv.z, hbar.z, v.z, mu.z, sg.z, cv.z), mbstd::dx_of(coef, hv.w, hbar.w, v.w, mu.w, sg.w, cv.w)));
        }
        t = f4sum_d(F4_EACH(hd.x / sg.x, hd.y / sg.y, hd.z / sg.z, hd.w / sg.w));
    }
    t = block_sum_d(t, sh);
    if (threadIdx.x == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// ---- the field family -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 taps4(const float* __restrict__ w_std, int co, int y, int x, int H, int W) {
    return F4_EACH(mbstd::field_taps(w_std + (co + 0) * 9, y, x, H, W), mbstd::field_taps(w_std + (co + 1) * 9, y, x, H, W),
                   mbstd::field_taps(w_std + (co + 2) * 9, y, x, H, W), mbstd::field_taps(w_std + (co + 3) * 9, y, x, H, W));
}

__global__ __launch_bounds__(TPB) void k_stdfield_add(const float* c, const float* __restrict__ s, const float* __restrict__ w_std, float* out,
                                                      long total4, int H, int W, int C, float scale) {
    const long i4 = (long)blockIdx.x * TPB + threadIdx.x;
    if (i4 >= total4) return;
    const long pix = (4 * i4) / C;
    const int co = (int)((4 * i4) % C);
    const int xx = (int)(pix % W), yy = (int)((pix / W) % H);
    const long n = pix / ((long)W * H);
    const float4 t = taps4(w_std, co, yy, xx, H, W), cv = c ? ld4(c + 4 * i4) : f4zero();
    const float k = scale * s[n];
    st4(out + 4 * i4, F4_EACH(mbstd::field_add(cv.x, k, t.x), mbstd::field_add(cv.y, k, t.y), mbstd::field_add(cv.z, k, t.z),
                              mbstd::field_add(cv.w, k, t.w)));
}

// position class of a coordinate along one axis: 0 first, 2 last, 1 between (an extent of 1 has the class 0 alone), and a coordinate of
// that class; T depends on (y, x) through the two classes only
__device__ __forceinline__ int axis_class(int p, int n) { return p == 0 ? 0 : (p == n - 1 ? 2 : 1); }
__device__ __forceinline__ int class_coord(int cls, int n) { return cls == 0 ? 0 : (cls == 2 ? n - 1 : 1); }

// one block per sample.  T of the nine position classes goes to LDS first (9 C floats, formed by mbstd::field_taps at a coordinate of
// the class: the bits stdfield_add forms per pixel), so the stream over g costs one LDS read per float4 instead of 36 weight loads.
__global__ __launch_bounds__(TPB) void k_stdfield_ds(const float* __restrict__ g, const float* __restrict__ w_std, float* __restrict__ gs, int H,
                                                     int W, int C, float scale) {
    extern __shared__ __align__(16) float tab[];          // [9][C], then the block sum's four doubles (36 C bytes: a multiple of 16)
    double* sh = reinterpret_cast<double*>(tab + 9 * C);
    for (int i = threadIdx.x; i < 9 * C; i += TPB) {
        const int cls = i / C, co = i - cls * C;
        const int yy = class_coord(cls / 3, H), xx = class_coord(cls % 3, W);
        tab[i] = (yy < H && xx < W) ? mbstd::field_taps(w_std + co * 9, yy, xx, H, W) : 0.f;      // (a class the extent does not have)
    }
    __syncthreads();
    const int per4 = (H * W * C) >> 2;
    const float* gn = g + (long)blockIdx.x * H * W * C;
    double acc = 0.0;
#pragma unroll 4
    for (int i4 = threadIdx.x; i4 < per4; i4 += TPB) {
        const int pix = (4 * i4) / C, co = 4 * i4 - pix * C;
        const int cls = axis_class(pix / W, H) * 3 + axis_class(pix % W, W);
        const float4 t = *reinterpret_cast<const float4*>(tab + cls * C + co), gv = ld4(gn + 4 * i4);
        acc += f4sum_d(F4_EACH(gv.x * t.x, gv.y * t.y, gv.z * t.z, gv.w * t.w));
    }
    acc = block_sum_d(acc, sh);
    if (threadIdx.x == 0) gs[blockIdx.x] = (float)((double)scale * acc);
}

// one block per four output channels; a thread walks pixels (n, y, x) and keeps the nine tap sums of its four channels
__global__ __launch_bounds__(TPB) void k_stdfield_dw(const float* __restrict__ g, const float* __restrict__ s, float* __restrict__ gw, long npix,
                                                     int H, int W, int C, float scale) {
    __shared__ double sh[4][36];
    const int co = blockIdx.x * 4;
    double acc[4][9];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[i][k] = 0.0;
    for (long pix = threadIdx.x; pix < npix; pix += TPB) {
        const int xx = (int)(pix % W), yy = (int)((pix / W) % H);
        const float sv = s[pix / ((long)W * H)];
        const float4 gv = ld4(g + pix * C + co);
        const double p[4] = {(double)(sv * gv.x), (double)(sv * gv.y), (double)(sv * gv.z), (double)(sv * gv.w)};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
                if (mbstd::tap_inside(ky, yy, H) && mbstd::tap_inside(kx, xx, W)) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i][ky * 3 + kx] += p[i];
                }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double v = wave_sum_d(acc[i][k]);
            if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][i * 9 + k] = v;
        }
    __syncthreads();
    if (threadIdx.x < 36) {
        const int t = threadIdx.x;
        const double total = ((sh[0][t] + sh[1][t]) + sh[2][t]) + sh[3][t];
        gw[(long)co * 9 + t] = (float)((double)scale * total);          // (co + t / 9) * 9 + t % 9
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// the shape rules shared by the three statistic entry points
int check_groups(const char* what, int B, int H, int W, int C, int segments, int G_eff) {
    NGAN_REQUIRE(B > 0 && B < 65536, NGAN_ERR_SHAPE, "%s: B=%d unsupported (1 .. 65535 samples per call)", what, B);
    NGAN_REQUIRE(H > 0 && W > 0 && C > 0 && C % 4 == 0, NGAN_ERR_SHAPE, "%s: H=%d W=%d C=%d unsupported (C a positive multiple of 4)", what, H, W,
                 C);
    NGAN_REQUIRE((long)H * W * C <= (1L << 31), NGAN_ERR_SHAPE, "%s: H=%d W=%d C=%d: more than 2^31 features per sample", what, H, W, C);
    NGAN_REQUIRE(segments > 0 && B % segments == 0, NGAN_ERR_SHAPE, "%s: segments=%d does not divide B=%d", what, segments, B);
    NGAN_REQUIRE(G_eff > 0 && (B / segments) % G_eff == 0, NGAN_ERR_SHAPE, "%s: G_eff=%d does not divide the segment size %d", what, G_eff,
                 G_eff > 0 && segments > 0 ? B / segments : 0);
    return NGAN_OK;
}

int check_field(const char* what, int B, int H, int W, int C) {
    NGAN_REQUIRE(B > 0 && B < 65536, NGAN_ERR_SHAPE, "%s: B=%d unsupported (1 .. 65535 samples per call)", what, B);
    NGAN_REQUIRE(H > 0 && W > 0 && C > 0 && C % 4 == 0, NGAN_ERR_SHAPE, "%s: H=%d W=%d C=%d unsupported (C a positive multiple of 4)", what, H, W,
                 C);
    // stdfield_add runs one thread per four elements: its launch must stay below 2^32 threads (ngan_common.h)
    NGAN_REQUIRE((long)B * H * W * C < (1L << 34) - 1024, NGAN_ERR_SHAPE, "%s: B=%d H=%d W=%d C=%d too large (2^34 elements)", what, B, H, W, C);
    return NGAN_OK;
}

}  // namespace

extern "C" {

long ngan_mbstd_workspace_doubles(int B, int H, int W, int C, int G_eff) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4 || G_eff <= 0 || B % G_eff) return 0;
    const long J = (long)H * W * C;
    return (long)(B / G_eff) * ((J + FEATURES_PER_BLOCK - 1) / FEATURES_PER_BLOCK);
}

int ngan_mbstd_fwd(const float* x, float* s, double* workspace, int B, int H, int W, int C, int segments, int G_eff, void* stream) {
    NGAN_REQUIRE(x && s && workspace, NGAN_ERR_ARG, "mbstd_fwd: null pointer");
    NGAN_REQUIRE(aligned16(x) && aligned16(workspace), NGAN_ERR_ARG, "mbstd_fwd: x and workspace must start on a 16-byte boundary");
    if (int st = check_groups("mbstd_fwd", B, H, W, C, segments, G_eff)) return st;
    const long J = (long)H * W * C;
    const int nblk = ngan::ceil_div(J, FEATURES_PER_BLOCK), ngroups = B / G_eff;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mbstd_fwd, dim3(nblk, ngroups), dim3(TPB), 0, st, x, workspace, J, G_eff);
    if (int e = ngan::launch_status("mbstd_fwd")) return e;
    hipLaunchKernelGGL(k_mbstd_finish, dim3(ngroups), dim3(64), 0, st, workspace, nblk, (double)J, s, G_eff);
    return ngan::launch_status("mbstd_fwd (finish)");
}

int ngan_mbstd_bwd(const float* gs, const float* x, float* gx, int B, int H, int W, int C, int segments, int G_eff, void* stream) {
    NGAN_REQUIRE(gs && x && gx, NGAN_ERR_ARG, "mbstd_bwd: null pointer");
    NGAN_REQUIRE(aligned16(x) && aligned16(gx), NGAN_ERR_ARG, "mbstd_bwd: x and gx must start on a 16-byte boundary");
    if (int st = check_groups("mbstd_bwd", B, H, W, C, segments, G_eff)) return st;
    const long J = (long)H * W * C;
    hipLaunchKernelGGL(k_mbstd_bwd, dim3(ngan::ceil_div(J, FEATURES_PER_BLOCK), B / G_eff), dim3(TPB), 0, (hipStream_t)stream, gs, x, gx, J,
                       G_eff);
    return ngan::launch_status("mbstd_bwd");
}

int ngan_mbstd_bwdbwd(const float* h, const float* gs, const float* x, float* dgs, float* dx, double* workspace, int B, int H, int W,
                      int C, int segments, int G_eff, void* stream) {
    NGAN_REQUIRE(h && gs && x && dgs && dx && workspace, NGAN_ERR_ARG, "mbstd_bwdbwd: null pointer");
    NGAN_REQUIRE(aligned16(h) && aligned16(x) && aligned16(dx) && aligned16(workspace), NGAN_ERR_ARG,
                 "mbstd_bwdbwd: h, x, dx and workspace must start on a 16-byte boundary");
    if (int st = check_groups("mbstd_bwdbwd", B, H, W, C, segments, G_eff)) return st;
    const long J = (long)H * W * C;
    const int nblk = ngan::ceil_div(J, FEATURES_PER_BLOCK), ngroups = B / G_eff;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_mbstd_bwdbwd, dim3(nblk, ngroups), dim3(TPB), 0, st, h, gs, x, workspace, dx, J, G_eff);
    if (int e = ngan::launch_status("mbstd_bwdbwd")) return e;
    hipLaunchKernelGGL(k_mbstd_finish, dim3(ngroups), dim3(64), 0, st, workspace, nblk, (double)G_eff * (double)J, dgs, G_eff);
    return ngan::launch_status("mbstd_bwdbwd (finish)");
}

int ngan_stdfield_add(const float* c, const float* s, const float* w_std, float* out, int B, int H, int W, int C, float scale, void* stream) {
    NGAN_REQUIRE(s && w_std && out, NGAN_ERR_ARG, "stdfield_add: null pointer");
    NGAN_REQUIRE(aligned16(c) && aligned16(out), NGAN_ERR_ARG, "stdfield_add: c and out must start on a 16-byte boundary");
    if (int st = check_field("stdfield_add", B, H, W, C)) return st;
    const long total4 = ((long)B * H * W * C) >> 2;
    hipLaunchKernelGGL(k_stdfield_add, dim3(ngan::ceil_div(total4, TPB)), dim3(TPB), 0, (hipStream_t)stream, c, s, w_std, out, total4, H, W, C,
                       scale);
    return ngan::launch_status("stdfield_add");
}

int ngan_stdfield_ds(const float* g, const float* w_std, float* gs, int B, int H, int W, int C, float scale, void* stream) {
    NGAN_REQUIRE(g && w_std && gs, NGAN_ERR_ARG, "stdfield_ds: null pointer");
    NGAN_REQUIRE(aligned16(g), NGAN_ERR_ARG, "stdfield_ds: g must start on a 16-byte boundary");
    if (int st = check_field("stdfield_ds", B, H, W, C)) return st;
    NGAN_REQUIRE((long)H * W * C < (1L << 29) && C <= 4096, NGAN_ERR_SHAPE, "stdfield_ds: H=%d W=%d C=%d too large (H*W*C below 2^29, C at most 4096)", H, W, C);
    hipLaunchKernelGGL(k_stdfield_ds, dim3(B), dim3(TPB), 9 * C * sizeof(float) + 4 * sizeof(double), (hipStream_t)stream, g, w_std, gs, H, W, C, scale);
    return ngan::launch_status("stdfield_ds");
}

int ngan_stdfield_dw(const float* g, const float* s, float* gw, int B, int H, int W, int C, float scale, void* stream) {
    NGAN_REQUIRE(g && s && gw, NGAN_ERR_ARG, "stdfield_dw: null pointer");
    NGAN_REQUIRE(aligned16(g), NGAN_ERR_ARG, "stdfield_dw: g must start on a 16-byte boundary");
    if (int st = check_field("stdfield_dw", B, H, W, C)) return st;
    hipLaunchKernelGGL(k_stdfield_dw, dim3(C / 4), dim3(TPB), 0, (hipStream_t)stream, g, s, gw, (long)B * H * W, H, W, C, scale);
    return ngan::launch_status("stdfield_dw");
}

}  // extern "C"
