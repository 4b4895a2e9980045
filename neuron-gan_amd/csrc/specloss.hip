// Spectral regularisation of the generator (Durall et al. 2020): the kernels behind ops.SpectralLoss (include/ngan_spectral.h).  Per
// image x (one colour channel, R x R) with the radial spectrum S of csrc/spectrum.hip (window w, F = fft2(w x), norm = sum w^2) and a
// target t:  r = S / t,  q = ln((r + floor) / (1 + floor)),  l[b] = sum_{k=1..R/2} q^2 / (R/2),  L = scale sum_b l[b]  (scale is
// lambda / B_global);  c[b][k] = dL/dS[b][k] = scale / (R/2) 2 q / (t (r + floor)), 0 for bin 0 and where t <= 0; and
//     dL/dx = 2 w Re(sum_f a[f] F[f] exp(+2 pi i f.p / R)),   a[f] = c[ring(f)] / (n_ring(f) norm), 0 in the corners beyond R/2.
//   forward      row_kernel, col_kernel and fold_kernel of spectrum_fft.h: the metric's own launches (the radial values are the
//                metric's, bit for bit); the column pass also keeps the half-plane transform F[b][v][fy], v = 0 .. R/2, and the
//                fold the divisors n_k norm of its bins.
//   head_kernel  ONE workgroup of 16 waves, a wave per image (image b on wave b mod 16): lane j forms q and c of bins j, j + 64, ... in
//                fp64 and adds their squares ascending, the lanes' sums meet in a fixed butterfly; a wave adds its images' l[b]
//                ascending and thread 0 the 16 waves' sums, ascending: one order for a given B, whatever the images hold.  c is
//                rounded once to fp32; the adjoint's coefficient a[b][k] = c / (n_k norm) is divided in fp64 from the unrounded c
//                and rounded once.  n_k norm is the forward's own divisor, handed over as a table of R/2 + 1 doubles.
//   col_adj      mirrors col_kernel's tiling: a block of COLS columns of F, each element scaled on load by a[b][ring(u, v)] (the
//                image's table in LDS; the ring from signed frequencies by the integer rule of spectrum_ring.h) and conjugated;
//                fft_lds; conjugated again on the way out: the inverse transform along y in the forward's butterfly order.  Written
//                transposed, H[b][y][v].
//   row_adj      mirrors row_kernel's: ROWS rows of H.  Rows 2t and 2t+1 are completed to the Hermitian whole (columns 0 and R/2
//                are their own conjugates: their real parts count, once) and packed as H0 + i H1: Z[v] = X0[v] + i X1[v],
//                Z[R-v] = conj X0[v] + i conj X1[v]; conjugate, fft_lds, conjugate: Re and Im are the two rows.  Each value is
//                multiplied by 2 w[y][x] (w = h[y] h[x] one product, the doubling exact) and then by the upstream gradient of L,
//                read from device memory; an optional incoming image gradient is added on the store (addend + value, one rounding).
// No atomics, no state between calls, no inline assembly; contraction is off (spectrum_fft.h), so tests/specloss_cases.py emulates
// the adjoint operation by operation.  LDS at R = 1024: 8 x 1026 float2 + 1024 float2 twiddles + 1024 taps (or 513 coefficients)
// = 77 952 bytes (76 KB) of the 160 KB a workgroup may hold, the forward's own figure.
#include "spectrum_fft.h"
#include "../../include/ngan_spectral.h"

namespace {

constexpr int KMAX = 513;
constexpr int HT = 1024, HW = HT / 64;                         // threads and waves of the head's one workgroup

// grid (1)
__global__ __launch_bounds__(HT) void head_kernel(const double* __restrict__ S, const double* __restrict__ tgt,
                                                  const double* __restrict__ ring_norm, int B, int R, double scale, double floor,
                                                  double* __restrict__ per_image, float* __restrict__ loss, float* __restrict__ dS,
                                                  float* __restrict__ coef, int* __restrict__ skipped) {
    __shared__ double nn[KMAX], tk[KMAX], wsum[HW];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = R / 2, K = half + 1;
    for (int k = tid; k < K; k += HT) {
        nn[k] = ring_norm[k];                                  // n_k norm, as the forward's fold divided by it
        tk[k] = tgt[k];
    }
    __syncthreads();
    const double per_bin = scale / (double)half, one_floor = 1.0 + floor;
    double mine = 0.0;                                         // this wave's images, ascending
    for (int b = wave; b < B; b += HW) {
        const long row = (long)b * K;
        double part = 0.0;                                     // this lane's bins, ascending
        for (int k = lane; k < K; k += 64) {
            double c = 0.0;
            const double t = tk[k];
            if (k >= 1 && t > 0.0) {
                const double r = S[row + k] / t;
                const double q = log((r + floor) / one_floor);
                part += q * q;
                c = per_bin * (2.0 * q / (t * (r + floor)));
            }
            dS[row + k] = (float)c;
            coef[row + k] = (float)(c / nn[k]);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);      // a fixed butterfly: every lane ends with the same sum
        const double l = part / (double)half;
        if (lane == 0) per_image[b] = l;
        mine += l;
    }
    if (lane == 0) wsum[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int w = 0; w < HW; ++w) total += wsum[w];
        *loss = (float)(scale * total);
        int n = 0;
        for (int k = 1; k < K; ++k) n += tk[k] > 0.0 ? 0 : 1;
        *skipped = n;
    }
}

// grid (ceil(K / COLS), 1, B)
template <int R>
__global__ __launch_bounds__(NT) void col_adj_kernel(const float2* __restrict__ F, const float* __restrict__ coef, float2* __restrict__ H) {
    constexpr int T = rows_of(R) / 2, P = pitch_of(R), K = R / 2 + 1, HALF = R / 2;
    __shared__ __attribute__((aligned(16))) float2 buf[T * P];
    __shared__ float2 tw[R];
    __shared__ float a[K];
    const int tid = threadIdx.x;
    const int v0 = blockIdx.x * T;
    const int valid = K - v0 < T ? K - v0 : T;                 // columns of this tile that exist
    const long b = blockIdx.z;
    build_twiddles<R>(tw);
    for (int k = tid; k < K; k += NT) a[k] = k >= 1 ? coef[b * K + k] : 0.f;
    __syncthreads();
    {
        const float2* src = F + (b * K + v0) * (long)R;        // columns v0 .. v0 + valid: one contiguous block
        for (int e2 = tid; e2 < T * R / 2; e2 += NT) {         // two complex values per load
            const int t = (2 * e2) / R, fy = 2 * e2 - t * R;
            float4 o = f4zero();
            if (t < valid) {
                const float4 v = ld4(reinterpret_cast<const float*>(src + 2 * e2));
                const int u0 = fy < HALF ? fy : fy - R, u1 = fy + 1 < HALF ? fy + 1 : fy + 1 - R;
                const int k0 = ring_of_pair(u0, v0 + t), k1 = ring_of_pair(u1, v0 + t);
                const float c0 = k0 <= HALF ? a[k0] : 0.f, c1 = k1 <= HALF ? a[k1] : 0.f;
                o = make_float4(v.x * c0, -(v.y * c0), v.z * c1, -(v.w * c1));      // conj(a F)
            }
            *reinterpret_cast<float4*>(buf + t * P + fy) = o;
        }
    }
    __syncthreads();
    fft_lds<R, T>(buf, tw);
    float2* out = H + b * (long)R * K + v0;                    // H[b][y][v0 + t]
    for (int e = tid; e < R * T; e += NT) {
        const int y = e / T, t = e - y * T;
        if (t < valid) {
            const float2 z = buf[t * P + y];
            out[(long)y * K + t] = make_float2(z.x, -z.y);
        }
    }
}

// grid (R / ROWS, 1, B)
template <int R>
__global__ __launch_bounds__(NT) void row_adj_kernel(const float2* __restrict__ H, const float* __restrict__ upstream,
                                                     const float* __restrict__ addend, float* __restrict__ grad, int window) {
    constexpr int ROWS = rows_of(R), T = ROWS / 2, P = pitch_of(R), K = R / 2 + 1, HALF = R / 2;
    __shared__ __attribute__((aligned(16))) float2 buf[T * P];
    __shared__ float2 tw[R];
    __shared__ float h[R];
    const int tid = threadIdx.x;
    const int y0 = blockIdx.x * ROWS;
    const long b = blockIdx.z;
    build_twiddles<R>(tw);
    if (window)
        for (int i = tid; i < R; i += NT) h[i] = (float)(0.5 - 0.5 * cospi(2.0 * (double)i / (double)R));
    {
        const float2* src = H + (b * R + y0) * (long)K;        // rows y0 .. y0 + ROWS: one contiguous block
        for (int e = tid; e < T * K; e += NT) {
            const int t = e / K, v = e - t * K;
            const float2 x0 = src[(long)(2 * t) * K + v], x1 = src[(long)(2 * t + 1) * K + v];
            float2* z = buf + t * P;
            if (v == 0 || v == HALF) z[v] = make_float2(x0.x, -x1.x);              // conj(Re X0 + i Re X1)
            else {
                z[v] = make_float2(x0.x - x1.y, -(x0.y + x1.x));                   // conj(X0 + i X1)
                z[R - v] = make_float2(x0.x + x1.y, -(x1.x - x0.y));               // conj(conj X0 + i conj X1)
            }
        }
    }
    __syncthreads();
    fft_lds<R, T>(buf, tw);
    const float up = *upstream;
    for (int e4 = tid; e4 < ROWS * R / 4; e4 += NT) {
        const int r = (4 * e4) / R, x = 4 * e4 - r * R;
        const float2* z = buf + (r >> 1) * P + x;
        float val[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const float g = (r & 1) ? -z[m].y : z[m].x;
            float w2 = 2.0f;
            if (window) {
                const float w = h[y0 + r] * h[x + m];
                w2 = 2.0f * w;
            }
            const float gw = g * w2;
            val[m] = gw * up;
        }
        const long at = ((b * R + y0 + r) * (long)R) + x;
        float4 o = make_float4(val[0], val[1], val[2], val[3]);
        if (addend) {
            const float4 q = ld4(addend + at);
            o = make_float4(q.x + o.x, q.y + o.y, q.z + o.z, q.w + o.w);
        }
        st4(grad + at, o);
    }
}

size_t partials_bytes(int B, int R) { return (size_t)B * col_groups(R) * (R / 2 + 1) * sizeof(double); }

template <int R>
void launch_fwd(const float* images, double* radial, float2* F, double* ring_norm, void* workspace, int B, int window, double norm,
                hipStream_t s) {
    float2* G = reinterpret_cast<float2*>(workspace);
    double* partials = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + half_plane_bytes(B, R, 1));
    const dim3 rows(R / rows_of(R), 1, B), cols(col_groups(R), 1, B);
    hipLaunchKernelGGL((row_kernel<R, 1>), rows, dim3(NT), 0, s, images, G, window);
    hipLaunchKernelGGL(col_kernel<R>, cols, dim3(NT), 0, s, G, partials, (float*)nullptr, F, norm);
    hipLaunchKernelGGL(fold_kernel, dim3(B), dim3(NT), 0, s, partials, radial, ring_norm, R, 1, col_groups(R), norm);
}

template <int R>
void launch_bwd(const float2* F, const float* coef, const float* upstream, const float* addend, float* grad, void* workspace, int B,
                int window, hipStream_t s) {
    float2* H = reinterpret_cast<float2*>(workspace);
    const dim3 rows(R / rows_of(R), 1, B), cols(col_groups(R), 1, B);
    hipLaunchKernelGGL(col_adj_kernel<R>, cols, dim3(NT), 0, s, F, coef, H);
    hipLaunchKernelGGL(row_adj_kernel<R>, rows, dim3(NT), 0, s, H, upstream, addend, grad, window);
}

bool shape_ok(const char* who, int B, int R, int C) {
    if (!supported(R)) {
        ngan::set_error("%s: R=%d unsupported (a power of two, 16 .. 1024)", who, R);
        return false;
    }
    if (C != 1) {
        ngan::set_error("%s: C=%d unsupported (one colour channel: the generator's image tensor is planar greyscale)", who, C);
        return false;
    }
    if (B <= 0 || B > 65535) {
        ngan::set_error("%s: B=%d unsupported (1 .. 65535 images per call)", who, B);
        return false;
    }
    return true;
}

}  // namespace

extern "C" size_t ngan_specloss_fwd_workspace_bytes(int B, int R, int C) {
    if (B <= 0 || B > 65535 || !supported(R) || C != 1) return 0;
    return half_plane_bytes(B, R, 1) + partials_bytes(B, R);
}

extern "C" size_t ngan_specloss_bwd_workspace_bytes(int B, int R, int C) {
    if (B <= 0 || B > 65535 || !supported(R) || C != 1) return 0;
    return half_plane_bytes(B, R, 1);
}

extern "C" int ngan_specloss_fwd(const float* images, double* radial, float* transform, double* ring_norm, void* workspace, int B, int R,
                                 int C, int window, void* stream) {
    NGAN_REQUIRE(images && radial && transform && ring_norm, NGAN_ERR_ARG, "specloss_fwd: null pointer");
    NGAN_REQUIRE(workspace, NGAN_ERR_ARG, "specloss_fwd: null workspace (ngan_specloss_fwd_workspace_bytes names its size)");
    if (!shape_ok("specloss_fwd", B, R, C)) return NGAN_ERR_SHAPE;
    NGAN_REQUIRE(((uintptr_t)images | (uintptr_t)workspace | (uintptr_t)transform) % 16 == 0 && ((uintptr_t)radial | (uintptr_t)ring_norm) % 8 == 0,
                 NGAN_ERR_ARG, "specloss_fwd: images, transform and workspace must start on a 16-byte boundary, radial and ring_norm on an 8-byte one");
    const double norm = spectrum_norm(R, window);
    hipStream_t s = (hipStream_t)stream;
    float2* F = reinterpret_cast<float2*>(transform);
    switch (R) {
        case 16: launch_fwd<16>(images, radial, F, ring_norm, workspace, B, window != 0, norm, s); break;
        case 32: launch_fwd<32>(images, radial, F, ring_norm, workspace, B, window != 0, norm, s); break;
        case 64: launch_fwd<64>(images, radial, F, ring_norm, workspace, B, window != 0, norm, s); break;
        case 128: launch_fwd<128>(images, radial, F, ring_norm, workspace, B, window != 0, norm, s); break;
        case 256: launch_fwd<256>(images, radial, F, ring_norm, workspace, B, window != 0, norm, s); break;
        case 512: launch_fwd<512>(images, radial, F, ring_norm, workspace, B, window != 0, norm, s); break;
        default: launch_fwd<1024>(images, radial, F, ring_norm, workspace, B, window != 0, norm, s); break;
    }
    return ngan::launch_status("ngan_specloss_fwd");
}

extern "C" int ngan_specloss_head(const double* radial, const double* target, const double* ring_norm, int B, int R, double scale,
                                  double floor, double* per_image, float* loss, float* dradial, float* coef, int* skipped, void* stream) {
    NGAN_REQUIRE(radial && target && ring_norm && per_image && loss && dradial && coef && skipped, NGAN_ERR_ARG, "specloss_head: null pointer");
    if (!shape_ok("specloss_head", B, R, 1)) return NGAN_ERR_SHAPE;
    NGAN_REQUIRE(floor > 0.0 && std::isfinite(floor) && std::isfinite(scale), NGAN_ERR_ARG,
                 "specloss_head: floor=%g must be positive and finite, scale=%g finite", floor, scale);
    NGAN_REQUIRE(((uintptr_t)radial | (uintptr_t)target | (uintptr_t)ring_norm | (uintptr_t)per_image) % 8 == 0 &&
                     ((uintptr_t)loss | (uintptr_t)dradial | (uintptr_t)coef | (uintptr_t)skipped) % 4 == 0,
                 NGAN_ERR_ARG, "specloss_head: fp64 arrays must start on an 8-byte boundary, fp32 and int ones on a 4-byte one");
    hipLaunchKernelGGL(head_kernel, dim3(1), dim3(HT), 0, (hipStream_t)stream, radial, target, ring_norm, B, R, scale, floor, per_image, loss,
                       dradial, coef, skipped);
    return ngan::launch_status("ngan_specloss_head");
}

extern "C" int ngan_specloss_bwd(const float* transform, const float* coef, const float* upstream, const float* addend_or_null,
                                 float* grad, void* workspace, int B, int R, int C, int window, void* stream) {
    NGAN_REQUIRE(transform && coef && upstream && grad, NGAN_ERR_ARG, "specloss_bwd: null pointer");
    NGAN_REQUIRE(workspace, NGAN_ERR_ARG, "specloss_bwd: null workspace (ngan_specloss_bwd_workspace_bytes names its size)");
    if (!shape_ok("specloss_bwd", B, R, C)) return NGAN_ERR_SHAPE;
    NGAN_REQUIRE(((uintptr_t)transform | (uintptr_t)workspace | (uintptr_t)grad | (uintptr_t)addend_or_null) % 16 == 0 &&
                     ((uintptr_t)coef | (uintptr_t)upstream) % 4 == 0,
                 NGAN_ERR_ARG, "specloss_bwd: transform, addend, grad and workspace must start on a 16-byte boundary, coef and upstream on a 4-byte one");
    hipStream_t s = (hipStream_t)stream;
    const float2* F = reinterpret_cast<const float2*>(transform);
    switch (R) {
        case 16: launch_bwd<16>(F, coef, upstream, addend_or_null, grad, workspace, B, window != 0, s); break;
        case 32: launch_bwd<32>(F, coef, upstream, addend_or_null, grad, workspace, B, window != 0, s); break;
        case 64: launch_bwd<64>(F, coef, upstream, addend_or_null, grad, workspace, B, window != 0, s); break;
        case 128: launch_bwd<128>(F, coef, upstream, addend_or_null, grad, workspace, B, window != 0, s); break;
        case 256: launch_bwd<256>(F, coef, upstream, addend_or_null, grad, workspace, B, window != 0, s); break;
        case 512: launch_bwd<512>(F, coef, upstream, addend_or_null, grad, workspace, B, window != 0, s); break;
        default: launch_bwd<1024>(F, coef, upstream, addend_or_null, grad, workspace, B, window != 0, s); break;
    }
    return ngan::launch_status("ngan_specloss_bwd");
}
