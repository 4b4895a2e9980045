// The WGAN nets' layers (reference models.py:728-790): 4x4 stride-2 pad-1 convolutions, plain ("down", Conv2d) and transposed ("up",
// ConvTranspose2d), on channels-last fp32 tensors as implicit GEMMs on v_mfma_f32_16x16x4_f32 (exact fp32 MFMA, gfx950), plus the
// training-mode BatchNorm2d that sits between them, the biased stem Linear of Generator_wgan and the per-channel reductions.
//
// One family covers all six convolution passes because the two convolutions are adjoints of each other:
//   down(x, W)  out[b,oy,ox,m] = sum_{ky,kx,c} W[m][c][ky][kx] * x[b, 2oy-1+ky, 2ox-1+kx, c]
//   up(x, W)    out[b,oy,ox,m] = sum over the 2x2 taps of its parity of W[c][m][ky][kx] * x[b, iy, ix, c],  oy + 1 = 2 iy + ky
// The input gradient of down with W is up with W and vice versa (the weight tensor is read in its torch layout either way).  One
// weight-gradient kernel correlates a half-size and a full-size tensor:
//   wgrad       dW[h][f][ky][kx] = sum_{b,i,j} half[b,i,j,h] * full[b, 2i-1+ky, 2j-1+kx, f]
// which is Conv2d's (half = output gradient, full = input) and ConvTranspose2d's (half = input, full = output gradient) alike.
//
// BatchNorm-on-load: every input of these kernels can carry a per-channel transform applied while it is read,
//   v -> act(scale[c] * v + shift[c]),  act = identity or LeakyReLU(slope),
// so a BatchNorm2d -> LeakyReLU between two convolutions never writes its output: the consumer reads the producer's raw output.
// Training-mode BatchNorm folds its batch statistics into (scale, shift) = (gamma * rstd, beta - mean * gamma * rstd) (ngan_bn_stats),
// eval mode folds the running statistics the same way (ngan_bn_fold_eval).  Zero padding is applied AFTER the transform, as in the
// reference, where the convolution pads the activated tensor.
//
// Every reduction is two-stage with fixed partition and fixed order: no float atomics, so graph replay is bit-equal to eager.
#include "ngan_common.h"

namespace {

struct Xform {            // per-channel input transform applied on load
    const float* scale;   // nullptr: no affine part
    const float* shift;
    int act;              // 1: LeakyReLU after the affine part
    float slope;
};

__device__ __forceinline__ float xf(const Xform& t, float v, int c) {
    if (t.scale) v = fmaf(t.scale[c], v, t.shift[c]);
    if (t.act) v = v > 0.f ? v : t.slope * v;
    return v;
}
__device__ __forceinline__ float4 xf4(const Xform& t, float4 v, int c) {
    return make_float4(xf(t, v.x, c), xf(t, v.y, c + 1), xf(t, v.z, c + 2), xf(t, v.w, c + 3));
}

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }

// ---------------------------------------------------------------------------------------------------------------------------------
// weight packing: Wp[tap = ky*4+kx][m][c], m padded to a multiple of 64 (MP), c to a multiple of 16 (CP), zero filled.
//   up == 0: A(m, c) = W[m][c][ky][kx]  (W is d0 x d1 = M x C)      up == 1: A(m, c) = W[c][m][ky][kx]  (W is d0 x d1 = C x M)
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void s2_pack_kernel(const float* __restrict__ W, float* __restrict__ Wp, int M, int C, int MP, int CP,
                                                      int up) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = 16L * MP * CP;
    if (i >= n) return;
    const int c = (int)(i % CP);
    const int m = (int)((i / CP) % MP);
    const int tap = (int)(i / ((long)CP * MP));
    float v = 0.f;
    if (m < M && c < C) v = up ? W[((long)c * M + m) * 16 + tap] : W[((long)m * C + c) * 16 + tap];
    Wp[i] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// forward kernel (down / up).  256 threads = 4 waves; a wave owns 16 output pixels x MT*16 output channels; the contraction runs over
// (tap, 16-channel group), four MFMAs per group with the k-order inside a group permuted identically on both operands (lane q holds
// channels 4q..4q+3 of its pixel and of its weight row).  VEC: C % 4 == 0 (one float4 per lane per group); otherwise scalar loads
// with a channel mask (the 1- and 3-channel image ends).
//   down: pixels n = (b, oy, ox) of the half-size output, 16 taps.
//   up:   blockIdx.z = output parity (py, px); pixels n = (b, hy, hx) enumerate that parity's quarter of the output, 4 taps.
// Epilogue: + bias, optional tanh, channel-masked store.
// ---------------------------------------------------------------------------------------------------------------------------------
struct S2Args {
    const float* x; const float* wp; const float* bias; float* y;
    Xform t;
    int B, Hin, Win, C, M, MP, CP;
    int Hq, Wq;           // pixel grid the kernel enumerates: down = output size, up = input size (one parity)
    int tanh_out;
};

template <int UP, int MT, bool VEC>
__global__ __launch_bounds__(256) void s2_conv_kernel(S2Args a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = lane & 15, q = lane >> 4;
    const long npix = (long)a.B * a.Hq * a.Wq;
    const long n = ((long)blockIdx.x * 4 + wave) * 16 + p;     // this lane's pixel (B operand column / output column)
    const int m0 = blockIdx.y * (MT * 16);
    const int py = UP ? (int)(blockIdx.z >> 1) : 0, px = UP ? (int)(blockIdx.z & 1) : 0;
    const bool nvalid = n < npix;
    int b = 0, qy = 0, qx = 0;
    if (nvalid) {
        qx = (int)(n % a.Wq);
        const long r = n / a.Wq;
        qy = (int)(r % a.Hq);
        b = (int)(r / a.Hq);
    }
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    constexpr int NT = UP ? 4 : 16;
    for (int t = 0; t < NT; ++t) {
        int ky, kx, iy, ix;
        if (UP) {
            const int ty = t >> 1, tx = t & 1;
            ky = (1 - py) + 2 * ty; kx = (1 - px) + 2 * tx;
            iy = qy + py - ty; ix = qx + px - tx;
        } else {
            ky = t >> 2; kx = t & 3;
            iy = 2 * qy - 1 + ky; ix = 2 * qx - 1 + kx;
        }
        const bool inb = nvalid && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
        const float* xrow = a.x + (((long)b * a.Hin + (inb ? iy : 0)) * a.Win + (inb ? ix : 0)) * a.C;
        const float* wrow = a.wp + ((long)(ky * 4 + kx) * a.MP + m0 + p) * a.CP;
        for (int c0 = 0; c0 < a.C; c0 += 16) {
            const int c = c0 + 4 * q;
            float xv[4];
            if (VEC) {
                float4 v = f4zero();
                if (inb && c < a.C) v = xf4(a.t, ld4(xrow + c), c);
                xv[0] = v.x; xv[1] = v.y; xv[2] = v.z; xv[3] = v.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) xv[i] = (inb && c + i < a.C) ? xf(a.t, xrow[c + i], c + i) : 0.f;
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const float4 w4 = ld4(wrow + (long)mt * 16 * a.CP + c);     // c < CP always (CP = C rounded up to 16)
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.x, xv[0], acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.y, xv[1], acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.z, xv[2], acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.w, xv[3], acc[mt], 0, 0, 0);
            }
        }
    }
    if (!nvalid) return;
    long opix;
    if (UP) {
        const int Wo = 2 * a.Win;
        opix = ((long)b * 2 * a.Hin + 2 * qy + py) * Wo + 2 * qx + px;
    } else {
        opix = ((long)b * a.Hq + qy) * a.Wq + qx;
    }
    float* o = a.y + opix * a.M;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int mb = m0 + mt * 16 + 4 * q;     // lane holds output channels mb..mb+3 of pixel n
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = mb + r;
            if (m < a.M) {
                float v = acc[mt][r] + (a.bias ? a.bias[m] : 0.f);
                if (a.tanh_out) v = tanhf(v);
                o[m] = v;
            }
        }
    }
}

template <int UP, int MT>
int launch_s2(const S2Args& a, hipStream_t s) {
    const long npix = (long)a.B * a.Hq * a.Wq;
    dim3 grid(ngan::ceil_div(npix, 64), ngan::ceil_div(a.M, MT * 16), UP ? 4 : 1);
    if (a.C % 4 == 0) hipLaunchKernelGGL((s2_conv_kernel<UP, MT, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((s2_conv_kernel<UP, MT, false>), grid, dim3(256), 0, s, a);
    return ngan::launch_status(UP ? "ngan_s2_conv(up)" : "ngan_s2_conv(down)");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// weight gradient: one wave per (16 h-rows, 16 f-columns, k-split) work item, all 16 taps: acc[tap] += half^T * shifted full.
// Lane (p, q): A = half[pix_k][h0 + p], B = full[pix_k + tap offset][f0 + p], pix_k = k0 + q.  Partials per split go to `work`
// [split][HP][FP][16]; s2_wgrad_reduce sums the splits in order and writes dW[h][f][tap] for h < H, f < F.
// ---------------------------------------------------------------------------------------------------------------------------------
struct WgArgs {
    const float* half; const float* full; float* work;
    Xform th, tf;
    int B, Hh, Wh, CH, CF, HB, FB, nsplit;
    long kper;
};

__global__ __launch_bounds__(256) void s2_wgrad_kernel(WgArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = lane & 15, q = lane >> 4;
    const long item = (long)blockIdx.x * 4 + wave;
    const long nitems = (long)a.HB * a.FB * a.nsplit;
    if (item >= nitems) return;
    const int split = (int)(item % a.nsplit);
    const int fb = (int)((item / a.nsplit) % a.FB);
    const int hb = (int)(item / ((long)a.nsplit * a.FB));
    const int h = hb * 16 + p, f = fb * 16 + p;
    const bool hv = h < a.CH, fv = f < a.CF;
    const long K = (long)a.B * a.Hh * a.Wh;
    const long k_begin = split * a.kper;
    const long k_end = min(K, k_begin + a.kper);
    const int Hf = 2 * a.Hh, Wf = 2 * a.Wh;
    f32x4 acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (long k0 = k_begin; k0 < k_end; k0 += 4) {
        const long k = k0 + q;
        const bool kv = k < k_end;
        int i = 0, j = 0, b = 0;
        if (kv) {
            j = (int)(k % a.Wh);
            const long r = k / a.Wh;
            i = (int)(r % a.Hh);
            b = (int)(r / a.Hh);
        }
        const float av = (kv && hv) ? xf(a.th, a.half[k * a.CH + h], h) : 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int yy = 2 * i - 1 + (t >> 2), xx = 2 * j - 1 + (t & 3);
            const bool ok = kv && fv && yy >= 0 && yy < Hf && xx >= 0 && xx < Wf;
            const float bv = ok ? xf(a.tf, a.full[(((long)b * Hf + yy) * Wf + xx) * a.CF + f], f) : 0.f;
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
        }
    }
    // lane (p, q) holds rows h = hb*16 + 4q + r, column f = fb*16 + p
    const int HP = a.HB * 16, FP = a.FB * 16;
    float* w = a.work + (long)split * HP * FP * 16;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int hh = hb * 16 + 4 * q + r;
        float* o = w + ((long)hh * FP + f) * 16;
#pragma unroll
        for (int t = 0; t < 16; t += 4) st4(o + t, make_float4(acc[t][r], acc[t + 1][r], acc[t + 2][r], acc[t + 3][r]));
    }
}

__global__ __launch_bounds__(256) void s2_wgrad_reduce(const float* __restrict__ work, float* __restrict__ dW, int CH, int CF, int HP, int FP,
                                                       int nsplit) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = (long)CH * CF * 16;
    if (i >= n) return;
    const int t = (int)(i & 15);
    const int f = (int)((i >> 4) % CF);
    const int h = (int)((i >> 4) / CF);
    const long off = ((long)h * FP + f) * 16 + t;
    const long stride = (long)HP * FP * 16;
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += work[k * stride + off];
    dW[i] = s;
}

void wgrad_plan(int B, int Hh, int Wh, int CH, int CF, int& HB, int& FB, int& nsplit, long& kper) {
    HB = ngan::ceil_div(CH, 16);
    FB = ngan::ceil_div(CF, 16);
    const long K = (long)B * Hh * Wh;
    const long tiles = (long)HB * FB;
    // >= ~4096 waves in flight, and at least 128 pixels per split (amortise the partial store), at most 1024 splits
    long want = (4096 + tiles - 1) / tiles;
    long most = (K + 127) / 128;
    long ns = want < most ? want : most;
    if (ns > 1024) ns = 1024;
    if (ns < 1) ns = 1;
    kper = (K + ns - 1) / ns;
    kper = (kper + 3) / 4 * 4;
    nsplit = (int)((K + kper - 1) / kper);
    if (nsplit < 1) nsplit = 1;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// per-channel reductions over an (npix, C) channels-last tensor, in two fixed-order stages.
// Stage 1: workgroup g sums pixels [g*chunk, (g+1)*chunk); thread tid owns one channel and one pixel lane (see the kernel).
//   (the BN moments, s0 = sum (y - y[0,c]) and s1 = sum (y - y[0,c])^2, have a stage 1 of their own in fp64: bn_stats_stage1)
//   mode 1 (BN backward):     gz = g * act'(z),  z = scale*y + shift;  s0 = sum gz,  s1 = sum gz * xhat,  xhat = (y - mean) * rstd
//   mode 2 (plain sum):       s0 = sum g
// Partials: part[g][2][C].  Stage 2 (one thread per channel) sums the chunks in order.
// ---------------------------------------------------------------------------------------------------------------------------------
struct RedArgs {
    const float* y; const float* g;
    const float* scale; const float* shift; const float* mean; const float* rstd;
    float slope; int act;
    long npix; int C; long chunk;
    float* part;
};

template <int MODE>
__global__ __launch_bounds__(256) void chan_reduce_stage1(RedArgs a) {
    __shared__ float sm[2][256];
    const int tid = threadIdx.x;
    // thread layout: C <= 256: L = floor(256 / C) pixel lanes per channel (threads tid >= L*C idle); C > 256: one lane, channels
    // strided by 256
    const bool split = a.C <= 256;
    const int L = split ? 256 / a.C : 1;
    const int CW = split ? a.C : 256;           // channels per pass
    const long p0 = (long)blockIdx.x * a.chunk;
    const long p1 = min(a.npix, p0 + a.chunk);
    for (int cbase = 0; cbase < a.C; cbase += CW) {
        const int c = split ? tid % a.C : cbase + tid;
        const int lane = split ? tid / a.C : 0;
        float s0 = 0.f, s1 = 0.f;
        if (c < a.C && lane < L) {
            const float sc = (MODE == 1 && a.scale) ? a.scale[c] : 1.f, sh = (MODE == 1 && a.scale) ? a.shift[c] : 0.f;
            const float mu = (MODE == 1 && a.mean) ? a.mean[c] : 0.f, rs = (MODE == 1 && a.rstd) ? a.rstd[c] : 1.f;
            for (long pix = p0 + lane; pix < p1; pix += L) {
                const long i = pix * a.C + c;
                if (MODE == 1) {
                    const float yv = a.y[i];
                    const float z = fmaf(sc, yv, sh);
                    float gz = a.g[i];
                    if (a.act && !(z > 0.f)) gz *= a.slope;
                    s0 += gz;
                    s1 = fmaf(gz, (yv - mu) * rs, s1);
                } else {
                    s0 += a.g[i];
                }
            }
        }
        sm[0][tid] = s0;
        sm[1][tid] = s1;
        __syncthreads();
        if (tid < CW && cbase + tid < a.C) {
            float t0 = 0.f, t1 = 0.f;
            for (int l = 0; l < L; ++l) {       // the lanes of channel tid: threads tid + l*C (split) / just tid; l*C + tid < 256
                t0 += sm[0][tid + l * (split ? a.C : 0)];
                t1 += sm[1][tid + l * (split ? a.C : 0)];
            }
            const int cc = split ? tid : cbase + tid;
            a.part[((long)blockIdx.x * 2 + 0) * a.C + cc] = t0;
            a.part[((long)blockIdx.x * 2 + 1) * a.C + cc] = t1;
        }
        __syncthreads();
    }
}

// BN statistics, stage 1: chan_reduce_stage1's partition and order; fp32 sums of d = y - y[0,c] and d^2 (part32[g][2][C]: the one-pass
// fp32 form the single-GPU path had before, bit for bit), and beside them the same two sums in fp64 (part[g][2][C] doubles).  The variance is
// s1/n - (s0/n)^2, which cancels by a factor 1 + 2 (s0/n)^2 / var: in fp32 a first pixel six sigma from its channel's mean costs 73
// roundings' worth of the variance, in fp64 nothing that an fp32 result can show.  bn_stats_finish keeps the fp32 moments where the
// fp64 ones confirm them and takes the fp64 ones elsewhere.  F32 = false (ngan_bn_moments, the synchronised path: its record is fp64
// and nothing downstream reads an fp32 moment) leaves the fp32 sums out.
template <bool F32>
__global__ __launch_bounds__(256) void bn_stats_stage1(RedArgs a, double* __restrict__ part) {
    __shared__ double sm[2][256];
    __shared__ float sm32[2][F32 ? 256 : 1];
    const int tid = threadIdx.x;
    const bool split = a.C <= 256;
    const int L = split ? 256 / a.C : 1;
    const int CW = split ? a.C : 256;
    const long p0 = (long)blockIdx.x * a.chunk;
    const long p1 = min(a.npix, p0 + a.chunk);
    for (int cbase = 0; cbase < a.C; cbase += CW) {
        const int c = split ? tid % a.C : cbase + tid;
        const int lane = split ? tid / a.C : 0;
        double s0 = 0.0, s1 = 0.0;
        float f0 = 0.f, f1 = 0.f;
        if (c < a.C && lane < L) {
            const float piv = a.y[c];
            for (long pix = p0 + lane; pix < p1; pix += L) {
                const float yv = a.y[pix * a.C + c];
                if (F32) {
                    const float df = yv - piv;
                    f0 += df;
                    f1 = fmaf(df, df, f1);
                }
                const double d = (double)yv - (double)piv;
                s0 += d;
                s1 = fma(d, d, s1);
            }
        }
        sm[0][tid] = s0;
        sm[1][tid] = s1;
        if (F32) {
            sm32[0][tid] = f0;
            sm32[1][tid] = f1;
        }
        __syncthreads();
        if (tid < CW && cbase + tid < a.C) {
            double t0 = 0.0, t1 = 0.0;
            float u0 = 0.f, u1 = 0.f;
            for (int l = 0; l < L; ++l) {       // l*C + tid < 256, as in chan_reduce_stage1
                const int j = tid + l * (split ? a.C : 0);
                t0 += sm[0][j];
                t1 += sm[1][j];
                if (F32) {
                    u0 += sm32[0][j];
                    u1 += sm32[1][j];
                }
            }
            const int cc = split ? tid : cbase + tid;
            part[((long)blockIdx.x * 2 + 0) * a.C + cc] = t0;
            part[((long)blockIdx.x * 2 + 1) * a.C + cc] = t1;
            if (F32) {
                a.part[((long)blockIdx.x * 2 + 0) * a.C + cc] = u0;
                a.part[((long)blockIdx.x * 2 + 1) * a.C + cc] = u1;
            }
        }
        __syncthreads();
    }
}

// BN statistics finish: mean, rstd (biased variance), (scale, shift), running-statistics update (unbiased variance, momentum),
// num_batches_tracked += 1 (channel 0's thread).  The chunks are summed in order, in fp32 and in fp64.  The fp32 moments stand where
// they agree with the fp64 ones (the variance within 2^-22 of it, the mean within 2^-23 of |mean| + sigma), which is everywhere the
// first pixel is an ordinary one: there the results are, bit for bit, those of the one-pass fp32 form.  Elsewhere the fp64 moments,
// rounded once, take their place.  Everything after the moments is fp32.
__global__ void bn_stats_finish(const double* __restrict__ part, const float* __restrict__ part32, int nparts, const float* __restrict__ y,
                                long npix, int C, const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ mean,
                                float* __restrict__ rstd, float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ run_mean,
                                float* __restrict__ run_var, long long* __restrict__ nbt, float momentum, float eps) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
    float f0 = 0.f, f1 = 0.f;
    for (int k = 0; k < nparts; ++k) {
        s0 += part[((long)k * 2 + 0) * C + c];
        s1 += part[((long)k * 2 + 1) * C + c];
        f0 += part32[((long)k * 2 + 0) * C + c];
        f1 += part32[((long)k * 2 + 1) * C + c];
    }
    const double nd = (double)npix;
    const double dd = s0 / nd;
    const double var64 = fmax(s1 / nd - dd * dd, 0.0);
    const double mu64 = (double)y[c] + dd;
    const float n = (float)npix;
    const float d32 = f0 / n;
    const float var32 = fmaxf(f1 / n - d32 * d32, 0.f);
    const float mu32 = y[c] + d32;
    const float var = fabs((double)var32 - var64) <= 0x1p-22 * var64 ? var32 : (float)var64;
    const float mu = fabs((double)mu32 - mu64) <= 0x1p-23 * (fabs(mu64) + sqrt(var64)) ? mu32 : (float)mu64;
    const float r = 1.0f / sqrtf(var + eps);
    mean[c] = mu;
    rstd[c] = r;
    const float gs = gamma[c] * r;
    scale[c] = gs;
    shift[c] = beta[c] - mu * gs;
    if (run_mean) {
        const float unb = npix > 1 ? var * (n / (n - 1.0f)) : var;
        run_mean[c] = (1.0f - momentum) * run_mean[c] + momentum * mu;
        run_var[c] = (1.0f - momentum) * run_var[c] + momentum * unb;
    }
    if (nbt && c == 0) nbt[0] += 1;
}

__global__ void bn_fold_eval_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ run_mean,
                                    const float* __restrict__ run_var, float eps, float* __restrict__ scale, float* __restrict__ shift, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float gs = gamma[c] / sqrtf(run_var[c] + eps);
    scale[c] = gs;
    shift[c] = beta[c] - run_mean[c] * gs;
}

// BN backward finish: sums -> dgamma = sum gz*xhat, dbeta = sum gz (written when the pointers are non-null), and the per-channel
// coefficients of the input gradient  gy = k1*gz + k2 + k3*y  with  k1 = gamma*rstd,  k2 = -k1*(s0 - mean*rstd*s1... ) (below)
__global__ void bn_bwd_finish(const float* __restrict__ part, int nparts, long npix, int C, const float* __restrict__ gamma,
                              const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ dgamma,
                              float* __restrict__ dbeta, float* __restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float s0 = 0.f, s1 = 0.f;
    for (int k = 0; k < nparts; ++k) {
        s0 += part[((long)k * 2 + 0) * C + c];
        s1 += part[((long)k * 2 + 1) * C + c];
    }
    if (dgamma) dgamma[c] = s1;
    if (dbeta) dbeta[c] = s0;
    // gy = gamma*rstd * (gz - s0/n - xhat * s1/n),  xhat = (y - mean)*rstd
    const float n = (float)npix;
    const float k1 = gamma[c] * rstd[c];
    const float m0 = s0 / n, m1 = s1 / n;
    coef[c] = k1;
    coef[C + c] = m0;
    coef[2 * C + c] = m1;
}

__global__ __launch_bounds__(256) void chan_sum_finish(const float* __restrict__ part, int nparts, int C, float* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float s0 = 0.f;
    for (int k = 0; k < nparts; ++k) s0 += part[(long)k * 2 * C + c];
    out[c] = s0;
}

// elementwise input gradient of (BatchNorm ->) activation: gy = act'(z) * g  [* BN terms]
__global__ __launch_bounds__(256) void bn_act_bwd_apply(const float* __restrict__ y, const float* __restrict__ g, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, const float* __restrict__ coef, int act, float slope,
                                                        long n, int C, float* __restrict__ gy) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const float yv = y[i];
    const float z = scale ? fmaf(scale[c], yv, shift[c]) : yv;
    float gz = g[i];
    if (act && !(z > 0.f)) gz *= slope;
    if (coef) {
        const float xh = (yv - mean[c]) * rstd[c];
        gz = coef[c] * (gz - coef[C + c] - xh * coef[2 * C + c]);
    }
    gy[i] = gz;
}

__global__ __launch_bounds__(256) void bn_act_apply_kernel(const float* __restrict__ y, const float* __restrict__ scale, const float* __restrict__ shift,
                                                           int act, float slope, long n, int C, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    Xform t{scale, shift, act, slope};
    out[i] = xf(t, y[i], c);
}

__global__ __launch_bounds__(256) void tanh_bwd_kernel(const float* __restrict__ t, const float* __restrict__ g, float* __restrict__ o, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float tv = t[i];
    o[i] = g[i] * (1.0f - tv * tv);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// stem Linear of Generator_wgan with its outputs permuted from NCHW to NHWC order:  y[b][p][c] = bias[c*S+p] + sum_k z[b][k] W[c*S+p][k]
// one wave per output feature row n = c*S+p, lanes over k, a butterfly sum per batch row (B <= 64 rows at a time)
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void stem_fwd_kernel(const float* __restrict__ z, const float* __restrict__ W, const float* __restrict__ bias,
                                                       float* __restrict__ y, int B, int K, int S, int C) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)S * C) return;
    const int c = (int)(row / S), p = (int)(row % S);
    const float* w = W + row * K;
    for (int b = 0; b < B; ++b) {
        float s = 0.f;
        for (int k = lane; k < K; k += 64) s = fmaf(z[(long)b * K + k], w[k], s);
        s = group_sum<64>(s);
        if (lane == 0) y[((long)b * S + p) * C + c] = s + bias[row];
    }
}

// gW[c*S+p][k] = sum_b g[b][p][c] z[b][k];  gb[c*S+p] = sum_b g[b][p][c]
__global__ __launch_bounds__(256) void stem_grad_kernel(const float* __restrict__ z, const float* __restrict__ g, float* __restrict__ gW,
                                                        float* __restrict__ gb, int B, int K, int S, int C) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = (long)S * C * K;
    if (i >= n) return;
    const int k = (int)(i % K);
    const long row = i / K;
    const int c = (int)(row / S), p = (int)(row % S);
    float s = 0.f, sb = 0.f;
    for (int b = 0; b < B; ++b) {
        const float gv = g[((long)b * S + p) * C + c];
        s = fmaf(gv, z[(long)b * K + k], s);
        sb += gv;
    }
    if (gW) gW[i] = s;
    if (gb && k == 0) gb[row] = sb;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// synchronised BatchNorm (data parallel): per-rank records in fp64 that are all-gathered and merged in rank order.
//   moments record  [count, mean[C], M2[C]]     (M2 = sum of squared deviations from the record's own mean)
//   backward record [S0[C], S1[C]]               (S0 = sum gz, S1 = sum gz * xhat, xhat from the GLOBAL statistics)
// The moments' stage-1 partials are fp64 (bn_stats_stage1<false>: the sums about the rank's first pixel cancel in M2 = s1 - s0 d, and
// fp32 partials lost tens of roundings of rstd to an outlying first pixel); the backward's are the fp32 ones of chan_reduce_stage1<1>,
// as on the single-GPU path.  sum_parts_f64 adds either kind in fp64 with a block of 16 channels x 16 lanes (lane l takes the partials
// l, l + 16, ... in order, then the channel's thread adds the 16 lane sums in order).
// ---------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ bool sum_parts_f64(const T* __restrict__ part, int nparts, int C, double& s0, double& s1, int& c) {
    __shared__ double sm[2][256];
    const int t = threadIdx.x;
    const int cc = blockIdx.x * 16 + (t & 15), lane = t >> 4;
    double a0 = 0.0, a1 = 0.0;
    if (cc < C) {
        for (int k = lane; k < nparts; k += 16) {
            a0 += (double)part[((long)k * 2 + 0) * C + cc];
            a1 += (double)part[((long)k * 2 + 1) * C + cc];
        }
    }
    sm[0][t] = a0;
    sm[1][t] = a1;
    __syncthreads();
    c = cc;
    if (t >= 16 || cc >= C) return false;
    s0 = 0.0;
    s1 = 0.0;
    for (int l = 0; l < 16; ++l) {
        s0 += sm[0][l * 16 + t];
        s1 += sm[1][l * 16 + t];
    }
    return true;
}

// shifted sums (pivot y[0, c]) -> this rank's moments record
__global__ __launch_bounds__(256) void bn_moments_finish(const double* __restrict__ part, int nparts, const float* __restrict__ y, long npix,
                                                         int C, double* __restrict__ rec) {
    if (blockIdx.x == 0 && threadIdx.x == 0) rec[0] = (double)npix;
    double s0, s1;
    int c;
    if (!sum_parts_f64(part, nparts, C, s0, s1, c)) return;
    const double d = s0 / (double)npix;
    rec[1 + c] = (double)y[c] + d;
    rec[1 + C + c] = fmax(s1 - s0 * d, 0.0);
}

// merge of the gathered moments records in rank order (Chan et al.), then what bn_stats_finish writes, plus the global count
__global__ __launch_bounds__(256) void bn_merge_fold_kernel(const double* __restrict__ recs, int world, int C, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ mean, float* __restrict__ rstd,
                                                            float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ run_mean,
                                                            float* __restrict__ run_var, long long* __restrict__ nbt, float momentum, float eps,
                                                            double* __restrict__ n_total) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const long R = 1 + 2L * C;
    double n = recs[0], mu = recs[1 + c], m2 = recs[1 + C + c];
    for (int r = 1; r < world; ++r) {
        const double* q = recs + r * R;
        const double nb = q[0];
        const double nn = n + nb;
        const double d = q[1 + c] - mu;
        mu += d * (nb / nn);
        m2 += q[1 + C + c] + d * d * (n * nb / nn);
        n = nn;
    }
    const double var = m2 / n;
    const float r = (float)(1.0 / sqrt(var + (double)eps));
    const float muf = (float)mu;
    mean[c] = muf;
    rstd[c] = r;
    const float gs = gamma[c] * r;
    scale[c] = gs;
    shift[c] = beta[c] - muf * gs;
    if (run_mean) {
        const double unb = n > 1.0 ? m2 / (n - 1.0) : var;
        run_mean[c] = (float)((1.0 - (double)momentum) * run_mean[c] + (double)momentum * mu);
        run_var[c] = (float)((1.0 - (double)momentum) * run_var[c] + (double)momentum * unb);
    }
    if (c == 0) {
        n_total[0] = n;
        if (nbt) nbt[0] += 1;
    }
}

// sum gz, sum gz * xhat over this rank's pixels -> its backward record
__global__ __launch_bounds__(256) void bn_bwd_partial_finish(const float* __restrict__ part, int nparts, int C, double* __restrict__ rec) {
    double s0, s1;
    int c;
    if (!sum_parts_f64(part, nparts, C, s0, s1, c)) return;
    rec[c] = s0;
    rec[C + c] = s1;
}

// the gathered backward records summed in rank order -> the coefficients of bn_act_bwd_apply over the global count; dgamma / dbeta are
// THIS rank's share (the flat gradient all-reduce adds the ranks' shares)
__global__ __launch_bounds__(256) void bn_bwd_merged_finish(const double* __restrict__ recs, int world, int rank, int C,
                                                            const double* __restrict__ n_total, const float* __restrict__ gamma,
                                                            const float* __restrict__ rstd, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, float* __restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0, s1 = 0.0;
    for (int r = 0; r < world; ++r) {
        s0 += recs[(long)r * 2 * C + c];
        s1 += recs[(long)r * 2 * C + C + c];
    }
    const double* own = recs + (long)rank * 2 * C;
    if (dgamma) dgamma[c] = (float)own[C + c];
    if (dbeta) dbeta[c] = (float)own[c];
    const double n = n_total[0];
    coef[c] = gamma[c] * rstd[c];
    coef[C + c] = (float)(s0 / n);
    coef[2 * C + c] = (float)(s1 / n);
}

long red_chunk(long npix, int C, int& nparts) {
    // about 16K elements per workgroup, at most 1024 workgroups
    long chunk = (16384 + C - 1) / C;
    if (chunk < 1) chunk = 1;
    long np = (npix + chunk - 1) / chunk;
    if (np > 1024) {
        chunk = (npix + 1023) / 1024;
        np = (npix + chunk - 1) / chunk;
    }
    nparts = (int)np;
    return chunk;
}

}  // namespace

extern "C" {

long ngan_s2_packed_floats(int M, int C) { return 16L * round_up(M, 64) * round_up(C, 16); }

int ngan_s2_pack(const float* W, float* Wp, int M, int C, int up, void* stream) {
    NGAN_REQUIRE(W && Wp, NGAN_ERR_ARG, "s2_pack: null pointer");
    NGAN_REQUIRE(M > 0 && C > 0, NGAN_ERR_SHAPE, "s2_pack: M=%d C=%d", M, C);
    const long n = ngan_s2_packed_floats(M, C);
    hipLaunchKernelGGL(s2_pack_kernel, dim3(ngan::ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, W, Wp, M, C, round_up(M, 64),
                       round_up(C, 16), up);
    return ngan::launch_status("ngan_s2_pack");
}

int ngan_s2_conv(const float* x, const float* Wp, const float* bias, const float* in_scale, const float* in_shift, int in_act, float slope,
                 float* y, int B, int Hin, int Win, int C, int M, int up, int tanh_out, void* stream) {
    NGAN_REQUIRE(x && Wp && y, NGAN_ERR_ARG, "s2_conv: null pointer");
    NGAN_REQUIRE((in_scale == nullptr) == (in_shift == nullptr), NGAN_ERR_ARG, "s2_conv: scale and shift go together");
    NGAN_REQUIRE(B > 0 && C > 0 && M > 0 && Hin > 0 && Win > 0, NGAN_ERR_SHAPE, "s2_conv: B=%d H=%d W=%d C=%d M=%d", B, Hin, Win, C, M);
    NGAN_REQUIRE(up || (Hin % 2 == 0 && Win % 2 == 0), NGAN_ERR_SHAPE, "s2_conv(down): input %dx%d is not even", Hin, Win);
    S2Args a{x, Wp, bias, y, Xform{in_scale, in_shift, in_act, slope}, B, Hin, Win, C, M, round_up(M, 64), round_up(C, 16),
             up ? Hin : Hin / 2, up ? Win : Win / 2, tanh_out};
    NGAN_REQUIRE_THREADS("s2_conv", 4L * B * a.Hq * a.Wq);        // one wave per 16 output pixels of a parity: 4 threads per pixel
    hipStream_t s = (hipStream_t)stream;
    const int mt = M > 32 ? 4 : (M > 16 ? 2 : 1);
    if (up) return mt == 4 ? launch_s2<1, 4>(a, s) : mt == 2 ? launch_s2<1, 2>(a, s) : launch_s2<1, 1>(a, s);
    return mt == 4 ? launch_s2<0, 4>(a, s) : mt == 2 ? launch_s2<0, 2>(a, s) : launch_s2<0, 1>(a, s);
}

long ngan_s2_wgrad_workspace_floats(int B, int Hh, int Wh, int CH, int CF) {
    int HB, FB, ns;
    long kper;
    wgrad_plan(B, Hh, Wh, CH, CF, HB, FB, ns, kper);
    return (long)ns * HB * 16 * FB * 16 * 16;
}

int ngan_s2_wgrad(const float* half, const float* full, const float* h_scale, const float* h_shift, int h_act, const float* f_scale,
                  const float* f_shift, int f_act, float slope, float* dW, float* work, int B, int Hh, int Wh, int CH, int CF, void* stream) {
    NGAN_REQUIRE(half && full && dW && work, NGAN_ERR_ARG, "s2_wgrad: null pointer");
    NGAN_REQUIRE(B > 0 && Hh > 0 && Wh > 0 && CH > 0 && CF > 0, NGAN_ERR_SHAPE, "s2_wgrad: B=%d H=%d W=%d CH=%d CF=%d", B, Hh, Wh, CH, CF);
    WgArgs a{half, full, work, Xform{h_scale, h_shift, h_act, slope}, Xform{f_scale, f_shift, f_act, slope}, B, Hh, Wh, CH, CF, 0, 0, 0, 0};
    wgrad_plan(B, Hh, Wh, CH, CF, a.HB, a.FB, a.nsplit, a.kper);
    hipStream_t s = (hipStream_t)stream;
    const long items = (long)a.HB * a.FB * a.nsplit;
    hipLaunchKernelGGL(s2_wgrad_kernel, dim3(ngan::ceil_div(items, 4)), dim3(256), 0, s, a);
    int st = ngan::launch_status("ngan_s2_wgrad");
    if (st) return st;
    const long n = (long)CH * CF * 16;
    hipLaunchKernelGGL(s2_wgrad_reduce, dim3(ngan::ceil_div(n, 256)), dim3(256), 0, s, work, dW, CH, CF, a.HB * 16, a.FB * 16, a.nsplit);
    return ngan::launch_status("ngan_s2_wgrad(reduce)");
}

long ngan_chan_reduce_workspace_floats(long npix, int C) {
    int np;
    red_chunk(npix, C, np);
    return 6L * np * C;      // ngan_bn_stats: part[np][2][C] as doubles, then as floats; ngan_bn_moments: the doubles; the fp32
                             // reductions use the first third
}

int ngan_bn_stats(const float* y, long npix, int C, const float* gamma, const float* beta, float* mean, float* rstd, float* scale,
                  float* shift, float* run_mean, float* run_var, long long* nbt, float momentum, float eps, float* work, void* stream) {
    NGAN_REQUIRE(y && gamma && beta && mean && rstd && scale && shift && work, NGAN_ERR_ARG, "bn_stats: null pointer");
    NGAN_REQUIRE((run_mean == nullptr) == (run_var == nullptr), NGAN_ERR_ARG, "bn_stats: running mean and variance go together");
    NGAN_REQUIRE(npix > 0 && C > 0, NGAN_ERR_SHAPE, "bn_stats: npix=%ld C=%d", npix, C);
    NGAN_REQUIRE(reinterpret_cast<uintptr_t>(work) % sizeof(double) == 0, NGAN_ERR_ARG, "bn_stats: work must be 8-byte aligned");
    int np;
    RedArgs a{y, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0, npix, C, red_chunk(npix, C, np), work};
    hipStream_t s = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(work);       // 2 np C doubles, then the 2 np C floats of the fp32 sums
    a.part = work + 4L * np * C;
    hipLaunchKernelGGL(bn_stats_stage1<true>, dim3(np), dim3(256), 0, s, a, part);
    int st = ngan::launch_status("ngan_bn_stats");
    if (st) return st;
    hipLaunchKernelGGL(bn_stats_finish, dim3(ngan::ceil_div(C, 256)), dim3(256), 0, s, part, a.part, np, y, npix, C, gamma, beta, mean, rstd,
                       scale, shift, run_mean, run_var, nbt, momentum, eps);
    return ngan::launch_status("ngan_bn_stats(finish)");
}

int ngan_bn_fold_eval(const float* gamma, const float* beta, const float* run_mean, const float* run_var, float eps, float* scale,
                      float* shift, int C, void* stream) {
    NGAN_REQUIRE(gamma && beta && run_mean && run_var && scale && shift, NGAN_ERR_ARG, "bn_fold_eval: null pointer");
    NGAN_REQUIRE(C > 0, NGAN_ERR_SHAPE, "bn_fold_eval: C=%d", C);
    hipLaunchKernelGGL(bn_fold_eval_kernel, dim3(ngan::ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, gamma, beta, run_mean, run_var,
                       eps, scale, shift, C);
    return ngan::launch_status("ngan_bn_fold_eval");
}

int ngan_bn_act_bwd(const float* y, const float* g, const float* scale, const float* shift, const float* mean, const float* rstd,
                    const float* gamma, int act, float slope, long npix, int C, float* gy, float* dgamma, float* dbeta, float* work,
                    void* stream) {
    NGAN_REQUIRE(y && g && gy, NGAN_ERR_ARG, "bn_act_bwd: null pointer");
    NGAN_REQUIRE((scale == nullptr) == (shift == nullptr), NGAN_ERR_ARG, "bn_act_bwd: scale and shift go together");
    NGAN_REQUIRE(!gamma || (scale && mean && rstd && work), NGAN_ERR_ARG, "bn_act_bwd: training-mode BatchNorm needs its statistics");
    NGAN_REQUIRE(npix > 0 && C > 0, NGAN_ERR_SHAPE, "bn_act_bwd: npix=%ld C=%d", npix, C);
    NGAN_REQUIRE_THREADS("bn_act_bwd", npix * C);           // the apply pass: one thread per element
    hipStream_t s = (hipStream_t)stream;
    float* coef = nullptr;
    if (gamma) {
        int np;
        RedArgs a{y, g, scale, shift, mean, rstd, slope, act, npix, C, red_chunk(npix, C, np), work};
        hipLaunchKernelGGL(chan_reduce_stage1<1>, dim3(np), dim3(256), 0, s, a);
        int st = ngan::launch_status("ngan_bn_act_bwd(reduce)");
        if (st) return st;
        coef = work + 2L * np * C;      // 3 C floats behind the partials (ngan_bn_act_bwd_workspace_floats)
        hipLaunchKernelGGL(bn_bwd_finish, dim3(ngan::ceil_div(C, 256)), dim3(256), 0, s, work, np, npix, C, gamma, mean, rstd, dgamma, dbeta,
                           coef);
        st = ngan::launch_status("ngan_bn_act_bwd(finish)");
        if (st) return st;
    }
    const long n = npix * C;
    hipLaunchKernelGGL(bn_act_bwd_apply, dim3(ngan::ceil_div(n, 256)), dim3(256), 0, s, y, g, scale, shift, mean, rstd, coef, act, slope, n,
                       C, gy);
    return ngan::launch_status("ngan_bn_act_bwd");
}

long ngan_bn_act_bwd_workspace_floats(long npix, int C) { return ngan_chan_reduce_workspace_floats(npix, C) + 3L * C; }

int ngan_bn_act_apply(const float* y, const float* scale, const float* shift, int act, float slope, long npix, int C, float* out,
                      void* stream) {
    NGAN_REQUIRE(y && out, NGAN_ERR_ARG, "bn_act_apply: null pointer");
    NGAN_REQUIRE((scale == nullptr) == (shift == nullptr), NGAN_ERR_ARG, "bn_act_apply: scale and shift go together");
    const long n = npix * C;
    NGAN_REQUIRE(n > 0, NGAN_ERR_SHAPE, "bn_act_apply: npix=%ld C=%d", npix, C);
    NGAN_REQUIRE_THREADS("bn_act_apply", n);
    hipLaunchKernelGGL(bn_act_apply_kernel, dim3(ngan::ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, y, scale, shift, act, slope, n,
                       C, out);
    return ngan::launch_status("ngan_bn_act_apply");
}

int ngan_chan_sum(const float* g, long npix, int C, float* out, float* work, void* stream) {
    NGAN_REQUIRE(g && out && work, NGAN_ERR_ARG, "chan_sum: null pointer");
    NGAN_REQUIRE(npix > 0 && C > 0, NGAN_ERR_SHAPE, "chan_sum: npix=%ld C=%d", npix, C);
    int np;
    RedArgs a{nullptr, g, nullptr, nullptr, nullptr, nullptr, 0.f, 0, npix, C, red_chunk(npix, C, np), work};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(chan_reduce_stage1<2>, dim3(np), dim3(256), 0, s, a);
    int st = ngan::launch_status("ngan_chan_sum");
    if (st) return st;
    hipLaunchKernelGGL(chan_sum_finish, dim3(ngan::ceil_div(C, 256)), dim3(256), 0, s, work, np, C, out);
    return ngan::launch_status("ngan_chan_sum(finish)");
}

int ngan_tanh_bwd(const float* t, const float* g, float* out, long n, void* stream) {
    NGAN_REQUIRE(t && g && out, NGAN_ERR_ARG, "tanh_bwd: null pointer");
    NGAN_REQUIRE(n > 0, NGAN_ERR_SHAPE, "tanh_bwd: n=%ld", n);
    NGAN_REQUIRE_THREADS("tanh_bwd", n);
    hipLaunchKernelGGL(tanh_bwd_kernel, dim3(ngan::ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, t, g, out, n);
    return ngan::launch_status("ngan_tanh_bwd");
}

int ngan_wgan_stem_fwd(const float* z, const float* W, const float* bias, float* y, int B, int K, int S, int C, void* stream) {
    NGAN_REQUIRE(z && W && bias && y, NGAN_ERR_ARG, "wgan_stem_fwd: null pointer");
    NGAN_REQUIRE(B > 0 && K > 0 && S > 0 && C > 0, NGAN_ERR_SHAPE, "wgan_stem_fwd: B=%d K=%d S=%d C=%d", B, K, S, C);
    hipLaunchKernelGGL(stem_fwd_kernel, dim3(ngan::ceil_div((long)S * C, 4)), dim3(256), 0, (hipStream_t)stream, z, W, bias, y, B, K, S, C);
    return ngan::launch_status("ngan_wgan_stem_fwd");
}

int ngan_wgan_stem_grad(const float* z, const float* g, float* gW, float* gb, int B, int K, int S, int C, void* stream) {
    NGAN_REQUIRE(z && g && (gW || gb), NGAN_ERR_ARG, "wgan_stem_grad: null pointer");
    NGAN_REQUIRE(B > 0 && K > 0 && S > 0 && C > 0, NGAN_ERR_SHAPE, "wgan_stem_grad: B=%d K=%d S=%d C=%d", B, K, S, C);
    const long n = (long)S * C * K;
    hipLaunchKernelGGL(stem_grad_kernel, dim3(ngan::ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, z, g, gW, gb, B, K, S, C);
    return ngan::launch_status("ngan_wgan_stem_grad");
}

int ngan_bn_moments(const float* y, long npix, int C, double* rec, float* work, void* stream) {
    NGAN_REQUIRE(y && rec && work, NGAN_ERR_ARG, "bn_moments: null pointer");
    NGAN_REQUIRE(npix > 0 && C > 0, NGAN_ERR_SHAPE, "bn_moments: npix=%ld C=%d", npix, C);
    NGAN_REQUIRE(reinterpret_cast<uintptr_t>(work) % sizeof(double) == 0, NGAN_ERR_ARG, "bn_moments: work must be 8-byte aligned");
    int np;
    RedArgs a{y, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0, npix, C, red_chunk(npix, C, np), nullptr};
    hipStream_t s = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(work);       // 2 np C doubles, the first two thirds of the workspace
    hipLaunchKernelGGL(bn_stats_stage1<false>, dim3(np), dim3(256), 0, s, a, part);
    int st = ngan::launch_status("ngan_bn_moments");
    if (st) return st;
    hipLaunchKernelGGL(bn_moments_finish, dim3(ngan::ceil_div(C, 16)), dim3(256), 0, s, part, np, y, npix, C, rec);
    return ngan::launch_status("ngan_bn_moments(finish)");
}

int ngan_bn_merge_fold(const double* recs, int world, int C, const float* gamma, const float* beta, float* mean, float* rstd, float* scale,
                       float* shift, float* run_mean, float* run_var, long long* nbt, float momentum, float eps, double* n_total, void* stream) {
    NGAN_REQUIRE(recs && gamma && beta && mean && rstd && scale && shift && n_total, NGAN_ERR_ARG, "bn_merge_fold: null pointer");
    NGAN_REQUIRE((run_mean == nullptr) == (run_var == nullptr), NGAN_ERR_ARG, "bn_merge_fold: running mean and variance go together");
    NGAN_REQUIRE(world >= 1 && C > 0, NGAN_ERR_SHAPE, "bn_merge_fold: world=%d C=%d", world, C);
    hipLaunchKernelGGL(bn_merge_fold_kernel, dim3(ngan::ceil_div(C, 256)), dim3(256), 0, (hipStream_t)stream, recs, world, C, gamma, beta,
                       mean, rstd, scale, shift, run_mean, run_var, nbt, momentum, eps, n_total);
    return ngan::launch_status("ngan_bn_merge_fold");
}

int ngan_bn_act_bwd_partial(const float* y, const float* g, const float* scale, const float* shift, const float* mean, const float* rstd,
                            int act, float slope, long npix, int C, double* rec, float* work, void* stream) {
    NGAN_REQUIRE(y && g && scale && shift && mean && rstd && rec && work, NGAN_ERR_ARG, "bn_act_bwd_partial: null pointer");
    NGAN_REQUIRE(npix > 0 && C > 0, NGAN_ERR_SHAPE, "bn_act_bwd_partial: npix=%ld C=%d", npix, C);
    int np;
    RedArgs a{y, g, scale, shift, mean, rstd, slope, act, npix, C, red_chunk(npix, C, np), work};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(chan_reduce_stage1<1>, dim3(np), dim3(256), 0, s, a);
    int st = ngan::launch_status("ngan_bn_act_bwd_partial");
    if (st) return st;
    hipLaunchKernelGGL(bn_bwd_partial_finish, dim3(ngan::ceil_div(C, 16)), dim3(256), 0, s, work, np, C, rec);
    return ngan::launch_status("ngan_bn_act_bwd_partial(finish)");
}

int ngan_bn_act_bwd_merged(const float* y, const float* g, const float* scale, const float* shift, const float* mean, const float* rstd,
                           const float* gamma, int act, float slope, long npix, int C, const double* recs, int world, int rank,
                           const double* n_total, float* gy, float* dgamma, float* dbeta, float* work, void* stream) {
    NGAN_REQUIRE(y && g && scale && shift && mean && rstd && gamma && recs && n_total && gy && work, NGAN_ERR_ARG,
                 "bn_act_bwd_merged: null pointer");
    NGAN_REQUIRE(world >= 1 && rank >= 0 && rank < world && npix > 0 && C > 0, NGAN_ERR_SHAPE,
                 "bn_act_bwd_merged: world=%d rank=%d npix=%ld C=%d", world, rank, npix, C);
    NGAN_REQUIRE_THREADS("bn_act_bwd_merged", npix * C);    // the apply pass: one thread per element
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_bwd_merged_finish, dim3(ngan::ceil_div(C, 256)), dim3(256), 0, s, recs, world, rank, C, n_total, gamma, rstd,
                       dgamma, dbeta, work);
    int st = ngan::launch_status("ngan_bn_act_bwd_merged(finish)");
    if (st) return st;
    const long n = npix * C;
    hipLaunchKernelGGL(bn_act_bwd_apply, dim3(ngan::ceil_div(n, 256)), dim3(256), 0, s, y, g, scale, shift, mean, rstd, work, act, slope, n, C,
                       gy);
    return ngan::launch_status("ngan_bn_act_bwd_merged");
}

}  // extern "C"
