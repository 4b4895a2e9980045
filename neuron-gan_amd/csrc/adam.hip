// Fused multi-tensor Adam over a flat parameter buffer.  Replaces optim.Adam.step
// (/root/reference/train.py:224-225, 366, 385: betas (beta1, 0.999), eps 1e-8, no weight decay, no amsgrad),
// i.e. the ATen lerp_/addcmul_/sqrt/addcdiv_ chain per parameter tensor.
// Per-tensor step counts are kept because a progressively grown net activates tensors at different times:
// torch skips parameters whose .grad is None, so their bias correction starts when they first receive one.
// Hyper-parameters and step counts live in device memory so a captured graph replays with fresh values.
// ngan_adam_step_clip / ngan_rmsprop_step_clip (the WGAN critic's weight clipping, reference train.py:489-490) clamp each updated
// parameter to [-clip, clip] before it is stored: the same bits as the unclipped step followed by p.clamp_(-clip, clip).
// ngan_rmsprop_step is the same launch pair for optim.RMSprop.step (train.py:220-222, the reference's --RMSprop switch): one state
// buffer (square_avg) instead of two, same work list, same per-tensor step counts (torch keeps state['step'] for RMSprop too).
// ngan_adam_step_ema / ngan_rmsprop_step_ema also keep an exponential moving average of the parameters (no reference counterpart,
// opt-in): e' = fmaf(w, p' - e, e) with the new parameter p' still in its register, w = 1 - beta read from one device float.
// ngan_ema_step is that update alone over the same work list (the form the folded ones are compared with).
#include "ngan_common.h"

namespace {

__global__ void adam_advance_kernel(const int* __restrict__ active, float* __restrict__ step, int n_seg) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_seg && active[i]) step[i] += 1.0f;
}

constexpr int CHUNK = 4096;

// clamp_(-c, c) as torch forms it: min(max(p, -c), c) with NaN passed through
__device__ __forceinline__ float clamp_sym(float p, float c) { return p < -c ? -c : (p > c ? c : p); }

template <bool CLIP, bool EMA = false>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, const long* __restrict__ seg_off,
                                                   const long* __restrict__ seg_len, const int* __restrict__ seg_active,
                                                   const float* __restrict__ seg_step, const int* __restrict__ chunk_seg,
                                                   const long* __restrict__ chunk_off, const float* __restrict__ hyper, float clip,
                                                   float* __restrict__ ema = nullptr, const float* __restrict__ ema_w = nullptr) {
    const int seg = chunk_seg[blockIdx.x];
    if (!seg_active[seg]) return;
    const AdamCoef k = adam_coef(hyper, seg_step[seg]);
    const float w = EMA ? ema_w[0] : 0.f;
    const long off = chunk_off[blockIdx.x];
    const long base = seg_off[seg] + off;
    const long n = min((long)CHUNK, seg_len[seg] - off);
    for (long i = threadIdx.x; i < n; i += 256) {
        const long j = base + i;
        float pv = p[j], mv = m[j], vv = v[j];
        adam_update(k, g[j], pv, mv, vv);
        m[j] = mv;
        v[j] = vv;
        p[j] = CLIP ? clamp_sym(pv, clip) : pv;
        if (EMA) ema[j] = ema_update(w, pv, ema[j]);
    }
}

template <bool CLIP, bool EMA = false>
__global__ __launch_bounds__(256) void rmsprop_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ v,
                                                      const long* __restrict__ seg_off, const long* __restrict__ seg_len,
                                                      const int* __restrict__ seg_active, const int* __restrict__ chunk_seg,
                                                      const long* __restrict__ chunk_off, const float* __restrict__ hyper, float clip,
                                                      float* __restrict__ ema = nullptr, const float* __restrict__ ema_w = nullptr) {
    const int seg = chunk_seg[blockIdx.x];
    if (!seg_active[seg]) return;
    const RmspropCoef k = rmsprop_coef(hyper);
    const float w = EMA ? ema_w[0] : 0.f;
    const long off = chunk_off[blockIdx.x];
    const long base = seg_off[seg] + off;
    const long n = min((long)CHUNK, seg_len[seg] - off);
    for (long i = threadIdx.x; i < n; i += 256) {
        const long j = base + i;
        float pv = p[j], vv = v[j];
        rmsprop_update(k, g[j], pv, vv);
        v[j] = vv;
        p[j] = CLIP ? clamp_sym(pv, clip) : pv;
        if (EMA) ema[j] = ema_update(w, pv, ema[j]);
    }
}

// the average alone, over the work list of the steps above: e' = fmaf(w, p - e, e) for the chunks of active tensors
__global__ __launch_bounds__(256) void ema_kernel(const float* __restrict__ p, float* __restrict__ ema, const long* __restrict__ seg_off,
                                                  const long* __restrict__ seg_len, const int* __restrict__ seg_active,
                                                  const int* __restrict__ chunk_seg, const long* __restrict__ chunk_off,
                                                  const float* __restrict__ ema_w) {
    const int seg = chunk_seg[blockIdx.x];
    if (!seg_active[seg]) return;
    const float w = ema_w[0];
    const long off = chunk_off[blockIdx.x];
    const long base = seg_off[seg] + off;
    const long n = min((long)CHUNK, seg_len[seg] - off);
    for (long i = threadIdx.x; i < n; i += 256) {
        const long j = base + i;
        ema[j] = ema_update(w, p[j], ema[j]);
    }
}

}  // namespace

extern "C" int ngan_adam_step(float* p, const float* g, float* m, float* v, const long* seg_off, const long* seg_len,
                              const int* seg_active, float* seg_step, int n_seg, const int* chunk_seg, const long* chunk_off,
                              int n_chunks, const float* hyper, int n_hyper, void* stream) {
    NGAN_REQUIRE(p && g && m && v && seg_off && seg_len && seg_active && seg_step && chunk_seg && chunk_off && hyper,
                 NGAN_ERR_ARG, "adam_step: null pointer");
    NGAN_REQUIRE(n_hyper == NGAN_ADAM_HYPER_FLOATS, NGAN_ERR_ARG, "adam_step: hyper holds %d floats, this library reads %d (include/ngan.h)",
                 n_hyper, NGAN_ADAM_HYPER_FLOATS);
    NGAN_REQUIRE(n_seg > 0 && n_chunks > 0, NGAN_ERR_SHAPE, "adam_step: n_seg=%d n_chunks=%d", n_seg, n_chunks);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_advance_kernel, dim3(ngan::ceil_div(n_seg, 256)), dim3(256), 0, s, seg_active, seg_step, n_seg);
    int st = ngan::launch_status("ngan_adam_step(advance)");
    if (st) return st;
    hipLaunchKernelGGL(adam_kernel<false>, dim3(n_chunks), dim3(256), 0, s, p, g, m, v, seg_off, seg_len, seg_active, seg_step,
                       chunk_seg, chunk_off, hyper, 0.f);
    return ngan::launch_status("ngan_adam_step");
}

extern "C" int ngan_rmsprop_step(float* p, const float* g, float* v, const long* seg_off, const long* seg_len, const int* seg_active,
                                 float* seg_step, int n_seg, const int* chunk_seg, const long* chunk_off, int n_chunks,
                                 const float* hyper, int n_hyper, void* stream) {
    NGAN_REQUIRE(p && g && v && seg_off && seg_len && seg_active && seg_step && chunk_seg && chunk_off && hyper,
                 NGAN_ERR_ARG, "rmsprop_step: null pointer");
    NGAN_REQUIRE(n_hyper == NGAN_RMSPROP_HYPER_FLOATS, NGAN_ERR_ARG,
                 "rmsprop_step: hyper holds %d floats, this library reads %d (include/ngan.h)", n_hyper, NGAN_RMSPROP_HYPER_FLOATS);
    NGAN_REQUIRE(n_seg > 0 && n_chunks > 0, NGAN_ERR_SHAPE, "rmsprop_step: n_seg=%d n_chunks=%d", n_seg, n_chunks);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_advance_kernel, dim3(ngan::ceil_div(n_seg, 256)), dim3(256), 0, s, seg_active, seg_step, n_seg);
    int st = ngan::launch_status("ngan_rmsprop_step(advance)");
    if (st) return st;
    hipLaunchKernelGGL(rmsprop_kernel<false>, dim3(n_chunks), dim3(256), 0, s, p, g, v, seg_off, seg_len, seg_active, chunk_seg, chunk_off,
                       hyper, 0.f);
    return ngan::launch_status("ngan_rmsprop_step");
}

extern "C" int ngan_adam_step_clip(float* p, const float* g, float* m, float* v, const long* seg_off, const long* seg_len,
                                   const int* seg_active, float* seg_step, int n_seg, const int* chunk_seg, const long* chunk_off,
                                   int n_chunks, const float* hyper, int n_hyper, float clip, void* stream) {
    NGAN_REQUIRE(p && g && m && v && seg_off && seg_len && seg_active && seg_step && chunk_seg && chunk_off && hyper,
                 NGAN_ERR_ARG, "adam_step_clip: null pointer");
    NGAN_REQUIRE(n_hyper == NGAN_ADAM_HYPER_FLOATS, NGAN_ERR_ARG, "adam_step_clip: hyper holds %d floats, this library reads %d (include/ngan.h)",
                 n_hyper, NGAN_ADAM_HYPER_FLOATS);
    NGAN_REQUIRE(n_seg > 0 && n_chunks > 0, NGAN_ERR_SHAPE, "adam_step_clip: n_seg=%d n_chunks=%d", n_seg, n_chunks);
    NGAN_REQUIRE(clip >= 0.f, NGAN_ERR_ARG, "adam_step_clip: clip=%g", clip);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_advance_kernel, dim3(ngan::ceil_div(n_seg, 256)), dim3(256), 0, s, seg_active, seg_step, n_seg);
    int st = ngan::launch_status("ngan_adam_step_clip(advance)");
    if (st) return st;
    hipLaunchKernelGGL(adam_kernel<true>, dim3(n_chunks), dim3(256), 0, s, p, g, m, v, seg_off, seg_len, seg_active, seg_step,
                       chunk_seg, chunk_off, hyper, clip);
    return ngan::launch_status("ngan_adam_step_clip");
}

extern "C" int ngan_rmsprop_step_clip(float* p, const float* g, float* v, const long* seg_off, const long* seg_len, const int* seg_active,
                                      float* seg_step, int n_seg, const int* chunk_seg, const long* chunk_off, int n_chunks,
                                      const float* hyper, int n_hyper, float clip, void* stream) {
    NGAN_REQUIRE(p && g && v && seg_off && seg_len && seg_active && seg_step && chunk_seg && chunk_off && hyper,
                 NGAN_ERR_ARG, "rmsprop_step_clip: null pointer");
    NGAN_REQUIRE(n_hyper == NGAN_RMSPROP_HYPER_FLOATS, NGAN_ERR_ARG,
                 "rmsprop_step_clip: hyper holds %d floats, this library reads %d (include/ngan.h)", n_hyper, NGAN_RMSPROP_HYPER_FLOATS);
    NGAN_REQUIRE(n_seg > 0 && n_chunks > 0, NGAN_ERR_SHAPE, "rmsprop_step_clip: n_seg=%d n_chunks=%d", n_seg, n_chunks);
    NGAN_REQUIRE(clip >= 0.f, NGAN_ERR_ARG, "rmsprop_step_clip: clip=%g", clip);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_advance_kernel, dim3(ngan::ceil_div(n_seg, 256)), dim3(256), 0, s, seg_active, seg_step, n_seg);
    int st = ngan::launch_status("ngan_rmsprop_step_clip(advance)");
    if (st) return st;
    hipLaunchKernelGGL(rmsprop_kernel<true>, dim3(n_chunks), dim3(256), 0, s, p, g, v, seg_off, seg_len, seg_active, chunk_seg, chunk_off,
                       hyper, clip);
    return ngan::launch_status("ngan_rmsprop_step_clip");
}

extern "C" int ngan_adam_step_ema(float* p, const float* g, float* m, float* v, const long* seg_off, const long* seg_len,
                                  const int* seg_active, float* seg_step, int n_seg, const int* chunk_seg, const long* chunk_off,
                                  int n_chunks, const float* hyper, int n_hyper, float* ema, const float* ema_w, void* stream) {
    NGAN_REQUIRE(p && g && m && v && seg_off && seg_len && seg_active && seg_step && chunk_seg && chunk_off && hyper && ema && ema_w,
                 NGAN_ERR_ARG, "adam_step_ema: null pointer");
    NGAN_REQUIRE(n_hyper == NGAN_ADAM_HYPER_FLOATS, NGAN_ERR_ARG, "adam_step_ema: hyper holds %d floats, this library reads %d (include/ngan.h)",
                 n_hyper, NGAN_ADAM_HYPER_FLOATS);
    NGAN_REQUIRE(n_seg > 0 && n_chunks > 0, NGAN_ERR_SHAPE, "adam_step_ema: n_seg=%d n_chunks=%d", n_seg, n_chunks);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_advance_kernel, dim3(ngan::ceil_div(n_seg, 256)), dim3(256), 0, s, seg_active, seg_step, n_seg);
    int st = ngan::launch_status("ngan_adam_step_ema(advance)");
    if (st) return st;
    hipLaunchKernelGGL((adam_kernel<false, true>), dim3(n_chunks), dim3(256), 0, s, p, g, m, v, seg_off, seg_len, seg_active, seg_step,
                       chunk_seg, chunk_off, hyper, 0.f, ema, ema_w);
    return ngan::launch_status("ngan_adam_step_ema");
}

extern "C" int ngan_rmsprop_step_ema(float* p, const float* g, float* v, const long* seg_off, const long* seg_len, const int* seg_active,
                                     float* seg_step, int n_seg, const int* chunk_seg, const long* chunk_off, int n_chunks,
                                     const float* hyper, int n_hyper, float* ema, const float* ema_w, void* stream) {
    NGAN_REQUIRE(p && g && v && seg_off && seg_len && seg_active && seg_step && chunk_seg && chunk_off && hyper && ema && ema_w,
                 NGAN_ERR_ARG, "rmsprop_step_ema: null pointer");
    NGAN_REQUIRE(n_hyper == NGAN_RMSPROP_HYPER_FLOATS, NGAN_ERR_ARG,
                 "rmsprop_step_ema: hyper holds %d floats, this library reads %d (include/ngan.h)", n_hyper, NGAN_RMSPROP_HYPER_FLOATS);
    NGAN_REQUIRE(n_seg > 0 && n_chunks > 0, NGAN_ERR_SHAPE, "rmsprop_step_ema: n_seg=%d n_chunks=%d", n_seg, n_chunks);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_advance_kernel, dim3(ngan::ceil_div(n_seg, 256)), dim3(256), 0, s, seg_active, seg_step, n_seg);
    int st = ngan::launch_status("ngan_rmsprop_step_ema(advance)");
    if (st) return st;
    hipLaunchKernelGGL((rmsprop_kernel<false, true>), dim3(n_chunks), dim3(256), 0, s, p, g, v, seg_off, seg_len, seg_active, chunk_seg,
                       chunk_off, hyper, 0.f, ema, ema_w);
    return ngan::launch_status("ngan_rmsprop_step_ema");
}

extern "C" int ngan_ema_step(const float* p, float* ema, const long* seg_off, const long* seg_len, const int* seg_active,
                             const int* chunk_seg, const long* chunk_off, int n_chunks, const float* ema_w, void* stream) {
    NGAN_REQUIRE(p && ema && seg_off && seg_len && seg_active && chunk_seg && chunk_off && ema_w, NGAN_ERR_ARG, "ema_step: null pointer");
    NGAN_REQUIRE(n_chunks > 0, NGAN_ERR_SHAPE, "ema_step: n_chunks=%d", n_chunks);
    hipLaunchKernelGGL(ema_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, p, ema, seg_off, seg_len, seg_active, chunk_seg,
                       chunk_off, ema_w);
    return ngan::launch_status("ngan_ema_step");
}
