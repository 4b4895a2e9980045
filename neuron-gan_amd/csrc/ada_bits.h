// Per-element arithmetic of the adaptive augmentation controller (include/ngada.h), shared by the kernels of ada.hip and by host code
// (tools/ada_host_check.cpp compiles it under sanitizers).  Counts are 64-bit integers; everything else is fp64 with one operation
// per rounding and contraction off, so the device, the host and the emulation of tests/ada_cases.py form the same bits.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ADA_HD __host__ __device__ inline
#else
#define ADA_HD inline
#endif

namespace ada {

constexpr int N_MIN = 1, N_MAX = 65536;      // scores per side of one ngada_accumulate call
constexpr int THREADS = 256;                 // the one workgroup: thread k owns elements k, k + 256, ... in ascending order

// +1 for a score above the threshold, -1 below, 0 for a tie or when either is NaN; compared as doubles (every float is one exactly)
ADA_HD int side(float s, double t) {
    const double v = (double)s;
    return (int)(v > t) - (int)(v < t);
}

// the midpoint of the two batch means from their fp64 sums: two divisions, one addition, one (exact) halving
ADA_HD double midpoint(double sum_real, int n_real, double sum_fake, int n_fake) {
#pragma clang fp contract(off)
    const double mr = sum_real / (double)n_real;
    const double mf = sum_fake / (double)n_fake;
    const double m = mr + mf;
    return 0.5 * m;
}

// One step of the controller.  s = sign((pos - neg) - target n): 0 for a zero or NaN difference and for n = 0.  pos - neg and n are
// exact in fp64 (|.| < 2^53); the product target n is rounded once.
struct Step { float p, r; };
ADA_HD Step update(long pos, long neg, long n, float p, float last_r, float target, double span, float p_max) {
#pragma clang fp contract(off)
    const double diff = (double)(pos - neg);
    const double nd = (double)n;
    const double tn = (double)target * nd;
    const double d = diff - tn;
    const double s = n == 0 ? 0.0 : (double)((int)(d > 0.0) - (int)(d < 0.0));
    const double sn = s * nd;                               // exact
    const double move = sn / span;
    double q = (double)p + move;
    q = q > 0.0 ? q : 0.0;                                   // max(0, q); a NaN p lands here: 0
    q = q < (double)p_max ? q : (double)p_max;               // min(p_max, q)
    Step out;
    out.p = (float)q;
    out.r = n ? (float)(diff / nd) : last_r;
    return out;
}

}  // namespace ada
