// Per-pixel arithmetic of the geometric augmentation (diffgeo.hip; include/ngan_geoaug.h holds the definition), compiled for the device
// and -- by tools/diffgeo_host_check.cpp, under the address and undefined-behaviour sanitizers -- for the host.
//   geo_cell    an output pixel's source cell and fractions: the two fused multiply-add pairs IN DOUBLE (the products of an fp32
//               entry and a pixel index are exact there, so a coordinate carries two roundings at 2^-53), floor, and the guard that
//               keeps a position off the image (or not a number at all) away from the integer conversion
//   geo_weight  the bilinear weight of one of the cell's four taps, in double; forward and adjoint call the same expression
//   geo_window  the output pixels that can read a given input pixel: the image of the 2 x 2 box around it under the inverse matrix,
//               plus slack, clamped to the image.  A row outside the supported range gets an empty window or one capped in size:
//               its gradient is unspecified, its accesses are not.
// Values are fp32 in memory; between a load and the one rounding of a store everything is double.
// The caller keeps contraction off (#pragma clang fp contract(off)): the only fused operations are the explicit fma.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GEO_HD __host__ __device__ inline
#else
#define GEO_HD inline
#endif

namespace geo {

struct Row {                               // one per sample, 32 bytes: source (si, sj) = (a00 i + a01 j + a02, a10 i + a11 j + a12)
    float a00, a01, a02, a10, a11, a12, pad0, pad1;
};
static_assert(sizeof(Row) == 32, "the parameter row is 32 bytes");

struct Cell {
    int i0, j0;                            // the cell's top left tap, each in [-1, R - 1] when `near`
    double ti, tj;                         // fractions in [0, 1)
    bool near;                             // false: every tap lies outside the image (i0, j0, ti, tj are then 0)
};

struct Window {
    int ilo, ihi, jlo, jhi;                // inclusive, inside [0, R - 1]; empty when lo > hi
};

constexpr double WINDOW_SLACK = 0.125;     // output pixels; ample: the double coordinates are off by 1e-11 of a pixel at R = 16384
constexpr double WINDOW_REACH = 3.0;       // the box's half extent under the inverse is at most 2 sqrt 2 for singular values >= 1/2

GEO_HD double src_coord(float a0, float a1, float a2, int i, int j) { return fma((double)a0, (double)i, fma((double)a1, (double)j, (double)a2)); }

GEO_HD Cell geo_cell(const Row& r, int R, int i, int j) {
    const double si = src_coord(r.a00, r.a01, r.a02, i, j), sj = src_coord(r.a10, r.a11, r.a12, i, j);
    Cell c{0, 0, 0.0, 0.0, false};
    // written so that a NaN fails it; inside, floor lies in [-1, R - 1] and the conversion is safe
    if (!(si > -1.0 && si < (double)R && sj > -1.0 && sj < (double)R)) return c;
    const double fi = floor(si), fj = floor(sj);
    c.i0 = (int)fi;
    c.j0 = (int)fj;
    c.ti = si - fi;
    c.tj = sj - fj;
    c.near = true;
    return c;
}

// weight of tap (i0 + di, j0 + dj), di, dj in {0, 1}
GEO_HD double geo_weight(const Cell& c, int di, int dj) { return (di ? c.ti : 1.0 - c.ti) * (dj ? c.tj : 1.0 - c.tj); }

GEO_HD bool geo_inside(int i, int j, int R) { return (unsigned)i < (unsigned)R && (unsigned)j < (unsigned)R; }

GEO_HD int clamp_index(double v, int R) {  // v finite
    const double lo = v < 0.0 ? 0.0 : v;
    return (int)(lo > (double)(R - 1) ? (double)(R - 1) : lo);
}

// Output pixels p with source position inside [qi - 1, qi + 1] x [qj - 1, qj + 1]: p = A^-1 (s - t), so the box maps to a
// parallelogram about A^-1 ((qi, qj) - t) with half extents |inv00| + |inv01| and |inv10| + |inv11|.
GEO_HD Window geo_window(const Row& r, int R, int qi, int qj) {
    const Window none{1, 0, 1, 0};
    const double a00 = r.a00, a01 = r.a01, a10 = r.a10, a11 = r.a11;
    const double det = a00 * a11 - a01 * a10;
    if (!(fabs(det) >= 1.0 / 16 && fabs(det) <= 16.0)) return none;        // singular values in [1/2, 2] give [1/4, 4]; NaN fails
    const double v00 = a11 / det, v01 = -a01 / det, v10 = -a10 / det, v11 = a00 / det;
    const double di = (double)qi - (double)r.a02, dj = (double)qj - (double)r.a12;
    const double pi = v00 * di + v01 * dj, pj = v10 * di + v11 * dj;
    if (!(fabs(pi) < 1e9 && fabs(pj) < 1e9)) return none;                  // far outside any image
    const double ei = fmin(fabs(v00) + fabs(v01), WINDOW_REACH) + WINDOW_SLACK;
    const double ej = fmin(fabs(v10) + fabs(v11), WINDOW_REACH) + WINDOW_SLACK;
    if (pi + ei < 0.0 || pi - ei > (double)(R - 1) || pj + ej < 0.0 || pj - ej > (double)(R - 1)) return none;
    return Window{clamp_index(ceil(pi - ei), R), clamp_index(floor(pi + ei), R), clamp_index(ceil(pj - ej), R),
                  clamp_index(floor(pj + ej), R)};
}

// forward value of one output pixel from its four taps (v[2 di + dj]; a tap outside the image holds `fill`): the tap itself for zero
// fractions, else the weighted sum in double, rounded to fp32 once
GEO_HD float geo_blend(const Cell& c, const float v[4]) {
    if (c.ti == 0.0 && c.tj == 0.0) return v[0];
    double s = geo_weight(c, 0, 0) * (double)v[0];
    s += geo_weight(c, 0, 1) * (double)v[1];
    s += geo_weight(c, 1, 0) * (double)v[2];
    s += geo_weight(c, 1, 1) * (double)v[3];
    return (float)s;
}

// forward: y at output pixel (i, j) of one R x R plane
GEO_HD float geo_forward(const float* plane, const Row& r, int R, int i, int j, float fill) {
    const Cell c = geo_cell(r, R, i, j);
    if (!c.near) return fill;
    float v[4];                            // (a near cell has i0 and j0 in [-1, R - 1]: at least one tap is inside)
    for (int t = 0; t < 4; ++t) {
        const int ti = c.i0 + (t >> 1), tj = c.j0 + (t & 1);
        v[t] = geo_inside(ti, tj, R) ? plane[(long)ti * R + tj] : fill;
    }
    return geo_blend(c, v);
}

// adjoint: gx at input pixel (qi, qj) of one plane: the window's candidates in row-major order, each cell recomputed; the sum is
// carried in double and rounded to fp32 once; a single zero-fraction reader hands its value over bit for bit
GEO_HD float geo_adjoint(const float* gplane, const Row& r, int R, int qi, int qj) {
    const Window w = geo_window(r, R, qi, qj);
    double acc = 0.0;
    bool first = true;
    for (int i = w.ilo; i <= w.ihi; ++i)
        for (int j = w.jlo; j <= w.jhi; ++j) {
            const Cell c = geo_cell(r, R, i, j);
            if (!c.near) continue;
            const int di = qi - c.i0, dj = qj - c.j0;
            if ((unsigned)di > 1u || (unsigned)dj > 1u) continue;
            const double g = (double)gplane[(long)i * R + j];
            double term;
            if (c.ti == 0.0 && c.tj == 0.0) {
                if (di | dj) continue;     // the forward pass read the one tap
                term = g;
            } else {
                term = geo_weight(c, di, dj) * g;
            }
            acc = first ? term : acc + term;
            first = false;
        }
    return (float)acc;
}

// ---- the parameter row of one sample from its eight uniforms (policy bits: 1 blit, 2 geometry) ---------------------------------------
GEO_HD int draw_int(float u, int n) {      // min(n - 1, floor(u n)) in fp32: u = 1 - 2^-24 times n can round up to n
    const int k = (int)floorf(u * (float)n);
    return k < n - 1 ? k : n - 1;
}

// The row maps an output pixel to its source: s = c + A (p - c), c = ((R - 1) / 2, (R - 1) / 2), A = Blit . (1 / s) . Rot(theta), with
// Blit = Flip . Quarter^k, Flip = [[1, 0], [0, -1]] (mirror the columns), Quarter = [[0, 1], [-1, 0]] (numpy's rot90).  Formed in double,
// each entry rounded once.
GEO_HD Row geo_params(const float* u, int R, int policy, float p) {
    double b00 = 1, b01 = 0, b10 = 0, b11 = 1;
    if (policy & 1) {
        int k = 0;
        const bool flip = u[0] < p && u[1] < 0.5f;
        if (u[2] < p) k = draw_int(u[3], 4);
        for (int t = 0; t < k; ++t) {      // B <- B Quarter
            const double n00 = -b01, n01 = b00, n10 = -b11, n11 = b10;
            b00 = n00; b01 = n01; b10 = n10; b11 = n11;
        }
        if (flip) { b10 = -b10; b11 = -b11; }                              // B <- Flip B
    }
    double g00 = 1, g01 = 0, g10 = 0, g11 = 1;                             // (1 / s) Rot(theta)
    if (policy & 2) {
        double inv = 1.0, co = 1.0, sn = 0.0;
        if (u[4] < p) inv = exp2(-((2.0 * (double)u[5] - 1.0) * 0.35));
        if (u[6] < p) {
            const double theta = (2.0 * (double)u[7] - 1.0) * 3.14159265358979323846;
            co = cos(theta);
            sn = sin(theta);
        }
        g00 = inv * co; g01 = -(inv * sn); g10 = inv * sn; g11 = inv * co;
        if (sn == 0.0) { g01 = 0.0; g10 = 0.0; }                           // no -0 entries
    }
    const double a00 = b00 * g00 + b01 * g10 + 0.0, a01 = b00 * g01 + b01 * g11 + 0.0;      // (+ 0.0: no -0 entries)
    const double a10 = b10 * g00 + b11 * g10 + 0.0, a11 = b10 * g01 + b11 * g11 + 0.0;
    const double c = 0.5 * (double)(R - 1);
    Row r;
    r.a00 = (float)a00; r.a01 = (float)a01; r.a02 = (float)(c - (a00 + a01) * c);
    r.a10 = (float)a10; r.a11 = (float)a11; r.a12 = (float)(c - (a10 + a11) * c);
    r.pad0 = 0.f; r.pad1 = 0.f;
    return r;
}

}  // namespace geo
