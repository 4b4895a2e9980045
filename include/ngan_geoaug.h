/* ngan_geoaug.h -- extension section of ngan.h (which includes it: include ngan.h, not this file): the geometric groups of the
 * differentiable augmentation -- mirror and quarter turns ("blit"), isotropic scale and rotation ("geometry") -- as one bilinear
 * resampling per sample, and its adjoint.  Same conventions as ngan.h: status-returning, the trailing void* is the hipStream_t,
 * device pointers, no state between calls.  Python binding: _C.SIGNATURES.
 *
 * Images are contiguous fp32 (B, C, R, R), square, R a multiple of 4 (4 .. 16384), fp32 in every arithmetic mode.  Sample n has a
 * 32-byte row of eight floats {a00, a01, a02, a10, a11, a12, 0, 0} that maps output pixel (row i, column j) to a source position in
 * absolute pixel coordinates:
 *     si = fma(a00, i, fma(a01, j, a02)),   sj = fma(a10, i, fma(a11, j, a12))      evaluated in DOUBLE from the fp32 entries
 * (the products are exact there; an fp32 evaluation would put up to 2^-24 |s| of a pixel into every fraction, 3e-5 at 512 x 512,
 * which is more than the whole blend's rounding).  Values are fp32 in memory; between a load and the one rounding of a store the
 * arithmetic is double.
 * forward:  y[i, j] = sum over the four taps of the cell (floor si, floor sj) of w . tap, fractions (ti, tj) = (si - floor si,
 *           sj - floor sj), w = {(1 - ti)(1 - tj), (1 - ti) tj, ti (1 - tj), ti tj}; a tap outside the image holds the constant
 *           `fill`; the sum is rounded to fp32 once.  Where both fractions are 0 the output is the tap itself, bit for bit (the
 *           sign of a zero included): the identity row and the eight blit rows copy values exactly.
 * adjoint:  gx[q] = sum over all output pixels p of w_p(q) gy[p], w_p(q) the weight with which p reads q, by the forward's own
 *           expressions; the fill has derivative 0.  No atomics: a thread owns an input pixel, visits in row-major order the window
 *           of output pixels that can reach it (the image of the 2 x 2 box about the pixel under the inverse matrix, plus slack,
 *           clamped to the image) and adds, in double, where the recomputed cell touches its pixel; one rounding at the end.
 *           Bit-reproducible, independent of the rest of the batch, an exact transpose of the forward as computed.
 * Range:    the adjoint is correct for every row whose linear part has singular values in [1/2, 2]; ngan_diffgeo_params never leaves
 *           that range.  A row outside it gives an UNSPECIFIED gradient (a determinant outside [1/16, 16]: zero).  No row, finite or
 *           not, makes either launch read or write outside the images: the window is clamped and capped, and a source position off
 *           the image never reaches an integer conversion.
 * Aliasing: bilinear taps alias under zoom-out; with the scale range below (at most 2^0.35 = 1.27) that is accepted.
 * NGAN_ERR_ARG for a null pointer, images or a table off a 16-byte boundary, a table shorter than the batch, a fill that is not
 * finite, a policy mask outside 0 .. 3, p outside [0, 1]; NGAN_ERR_SHAPE for H != W, R no multiple of 4 or outside 4 .. 16384, B
 * outside 1 .. 65535, a sample of 2^31 values or more. */
#ifndef NGAN_GEOAUG_H
#define NGAN_GEOAUG_H

#ifdef __cplusplus
extern "C" {
#endif

/* rows 0 .. B-1 of `table` from (B, 8) uniforms in [0, 1), one thread per sample; draw(u, n) = min(n - 1, floor(u n)) in fp32.
 * policy bits: 1 blit, 2 geometry.
 *   blit      u0 < p and u1 < 0.5: mirror the columns;        u2 < p: k = draw(u3, 4) quarter turns (numpy's rot90)
 *   geometry  u4 < p: zoom in by s = exp2((2 u5 - 1) 0.35);   u6 < p: rotate by theta = (2 u7 - 1) pi
 * The row is the composition blit, then scale, then rotation, about the image centre c = ((R - 1) / 2, (R - 1) / 2):
 *   A = Flip . Quarter^k . (1 / s) . [[cos, -sin], [sin, cos]],  a02 = c - (a00 + a01) c,  a12 = c - (a10 + a11) c,
 * formed in double, each entry rounded to fp32 once.  With both geometry gates closed the entries are exactly in {0, +-1} and the
 * offsets exactly in {0, R - 1}. */
int ngan_diffgeo_params(const float* uniforms, void* table, int B, int H, int W, int table_rows, int policy, float p, void* stream);
/* y = T(x); y may be a row range of a larger buffer */
int ngan_diffgeo_fwd(const float* x, const void* table, float* y, int B, int C, int H, int W, int table_rows, float fill, void* stream);
/* gx = T^T(gy) */
int ngan_diffgeo_bwd(const float* gy, const void* table, float* gx, int B, int C, int H, int W, int table_rows, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NGAN_GEOAUG_H */
