/* ngan_first_block.h -- extension section of ngan.h (which includes it: include ngan.h, not this file): the launch plan of the folded
 * critic first block (ngan_first_block_fwd / _bwd / _dx of ngan.h) as a host query.  Python binding: _C.NON_STATUS.
 *
 * ngan_first_block_plan makes no HIP call and launches nothing.  out4 = { workgroups along x (256 / (N/4) pixels each), image rows
 * per workgroup of bwd's sums kernel, row chunks per sample, slabs = their product with B }.  The rows start at 8 and double until the
 * launch has at most 1024 slabs or one workgroup owns a whole column; the forward and the image gradient always take 8 rows.
 * The status is the one fwd, bwd and dx (dx with C = 1) return for the shape, and they take it from the same plan:
 *   NGAN_ERR_ARG    out4 null
 *   NGAN_ERR_SHAPE  outside B, H, W, C > 0, C <= 64, N in {16, 32}, B * ceil(H / 8) < 65536, B * H * W * N < 2^31, or where the plan
 *                   needs more than 1024 slabs (grid.x * B > 1024).  out4 then holds what was planned up to the refusal and slabs = 0. */
#ifndef NGAN_FIRST_BLOCK_H
#define NGAN_FIRST_BLOCK_H

#ifdef __cplusplus
extern "C" {
#endif

int ngan_first_block_plan(int B, int H, int W, int C, int N, int* out4);

#ifdef __cplusplus
}
#endif
#endif /* NGAN_FIRST_BLOCK_H */
