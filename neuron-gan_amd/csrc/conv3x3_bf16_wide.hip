// bf16-storage 3x3 convolution, every contraction width other than 16 / 32 / 64 / 128 (a multiple of 16 up to 1024): the WIDE instances of
// conv3x3_bf16_impl.h's kernel template, the K = 128 kernel looped over 128-channel slices.  Design notes: conv3x3_bf16.hip.
#include "conv3x3_bf16_impl.h"

int ngan::conv3x3_bf16_launch_wide(ConvArgsB a, int N, int pgt, bool narrow, hipStream_t s) { return dispatch_n<128, true>(a, N, pgt, narrow, s); }
