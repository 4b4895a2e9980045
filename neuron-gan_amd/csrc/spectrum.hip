// Radial power spectrum of images (Durall et al. 2020): the kernels behind metrics.radial_spectrum.  A batched two-dimensional real
// transform in LDS, |F|^2 binned into integer rings in fp64; no vendor FFT library, no atomics, no workspace state between calls.
//   row_kernel   one workgroup per ROWS consecutive rows of one image and colour channel (ROWS = 16 from R = 128 on; 32 at R = 32
//                and 64; 16 at R = 16).  float4 loads along the rows (for C = 3 the other two channels' lanes are skipped), the Hann
//                window applied on load (w = h[y] h[x] one product, x w one product), rows 2t and 2t+1 packed as re + i im of one
//                complex length-R transform (real-input symmetry), transformed in LDS, split by A[v] = (Z[v] + conj Z[R-v]) / 2,
//                B[v] = (Z[v] - conj Z[R-v]) / 2i, and the Hermitian half v = 0 .. R/2 written transposed, G[b][c][v][y]: a run of
//                ROWS float2 per v, 128 bytes and more.
//   col_kernel   one workgroup per COLS = ROWS / 2 consecutive columns v of one image and channel: a contiguous block of G, float4
//                loads (columns past R/2 in the last workgroup are zero fill and take part in nothing), the transform along y in
//                LDS, then |F|^2 = re re + im im in fp32 and the ring sums in fp64.  Thread k owns bin k (and k + 256, k + 512): for
//                every column of the tile, ascending, it finds the interval of |u| whose d = u^2 + v^2 falls in ring k in integers
//                ((2k-1)^2 <= 4d < (2k+1)^2) and adds the negative frequencies, ascending, then the positive ones, with Hermitian
//                weight 2 for 0 < v < R/2 and 1 for v = 0 and v = R/2.  One thread per bin and one fixed order: the workgroup's
//                partial needs no combination across threads; it goes to the workspace.  With `power` the tile is also stored as
//                P = |F|^2 / norm, (B, C, R, R/2 + 1) fp32, divided in fp64 and rounded once.
//   fold_kernel  radial[b][k] = (sum over channels, then column groups, ascending, of the partials) / (C n_k norm); n_k is counted
//                from the same interval function.
// The transform is Stockham's autosort form, radix 4 with one radix-2 stage at the end for odd log2 R; every butterfly reads its
// inputs, waits at a barrier and writes in place, so one buffer of COLS x (R + 2) float2 serves (the pad keeps the split step's and
// the power store's column-strided reads on different banks).  Twiddles: a table exp(-2 pi i k / R), k < R, built in LDS at kernel
// start from sincospi in double and rounded once (exact on the axes); the window taps are built the same way, 0.5 - 0.5 cospi(2 i / R)
// in double, rounded once.  Contraction is switched off for this file (`#pragma clang fp contract(off)`) and there is no fmaf: every
// fp32 product, sum and difference rounds on its own, in the source's order -- a complex product is (wr tr - wi ti, wr ti + wi tr)
// -- and tests/spectrum_cases.py emulates exactly that.  Only plain C++: no inline assembly.
// The transform and the three kernels live in spectrum_fft.h (shared with csrc/specloss.hip), the integer ring rule in spectrum_ring.h.
#include "spectrum_fft.h"

namespace {

template <int R>
void launch(const float* images, double* radial, float* power, void* workspace, int B, int C, int window, double norm, hipStream_t s) {
    float2* G = reinterpret_cast<float2*>(workspace);
    double* partials = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + half_plane_bytes(B, R, C));
    const dim3 rows(R / rows_of(R), C, B), cols(col_groups(R), C, B);
    if (C == 1) hipLaunchKernelGGL((row_kernel<R, 1>), rows, dim3(NT), 0, s, images, G, window);
    else hipLaunchKernelGGL((row_kernel<R, 3>), rows, dim3(NT), 0, s, images, G, window);
    hipLaunchKernelGGL(col_kernel<R>, cols, dim3(NT), 0, s, G, partials, power, (float2*)nullptr, norm);
    hipLaunchKernelGGL(fold_kernel, dim3(B), dim3(NT), 0, s, partials, radial, (double*)nullptr, R, C, col_groups(R), norm);
}

}  // namespace

extern "C" int ngan_spectrum_window(float* taps, int R) {
    NGAN_REQUIRE(taps, NGAN_ERR_ARG, "spectrum_window: null pointer");
    NGAN_REQUIRE(supported(R), NGAN_ERR_SHAPE, "spectrum_window: R=%d unsupported (a power of two, 16 .. 1024)", R);
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < R; ++i) taps[i] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)i / (double)R));
    return NGAN_OK;
}

extern "C" int ngan_spectrum_ring_counts(int* counts, int R) {
    NGAN_REQUIRE(counts, NGAN_ERR_ARG, "spectrum_ring_counts: null pointer");
    NGAN_REQUIRE(supported(R), NGAN_ERR_SHAPE, "spectrum_ring_counts: R=%d unsupported (a power of two, 16 .. 1024)", R);
    const int half = R / 2;
    for (int k = 0; k <= half; ++k) counts[k] = 0;
    for (int u = -half; u < half; ++u)                         // the definition itself, over the whole plane
        for (int v = -half; v < half; ++v) {
            const long d4 = 4L * (u * u + v * v);
            long k = (long)std::floor(std::sqrt((double)(u * u + v * v)) + 0.5);
            while (k > 0 && (2 * k - 1) * (2 * k - 1) > d4) --k;
            while ((2 * k + 1) * (2 * k + 1) <= d4) ++k;
            if (k <= half) ++counts[k];
        }
    return NGAN_OK;
}

extern "C" size_t ngan_spectrum_workspace_bytes(int B, int R, int C) {
    if (B <= 0 || B > 65535 || !supported(R) || (C != 1 && C != 3)) return 0;
    return half_plane_bytes(B, R, C) + (size_t)B * C * col_groups(R) * (R / 2 + 1) * sizeof(double);
}

extern "C" int ngan_spectrum_radial(const float* images, double* radial, float* power_or_null, void* workspace, int B, int R, int C,
                                    int window, void* stream) {
    NGAN_REQUIRE(images && radial, NGAN_ERR_ARG, "spectrum_radial: null pointer");
    NGAN_REQUIRE(workspace, NGAN_ERR_ARG, "spectrum_radial: null workspace (ngan_spectrum_workspace_bytes names its size)");
    NGAN_REQUIRE(supported(R), NGAN_ERR_SHAPE, "spectrum_radial: R=%d unsupported (a power of two, 16 .. 1024)", R);
    NGAN_REQUIRE(C == 1 || C == 3, NGAN_ERR_SHAPE, "spectrum_radial: C=%d unsupported (1 or 3 colour channels)", C);
    NGAN_REQUIRE(B > 0 && B < 65536, NGAN_ERR_SHAPE, "spectrum_radial: B=%d unsupported (1 .. 65535 images per call)", B);
    NGAN_REQUIRE(((uintptr_t)images | (uintptr_t)workspace | (uintptr_t)power_or_null) % 16 == 0 && (uintptr_t)radial % 8 == 0,
                 NGAN_ERR_ARG, "spectrum_radial: images, power and workspace must start on a 16-byte boundary, radial on an 8-byte one");
    double norm = (double)R * (double)R;
    if (window) {
        float taps[1024];
        ngan_spectrum_window(taps, R);
        double s = 0.0;
        for (int i = 0; i < R; ++i) s += (double)taps[i] * (double)taps[i];
        norm = s * s;
    }
    hipStream_t s = (hipStream_t)stream;
    switch (R) {
        case 16: launch<16>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
        case 32: launch<32>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
        case 64: launch<64>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
        case 128: launch<128>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
        case 256: launch<256>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
        case 512: launch<512>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
        default: launch<1024>(images, radial, power_or_null, workspace, B, C, window != 0, norm, s); break;
    }
    return ngan::launch_status("ngan_spectrum_radial");
}
