// csc_bpdn_product.h -- the one product routine of the dense (patch-based) kernels, shared by csc_bpdn.hip and
// csc_cmod.hip (device code; the translation units that include it are compiled with -ffp-contract=off).
#pragma once

#include "csc_bpdn.h"
#include "csc_kernels_dev.h"

namespace sporco_amd {

// OUT (lda rows, 16 NCT columns) = A . TILE, k over [0, Kd4).  ak: [Kd4][lda] k-major, zero padded, lda a multiple of
// 16, Kd4 of 4; tile: [Kd4][ldb] in LDS, zero padded.  Wave w takes the slabs of rows 16 w, 16 (w + 4), ...; lane l
// ends with rows i0 + 4 (l >> 4) + r, r < 4, of column 16 ct + (l & 15), handed to epi(row, column, value).
template <typename T, int NCT, int FORM, typename Epi>
__device__ __forceinline__ void bpdn_product(const T *__restrict__ ak, int lda, int Kd4, const T *tile, int ldb, Epi &&epi) {
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
    const int lc = lane & 15, lh = lane >> 4;
    for (int i0 = wave * 16; i0 < lda; i0 += 16 * (kThreads / kWave)) {
        T acc[NCT][4];
#ifndef SPORCO_AMD_HOSTSIM
        if constexpr (FORM == BPDN_FORM_MFMA) {
            // A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]; D: column l & 15, rows 4 (l >> 4) + r
            sa_floatx4 c[NCT];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) c[ct] = sa_floatx4{0.f, 0.f, 0.f, 0.f};
            const T *ap = ak + (int64_t)lh * lda + i0 + lc;
            const T *bp = tile + lh * ldb + lc;
            for (int k0 = 0; k0 < Kd4; k0 += 4) {
                const float av = ap[(int64_t)k0 * lda];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) c[ct] = sa_mfma_f32_16x16x4(av, bp[k0 * ldb + 16 * ct], c[ct]);
            }
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                acc[ct][0] = c[ct].x;
                acc[ct][1] = c[ct].y;
                acc[ct][2] = c[ct].z;
                acc[ct][3] = c[ct].w;
            }
        } else
#endif
        {
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[ct][r] = T(0);
            const T *ap = ak + i0 + 4 * lh;
            const T *bp = tile + lc;
            for (int k = 0; k < Kd4; ++k) {
                const Vec<T, 4> av = *reinterpret_cast<const Vec<T, 4> *>(ap + (int64_t)k * lda);
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const T bv = bp[k * ldb + 16 * ct];
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[ct][r] = fma1(av.v[r], bv, acc[ct][r]);
                }
            }
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) epi(i0 + 4 * lh + r, 16 * ct + lc, acc[ct][r]);
    }
}

}  // namespace sporco_amd
