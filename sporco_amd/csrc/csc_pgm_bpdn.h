// csc_pgm_bpdn.h -- dense (patch-based) sparse coding by proximal gradient steps, sporco.pgm.bpdn BPDN / WeightedBPDN
// (sporco/pgm/bpdn.py:26-375, the loop and its rules: sporco/pgm/pgm.py:284-702, backtrack.py, stepsize.py):
//     minimise (1/2) || D x - s ||^2_W + lmbda || wl1 x ||_1,   W diagonal, given as an array w that multiplies (D x - s)^2
// with D (N, M), S (N, K) and X, Y, G (M, K).  Every array is row-major as NumPy has it.
//
// bpdn_pgm_step, per block of KB columns (bpdn_kb; the operands dk / dtk and the product routine are csc_bpdn.h's),
// runs the phases its caller asks for:
//   gradient phase   1. the Y tile (M, KB) -> LDS: loaded, or formed on the way in and stored,
//                           momentum   Y = Xprv + beta (Xprv - Xold)           (Xold: what the output array X still holds)
//                           robust     [Z += zc (Xprv - Yprv);]  Y = (tk Xprv + t Z) / T
//                    2. R = w (D Y - S) -> the second LDS tile (N, KB); by-product f(Y) = (1/2) sum w (D Y - S)^2
//                    3. G = D^T R; stored where a rule needs it afterwards; sums || G ||^2 and, for the
//                       Barzilai-Borwein rule, <Xprv - Xold, G - Gold>, || G - Gold ||^2
//                       [Cauchy rule: G -> LDS, || D G ||^2 by one more product]
//   prox phase       (in the epilogue of 3 when both phases run, else from Y and G in global memory)
//                       V = Y - G / L;  X' = soft(V, (lmbda / L) wl1) [max(., 0)]  (revert: X' = Xprv);  X' stored
//                       sums <X' - Y, G>, || X' - Y ||^2, || wl1 X' ||_1, || X' ||^2, || X' - Yprv ||^2;  X' -> LDS
//                    4. F(X') = (1/2) sum w (D X' - S)^2 by the product routine
// so one launch with both phases yields the iterate and every scalar of F, Q_L, Rsdl, DFid and RegL1.  A rule that
// must know G before it fixes L (Cauchy, Barzilai-Borwein) launches the phases one after the other.
// bpdn_pgm_ystep is the Y update as a launch of its own (Monotone, whose revert is a global decision):
//     Y = X + gamma (ZZ - X) + beta (X - Xprv),  sum (X - Y)^2.
// Sums are per-workgroup partials in double, reduced by launch_finalize in a fixed order: no floating-point
// atomics, two runs agree bit for bit; the two product forms of csc_bpdn.h agree bit for bit here as well.
#pragma once

#include "csc_bpdn.h"

namespace sporco_amd {

constexpr int kPgmBpdnSums = 12;     // doubles a workgroup of bpdn_pgm_step leaves (pgm_bpdn_sums)
// (the halves of FY / FX are applied by launch_finalize's scale)
enum pgm_bpdn_sums {
    PGMB_FY = 0,     // sum w (D Y - S)^2
    PGMB_FX,         // sum w (D X' - S)^2
    PGMB_DXG,        // <X' - Y, G>
    PGMB_DXY2,       // || X' - Y ||^2
    PGMB_L1,         // || wl1 X' ||_1
    PGMB_X2,         // || X' ||^2
    PGMB_RS2,        // || X' - Yprv ||^2  (bpdn_pgm_ystep: || X - Y ||^2)
    PGMB_G2,         // || G ||^2
    PGMB_DG2,        // || D G ||^2 (Cauchy)
    PGMB_BBXG,       // <Xprv - Xold, G - Gold>
    PGMB_BBG2,       // || G - Gold ||^2
    PGMB_SPARE
};
enum pgm_bpdn_phase { PGMB_PHASE_GRAD = 1, PGMB_PHASE_PROX = 2 };
enum pgm_bpdn_ymode { PGMB_Y_LOAD = 0, PGMB_Y_MOMENTUM = 1, PGMB_Y_ROBUST = 2 };

template <typename T> inline size_t pgm_bpdn_lds_bytes(int M, int N) {
    const int R = bpdn_up(M > N ? M : N, 4), KB = bpdn_kb<T>(M, N);
    return (size_t)2 * R * bpdn_ldb(KB) * sizeof(T) + sizeof(double) * kPgmBpdnSums * 4;
}

template <typename T> struct PgmBpdnArgs {
    const T *dk = nullptr, *dtk = nullptr;     // k-major, zero padded: dk [N4][M16] = D (for D^T .); dtk [M4][N16] = D^T
    const T *s = nullptr;                      // (N, K)
    const T *w = nullptr;                      // (N, K) weight of the data fidelity term, or nullptr: w_s
    const T *wl1 = nullptr;                    // (M, K) L1Weight array, or nullptr: wl1_s
    T *x = nullptr;                            // (M, K) out: X'; on entry Xold, the iterate before Xprv
    const T *xprv = nullptr;                   // (M, K) the iterate the step starts from
    T *y = nullptr;                            // (M, K) read (PGMB_Y_LOAD) or written
    const T *yprv = nullptr;                   // (M, K) robust: the Y of the iteration before; nullptr: Y itself
    T *g = nullptr;                            // (M, K) G: written by the gradient phase, read by a prox phase alone
    T *z = nullptr, *zz = nullptr;             // (M, K) robust: Z; Monotone: the unreverted X'
    T w_s = T(1), wl1_s = T(1);
    T L = T(1), lmbda = T(0), beta = T(0), tk = T(0), tt = T(0), TT = T(1), zc = T(0);
    int phase = PGMB_PHASE_GRAD | PGMB_PHASE_PROX, ymode = PGMB_Y_LOAD;
    int nonneg = 0, revert = 0, z_update = 0, cauchy = 0, bb = 0, form = BPDN_FORM_PLAIN;
    int M = 1, N = 1, KB = 16;
    int64_t K = 1;
    double *partials = nullptr;                // kPgmBpdnSums doubles per workgroup
};

// The phases of one step.  Returns the workgroups.
template <typename T> int launch_bpdn_pgm_step(hipStream_t st, const PgmBpdnArgs<T> &a);
// y = x + gamma (zz - x) + beta (x - xprv) (zz == nullptr: without that term) over n elements;
// partials[b] = sum (x - y)^2 of workgroup b.  Returns the workgroups.
template <typename T>
int launch_bpdn_pgm_ystep(hipStream_t st, const T *x, const T *xprv, const T *zz, T *y, T beta, T gamma, int64_t n,
                          double *partials);

}  // namespace sporco_amd
