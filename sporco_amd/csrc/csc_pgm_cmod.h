// csc_pgm_cmod.h -- the dictionary update of the dense (patch-based) family by proximal gradient steps,
// sporco.pgm.cmod CnstrMOD / WeightedCnstrMOD (sporco/pgm/cmod.py:24-407; the loop and its rules: sporco/pgm/pgm.py:284-702,
// backtrack.py, stepsize.py):
//     minimise (1/2) || D Z - S ||^2_W  such that  || d_m || = 1 [, mean(d_m) = 0 | d_m >= 0],
// W given as an array w that multiplies (D Z - S)^2.  Z is (M, K), S and w (N, K), row-major as NumPy has them; the
// dictionary iterates X, Y, G are (N, M) and kept k-major and zero padded, [M4][N16] with element (n, m) at m N16 + n,
// as the kernels of csc_cmod.h keep theirs.
//
// cmod_pgm_grad: G = (w (Y Z - S)) Z^T, an (N, M) reduction over K that has to stream Z, S and w: the weight sits
// between the two products, so no Gram matrix serves.  A workgroup owns a block of kPgmCmodRows = 32 rows of N and one
// slab of K (cmod_slab of csc_cmod.h).  Per step of kCmodKS columns it stages the Z tile (all M rows, zero padded to
// M16 rows and beyond the slab's end) in LDS; wave w forms the 16 x 16 tile (row half w >> 1, column half w & 1) of
//     r = Y_blk . Ztile - S_blk,  R = w r   -> the second LDS tile,  f(Y) += w r^2,
// the left operand Y read from global memory (k-major, at most 1 MiB and cache resident); then wave w accumulates
// G_blk += R . Ztile^T for the 16-column tiles w, w + 4, ... of M and both row halves, in the accumulator map of
// v_mfma_f32_16x16x4_f32 (lane l: rows 4 (l >> 4) + r of column l & 15), through every step of the slab.  The two
// forms of csc_bpdn.h fill the map and agree bit for bit.  Slab partials go to global memory in the working
// precision; cmod_pgm_reduce adds them in slab order in double, leaves G and the sums || G ||^2 and, for the
// Barzilai-Borwein rule, <Xprv - Xold, G - Gold>, || G - Gold ||^2 (the rule fixes L before the prox step, so these
// sums belong to the gradient's side).
//
// cmod_pgm_prox: a workgroup owns 16 dictionary columns and all N rows, as cmod_iter does:
//     V = Y - G / L;  X' = Pcn(V)  (revert: X' = Xprv);  Ynext = X' + gamma (ZZ - X') + beta (X' - Xprv)
// with the column mean and norm reduced inside the workgroup in a fixed order (norm 0 -> 1), and the sums of
// pgm_cmod_sums.  F(X') and || G Z ||^2 (Cauchy) come from cmod_dfid of csc_cmod.h, which takes the weight.
// cmod_pgm_yrobust is the Y of the robust backtracking rule, [Z += zc (Xprv - Yprv);] Y = (tk Xprv + t Z) / T.
// Sums are per-workgroup partials in double, reduced by launch_finalize in a fixed order: no floating-point atomics,
// two runs agree bit for bit.
#pragma once

#include "csc_cmod.h"

namespace sporco_amd {

constexpr int kPgmCmodRows = 32;     // rows of N a workgroup of cmod_pgm_grad owns
constexpr int kPgmCmodSums = 12;     // doubles of a row of the handle's partial-sum table (pgm_cmod_sums)
// (the order of bpdn's pgm_bpdn_sums where the meaning is shared; the halves of FY / FX are launch_finalize's scale)
enum pgm_cmod_sums {
    PGMC_FY = 0,     // sum w (Y Z - S)^2                 cmod_pgm_grad
    PGMC_FX,         // sum w (X' Z - S)^2                cmod_dfid
    PGMC_DXG,        // <X' - Y, G>                       cmod_pgm_prox
    PGMC_DXY2,       // || X' - Y ||^2
    PGMC_CNSTR,      // || Pcn(X') - X' ||^2
    PGMC_SPARE0,
    PGMC_RS2,        // || X' - Yprv ||^2 (rs_ynext: || X' - Ynext ||^2)
    PGMC_G2,         // || G ||^2                         cmod_pgm_reduce
    PGMC_GZ2,        // || G Z ||^2 (Cauchy)              cmod_dfid
    PGMC_BBXG,       // <Xprv - Xold, G - Gold>           cmod_pgm_reduce
    PGMC_BBG2,       // || G - Gold ||^2
    PGMC_SPARE1
};

struct PgmCmodPlan {
    int M4, M16, N16, NRB, nsplit, ctw;      // ctw: 16-column tiles of G a wave accumulates (1, 2, 4 or 8)
    int64_t slab;
};
inline PgmCmodPlan pgm_cmod_plan(int N, int M, int64_t K) {
    PgmCmodPlan p;
    p.M4 = bpdn_up(M, 4);
    p.M16 = bpdn_up(M, 16);
    p.N16 = bpdn_up(N, 16);
    p.NRB = (p.N16 + kPgmCmodRows - 1) / kPgmCmodRows;
    p.slab = cmod_slab(K, p.NRB, &p.nsplit);
    const int per_wave = (p.M16 / 16 + 3) / 4;
    p.ctw = per_wave <= 1 ? 1 : per_wave <= 2 ? 2 : per_wave <= 4 ? 4 : 8;
    return p;
}
// workgroups of cmod_pgm_reduce: 256 threads, one per element of the k-major G
inline int pgm_cmod_reduce_blocks(int M, int N16) { return (M * N16 + 255) / 256; }
// cmod_pgm_grad: the Z tile [M16][kCmodLd], the R tile [32][kCmodLd], the block sum
template <typename T> inline size_t pgm_cmod_grad_lds_bytes(int M) {
    return sizeof(T) * (size_t)(bpdn_up(M, 16) + kPgmCmodRows) * kCmodLd + sizeof(double) * 4;
}
// cmod_pgm_prox: the tile of V, then of X' [N][16], 256 doubles of column scratch, the block sums
template <typename T> inline size_t pgm_cmod_prox_lds_bytes(int N) {
    return sizeof(T) * 16 * (size_t)bpdn_up(N, 16) + sizeof(double) * (256 + kPgmCmodSums * 4);
}

template <typename T> struct PgmCmodGradArgs {
    const T *z = nullptr;        // (M, K)
    const T *s = nullptr;        // (N, K)
    const T *w = nullptr;        // (N, K) weight, or nullptr: w_s
    T w_s = T(1);
    const T *yk = nullptr;       // [M4][N16]
    T *part = nullptr;           // [nsplit][M16][N16]
    T *gk = nullptr;             // [M4][N16]  reduce: out; on entry Gold
    const T *xprvk = nullptr, *xoldk = nullptr;      // reduce, bb
    int bb = 0, form = BPDN_FORM_PLAIN;
    int M = 1, N = 1;
    int64_t K = 1;
    PgmCmodPlan p;
    double *partials = nullptr;  // rows of `stride` doubles: grad writes column PGMC_FY, reduce PGMC_G2, _BBXG, _BBG2
    int stride = kPgmCmodSums;
};

template <typename T> struct PgmCmodProxArgs {
    const T *yk = nullptr, *gk = nullptr, *xprvk = nullptr;
    const T *yprvk = nullptr;    // nullptr: Y itself
    const T *zzk_in = nullptr;   // revert: the unreverted X'
    T *xk = nullptr;             // out: X'
    T *ynextk = nullptr;         // out, or nullptr
    T *zzk = nullptr;            // out, or nullptr: X' (not under revert)
    T L = T(1), beta = T(0), gamma = T(0);
    int zero_mean = 0, nonneg = 0, revert = 0;
    int rs_ynext = 0;            // PGMC_RS2 is || X' - Ynext ||^2 (the residual under Monotone, pgm.py:696-702)
    int M = 1, N = 1;
    double *partials = nullptr;  // rows of `stride` doubles: columns PGMC_DXG, _DXY2, _CNSTR, _RS2
    int stride = kPgmCmodSums;
};

// part <- the slab partials of G; partials column PGMC_FY.  Returns the workgroups.
template <typename T> int launch_cmod_pgm_grad(hipStream_t st, const PgmCmodGradArgs<T> &a);
// gk <- the partials added in slab order in double; partials columns PGMC_G2 [, _BBXG, _BBG2].  Returns the workgroups.
template <typename T> int launch_cmod_pgm_reduce(hipStream_t st, const PgmCmodGradArgs<T> &a);
// Returns the workgroups.
template <typename T> int launch_cmod_pgm_prox(hipStream_t st, const PgmCmodProxArgs<T> &a);
// [z += zc (xprv - yprv);]  y = (tk xprv + tt z) / TT over n elements
template <typename T>
void launch_cmod_pgm_yrobust(hipStream_t st, const T *xprv, const T *yprv, T *z, T *y, T tk, T tt, T TT, T zc, int z_update,
                             int n);

}  // namespace sporco_amd
