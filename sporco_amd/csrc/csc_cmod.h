// csc_cmod.h -- the dictionary update of the dense (patch-based) family, sporco.admm.cmod CnstrMOD
// (sporco/admm/cmod.py:21-342):
//     minimise || D Z - S ||^2  such that  || d_m || = 1 [and mean(d_m) = 0]
// by ADMM on d = g, with Z (M, K), S (N, K) row-major as NumPy has them (the K signals fastest) and the dictionary
// variables X, Y, U (N, M).
//
// cmod_gram: [Z; S] Z^T, reduced over K.  The output is cut into blocks of 64 x 64 (rows: the M16 rows of Z, then
// the N16 rows of S; M16, N16 = M, N rounded up to 16); the K axis into `nsplit` slabs of `slab` columns, a multiple
// of kCmodKS.  A workgroup owns one output block and one slab: per step of kCmodKS columns it stages its 64 rows of
// [Z; S] and its 64 rows of Z in LDS, zero padded beyond M, N and the slab's end, and each wave accumulates a
// 16 x 64 strip as four 16 x 16 tiles in the accumulator map of v_mfma_f32_16x16x4_f32 (lane l: rows 4 (l >> 4) + r
// of column l & 15), through every step of its slab.  The two forms of csc_bpdn.h fill the map, FORM_MFMA and
// FORM_PLAIN; both run k in the same order over the same padded range, so they agree bit for bit.  The symmetry of
// Z Z^T is not used: every block is computed.  Slab partials go to global memory in the working precision;
// cmod_gram_reduce adds them in slab order in double and leaves G = Z Z^T (M, M) and S Z^T (N, M) in double, and
// S Z^T in the working precision in the layout of the iteration.  No floating-point atomics.
//
// The iteration keeps every (N, M) array k-major and zero padded, [M4][N16] with element (n, m) at m N16 + n: the
// order in which bpdn_product (csc_bpdn_product.h) reads a left operand.
//     cmod_rhs   B = S Z^T + rho (Y - u_scale U), elementwise.
//     cmod_iter  a workgroup owns 16 columns of the dictionary and all N rows: X = B Q[:, block] by bpdn_product
//                (the tile is Q's column block, the left operand B), relax, Y' = Pcn(AX + U) with the column mean and
//                norm reduced inside the workgroup in a fixed order, U' = U + AX - Y', and the sums of cmod_sums.
//     cmod_dfid  sum w (F Z - S)^2 over column blocks of K: the left operand is X or Y as stored, the tile a block of Z;
//                the weight w (pgm.cmod, csc_pgm_cmod.h) is 1 unless it is given, and a product by 1 is exact.
// bpdn_product fits both products; B has to lie in global memory for it, which is why cmod_rhs is a launch of its own.
#pragma once

#include "csc_bpdn.h"

namespace sporco_amd {

constexpr int kCmodMaxDim = 512;       // the largest M and N served (SPORCO_AMD_CMOD_MAX_DIM; bpdn_product's LDS tiles set it)
constexpr int kCmodKS = 32;            // columns of K staged per step
constexpr int kCmodBlk = 64;           // rows and columns of an output block of cmod_gram
constexpr int kCmodLd = kCmodKS + 4;   // row pitch of a staged tile: the 16 rows x 4 k of a matrix-instruction read hit 64 banks
constexpr int kCmodMaxSplits = 512;    // the most slabs of K
constexpr int kCmodSums = 8;           // doubles a workgroup of cmod_iter leaves (cmod_sums)
enum cmod_sums { CMOD_R2 = 0, CMOD_X2, CMOD_Y2, CMOD_S2, CMOD_U2, CMOD_CNSTR, CMOD_SPARE0, CMOD_SPARE1 };

struct CmodPlan {
    int M16, N16, M4, RB, CB, nsplit;
    int64_t slab;
};
// the slab rule: `blocks` workgroups share a slab of K; about two workgroups a compute unit of a 256-unit device, at
// least one step a slab.  Returns the columns of a slab, a multiple of kCmodKS; *nsplit: the slabs.
inline int64_t cmod_slab(int64_t K, int blocks, int *nsplit) {
    int want = (512 + blocks - 1) / blocks;
    if (want > kCmodMaxSplits) want = kCmodMaxSplits;
    int64_t slab = (K + want - 1) / want;
    slab = (slab + kCmodKS - 1) / kCmodKS * kCmodKS;
    *nsplit = (int)((K + slab - 1) / slab);
    return slab;
}
inline CmodPlan cmod_plan(int N, int M, int64_t K) {
    CmodPlan p;
    p.M16 = bpdn_up(M, 16);
    p.N16 = bpdn_up(N, 16);
    p.M4 = bpdn_up(M, 4);
    p.RB = (p.M16 + p.N16 + kCmodBlk - 1) / kCmodBlk;
    p.CB = (p.M16 + kCmodBlk - 1) / kCmodBlk;
    p.slab = cmod_slab(K, p.RB * p.CB, &p.nsplit);
    return p;
}
template <typename T> inline size_t cmod_gram_lds_bytes() { return sizeof(T) * 2 * kCmodBlk * kCmodLd; }
// cmod_iter: the tile of Q (later of AX + U), the tile of X, 256 doubles of column scratch, the block sums
template <typename T> inline size_t cmod_iter_lds_bytes(int N, int M) {
    const int M4 = bpdn_up(M, 4), N16 = bpdn_up(N, 16);
    const int R = M4 > N16 ? M4 : N16;
    return sizeof(T) * 16 * ((size_t)R + N16) + sizeof(double) * (256 + kCmodSums * 4);
}

template <typename T> struct CmodGramArgs {
    const T *z = nullptr;        // (M, K)
    const T *s = nullptr;        // (N, K)
    T *part = nullptr;           // [nsplit][RB 64][CB 64]
    double *g = nullptr;         // (M, M)
    double *sztd = nullptr;      // (N, M)
    T *sztk = nullptr;           // [M4][N16]
    int M = 1, N = 1, form = BPDN_FORM_PLAIN;
    int64_t K = 1;
    CmodPlan p;
};

template <typename T> struct CmodArgs {
    const T *q = nullptr;        // (M, M) row-major
    const T *sztk = nullptr;
    T *bk = nullptr, *xk = nullptr, *yk = nullptr, *uk = nullptr;      // [M4][N16]
    T rho = T(1), rlx = T(1), u_scale = T(1);
    int zero_mean = 0, geval_y = 1, form = BPDN_FORM_PLAIN;
    int M = 1, N = 1;
    double *partials = nullptr;  // kCmodSums doubles per workgroup
};

template <typename T> struct CmodDfidArgs {
    const T *fk = nullptr;       // [M4][N16]  the dictionary variable
    const T *z = nullptr, *s = nullptr;       // s == nullptr: S = 0, the sum is || F Z ||^2
    const T *w = nullptr;        // (N, K) weight that multiplies (F Z - S)^2, or nullptr: w_s
    T w_s = T(1);
    int M = 1, N = 1, KB = 16, form = BPDN_FORM_PLAIN;
    int64_t K = 1;
    double *partials = nullptr;  // one double per workgroup, `stride` doubles apart
    int stride = 1;
};

// part <- the slab partials of [Z; S] Z^T.  Returns the workgroups.
template <typename T> int launch_cmod_gram(hipStream_t st, const CmodGramArgs<T> &a);
// g, sztd, sztk <- the partials added in slab order in double
template <typename T> void launch_cmod_gram_reduce(hipStream_t st, const CmodGramArgs<T> &a);
template <typename T> void launch_cmod_rhs(hipStream_t st, const CmodArgs<T> &a);
// Returns the workgroups.
template <typename T> int launch_cmod_iter(hipStream_t st, const CmodArgs<T> &a);
template <typename T> int launch_cmod_dfid(hipStream_t st, const CmodDfidArgs<T> &a);

}  // namespace sporco_amd
