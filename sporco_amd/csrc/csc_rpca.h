// csc_rpca.h -- robust PCA, sporco.admm.rpca RobustPCA (sporco/admm/rpca.py:23-262):
//     minimise || X ||_* + lambda || Y ||_1  such that  X + Y = S
// by ADMM, and the singular value thresholding behind it (sporco.prox prox_nuclear / norm_nuclear).  S, X, Y, U are
// (R, C) row-major as NumPy has them and stay in that layout.  n = min(R, C) <= kRpcaMaxDim is the short axis, L =
// max(R, C) the long one: "tall" (R >= C) has the short axis contiguous, "wide" the long one; element (l, i) of the
// long and the short axis lies at l n + i (tall) or i L + l (wide).
//
// The x step needs no SVD: with V = S - Y - U and G = V^T V (tall) or V V^T (wide) = W diag(sigma^2) W^T,
// prox_nuclear(V, alpha) = V T (tall) or T V (wide), T = W diag(max(0, 1 - alpha / sigma)) W^T.  The device forms
// G, the host T (n x n, float64), the device the rest.
//
// rpca_gram: G reduced over L.  The output is cut into blocks of 64 x 64, the long axis into `nsplit` slabs of `slab`
// positions, a multiple of kRpcaKS.  A workgroup owns one block and one slab: per step of kRpcaKS positions it
// stages its 64 + 64 short-axis lines of V in LDS as doubles, zero padded beyond n and the slab's end; V is formed
// in the working precision while it is staged (rpca_mode) and never stored.  Each wave accumulates a 16 x 64 strip
// as four 16 x 16 tiles in the accumulator map of v_mfma_f64_16x16x4_f64 (lane l: rows (l >> 4) + 4 r of column
// l & 15), FORM_MFMA by that instruction, FORM_PLAIN by a chain of double fused multiply-adds in the same k order.
// Products and sums are double for both dtypes.  The two forms are not promised to agree bit for bit (DESIGN.md
// 4.23).  The symmetry of G is used only where a diagonal block stages its lines once.  Slab partials go to global
// memory; rpca_gram_reduce adds them in slab order.  No floating-point atomics: a repeat is bitwise equal.
//
// rpca_iter: a workgroup takes blocks of KB = 16 or 32 positions of the long axis (bpdn_kb) and all n of the short
// one.  It stages the block of V as bpdn_product's tile [n4][ldb], forms X = T . tile with T as the left operand (T
// is symmetric, so the host's zero padded [n4][n16] array is k-major as it lies), parks X in a second LDS tile and
// then walks the block in memory order: relax, Y' = soft(S - AX - U, lambda / rho), U' = U + AX + Y' - S in the
// reference's arithmetic and order (admm.py relax_AX / ustep with B y = y, c = S), X, Y', U' stored in place and the
// workgroup's sums of rpca_sums left in double.  A workgroup reads only the lines it writes.  `apply` stores
// X = V T alone, with V = S (prox_nuclear).
#pragma once

#include "csc_bpdn.h"

namespace sporco_amd {

constexpr int kRpcaMaxDim = 512;       // the largest short side served (SPORCO_AMD_RPCA_MAX_DIM; bpdn_product's LDS tiles set it)
constexpr int kRpcaKS = 32;            // positions of the long axis staged per step of rpca_gram
constexpr int kRpcaBlk = 64;           // rows and columns of an output block of rpca_gram
constexpr int kRpcaLd = kRpcaKS + 4;   // row pitch of a staged tile, doubles: the 16 rows x 4 k of a matrix-instruction read hit 64 banks twice
constexpr int kRpcaMaxSplits = 512;    // the most slabs of the long axis
constexpr int kRpcaMaxBlocks = 16384;  // the most workgroups of rpca_iter (each loops over its blocks)
constexpr int kRpcaSums = 8;           // doubles a workgroup of rpca_iter leaves (rpca_sums)
enum rpca_sums { RPCA_R2 = 0, RPCA_S2, RPCA_X2, RPCA_Y2, RPCA_U2, RPCA_L1Y, RPCA_L1SX, RPCA_SPARE };
// what rpca_gram takes for V: S - Y - u_scale U (the x step), S - Y (NrmNuc without fEvalX), S (the stateless calls)
enum rpca_mode { RPCA_V_SYU = 0, RPCA_V_SY = 1, RPCA_V_S = 2 };

struct RpcaPlan {
    int n, n4, n16, NB, nsplit, KB, tall, nb_iter;
    int64_t L, slab;
};
template <typename T> inline RpcaPlan rpca_plan(int R, int C) {
    RpcaPlan p;
    p.tall = R >= C ? 1 : 0;
    p.n = p.tall ? C : R;
    p.L = p.tall ? R : C;
    p.n4 = bpdn_up(p.n, 4);
    p.n16 = bpdn_up(p.n, 16);
    p.NB = (p.n16 + kRpcaBlk - 1) / kRpcaBlk;
    // about two workgroups a compute unit of a 256-unit device, at least one step a slab
    int want = (512 + p.NB * p.NB - 1) / (p.NB * p.NB);
    if (want > kRpcaMaxSplits) want = kRpcaMaxSplits;
    int64_t slab = (p.L + want - 1) / want;
    slab = (slab + kRpcaKS - 1) / kRpcaKS * kRpcaKS;
    p.slab = slab;
    p.nsplit = (int)((p.L + slab - 1) / slab);
    p.KB = bpdn_kb<T>(p.n, p.n);
    const int64_t nblk = (p.L + p.KB - 1) / p.KB;
    p.nb_iter = (int)(nblk < kRpcaMaxBlocks ? nblk : kRpcaMaxBlocks);
    return p;
}
inline size_t rpca_gram_lds_bytes() { return sizeof(double) * 2 * kRpcaBlk * kRpcaLd; }
// rpca_iter: the tile of V [n4][ldb], the tile of X [n16][ldb], the block sums
template <typename T> inline size_t rpca_iter_lds_bytes(const RpcaPlan &p) {
    return sizeof(T) * ((size_t)p.n4 + p.n16) * bpdn_ldb(p.KB) + sizeof(double) * kRpcaSums * 4;
}

template <typename T> struct RpcaGramArgs {
    const T *s = nullptr, *y = nullptr, *u = nullptr;     // (R, C)
    T u_scale = T(1);
    int mode = RPCA_V_S, form = BPDN_FORM_PLAIN;
    double *part = nullptr;      // [nsplit][NB 64][NB 64]
    double *g = nullptr;         // (n, n)
    RpcaPlan p;
};

template <typename T> struct RpcaIterArgs {
    const T *s = nullptr;        // (R, C)
    T *x = nullptr, *y = nullptr, *u = nullptr;
    const T *tk = nullptr;       // [n4][n16]  T, zero padded
    T rlx = T(1), thr = T(0), u_scale = T(1);
    int apply = 0, form = BPDN_FORM_PLAIN;
    double *partials = nullptr;  // kRpcaSums doubles per workgroup
    RpcaPlan p;
};

// part <- the slab partials of G.  Returns the workgroups.
template <typename T> int launch_rpca_gram(hipStream_t st, const RpcaGramArgs<T> &a);
// g <- the partials added in slab order
template <typename T> void launch_rpca_gram_reduce(hipStream_t st, const RpcaGramArgs<T> &a);
// Returns the workgroups.
template <typename T> int launch_rpca_iter(hipStream_t st, const RpcaIterArgs<T> &a);
// partials[b] <- the workgroup's share of sum v^2 over `count` elements.  Returns the workgroups (at most 1024).
template <typename T> int launch_rpca_sumsq(hipStream_t st, const T *v, int64_t count, double *partials);

}  // namespace sporco_amd
