// csc_bpdn.h -- dense (patch-based) sparse coding, sporco.admm.bpdn BPDN / BPDNJoint / ElasticNet
// (sporco/admm/bpdn.py:24-748):
//     minimise (1/2) || D x - s ||^2 + lmbda || wl1 x ||_1 [+ mu || x ||_{2,1}] [+ (mu/2) || x ||^2]
// by ADMM on x = y, with D (N, M), S (N, K) and X, Y, U (M, K).  Every array is row-major as NumPy has it: the K
// signals are the fastest axis.
//
// The x step is X = P B with B = D^T S + rho (Y - U) and P = (D^T D + c I)^-1, formed by the host.  A workgroup owns
// a block of KB columns (16 or 32, bpdn_kb): it holds the (M, KB) tile of B in LDS, zero padded, and forms the
// (M, KB) tile of X by the one product routine of this file, bpdn_product: OUT (Mo, KB) = A (Mo, Kd) . TILE (Kd, KB),
// A read from global memory in k-major order ([Kd4][Mo16], zero padded by the host side of the handle: Kd4 and Mo16
// are Kd and Mo rounded up to 4 and 16).  A wave takes 16-row slabs of OUT; lane l holds rows 4 (l >> 4) + r, r < 4,
// of column l & 15 of each 16 x 16 tile -- the accumulator map of v_mfma_f32_16x16x4_f32.  Two forms fill it:
//     FORM_MFMA   float32 on the device: the exact f32-input matrix instruction, one per 4 steps of k;
//     FORM_PLAIN  a chain of fused multiply-adds in k order on the same map (float64, the CPU simulator, and
//                 float32 where SPORCO_AMD_BPDN_PLAIN is set when the handle is made).
// Both run k over the padded range, so both are the same fma chain from zero: their results agree bit for bit, and
// since the lane-to-element map is shared every sum that follows does too.
//
// bpdn_iter, one launch per iteration of BPDN and ElasticNet, per column block:
//     B -> LDS; X = P B -> LDS; relax; Y' = soft(AX + U, (lmbda / rho) wl1) [max(., 0)]; U' = U + AX - Y';
//     Y' (fEvalX: X) -> LDS; sum (D . - S)^2 by the product routine; the sums of bpdn_sums below.
// joint form (BPDNJoint): stops after the l1 shrinkage, writes Z and X and per-workgroup row sums of Z^2 (and of
// X^2); bpdn_joint_rows reduces them in a fixed order to the row factors max(0, 1 - (mu / rho) / || Z_m ||);
// bpdn_joint_apply does the rest of the iteration and leaves row sums of Y'^2; bpdn_joint_rows reduces those to
// sum_m || Y'_m ||.  Sums are per-workgroup partials in double, reduced by launch_finalize in a fixed order: no
// floating-point atomics, two runs agree bit for bit.
//
// projection mode (BpdnArgs::proj_l1, BPDNProjL1, sporco/admm/bpdn.py:750-914): the y step is the projection of every
// column of V = AX + U onto the l1 ball of radius gamma, Y' = soft(V, tau_j) with tau_j >= 0 such that
// sum_i max(|v_ij| - tau_j, 0) = gamma (0 where the column lies inside).  V takes the place of B in LDS and the
// thresholds are found there, by the column search of csc_bpdn.hip (bp_col_tau): 256 / KB lanes of one wave own a
// column, sum |v| and count the entries above the current threshold in double, reduce both by xor shuffles in a fixed
// order, and set tau = (sum - gamma) / count until the count comes back unchanged (Michelot's iteration: the active
// set only shrinks, so M + 1 passes bound it; the loop is capped there, and it ends at once on a count of zero,
// which is all a NaN or an infinite threshold leaves).  A wave goes on while any of its columns is unsettled; no
// barrier of the workgroup lies inside the loop.  A second search on the tile of g = Y' (gEvalY off: X) gives
// sum (proj_l1(g) - g)^2, the square of the reference's Cnstr, in the sum slot BPDN_CNSTR.  The thresholds of a block
// pass through the 32 doubles of the reduction scratch, which nothing else uses before the last block is done:
// the mode needs no LDS beyond bpdn_lds_bytes.  bpdn_proj_cols runs the same search on a plain (M, K) array.
#pragma once

#include "csc_kernels.h"

namespace sporco_amd {

constexpr int kBpdnMaxDim = 512;     // the largest M and N served
constexpr int kBpdnMaxBlocks = 1024; // the most workgroups of a kernel here; a workgroup loops over column blocks
constexpr int kBpdnSums = 8;         // doubles a workgroup of bpdn_iter / bpdn_joint_apply leaves (bpdn_sums)
constexpr int kBpdnLscSums = 3;      // ... and of bpdn_lsc
enum bpdn_sums { BPDN_R2 = 0, BPDN_X2, BPDN_Y2, BPDN_S2, BPDN_U2, BPDN_DFID, BPDN_L1, BPDN_SPARE };
constexpr int BPDN_CNSTR = BPDN_SPARE;   // projection mode: sum (proj_l1(g) - g)^2
enum bpdn_form { BPDN_FORM_PLAIN = 0, BPDN_FORM_MFMA = 1 };

inline int bpdn_up(int v, int m) { return (v + m - 1) / m * m; }
// the column block of a problem: 32 while the two LDS tiles stay within 64 KiB, else 16
template <typename T> inline int bpdn_kb(int M, int N) {
    const int R = bpdn_up(M > N ? M : N, 4);
    return (size_t)2 * R * 48 * sizeof(T) <= (size_t)64 * 1024 ? 32 : 16;
}
inline int bpdn_ldb(int KB) { return KB == 32 ? 48 : 16; }      // row pitch of an LDS tile, elements
template <typename T> inline size_t bpdn_lds_bytes(int M, int N) {
    const int R = bpdn_up(M > N ? M : N, 4), KB = bpdn_kb<T>(M, N);
    return (size_t)2 * R * bpdn_ldb(KB) * sizeof(T) + sizeof(double) * kBpdnSums * 4;
}
inline int bpdn_blocks(int64_t K, int KB) {
    const int64_t nb = (K + KB - 1) / KB;
    return (int)(nb < kBpdnMaxBlocks ? nb : kBpdnMaxBlocks);
}

template <typename T> struct BpdnArgs {
    // left operands, k-major and zero padded: pk [M4][M16] = P; dk [N4][M16] = D (for D^T .); dtk [M4][N16] = D^T
    const T *pk = nullptr, *dk = nullptr, *dtk = nullptr;
    const T *s = nullptr;        // (N, K)
    T *dts = nullptr;            // (M, K)  D^T S
    T *x = nullptr, *y = nullptr, *u = nullptr;     // (M, K)
    T *z = nullptr;              // (M, K)  joint: the l1-shrunk array between the two launches
    T *bsave = nullptr;          // (M, K)  LinSolveCheck: the right-hand side of the x step
    const T *wl1 = nullptr;      // (M, K)  L1Weight array, or nullptr: wl1_s
    const T *rowf = nullptr;     // (M)     joint: the row factors
    T wl1_s = T(1);
    T rho = T(1), lr = T(0), rlx = T(1), u_scale = T(1), c = T(1);     // lr = lmbda / rho, c = rho [+ mu]
    int nonneg = 0, feval_x = 0, geval_y = 1, want_x = 1, joint = 0, form = BPDN_FORM_PLAIN;
    int proj_l1 = 0;             // the y step projects onto l1 balls of radius gamma (lr, wl1 and wl1_s are not read)
    double gamma = 0.0;
    int M = 1, N = 1, KB = 16;
    int64_t K = 1;
    double *partials = nullptr;  // kBpdnSums doubles per workgroup
    double *rowp = nullptr;      // joint: [workgroup][M] row sums of Z^2 (iter) / Y'^2 (apply)
    double *rowpx = nullptr;     // joint, gEvalY off: [workgroup][M] row sums of X^2
};

// dts = D^T S.  form as in BpdnArgs.
template <typename T> void launch_bpdn_dts(hipStream_t st, const BpdnArgs<T> &a);
// One iteration (joint: its first half).  Returns the workgroups.
template <typename T> int launch_bpdn_iter(hipStream_t st, const BpdnArgs<T> &a);
// The second half of a joint iteration.  Returns the workgroups.
template <typename T> int launch_bpdn_joint_apply(hipStream_t st, const BpdnArgs<T> &a);
// rowp [nb][M] -> mode 0: rowf[m] = max(0, 1 - mr / sqrt(sum_b rowp[b][m])), 0 at a zero row (prox_l2,
// sporco/prox/_lp.py:284-290); mode 1: out[slot] = sum_m sqrt(sum_b rowp[b][m]).  One workgroup, fixed order.
template <typename T>
void launch_bpdn_joint_rows(hipStream_t st, const double *rowp, int nb, int M, int mode, T mr, T *rowf, double *out,
                            int slot);
// out (M, K) = proj_l1(v (M, K), gamma, axis=0), device arrays, M <= kBpdnMaxDim, by the column search of the
// projection mode on (M, KB) tiles, KB = bpdn_kb<T>(M, 1).  Returns the workgroups.
template <typename T> int launch_bpdn_proj_cols(hipStream_t st, const T *v, T *out, int M, int64_t K, double gamma);
// partials[0..2] = sum (D^T (D X) + c X - B)^2, (...)^2 of the left side, B^2 with B = bsave.  Returns the workgroups.
template <typename T> int launch_bpdn_lsc(hipStream_t st, const BpdnArgs<T> &a);

}  // namespace sporco_amd
