// csc_tv.h -- the y / u steps and the constraint adjoint of ConvBPDNScalarTV / ConvBPDNVectorTV
// (sporco/admm/cbpdntv.py:31-727) as two streaming kernels.
//
// The constraint is (Gamma_0; Gamma_1; I) x = (y_0; y_1; y_L): Y and U have three blocks.  The
// reference applies G_i and G_i^T through six FFT round trips per iteration; its gradient filters
// are the two-tap [1, -1] (signal.gradient_filters), so
//     G_i x   = x - roll(x, +1, axis i)        (x minus its predecessor along i, circular)
//     G_i^T v = v - roll(v, -1, axis i)        (v minus its successor along i, circular)
// and everything here is a stencil in the spatial domain.
//
// Layout: each block is an array (H, W, C, N, K) with the filter index fastest, the three blocks of
// Y (and of U) one after the other in one allocation: block b starts at b * E.  An x-neighbour is
// C N K elements away, a y-neighbour W C N K.  One workgroup owns a strip of TW columns of one
// image (c, n) with all K filters and walks down the rows of a row segment; a thread owns the same
// (column, filters) items in every row and carries what the stencil needs from the neighbouring
// row in registers -- the previous row of X (tv_ystep), the current row of Y_0 and U_0 while the
// next one is loaded (tv_adjoint) -- so every array is read once, plus one row per segment; the
// x-neighbour is a second load of a line the workgroup reads anyway (one halo column per strip).
// Accesses along K are 16 bytes wide when K is a multiple of 4 (float32) / 2 (float64).
#pragma once

#include "csc_kernels.h"

namespace sporco_amd {

template <typename T> struct TvArgs {
    const T *x = nullptr;     // X of this iteration (tv_ystep)
    T *y = nullptr;           // the three blocks of Y: (y_0, y_1, y_L), block b at y + b * E
    T *u = nullptr;           // ... and of U
    T *p = nullptr;           // P = A^T Y (tv_adjoint; the x step's "Y")
    T *q = nullptr;           // Q = A^T U (the x step's "U")
    const T *tvw = nullptr;   // Wtv, K values (TVWeight; 0 on a padding filter)
    Weight<T> wl1;            // L1Weight
    T rlx = T(1);             // RelaxParam
    T thr_l1 = T(0);          // lmbda / rho (times a scalar L1Weight)
    T thr_tv = T(0);          // mu / rho
    T u_scale = T(1);         // pending U /= rsf (admm.py:573), applied to U as it is read
    bool vector_tv = false;   // the l2 norm of the y step runs over the two components and the K filters of a
                              // pixel (cbpdntv.py:712); else over the whole array of gradient blocks (:319)
    bool norm_pass = false;   // scalar TV, first launch: partials[0] = sum ((AX + U)_{0,1})^2, nothing written
    const double *gn2 = nullptr;   // scalar TV, second launch: that sum
    bool geval_y = false;     // regulariser sums at Y (else at AXnr)
    int H = 1, W = 1, C = 1, N = 1, K = 1;
    double *partials = nullptr;   // 8 doubles per workgroup
};

// Strip width, row segments and item split of a launch.
struct TvPlan {
    int vec = 1;      // elements per access along K (16 bytes when K allows it)
    int kv = 1;       // items (accesses) per pixel: K / vec
    int TW = 1;       // columns of a strip
    int rows = 1, nseg = 1;
    int64_t blocks = 0;
};
template <typename T> TvPlan tv_plan(int H, int W, int CN, int K);

// relax_AX + ystep + ustep (cbpdntv.py:542-559, :314-321 / :707-715, admm.py:434-437) and the sums
// (scalar TV: two launches, norm_pass first -- the reference's prox_l2 call has no axis argument there,
// so one shrink factor serves the whole array and its norm has to be known before anything is written)
// partials[0..4] = sum (AXnr - Y)^2, sum AXnr^2, sum Y^2, sum |wl1 g_L|, sum sqrt(sum g_{0,1}^2).
// Returns the number of workgroups.
template <typename T> int64_t launch_tv_ystep(hipStream_t st, const TvArgs<T> &a, const TvPlan &pl);

// p = A^T Y, q = u_scale A^T U (cbpdntv.py:470-520) and partials[0..1] = sum (p - P_old)^2, sum q^2.
template <typename T> int64_t launch_tv_adjoint(hipStream_t st, const TvArgs<T> &a, const TvPlan &pl);

// The x step as the reference computes it when TVWeight holds DIFFERENT weights per filter: it hands
// the diagonal dd_k = rho Wtv_k^2 GHGf + rho to linalg.solvedbi_sm (cbpdntv.py:290-292,
// linalg.py:232-297), whose formula
//     x = (b - conj(Df) <c, b>) / dd,   c = Df / (<Df, conj Df> + dd),   b = conj(Df) Sf + rho yuf
// solves (Df^H Df + diag(dd)) x = b only for a diagonal that is constant along the filter axis.  The
// classes reproduce the reference (its fixtures), so this form exists; with equal weights the system
// is ConvBPDNGradReg's and runs on that class's kernels.  In place on the spectrum (npix, CN, K) in the
// natural layout; partials (4 per block): Parseval-weighted |Df.xf - Sf|^2, then |ax - b|^2, |ax|^2,
// |b|^2 of LinSolveCheck (:300-308).  Returns the number of blocks (<= kMaxPartialBlocks).
template <typename T> struct TvSmArgs {
    cx<T> *xf = nullptr;          // in: rfftn(A^T (Y - U)), out: Xf
    const cx<T> *df = nullptr, *sf = nullptr;
    GradTerm<T> g;                // mu = rho, wg = Wtv^2
    T rho = T(1);
    int64_t npix = 0;
    int CN = 1, K = 1, W = 1;
    int want_obj = 0, want_xrrs = 0;
    double *partials = nullptr;
};
template <typename T> int launch_tv_sm_ref(hipStream_t st, const TvSmArgs<T> &a);

}  // namespace sporco_amd
