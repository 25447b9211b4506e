// csc_tvd.h -- l2-TV denoising, sporco.admm.tvl2.TVL2Denoise (sporco/admm/tvl2.py:27-372),
//     minimise (1/2) || Wdf (x - s) ||^2 + lmbda || Wtv sqrt((G_0 x)^2 + (G_1 x)^2) ||_1,
// by ADMM on the constraint (G_0; G_1) x = (y_0; y_1).  Nothing in it is a transform: G_i is the forward
// difference along axis i whose last row is zero (sporco/signal.py:115-200, not circular),
//     (G_i x)[j]   = x[j + 1] - x[j]  (j < n - 1),   0  (j = n - 1)
//     (G_i^T v)[j] = v[j - 1] - v[j]  with v[-1] = 0 and v[n - 1] taken as 0,
// and every step is a nearest-neighbour stencil in the spatial domain.
//
// Layout: S, X, P, Q and the weights are C-ordered (H, W, P) arrays, P the product of the trailing
// (channel / image) axes; a W-neighbour is P elements away, an H-neighbour L = W P.  The two blocks of Y
// (and of U, and of dY = Y - Yprev) lie one after the other in one allocation: block b starts at b * E,
// E = H W P.  A row of the image is L contiguous elements and is cut into items:
//     planes independent (caxis=None): V consecutive elements of the row, one 16- or 8-byte access where
//         L allows it (for P = 1 they are V neighbouring pixels), each element its own l2 norm;
//     vector TV (caxis=2, P = C N):    the C channels of one (column, image) pair, N elements apart,
//         the l2 norm of the y step over the 2 C values.
// A workgroup owns a strip of 256 items and walks down the rows of a row segment; a thread owns the same
// item in every row and carries what the stencil needs from the rows above and below in registers, so
// every array is read once, plus one or two halo rows per segment; the W-neighbours are second loads of
// lines the workgroup reads anyway.
//
// One iteration (MaxGSIter = 2): tvd_sweep, tvd_sweep, tvd_ystep, tvd_adjoint.
//     tvd_sweep    one Jacobi sweep of the x step (tvl2.py:362-371; the reference calls it Gauss-Seidel,
//                  but a sweep reads only the previous X), X ping-pongs between two buffers
//     tvd_ystep    relax_AX + ystep + ustep (admm.py:396-437, tvl2.py:258-265), writes Y, U and
//                  dY = Y - Yprev, and forms every sum of the iteration that needs X: the residual norms,
//                  DFid, RegTV and the three norms of GSRelRes -- its rows already hold X's neighbours
//     tvd_adjoint  PD = A^T (Y - U), Q = A^T U, and || A^T dY ||^2, || Q ||^2 of the dual residual.  dY is
//                  differenced BEFORE the stencil: A^T Y - A^T Yprev cancels in float32 late in a run.
// A pending U /= rsf (admm.py:573) rides along as u_scale: the sweeps use PD + (1 - u_scale) Q, the y
// step reads u_scale U and stores the true U.
// Sums are per-workgroup partials in double (block_sum_store), reduced by launch_finalize in a fixed
// order: no floating-point atomics, two runs agree bit for bit.
#pragma once

#include "csc_kernels.h"

namespace sporco_amd {

constexpr int kTvdThreads = 256;   // items of a strip
constexpr int kTvdMinRows = 8;     // rows of a segment at least (each segment re-reads up to two halo rows)
constexpr int kTvdMaxChannels = 8;    // vector TV: channels of an item (its row state lives in registers)
constexpr int kTvdSums = 8;        // doubles a workgroup leaves per launch

// How (H, W, P) is cut into items, strips and row segments.
struct TvdPlan {
    int H = 1, W = 1;
    int64_t P = 1, L = 1;   // planes, elements of a row
    int vtv = 0;            // vector TV: item = the C channels of one (column, image) pair
    int C = 1, N = 1;       // vtv: P = C N
    int G = 1;              // elements of an item the kernel is built for: V, or 4 / 8 >= C
    int cnt = 1;            // elements of an item: V, or C
    int64_t estr = 1;       // distance between them: 1, or N
    int64_t items = 1;      // items per row: L / V, or W N
    int strips = 1;         // ceil(items / 256)
    int rows = 1, nseg = 1; // rows per segment (R), segments
    int64_t blocks() const { return (int64_t)strips * nseg; }
};
TvdPlan tvd_plan(size_t elem_size, int H, int W, int64_t P, int C, bool vtv);

template <typename T> struct TvdArgs {
    const T *s = nullptr;      // the signal
    const T *xin = nullptr;    // X (the sweep's source)
    T *xout = nullptr;         // tvd_sweep: the new X
    T *y = nullptr, *u = nullptr, *dy = nullptr;   // two blocks each (tvl1_*: three of y and u, no dy)
    T *pd = nullptr, *q = nullptr;                 // A^T (Y - U), A^T U
    const T *wdf = nullptr;    // DFidWeight array of S's shape, or nullptr: wdf_s
    const T *wtv = nullptr;    // TVWeight array of S's shape, or nullptr: wtv_s
    T wdf_s = T(1), wtv_s = T(1);
    T rho = T(1), thr = T(0);  // thr = lmbda / rho
    T rlx = T(1), u_scale = T(1);
    int geval_y = 1;
    double *partials = nullptr;   // kTvdSums doubles per workgroup
};

// X_out = (rho (Xss + P) + Wdf^2 S) / (Wdf^2 + rho lcw), Xss the sum of the four neighbours of X_in with
// zeros outside the image, lcw their number.
template <typename T> void launch_tvd_sweep(hipStream_t st, const TvdArgs<T> &a, const TvdPlan &pl);
// partials[0..7] = sum (AXnr - Y)^2, sum AXnr^2, sum Y^2, sum (Wdf (X - S))^2, sum Wtv sqrt(sum g^2),
// and |ax - b|^2, |ax|^2, |b|^2 of linalg.rrs(rho A^T A X + Wdf^2 X, Wdf^2 S + rho P) (tvl2.py:248-251).
// res_only: only the last three, nothing written (the per-sweep test of GSTol > 0).
template <typename T> void launch_tvd_ystep(hipStream_t st, const TvdArgs<T> &a, const TvdPlan &pl, bool res_only);
// partials[0..1] = sum (A^T dY)^2, sum (A^T U)^2.
template <typename T> void launch_tvd_adjoint(hipStream_t st, const TvdArgs<T> &a, const TvdPlan &pl);

// l1-TV denoising, sporco.admm.tvl1.TVL1Denoise (sporco/admm/tvl1.py:27-399),
//     minimise || Wdf (x - s) ||_1 + lmbda || Wtv sqrt((G_0 x)^2 + (G_1 x)^2) ||_1,
// by ADMM on (G_0; G_1; I) x - (y_0; y_1; y_d) = (0; 0; s): the same items, strips and segments, a third
// (data) block of Y and U at 2 E, and no dY -- the dual residual is rho || A^T U || (tvl1.py:362-372).
// One iteration (MaxGSIter = 2): tvd_sweep, tvd_sweep, tvl1_ystep, tvl1_adjoint.  The x step
// (tvl1.py:240-260) is GaussSeidelStep with rho = 1, W2 = 1 on S + (Y_d - U_d) and G^T (Y_g - U_g): with
// PD = A^T (Y - U) = G^T (Y_g - U_g) + (Y_d - U_d) and Q = A^T U = G^T U_g + U_d including the identity
// block it is tvd_sweep as it stands, called with rho = 1, wdf = nullptr, wdf_s = 1.
//
// partials[0..7] = sum (AXnr - Y - c)^2, sum AXnr^2, sum Y^2 over the three blocks (AXnr = (G X; X),
// c = (0; 0; S)), sum |Wdf g_d|, sum Wtv sqrt(sum g_g^2) (g = Y with geval_y, else (G X; X - S)), and
// |ax - b|^2, |ax|^2, |b|^2 of linalg.rrs(G^T G X + X, P + S) (tvl1.py:254-257).  The y step of the data
// block is prox_l1(AX_d + U_d - S, Wdf / rho): Wdf enters linearly, a zero weight leaves the value as it is.
// res_only: only the last three, nothing written.
template <typename T> void launch_tvl1_ystep(hipStream_t st, const TvdArgs<T> &a, const TvdPlan &pl, bool res_only);
// PD, Q with the identity block; partials[0..1] = sum (A^T U)^2, sum U^2 over the three blocks.
template <typename T> void launch_tvl1_adjoint(hipStream_t st, const TvdArgs<T> &a, const TvdPlan &pl);
// partials[b] = the part of sum s^2 of workgroup b, b < pl.blocks() (|| c ||^2 of the primal normaliser,
// formed once when S is set)
template <typename T> void launch_tvl1_s2(hipStream_t st, const T *s, const TvdPlan &pl, double *partials);

// out = x * y, elementwise (DeviceArray * DeviceArray)
template <typename T> void launch_tvd_mul(hipStream_t st, const T *x, const T *y, T *out, int64_t n);

}  // namespace sporco_amd
