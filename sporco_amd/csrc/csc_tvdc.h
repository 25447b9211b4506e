// csc_tvdc.h -- TV deconvolution, sporco.admm.tvl2.TVL2Deconv (sporco/admm/tvl2.py:377-702) and
// sporco.admm.tvl1.TVL1Deconv (sporco/admm/tvl1.py:403-758),
//     l2:  minimise (1/2) || H x - s ||^2   + lmbda || Wtv sqrt((G_0 x)^2 + (G_1 x)^2) ||_1
//     l1:  minimise || Wdf (H x - s) ||_1   + lmbda || Wtv sqrt((G_0 x)^2 + (G_1 x)^2) ||_1,
// H the circular convolution with a kernel A, by ADMM on (G_0; G_1) x = y (l2) or on
// (G_0; G_1; H) x - y = (0; 0; s) (l1).  The gradients are CIRCULAR here (sporco/signal.py:204-240 puts
// [1, -1] on each axis), unlike the Denoise classes of csc_tvd.h:
//     (G_i x)[j] = x[j] - x[j - 1],    (G_i^T v)[j] = v[j] - v[j + 1],    indices modulo the axis length,
// so they are nearest-neighbour stencils in the spatial domain and only H needs a transform.
//
// Layout: as csc_tvd.h -- S, the weights and the blocks of Y, U, dY are C-ordered (H, W, P) arrays, block b
// at b * E, E = H W P, cut into items, strips and row segments by the same TvdPlan.  The arrays that pass
// through a transform hold NZ planes per image plane side by side, NZ = 1 (l2) or 2 (l1): they are
// (H, W, NZ, P) and a W-neighbour is xs = NZ P elements away.  Those are
//     XH   l2: X;   l1: (X, H X), what one irfft2 over 2 P planes returns
//     RY   l2: G^T Y_g;   l1: (G^T Y_g, Y_d)
//     RU   the same of U.
//
// One iteration:
//     rfft2(RY - u_scale RU)   the existing transform pair (fft.h), NZ P planes
//     tvdc_solve               pointwise over the half spectrum, in place:
//                                l2: Xf = (AHSf + rho Zf) / (|Af|^2 + rho GHGf)
//                                l1: Xf = (AHSf + Zf_0 + conj(Af) Zf_1) / (|Af|^2 + GHGf), and Af Xf next to it
//                              GHGf = ch[k] + cw[l] from two cosine tables; by-products on request: the
//                              Parseval-weighted sum of |Af Xf - Sf|^2 and the sums of LinSolveCheck
//     irfft2                   NZ P planes -> XH
//     tvdc_ystep               the periodic gradient of X by stencil, relax, l2 shrinkage of the gradient
//                              blocks (l1: soft threshold of the data block), u step and the sums
//     tvdc_adjoint             RY, RU of the new Y, U and, l2, || G^T (Y - Yprev) ||^2, || G^T U ||^2
//     l1, when residuals are wanted: rfft2(RU), tvdc_dual -- || F(G^T U_g) + conj(Af) F(U_d) ||^2 by Parseval
// A pending U /= rsf (admm.py:573) is the s2 of the forward transform and the u_scale of the y step; the
// y step stores the true U.  Sums are per-workgroup partials in double, reduced by launch_finalize in a
// fixed order: no floating-point atomics, two runs agree bit for bit.
#pragma once

#include "csc_tvd.h"

namespace sporco_amd {

constexpr int kTvdcSolveSums = 4;   // doubles a workgroup of tvdc_solve leaves

template <typename T> struct TvdcArgs {
    const T *s = nullptr;       // the signal (l1)
    const T *xh = nullptr;      // XH
    T *y = nullptr, *u = nullptr;   // two (l1: three) blocks each
    T *dy = nullptr;            // l2: Y - Yprev, two blocks; nullptr: not wanted
    T *ry = nullptr, *ru = nullptr;
    const T *wdf = nullptr;     // l1: DFidWeight array of S's shape, or nullptr: wdf_s
    const T *wtv = nullptr;     // TVWeight array of S's shape, or nullptr: wtv_s
    T wdf_s = T(1), wtv_s = T(1);
    T rho = T(1), thr = T(0);   // thr = lmbda / rho
    T rlx = T(1), u_scale = T(1);
    int geval_y = 1;
    double *partials = nullptr;   // kTvdSums doubles per workgroup
};

// partials[0..5] = sum (AXnr - Y - c)^2, sum AXnr^2, sum Y^2, sum Wtv sqrt(sum g_g^2), sum U^2, (l1) sum
// |Wdf g_d| -- over the two (three) blocks, AXnr = (G X; H X), c = (0; 0; S), g = Y with geval_y, else
// AXnr - c.  Writes Y, U and, where a.dy is set, dY.
template <typename T> void launch_tvdc_ystep(hipStream_t st, const TvdcArgs<T> &a, const TvdPlan &pl, bool l1);
// RY, RU from Y, U; l2: partials[0..1] = sum (G^T dY)^2 (0 without a.dy), sum (G^T U)^2.
template <typename T> void launch_tvdc_adjoint(hipStream_t st, const TvdcArgs<T> &a, const TvdPlan &pl, bool l1);

template <typename T> struct TvdcSolveArgs {
    cx<T> *wf = nullptr;            // (H, Wf, NZ, P): the transformed right-hand side in, Xf (l1: Xf, Af Xf) out
    const cx<T> *ahsf = nullptr;    // (H, Wf, P)
    const cx<T> *sf = nullptr;      // (H, Wf, P)
    const cx<T> *af = nullptr;      // (H, Wf, PA), PA = P or 1
    const T *aha = nullptr;         // (H, Wf, PA)  |Af|^2
    const T *ch = nullptr, *cw = nullptr;   // 2 - 2 cos(2 pi k / H), k < H;  2 - 2 cos(2 pi l / W), l < Wf
    int H = 1, W = 1, Wf = 1;
    int64_t P = 1, PA = 1;
    T rho = T(1);
    int want_dfid = 0, want_lsc = 0;
    double *partials = nullptr;     // kTvdcSolveSums doubles per workgroup
};
// partials[0] = Parseval-weighted sum of |Af Xf - Sf|^2 (DC column 1, Nyquist column 1 for even W, else 2),
// partials[1..3] = sum |ax - b|^2, |ax|^2, |b|^2 of linalg.rrs over the half spectrum.  Returns the workgroups.
template <typename T> int launch_tvdc_solve(hipStream_t st, const TvdcSolveArgs<T> &a, bool l1);
template <typename T> int tvdc_solve_blocks(const TvdcSolveArgs<T> &a);
// l1: partials[b] = workgroup b's part of the Parseval-weighted sum of |wf_0 + conj(Af) wf_1|^2.
template <typename T> int launch_tvdc_dual(hipStream_t st, const TvdcSolveArgs<T> &a);
// aha = |af|^2 (when set), ahsf = conj(af) sf (when set)
template <typename T> void launch_tvdc_setup(hipStream_t st, const TvdcSolveArgs<T> &a, T *aha, cx<T> *ahsf);
// ch[k] = 2 - 2 cos(2 pi k / H), k < H;  cw[l] = 2 - 2 cos(2 pi l / W), l <= W / 2
template <typename T> void launch_tvdc_tables(hipStream_t st, int H, int W, T *ch, T *cw);

}  // namespace sporco_amd
