// csc_l1l1.h -- ConvL1L1Grd (sporco/admm/cbpdn.py:2488-2774): an l1 data fidelity term under a
// mask, an l1 penalty on the coefficient maps and an l2 penalty on their gradient,
//     minimise || W (D x - s) ||_1 + lambda || x ||_1 + (mu / 2) sum_i || G_i x ||_2^2,
// through the two-block constraint [D; I] x - [y0; y1] = [s; 0] of ConvBPDNMaskDcpl.  The x step is
// the gradient-regularised solve of csc_kernels.h with rho = 1 and mu / rho in mu's place, block 1
// the ADMM epilogue (launch_admm_post).  New here: the block-0 step, whose prox is a soft threshold
// by W / rho instead of the parent's division, and this class's own dual residual
//     s = rho || A^T (Yprev - Y) ||,   sn = rho || A^T U ||,   A^T v = irfftn(conj(Df) rfftn(v0)) + v1
// (cbpdn.py:2753-2763), both norms taken in the frequency domain.
#pragma once

#include "csc_kernels.h"

namespace sporco_amd {

// relax_AX / ystep / ustep of block 0 (cbpdn.py:1664-1677, :2716-2724, admm.py:434-437) given
// ax0nr = D x: v = ax + us u0 - s, y0 = sign(v) max(|v| - w / rho, 0) (w = 1 without a mask; w = 0
// passes v through), u0 = us u0 + ax - (y0 + s); dy0 (may be null) receives y0prev - y0.
// partials (5): |ax0nr - y0 - s|^2, |ax0nr|^2, |y0|^2, |u0|^2 (all new values) and sum |w g0| with
// g0 = y0 (geval_y) or ax0nr - s: DFid itself, an l1 sum with no factor 1/2 (:2744-2749).
template <typename T> struct L1Y0Args {
    const T *ax0nr = nullptr;
    T *y0 = nullptr;
    T *u0 = nullptr;
    const T *s = nullptr;
    T *dy0 = nullptr;
    Weight<T> w;
    T rho = T(1), rlx = T(1), us = T(1);
    int geval_y = 0;
    int H = 1, W = 1, C = 1, N = 1;
};
template <typename T> int launch_l1l1_y0step(hipStream_t st, const L1Y0Args<T> &a, double *partials);

// The two dual-residual sums in one read-only pass over four spectra and Df:
//     partial[0] = sum pw(wf) |sum_c conj(Df[pix, c, k]) dy0f[pix, c, cn] + dy1f[pix, cn, k]|^2
//     partial[1] = the same for (u0f, u1f)
// with the half-spectrum Parseval weights pw (the caller divides by H W).  Layouts: df (npix, Cd, K);
// dy0f, u0f (npix, Cd, CN) -- a single-channel dictionary has Cd = 1 here and CN = C N systems a
// pixel, a multi-channel one CN = N; dy1f, u1f (npix, CN, K).  Accumulated in double, nothing
// written but the partials (2 doubles a block).  Returns the number of blocks.
constexpr int kL1MaxCd = 8;        // (the iterated Sherman-Morrison solve's own limit)
template <typename T> struct L1DualArgs {
    const cx<T> *df = nullptr;
    const cx<T> *dy0f = nullptr, *u0f = nullptr;
    const cx<T> *dy1f = nullptr, *u1f = nullptr;
    int64_t npix = 0;
    int Cd = 1, CN = 1, K = 1, W = 1;
    double *partials = nullptr;
};
template <typename T> int launch_l1l1_dual(hipStream_t st, const L1DualArgs<T> &a);

}  // namespace sporco_amd
