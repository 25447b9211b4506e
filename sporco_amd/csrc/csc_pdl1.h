// csc_pdl1.h -- ConvProdDictL1L1Grd / ConvProdDictL1L1GrdJoint (sporco/admm/pdcsc.py:293-701): the
// product dictionary D (x) B of csc_pd.h under the l1 data fidelity and gradient penalty of csc_l1l1.h,
//     minimise || W (D X B^T - S) ||_1 + lambda ||X||_1 (or ||X||_2,1) + (mu / 2) sum_i ||G_i X||_2^2,
// through the two-block constraint  y0 = D X B^T - S (Cs channels),  y1 = X (Cb channels).
//
// With B^T B = Q Gamma Q^T the x step decouples in eigen-channels.  Per frequency pixel p and image
// n, d = Df[p, :], z0 = rfftn(y0 - u0 + s) (Cs values), z1 = rfftn(y1 - u1) (Cb K-vectors),
// dd_m = 1 + (mu / rho) w_m GHG[p]:
//     b_c'  = conj(d) sum_cs (BQ)[cs, c'] z0_cs + sum_c Q[c, c'] z1_c            (K-vectors)
//     P     = sum_m d_m b_c',m / dd_m,     g = sum_m |d_m|^2 / dd_m
//     xh_c' = b_c' / dd - conj(d) / dd gamma_c' P / (1 + gamma_c' g)
//     x_c   = sum_c' Q[c, c'] xh_c'
// (the reference's solvedbd_sm with sqrt(Gamma) folded into the dictionary; exact for a per-filter
// GradWeight; a zero eigenvalue gives xh = b / dd).  Since d . xh_c' = P / (1 + gamma_c' g), the block-0
// constraint spectrum A0 x = (BQ)(d . xh) is a by-product of the solve.
//
// Layouts as in csc_pd.h: spectra (npix, Cb N, K), signal-shaped spectra (npix, Cs N); tables PdTables.
#pragma once

#include "csc_pd.h"

namespace sporco_amd {

// pdl1_solve: xf and ax0f from z0f and z1f (one read of z1f, one write of xf; the two may NOT alias,
// nor may z0f and ax0f), and per-block partials (4 doubles): the Parseval-weighted sum of
// w_m GHG |xf|^2 (twice RegGrad, with want_obj), then |ax - b|^2, |ax|^2, |b|^2 of LinSolveCheck in
// eigen-coordinates (with want_xrrs), ax = gamma conj(d) (d . xh) + dd xh with d . xh summed from the
// xh actually stored.  Returns the number of blocks (<= kMaxPartialBlocks); *wave_form says which
// kernel ran (pd_wave_form's rule, unless force_generic).
template <typename T> struct Pdl1SolveArgs {
    const cx<T> *z0f = nullptr;     // rfftn(y0 - us u0 + s)      (npix, Cs N)
    const cx<T> *z1f = nullptr;     // rfftn(y1 - us u1)          (npix, Cb N, K)
    cx<T> *xf = nullptr;            // out                        (npix, Cb N, K)
    cx<T> *ax0f = nullptr;          // out                        (npix, Cs N)
    const cx<T> *df = nullptr;      //                            (npix, K)
    GradTerm<T> grad;               // GHG tables, per-filter weights or null; mu holds mu / rho
    PdTables<T> tab;
    int64_t npix = 0;
    int Cb = 1, Cs = 1, N = 1, K = 1, W = 1;
    int want_obj = 0, want_xrrs = 0, force_generic = 0;
    double *partials = nullptr;
};
template <typename T> int launch_pdl1_solve(hipStream_t st, const Pdl1SolveArgs<T> &a, bool *wave_form);

// pdl1_dual: the dual residual norm of these classes (pdcsc.py:568-578), || A^T u ||^2 with
// A^T u = irfftn(B^T conj(Df) rfftn(u0)) + u1, in one read-only pass:
//     partial[0] = sum pw(wf) |conj(Df[pix, k]) sum_cs B[cs, cb] u0f[pix, cs, n] + u1f[pix, cb, n, k]|^2
// with the half-spectrum Parseval weights pw (the caller divides by H W).  2 doubles a block, the
// first used.  Returns the number of blocks.
template <typename T> struct Pdl1DualArgs {
    const cx<T> *df = nullptr;      //                            (npix, K)
    const cx<T> *u0f = nullptr;     //                            (npix, Cs N)
    const cx<T> *u1f = nullptr;     //                            (npix, Cb N, K)
    const T *b = nullptr;           // B                          (Cs, Cb)
    int64_t npix = 0;
    int Cb = 1, Cs = 1, N = 1, K = 1, W = 1;
    double *partials = nullptr;
};
template <typename T> int launch_pdl1_dual(hipStream_t st, const Pdl1DualArgs<T> &a);

}  // namespace sporco_amd
