// csc_rtv.h -- ConvBPDNRecTV (sporco/admm/cbpdntv.py:733-1356): total variation of the
// reconstruction sum_m d_m * x_m.  The constraint is (I; Gamma_0; Gamma_1) x = (y0; y1) with
// Gamma_i x = G_i sum_m w_m d_m * x_m: Y and U have a coefficient block (K maps per image) and a
// gradient block (two maps per image).
//
// The reference solves the x step by a rank-3 iterated Sherman-Morrison over the rows Df,
// sqrt(rho) Gf_0 (w Df), sqrt(rho) Gf_1 (w Df).  The two gradient rows are collinear per frequency,
// so with GHG = sum_i |Gf_i|^2, tau = rho GHG and B = [Df^T; (w Df)^T] the system is
//     (B^H diag(1, tau) B + rho I) x = rho yu + B^H (Sf; rho zd),
// yu = Yf0 - us Uf0 and zd = Zyf - us Zuf the spectra of the adjoint maps Z = sum_i G_i^T v1_i of
// the gradient blocks.  With x = yu + B^H v this is the 2 x 2 real-matrix system
//     (diag(1, tau) B B^H + rho I) v = (Sf; rho zd) - diag(1, tau) B yu,
// and with equal weights w it collapses to ConvBPDN's rank-one step with the scale
// c = 1 + rho w^2 GHG:  x = yu + conj(Df) (Sf + rho w zd - c Df.yu) / (rho + c sum |Df|^2).
//
// The gradient filters are the two-tap [1, -1] (signal.gradient_filters), so G_i and G_i^T are
// stencils on signal-shaped maps: G_i r = r - roll(r, +1, i), G_i^T v = v - roll(v, -1, i).
//
// Layouts: spectra (npix = H Wf, CN, K) / (npix, CN) as everywhere on the generic chain; spatial
// coefficient arrays (H, W, C, N, K); signal-shaped maps (H, W, C, N); the gradient blocks
// (H, W, C, N, 2), the component fastest (the host's layout of Y[..., M:]).
#pragma once

#include "csc_kernels.h"

namespace sporco_amd {

// rtv_solve: Xf, the weighted reconstruction spectrum Rwf = sum_m w_m Df_m Xf_m, and per-block
// partials (4 doubles): Parseval-weighted |Df.Xf - Sf|^2, then |ax - b|^2, |ax|^2, |b|^2 of
// LinSolveCheck.  Returns the number of blocks (<= kMaxPartialBlocks).
template <typename T> struct RtvSolveArgs {
    const cx<T> *yf = nullptr, *uf = nullptr;     // rfftn(y0), rfftn(u0)      (npix, CN, K)
    cx<T> *xf = nullptr;                          // out                       (npix, CN, K)
    const cx<T> *df = nullptr;                    //                           (npix, K)
    const cx<T> *sf = nullptr;                    //                           (npix, CN)
    const cx<T> *zyf = nullptr, *zuf = nullptr;   // rfftn(sum_i G_i^T y1_i), ... of u1   (npix, CN)
    cx<T> *rwf = nullptr;                         // out                       (npix, CN)
    const T *gram = nullptr;                      // sum_k |Df|^2              (npix)
    const T *tvw = nullptr;                       // TVWeight, K values (0 on a padding filter)
    const T *ghh = nullptr, *ghw = nullptr;       // GHG[h, wf] = ghh[h] + ghw[wf]
    T rho = T(1), us = T(1);                      // us: pending U /= rsf, applied to uf and zuf
    int uniform = 1;                              // every filter has the same weight: the rank-one form
    int64_t npix = 0;
    int CN = 1, K = 1, W = 1;
    int want_obj = 0, want_xrrs = 0;
    double *partials = nullptr;
};
template <typename T> int launch_rtv_solve(hipStream_t st, const RtvSolveArgs<T> &a);

// rtv_ystep: relax_AX (cbpdntv.py:1319-1339), ystep (:1098-1106: prox_l1 on the coefficient block,
// prox_l2 over (channel, gradient component) per pixel on the gradient block), ustep
// (admm.py:434-437) and the sums.  Two launches: a streaming pass over the K-map arrays (x, y0, u0)
// and a pass over the signal-shaped ones (rw, y1, u1), whose partial rows follow the first's.
// partials (8 doubles a row): sum (AXnr - Y)^2, sum AXnr^2, sum Y^2, sum |wl1 g0|, sum sqrt(sum g1^2).
// Returns the number of rows.
template <typename T> struct RtvYArgs {
    const T *x = nullptr;          // X of this iteration            (H, W, C, N, K)
    T *y0 = nullptr, *u0 = nullptr;
    const T *rw = nullptr;         // irfftn(Rwf)                    (H, W, C, N)
    T *y1 = nullptr, *u1 = nullptr;   //                             (H, W, C, N, 2)
    Weight<T> wl1;
    T rlx = T(1), thr_l1 = T(0), thr_tv = T(0), us = T(1);
    bool geval_y = false;
    int H = 1, W = 1, C = 1, N = 1, K = 1;
    double *partials = nullptr;    // 2 * kMaxPartialBlocks rows
};
template <typename T> int launch_rtv_ystep(hipStream_t st, const RtvYArgs<T> &a);

// zy = sum_i G_i^T y1_i, zu = sum_i G_i^T u1_i (value minus its circular successor along axis i):
// a launch of its own, because a pixel needs its neighbours' UPDATED gradient blocks.
template <typename T>
void launch_rtv_adjoint(hipStream_t st, const T *y1, const T *u1, T *zy, T *zu, int H, int W, int CN);

// The residual norms of the general constraint in the frequency domain: with
// A^T v = v0 + Gamma^T v1 and rfftn(Gamma^T v1)_m = conj(w_m Df_m) Zf,
//     partials[0] = sum pw |(Yf0 - Yf0prev)_m + conj(w_m Df_m) (Zyf - Zyfprev)|^2
//     partials[1] = sum pw |Uf0_m + conj(w_m Df_m) Zuf|^2
// with the half-spectrum weights pw of fft.rfl2norm2 (the caller divides by H W).  4 doubles per
// block; returns the number of blocks.
template <typename T> struct RtvDualArgs {
    const cx<T> *yf = nullptr, *yfp = nullptr, *uf = nullptr;        // (npix, CN, K)
    const cx<T> *zyf = nullptr, *zyfp = nullptr, *zuf = nullptr;     // (npix, CN)
    const cx<T> *df = nullptr;
    const T *tvw = nullptr;
    int64_t npix = 0;
    int CN = 1, K = 1, W = 1;
    double *partials = nullptr;
};
template <typename T> int launch_rtv_dual(hipStream_t st, const RtvDualArgs<T> &a);

}  // namespace sporco_amd
