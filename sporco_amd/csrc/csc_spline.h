// csc_spline.h -- the l1-spline fit, sporco.admm.spline.SplineL1 (sporco/admm/spline.py:24-291),
//     minimise || Wdf (x - s) ||_1 + (lmbda / 2) || D x ||^2      by ADMM on  x - y = s,
// and the orthonormal DCT-II its x step needs (sporco/fft.py:318-372, dctii / idctii), computed through ONE
// real transform of the same size (Makhoul's reordering), never one of twice the length.
//
// The DCT of an (H, W, P) array, planes fastest.  Along an axis of length N the permutation is
//     v[n] = x[2 n], n < ceil(N / 2);    v[N - 1 - n] = x[2 n + 1], n < N / 2,
// applied along both axes.  With Vh = rfft2(v) (H, Wf = W / 2 + 1), w_j[k] = exp(-i pi k / (2 N_j)),
// a = Vh[k1, k2] and b = Vh[(H - k1) mod H, k2]:
//     Xu[k1, k2]     = 2 Re(w1[k1] (w2[k2] a + conj(w2[k2]) conj(b)))
//     Xu[k1, W - k2] = 2 Re(w1[k1] (w2[W - k2] conj(b) + conj(w2[W - k2]) a)),     0 < k2 < W - k2
//     X = Xu s1[k1] s2[k2],   s_j[0] = sqrt(1 / (4 N_j)),  s_j[k > 0] = sqrt(1 / (2 N_j)).
// Inverse, from Xu = X / (s1 s2) with Xu[H, .] = Xu[., W] = 0:
//     Z[k1, k2]  = (1/2) conj(w2[k2]) (Xu[k1, k2] - i Xu[k1, W - k2]),   k1 in [0, H], k2 <= W / 2
//     Vh[k1, k2] = (1/2) conj(w1[k1]) (Z[k1, k2] - i Z[H - k1, k2]),     v = irfft2(Vh).
// A thread owns the pair of stored rows {k1, H - k1} at one k2: it reads two complex values and holds the four
// real coefficients (k1, k2), (k1, W - k2), (H - k1, k2), (H - k1, W - k2) -- every coefficient exactly once;
// the self-paired cases (k1 = 0, 2 k1 = H, k2 = 0, 2 k2 = W) hold fewer.  Twiddles, scales and the eigenvalues
// alpha_j[k] = -2 + 2 cos(pi k / N_j) come from one table per axis (SplTab, formed in double).
//
// One iteration of SplineL1:
//     rfft2(RY - u_scale RU)    the existing transform pair (fft.h); RY = perm(Y + S), RU = perm(U)
//     spl_solve                 in place on the work spectrum: post-twiddle to Zhat, Xhat = Gamma Zhat with
//                               Gamma = 1 / (1 + (lmbda / rho) alpha^2), alpha = alpha_1[k1] + alpha_2[k2], and the
//                               inverse pre-twiddle of Xhat; by Parseval (the transform is orthonormal), on
//                               request: Reg = (1/2) sum (alpha Xhat)^2 and the sums of LinSolveCheck
//     irfft2                    -> XV = perm(X)
//     spl_ystep                 X read at its permuted place, relax, soft threshold, u step, the sums, and RY, RU
//                               of the new Y, U written at their permuted places
// A pending U /= rsf (admm.py:573) is the s2 of the forward transform and the u_scale of the y step, which
// stores the true U.  Sums are per-workgroup partials in double, reduced by launch_finalize in a fixed
// order: no floating-point atomics, two runs agree bit for bit.
#pragma once

#include "csc_kernels.h"

namespace sporco_amd {

constexpr int kSplSolveSums = 4;    // doubles a workgroup of spl_solve leaves
constexpr int kSplYstepSums = 6;    // ... and of spl_ystep
constexpr int kSplMaxBlocks = 1024; // the most workgroups a kernel here is launched with

// entry k of the table of an axis of length N: w[k] = (wr, wi), s[k], alpha[k]
template <typename T> struct alignas(4 * sizeof(T)) SplTab {
    T wr, wi, s, al;
};
template <typename T> void launch_spl_tables(hipStream_t st, int H, int W, SplTab<T> *th, SplTab<T> *tw);

template <typename T> struct SplSolveArgs {
    cx<T> *wf = nullptr;              // (H, Wf, P) half spectrum
    T *xr = nullptr;                  // (H, W, P) real coefficients: dct_post writes them, dct_pre reads them
    const SplTab<T> *th = nullptr, *tw = nullptr;
    int H = 1, W = 1, Wf = 1;
    int64_t P = 1;
    T lr = T(0);                      // lmbda / rho
    int want_reg = 0, want_lsc = 0;
    double *partials = nullptr;       // kSplSolveSums doubles per workgroup (spl_solve)
};
// In place on wf.  partials[0] = sum (alpha Xhat)^2, partials[1..3] = sum (den Xhat - Zhat)^2, (den Xhat)^2,
// Zhat^2 with den = 1 + lr alpha^2 (linalg.rrs).  Returns the workgroups.
template <typename T> int launch_spl_solve(hipStream_t st, const SplSolveArgs<T> &a);
template <typename T> int spl_solve_blocks(const SplSolveArgs<T> &a);
// xr = the orthonormal coefficients of the array whose permuted half spectrum is wf
template <typename T> void launch_dct_post(hipStream_t st, const SplSolveArgs<T> &a);
// wf = the half spectrum whose irfft2 is the permuted inverse DCT of xr
template <typename T> void launch_dct_pre(hipStream_t st, const SplSolveArgs<T> &a);

// dst = perm(src) (inverse: dst = perm^-1(src)) of an (H, W, P) array; src2: dst = perm(src + src2)
template <typename T>
void launch_spl_permute(hipStream_t st, const T *src, const T *src2, T *dst, int H, int W, int64_t P, bool inverse);

template <typename T> struct SplArgs {
    const T *s = nullptr;         // (H, W, P)
    const T *xv = nullptr;        // perm(X), what irfft2 returns
    T *y = nullptr, *u = nullptr;
    T *ry = nullptr, *ru = nullptr;   // perm(Y + S), perm(U)
    const T *wdf = nullptr;       // DFidWeight array of S's shape, or nullptr: wdf_s
    T wdf_s = T(1);
    T rho = T(1), rlx = T(1), u_scale = T(1);
    int geval_y = 1;
    int H = 1, W = 1;
    int64_t P = 1;
    double *partials = nullptr;   // kSplYstepSums doubles per workgroup
};
// partials[0..5] = sum (X - Y' - S)^2, X^2, Y'^2, (Y' - Y)^2, U'^2, |Wdf g|, g = Y' with geval_y, else X - S.
// Writes Y', U', RY, RU.  Returns the workgroups.
template <typename T> int launch_spl_ystep(hipStream_t st, const SplArgs<T> &a);
template <typename T> int spl_ystep_blocks(int H, int W, int64_t P);
// partials[b] = workgroup b's part of sum s^2 over n elements.  Returns the workgroups.
template <typename T> int launch_spl_sumsq(hipStream_t st, const T *s, int64_t n, double *partials);

}  // namespace sporco_amd
