// csc_pd.h -- ConvProdDictBPDN / ConvProdDictBPDNJoint (sporco/admm/pdcsc.py:28-287): sparse coding
// of multi-channel signals with a product dictionary D (x) B, D a single-channel convolutional
// dictionary and B a Cs x Cb standard dictionary over the channel axis:
//     minimise (1/2) || D X B^T - S ||^2 + lambda ||X||_1 (+ mu ||X||_2,1 over the channel axis),
// constraint X = Y.  The coefficient maps have Cb channels, the signal Cs.
//
// With B^T B = Q Gamma Q^T the x step decouples in eigen-channels.  Per frequency pixel p and image
// n, z = rfftn(Y - U), d = Df[p, :], g = sum_m |d_m|^2, sh = Sf (B Q) (Cb values):
//     zh_c' = sum_c Q[c, c'] z_c                                       (K-vectors)
//     b_c'  = conj(d) sh_c' + rho zh_c'
//     xh_c' = (b_c' - conj(d) gamma_c' (d . b_c') / (rho + gamma_c' g)) / rho
//     x_c   = sum_c' Q[c, c'] xh_c'
// (the reference's solvedbi_sm with sqrt(Gamma) folded into the dictionary; a zero eigenvalue gives
// xh = b / rho).  Since d . xh_c' = (d . b_c') / (rho + gamma_c' g), the reconstruction spectrum
// B (d . x) = (B Q) (d . xh) costs no further sum over the filters: the data fidelity
// sum_cs |sum_c' (BQ)[cs, c'] (d . xh_c') - Sf[cs]|^2 is a by-product of the solve.
//
// Layouts: spectra (npix = H Wf, Cb N, K), channel slower than image, as everywhere on the generic
// chain; signal-shaped spectra (npix, Cs N) / (npix, Cb N).  The small tables live in one device
// array `tab` of T: B Q (Cs x Cb, row-major), Q (Cb x Cb), Gamma (Cb), B (Cs x Cb).
#pragma once

#include "csc_kernels.h"

namespace sporco_amd {

constexpr int kPdMaxCb = 16;        // channels of the coefficient maps the kernels serve
constexpr int kPdWaveMaxCb = 8;     // ... with the system held in registers (the wave form)

template <typename T> struct PdTables {
    const T *bq = nullptr, *q = nullptr, *gamma = nullptr, *b = nullptr;
};

// pd_solve: Xf from zf (one read, one write; the two may NOT alias), and per-block partials (4
// doubles): Parseval-weighted |B Df.Xf - Sf|^2, then |ax - b|^2, |ax|^2, |b|^2 of LinSolveCheck in
// eigen-coordinates (Q is orthogonal), ax = gamma conj(d) (d . xh) + rho xh with d . xh summed from
// the xh actually stored.  Returns the number of blocks (<= kMaxPartialBlocks); *wave_form says
// which kernel ran.
template <typename T> struct PdSolveArgs {
    const cx<T> *zf = nullptr;      // rfftn(Y - us U)            (npix, Cb N, K)
    cx<T> *xf = nullptr;            // out                        (npix, Cb N, K)
    const cx<T> *df = nullptr;      //                            (npix, K)
    const cx<T> *shf = nullptr;     // rfftn(S (B Q))             (npix, Cb N)
    const cx<T> *sf = nullptr;      // rfftn(S)                   (npix, Cs N)
    const T *gram = nullptr;        // sum_k |Df|^2               (npix)
    PdTables<T> tab;
    T rho = T(1);
    int64_t npix = 0;
    int Cb = 1, Cs = 1, N = 1, K = 1, W = 1;
    int want_obj = 0, want_xrrs = 0;
    double *partials = nullptr;
};
// K even, K / 2 a power of two <= 64 and Cb <= kPdWaveMaxCb
bool pd_wave_form(int K, int Cb);
template <typename T> int launch_pd_solve(hipStream_t st, const PdSolveArgs<T> &a, bool *wave_form);

// pd_recon: Rf[p, cs, n] = sum_cb B[cs, cb] sum_m Df[p, m] Xf[p, cb, n, m] (rf may be null), and with
// sf the per-block partial (4 doubles a block, the first used) of the Parseval-weighted
// |Rf - Sf|^2.  Returns the number of blocks.
template <typename T> struct PdReconArgs {
    const cx<T> *xf = nullptr;      //                            (npix, Cb N, K)
    const cx<T> *df = nullptr;
    const cx<T> *sf = nullptr;      // null: no residual sum      (npix, Cs N)
    cx<T> *rf = nullptr;            // out, or null               (npix, Cs N)
    PdTables<T> tab;
    int64_t npix = 0;
    int Cb = 1, Cs = 1, N = 1, K = 1, W = 1;
    double *partials = nullptr;
};
template <typename T> int launch_pd_recon(hipStream_t st, const PdReconArgs<T> &a);

}  // namespace sporco_amd
