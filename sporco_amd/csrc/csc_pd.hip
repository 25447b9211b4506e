// csc_pd.hip -- the kernels of ConvProdDictBPDN / ConvProdDictBPDNJoint (csc_pd.h): pd_solve, the
// eigen-channel rank-one x step in the frequency domain, and pd_recon, the reconstruction spectrum
// through B.  float32 / float64, any H, W, N, K, Cs; Cb <= kPdMaxCb.
#include "csc_pd.h"
#include "csc_kernels_dev.h"

#include <algorithm>

namespace sporco_amd {

namespace {

constexpr int kPdScratch = 4 * (kThreads / kWave);   // doubles of LDS for block_sum_store<4>

// acc + s v
template <typename T> __device__ __forceinline__ cx<T> pd_axpy(cx<T> acc, T s, cx<T> v) {
    return mk<T>(fma1(s, v.re, acc.re), fma1(s, v.im, acc.im));
}

// Parseval-weighted |sum_c' (BQ)[cs, c'] dxh_c' - Sf[cs]|^2 over the Cs signal channels of a system
template <typename T>
__device__ __forceinline__ double pd_fidelity(const cx<T> *dxh, const T *bq, const cx<T> *sf, int64_t pix, int n,
                                              int Cb, int Cs, int N, int Wf, int W) {
    double s = 0.0;
    for (int cs = 0; cs < Cs; ++cs) {
        cx<T> r = mk<T>(T(0), T(0));
        for (int c = 0; c < Cb; ++c) r = pd_axpy(r, bq[cs * Cb + c], dxh[c]);
        s += (double)cabs2(r - sf[(pix * Cs + cs) * N + n]);
    }
    return parseval_weight((int)(pix % Wf), Wf, W) * s;
}

// K even and G = K / 2 a power of two <= 64, CB <= kPdWaveMaxCb: a lane owns two adjacent filters of
// all CB channels, G lanes a (pixel, image) system, the sums over the filters are wave shuffles (the
// lane layout of csc_rtv.hip rtv_solve_wave_kernel).  Q and Gamma are staged once in LDS.
template <typename T, int CB> __global__ void __launch_bounds__(kThreads) pd_solve_wave_kernel(const PdSolveArgs<T> a) {
    const int G = a.K >> 1, Wf = a.W / 2 + 1;
    const int64_t total = a.npix * a.N * G;
    const int64_t total_pad = (total + kWave - 1) / kWave * kWave;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    T *const q = reinterpret_cast<T *>(dyn_lds<double>() + kPdScratch);     // CB CB, then Gamma
    T *const gam = q + CB * CB;
    for (int i = threadIdx.x; i < CB * CB + CB; i += blockDim.x) q[i] = i < CB * CB ? a.tab.q[i] : a.tab.gamma[i - CB * CB];
    __syncthreads();
    const T rho = a.rho, irho = T(1) / a.rho;
    const cx<T> zero = mk<T>(T(0), T(0));
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total_pad;
         t += (int64_t)gridDim.x * blockDim.x) {
        const bool valid = t < total;
        const int64_t sys = t / G;
        const int lg = (int)(t - sys * G);
        const int64_t pix = sys / a.N;
        const int n = (int)(sys - pix * a.N);
        cxpair<T> z[CB], d;
        d.a = d.b = zero;
        T g = T(0);
#pragma unroll
        for (int c = 0; c < CB; ++c) z[c].a = z[c].b = zero;
        if (valid) {
#pragma unroll
            for (int c = 0; c < CB; ++c)
                z[c] = *reinterpret_cast<const cxpair<T> *>(a.zf + ((pix * CB + c) * a.N + n) * a.K + 2 * lg);
            d = *reinterpret_cast<const cxpair<T> *>(a.df + pix * a.K + 2 * lg);
            g = a.gram[pix];
        }
        // zh_c' = sum_c Q[c, c'] z_c
        cxpair<T> xh[CB];
#pragma unroll
        for (int cp = 0; cp < CB; ++cp) {
            cxpair<T> s;
            s.a = s.b = zero;
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                s.a = pd_axpy(s.a, q[c * CB + cp], z[c].a);
                s.b = pd_axpy(s.b, q[c * CB + cp], z[c].b);
            }
            xh[cp] = s;
        }
        cx<T> dxh[CB];
#pragma unroll
        for (int cp = 0; cp < CB; ++cp) {
            const cx<T> sh = valid ? a.shf[(pix * CB + cp) * a.N + n] : zero;
            // b = conj(d) sh + rho zh, xh = (b - conj(d) gamma (d . b) / (rho + gamma g)) / rho
            const cx<T> ba = cmulc_add(cscale(xh[cp].a, rho), d.a, sh), bb = cmulc_add(cscale(xh[cp].b, rho), d.b, sh);
            cx<T> p = cmul(d.a, ba) + cmul(d.b, bb);
            for (int m = G >> 1; m > 0; m >>= 1) {
                p.re += __shfl_xor(p.re, m, kWave);
                p.im += __shfl_xor(p.im, m, kWave);
            }
            const T gm = gam[cp], iden = T(1) / fma1(gm, g, rho);
            dxh[cp] = cscale(p, iden);
            const cx<T> al = cscale(p, gm * iden);
            xh[cp].a = cscale(ba - cmulc(d.a, al), irho);
            xh[cp].b = cscale(bb - cmulc(d.b, al), irho);
            if (a.want_xrrs) {
                cx<T> pa = cmul(d.a, xh[cp].a) + cmul(d.b, xh[cp].b);
                for (int m = G >> 1; m > 0; m >>= 1) {
                    pa.re += __shfl_xor(pa.re, m, kWave);
                    pa.im += __shfl_xor(pa.im, m, kWave);
                }
                if (valid) {
                    const cx<T> ga = cscale(pa, gm);
                    const cx<T> axa = cmulc_add(cscale(xh[cp].a, rho), d.a, ga), axb = cmulc_add(cscale(xh[cp].b, rho), d.b, ga);
                    acc[1] += (double)cabs2(axa - ba) + (double)cabs2(axb - bb);
                    acc[2] += (double)cabs2(axa) + (double)cabs2(axb);
                    acc[3] += (double)cabs2(ba) + (double)cabs2(bb);
                }
            }
        }
        // x_c = sum_c' Q[c, c'] xh_c'
        if (valid) {
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                cxpair<T> s;
                s.a = s.b = zero;
#pragma unroll
                for (int cp = 0; cp < CB; ++cp) {
                    s.a = pd_axpy(s.a, q[c * CB + cp], xh[cp].a);
                    s.b = pd_axpy(s.b, q[c * CB + cp], xh[cp].b);
                }
                *reinterpret_cast<cxpair<T> *>(a.xf + ((pix * CB + c) * a.N + n) * a.K + 2 * lg) = s;
            }
            if (a.want_obj && lg == 0) acc[0] += pd_fidelity(dxh, a.tab.bq, a.sf, pix, n, CB, a.Cs, a.N, Wf, a.W);
        }
    }
    block_sum_store<4>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * 4);
}

// Any K, Cb <= kPdMaxCb: one thread per (pixel, image) system, strided over its filters.
template <typename T> __global__ void __launch_bounds__(kThreads) pd_solve_generic_kernel(const PdSolveArgs<T> a) {
    const int Wf = a.W / 2 + 1, Cb = a.Cb;
    const int64_t total = a.npix * a.N;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const T rho = a.rho, irho = T(1) / a.rho;
    const T *q = a.tab.q;
    const cx<T> zero = mk<T>(T(0), T(0));
    for (int64_t sys = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; sys < total;
         sys += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = sys / a.N;
        const int n = (int)(sys - pix * a.N);
        const cx<T> *d = a.df + pix * a.K;
        const T g = a.gram[pix];
        const int64_t cstride = (int64_t)a.N * a.K;                  // from a channel to the next
        const cx<T> *z0 = a.zf + (pix * Cb * a.N + n) * a.K;
        cx<T> *x0 = a.xf + (pix * Cb * a.N + n) * a.K;
        // d . b_c' = g sh_c' + rho sum_c Q[c, c'] (d . z_c)
        cx<T> dz[kPdMaxCb], sh[kPdMaxCb], al[kPdMaxCb], dxh[kPdMaxCb], dxa[kPdMaxCb];
        for (int c = 0; c < Cb; ++c) {
            cx<T> s = zero;
            for (int k = 0; k < a.K; ++k) s = s + cmul(d[k], z0[c * cstride + k]);
            dz[c] = s;
        }
        for (int cp = 0; cp < Cb; ++cp) {
            cx<T> s = zero;
            for (int c = 0; c < Cb; ++c) s = pd_axpy(s, q[c * Cb + cp], dz[c]);
            sh[cp] = a.shf[(pix * Cb + cp) * a.N + n];
            const cx<T> p = cscale(sh[cp], g) + cscale(s, rho);
            const T gm = a.tab.gamma[cp], iden = T(1) / fma1(gm, g, rho);
            dxh[cp] = cscale(p, iden);
            al[cp] = cscale(p, gm * iden);
            dxa[cp] = zero;
        }
        double b2 = 0.0;
        for (int pass = 0; pass < (a.want_xrrs ? 2 : 1); ++pass) {
            double d2 = 0.0, ax2 = 0.0;
            for (int k = 0; k < a.K; ++k) {
                cx<T> zc[kPdMaxCb], xh[kPdMaxCb];
                for (int c = 0; c < Cb; ++c) zc[c] = z0[c * cstride + k];
                for (int cp = 0; cp < Cb; ++cp) {
                    cx<T> s = zero;
                    for (int c = 0; c < Cb; ++c) s = pd_axpy(s, q[c * Cb + cp], zc[c]);
                    const cx<T> b = cmulc_add(cscale(s, rho), d[k], sh[cp]);
                    xh[cp] = cscale(b - cmulc(d[k], al[cp]), irho);
                    if (pass == 0) {
                        if (a.want_xrrs) {
                            dxa[cp] = dxa[cp] + cmul(d[k], xh[cp]);
                            b2 += (double)cabs2(b);
                        }
                    } else {
                        // ax = gamma conj(d) (d . xh) + rho xh with d . xh summed from the xh stored
                        const cx<T> ax = cmulc_add(cscale(xh[cp], rho), d[k], cscale(dxa[cp], a.tab.gamma[cp]));
                        d2 += (double)cabs2(ax - b);
                        ax2 += (double)cabs2(ax);
                    }
                }
                if (pass == 0)
                    for (int c = 0; c < Cb; ++c) {
                        cx<T> s = zero;
                        for (int cp = 0; cp < Cb; ++cp) s = pd_axpy(s, q[c * Cb + cp], xh[cp]);
                        x0[c * cstride + k] = s;
                    }
            }
            if (pass == 1) {
                acc[1] += d2;
                acc[2] += ax2;
                acc[3] += b2;
            }
        }
        if (a.want_obj) acc[0] += pd_fidelity(dxh, a.tab.bq, a.sf, pix, n, Cb, a.Cs, a.N, Wf, a.W);
    }
    block_sum_store<4>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * 4);
}

// One thread per (pixel, image) system: the Cb inner products over the filters, then the Cs mixes.
template <typename T> __global__ void __launch_bounds__(kThreads) pd_recon_kernel(const PdReconArgs<T> a) {
    const int Wf = a.W / 2 + 1, Cb = a.Cb;
    const int64_t total = a.npix * a.N;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const cx<T> zero = mk<T>(T(0), T(0));
    for (int64_t sys = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; sys < total;
         sys += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = sys / a.N;
        const int n = (int)(sys - pix * a.N);
        const cx<T> *d = a.df + pix * a.K;
        cx<T> dx[kPdMaxCb];
        for (int c = 0; c < Cb; ++c) {
            const cx<T> *x = a.xf + ((pix * Cb + c) * a.N + n) * a.K;
            cx<T> s = zero;
            for (int k = 0; k < a.K; ++k) s = s + cmul(d[k], x[k]);
            dx[c] = s;
        }
        double s2 = 0.0;
        for (int cs = 0; cs < a.Cs; ++cs) {
            cx<T> r = zero;
            for (int c = 0; c < Cb; ++c) r = pd_axpy(r, a.tab.b[cs * Cb + c], dx[c]);
            const int64_t o = (pix * a.Cs + cs) * a.N + n;
            if (a.rf) a.rf[o] = r;
            if (a.sf) s2 += (double)cabs2(r - a.sf[o]);
        }
        acc[0] += parseval_weight((int)(pix % Wf), Wf, a.W) * s2;
    }
    block_sum_store<4>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * 4);
}

inline bool pd_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

template <typename T, int CB> void pd_launch_wave(hipStream_t st, const PdSolveArgs<T> &a, int grid) {
    const size_t lds = sizeof(double) * kPdScratch + sizeof(T) * (CB * CB + CB);
    hipLaunchKernelGGL((pd_solve_wave_kernel<T, CB>), dim3(grid), dim3(kThreads), lds, st, a);
}

}  // namespace

bool pd_wave_form(int K, int Cb) {
    return K % 2 == 0 && pd_pow2(K / 2) && K / 2 <= kWave && Cb >= 1 && Cb <= kPdWaveMaxCb;
}

template <typename T> int launch_pd_solve(hipStream_t st, const PdSolveArgs<T> &a, bool *wave_form) {
    SA_REQUIRE(a.Cb >= 1 && a.Cb <= kPdMaxCb, "pd_solve: 1 <= Cb <= 16");
    SA_REQUIRE(a.zf != a.xf, "pd_solve: the spectra may not alias");
    const bool wave = pd_wave_form(a.K, a.Cb);
    int grid;
    if (wave) {
        grid = grid_for(a.npix * a.N * (a.K / 2));
        switch (a.Cb) {
        case 1: pd_launch_wave<T, 1>(st, a, grid); break;
        case 2: pd_launch_wave<T, 2>(st, a, grid); break;
        case 3: pd_launch_wave<T, 3>(st, a, grid); break;
        case 4: pd_launch_wave<T, 4>(st, a, grid); break;
        case 5: pd_launch_wave<T, 5>(st, a, grid); break;
        case 6: pd_launch_wave<T, 6>(st, a, grid); break;
        case 7: pd_launch_wave<T, 7>(st, a, grid); break;
        default: pd_launch_wave<T, 8>(st, a, grid); break;
        }
    } else {
        grid = grid_for(a.npix * a.N);
        hipLaunchKernelGGL((pd_solve_generic_kernel<T>), dim3(grid), dim3(kThreads), sizeof(double) * kPdScratch, st, a);
    }
    SA_HIP(hipGetLastError());
    if (wave_form) *wave_form = wave;
    return grid;
}

template <typename T> int launch_pd_recon(hipStream_t st, const PdReconArgs<T> &a) {
    SA_REQUIRE(a.Cb >= 1 && a.Cb <= kPdMaxCb, "pd_recon: 1 <= Cb <= 16");
    const int grid = grid_for(a.npix * a.N);
    hipLaunchKernelGGL((pd_recon_kernel<T>), dim3(grid), dim3(kThreads), sizeof(double) * kPdScratch, st, a);
    SA_HIP(hipGetLastError());
    return grid;
}

#define SA_PD_INST(T)                                                                   \
    template int launch_pd_solve<T>(hipStream_t, const PdSolveArgs<T> &, bool *);        \
    template int launch_pd_recon<T>(hipStream_t, const PdReconArgs<T> &);
SA_PD_INST(float)
SA_PD_INST(double)

}  // namespace sporco_amd
