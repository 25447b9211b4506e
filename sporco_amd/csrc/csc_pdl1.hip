// csc_pdl1.hip -- the kernels of ConvProdDictL1L1Grd / ConvProdDictL1L1GrdJoint (csc_pdl1.h):
// pdl1_solve, the eigen-channel diagonal-plus-rank-one x step whose right-hand side mixes the
// Cs-channel block 0 with the Cb-channel block 1 and which writes the block-0 constraint spectrum as a
// by-product, and pdl1_dual, the norm of A^T u through B in one read-only pass.  float32 / float64,
// any H, W, N, K, Cs; Cb <= kPdMaxCb.
#include "csc_pdl1.h"
#include "csc_kernels_dev.h"

namespace sporco_amd {

namespace {

constexpr int kPdl1Scratch = 4 * (kThreads / kWave);   // doubles of LDS for block_sum_store<4>

// acc + s v
template <typename T> __device__ __forceinline__ cx<T> pl_axpy(cx<T> acc, T s, cx<T> v) {
    return mk<T>(fma1(s, v.re, acc.re), fma1(s, v.im, acc.im));
}

// s0_c' = sum_cs (BQ)[cs, c'] z0[cs] of one (pixel, image) system
template <typename T>
__device__ __forceinline__ void pl_mix0(const cx<T> *z0f, const T *bq, int64_t pix, int n, int Cb, int Cs, int N,
                                        cx<T> *s0) {
    for (int cp = 0; cp < Cb; ++cp) s0[cp] = mk<T>(T(0), T(0));
    for (int cs = 0; cs < Cs; ++cs) {
        const cx<T> z = z0f[(pix * Cs + cs) * N + n];
        for (int cp = 0; cp < Cb; ++cp) s0[cp] = pl_axpy(s0[cp], bq[cs * Cb + cp], z);
    }
}

// ax0f[cs] = sum_c' (BQ)[cs, c'] dxh_c' of one system
template <typename T>
__device__ __forceinline__ void pl_store_ax0(cx<T> *ax0f, const T *bq, const cx<T> *dxh, int64_t pix, int n, int Cb,
                                             int Cs, int N) {
    for (int cs = 0; cs < Cs; ++cs) {
        cx<T> r = mk<T>(T(0), T(0));
        for (int cp = 0; cp < Cb; ++cp) r = pl_axpy(r, bq[cs * Cb + cp], dxh[cp]);
        ax0f[(pix * Cs + cs) * N + n] = r;
    }
}

// K even and G = K / 2 a power of two <= 64, CB <= kPdWaveMaxCb: a lane owns two adjacent filters of
// all CB channels, G lanes a (pixel, image) system, the sums over the filters are wave shuffles (the
// lane layout of csc_pd.hip pd_solve_wave_kernel).  Q and Gamma are staged once in LDS.
template <typename T, int CB> __global__ void __launch_bounds__(kThreads) pdl1_solve_wave_kernel(const Pdl1SolveArgs<T> a) {
    const int G = a.K >> 1, Wf = a.W / 2 + 1;
    const int64_t total = a.npix * a.N * G;
    const int64_t total_pad = (total + kWave - 1) / kWave * kWave;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    T *const q = reinterpret_cast<T *>(dyn_lds<double>() + kPdl1Scratch);     // CB CB, then Gamma
    T *const gam = q + CB * CB;
    for (int i = threadIdx.x; i < CB * CB + CB; i += blockDim.x) q[i] = i < CB * CB ? a.tab.q[i] : a.tab.gamma[i - CB * CB];
    __syncthreads();
    const cx<T> zero = mk<T>(T(0), T(0));
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total_pad;
         t += (int64_t)gridDim.x * blockDim.x) {
        const bool valid = t < total;
        const int64_t sys = t / G;
        const int lg = (int)(t - sys * G);
        const int64_t pix = sys / a.N;
        const int n = (int)(sys - pix * a.N);
        cxpair<T> z[CB], d;
        cx<T> s0[CB];
        d.a = d.b = zero;
        T wa = T(0), wb = T(0), dda = T(1), ddb = T(1);      // w_m GHG and dd_m of the lane's two filters
#pragma unroll
        for (int c = 0; c < CB; ++c) z[c].a = z[c].b = s0[c] = zero;
        if (valid) {
#pragma unroll
            for (int c = 0; c < CB; ++c)
                z[c] = *reinterpret_cast<const cxpair<T> *>(a.z1f + ((pix * CB + c) * a.N + n) * a.K + 2 * lg);
            d = *reinterpret_cast<const cxpair<T> *>(a.df + pix * a.K + 2 * lg);
            const T gh = grad_gh(a.grad, pix, Wf);
            wa = grad_w(a.grad, 2 * lg) * gh;
            wb = grad_w(a.grad, 2 * lg + 1) * gh;
            dda = fma1(a.grad.mu, wa, T(1));
            ddb = fma1(a.grad.mu, wb, T(1));
            pl_mix0(a.z0f, a.tab.bq, pix, n, CB, a.Cs, a.N, s0);
        }
        const T ida = T(1) / dda, idb = T(1) / ddb;
        // g = sum_m |d_m|^2 / dd_m
        T g = fma1(cabs2(d.a), ida, cabs2(d.b) * idb);
        for (int m = G >> 1; m > 0; m >>= 1) g += __shfl_xor(g, m, kWave);
        cxpair<T> xh[CB];
        cx<T> dxh[CB];
#pragma unroll
        for (int cp = 0; cp < CB; ++cp) {
            // b = conj(d) s0 + sum_c Q[c, c'] z1_c
            cx<T> ba = zero, bb = zero;
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                ba = pl_axpy(ba, q[c * CB + cp], z[c].a);
                bb = pl_axpy(bb, q[c * CB + cp], z[c].b);
            }
            ba = cmulc_add(ba, d.a, s0[cp]);
            bb = cmulc_add(bb, d.b, s0[cp]);
            cx<T> p = cscale(cmul(d.a, ba), ida) + cscale(cmul(d.b, bb), idb);
            for (int m = G >> 1; m > 0; m >>= 1) {
                p.re += __shfl_xor(p.re, m, kWave);
                p.im += __shfl_xor(p.im, m, kWave);
            }
            const T gm = gam[cp];
            dxh[cp] = cscale(p, T(1) / fma1(gm, g, T(1)));
            const cx<T> al = cscale(dxh[cp], gm);
            xh[cp].a = cscale(ba - cmulc(d.a, al), ida);
            xh[cp].b = cscale(bb - cmulc(d.b, al), idb);
            if (a.want_xrrs) {
                cx<T> pa = cmul(d.a, xh[cp].a) + cmul(d.b, xh[cp].b);
                for (int m = G >> 1; m > 0; m >>= 1) {
                    pa.re += __shfl_xor(pa.re, m, kWave);
                    pa.im += __shfl_xor(pa.im, m, kWave);
                }
                if (valid) {
                    const cx<T> ga = cscale(pa, gm);
                    const cx<T> axa = cmulc_add(cscale(xh[cp].a, dda), d.a, ga), axb = cmulc_add(cscale(xh[cp].b, ddb), d.b, ga);
                    acc[1] += (double)cabs2(axa - ba) + (double)cabs2(axb - bb);
                    acc[2] += (double)cabs2(axa) + (double)cabs2(axb);
                    acc[3] += (double)cabs2(ba) + (double)cabs2(bb);
                }
            }
        }
        // x_c = sum_c' Q[c, c'] xh_c'
        if (valid) {
            double r2a = 0.0, r2b = 0.0;
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                cxpair<T> s;
                s.a = s.b = zero;
#pragma unroll
                for (int cp = 0; cp < CB; ++cp) {
                    s.a = pl_axpy(s.a, q[c * CB + cp], xh[cp].a);
                    s.b = pl_axpy(s.b, q[c * CB + cp], xh[cp].b);
                }
                *reinterpret_cast<cxpair<T> *>(a.xf + ((pix * CB + c) * a.N + n) * a.K + 2 * lg) = s;
                r2a += (double)cabs2(s.a);
                r2b += (double)cabs2(s.b);
            }
            if (a.want_obj) acc[0] += parseval_weight((int)(pix % Wf), Wf, a.W) * ((double)wa * r2a + (double)wb * r2b);
            if (lg == 0) pl_store_ax0(a.ax0f, a.tab.bq, dxh, pix, n, CB, a.Cs, a.N);
        }
    }
    block_sum_store<4>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * 4);
}

// Any K, Cb <= kPdMaxCb: one thread per (pixel, image) system, strided over its filters.
template <typename T> __global__ void __launch_bounds__(kThreads) pdl1_solve_generic_kernel(const Pdl1SolveArgs<T> a) {
    const int Wf = a.W / 2 + 1, Cb = a.Cb;
    const int64_t total = a.npix * a.N;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const T *q = a.tab.q;
    const cx<T> zero = mk<T>(T(0), T(0));
    for (int64_t sys = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; sys < total;
         sys += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = sys / a.N;
        const int n = (int)(sys - pix * a.N);
        const cx<T> *d = a.df + pix * a.K;
        const T gh = grad_gh(a.grad, pix, Wf);
        const int64_t cstride = (int64_t)a.N * a.K;                  // from a channel to the next
        const cx<T> *z1 = a.z1f + (pix * Cb * a.N + n) * a.K;
        cx<T> *x0 = a.xf + (pix * Cb * a.N + n) * a.K;
        cx<T> s0[kPdMaxCb], dz[kPdMaxCb], al[kPdMaxCb], dxh[kPdMaxCb], dxa[kPdMaxCb];
        pl_mix0(a.z0f, a.tab.bq, pix, n, Cb, a.Cs, a.N, s0);
        // P_c' = g s0_c' + sum_c Q[c, c'] sum_m d_m z1_c,m / dd_m
        T g = T(0);
        for (int c = 0; c < Cb; ++c) dz[c] = zero;
        for (int k = 0; k < a.K; ++k) {
            const T idd = T(1) / fma1(a.grad.mu, grad_w(a.grad, k) * gh, T(1));
            const cx<T> di = cscale(d[k], idd);
            g = fma1(cabs2(d[k]), idd, g);
            for (int c = 0; c < Cb; ++c) dz[c] = dz[c] + cmul(di, z1[c * cstride + k]);
        }
        for (int cp = 0; cp < Cb; ++cp) {
            cx<T> s = cscale(s0[cp], g);
            for (int c = 0; c < Cb; ++c) s = pl_axpy(s, q[c * Cb + cp], dz[c]);
            const T gm = a.tab.gamma[cp];
            dxh[cp] = cscale(s, T(1) / fma1(gm, g, T(1)));
            al[cp] = cscale(dxh[cp], gm);
            dxa[cp] = zero;
        }
        double b2 = 0.0, rg = 0.0;
        for (int pass = 0; pass < (a.want_xrrs ? 2 : 1); ++pass) {
            double d2 = 0.0, ax2 = 0.0;
            for (int k = 0; k < a.K; ++k) {
                const T wk = grad_w(a.grad, k) * gh, dd = fma1(a.grad.mu, wk, T(1)), idd = T(1) / dd;
                cx<T> zc[kPdMaxCb], xh[kPdMaxCb];
                for (int c = 0; c < Cb; ++c) zc[c] = z1[c * cstride + k];
                for (int cp = 0; cp < Cb; ++cp) {
                    cx<T> s = zero;
                    for (int c = 0; c < Cb; ++c) s = pl_axpy(s, q[c * Cb + cp], zc[c]);
                    const cx<T> b = cmulc_add(s, d[k], s0[cp]);
                    xh[cp] = cscale(b - cmulc(d[k], al[cp]), idd);
                    if (pass == 0) {
                        if (a.want_xrrs) {
                            dxa[cp] = dxa[cp] + cmul(d[k], xh[cp]);
                            b2 += (double)cabs2(b);
                        }
                    } else {
                        // ax = gamma conj(d) (d . xh) + dd xh with d . xh summed from the xh stored
                        const cx<T> ax = cmulc_add(cscale(xh[cp], dd), d[k], cscale(dxa[cp], a.tab.gamma[cp]));
                        d2 += (double)cabs2(ax - b);
                        ax2 += (double)cabs2(ax);
                    }
                }
                if (pass == 0) {
                    double r2 = 0.0;
                    for (int c = 0; c < Cb; ++c) {
                        cx<T> s = zero;
                        for (int cp = 0; cp < Cb; ++cp) s = pl_axpy(s, q[c * Cb + cp], xh[cp]);
                        x0[c * cstride + k] = s;
                        r2 += (double)cabs2(s);
                    }
                    rg += (double)wk * r2;
                }
            }
            if (pass == 1) {
                acc[1] += d2;
                acc[2] += ax2;
                acc[3] += b2;
            }
        }
        if (a.want_obj) acc[0] += parseval_weight((int)(pix % Wf), Wf, a.W) * rg;
        pl_store_ax0(a.ax0f, a.tab.bq, dxh, pix, n, Cb, a.Cs, a.N);
    }
    block_sum_store<4>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * 4);
}

// The B-mixing sibling of csc_l1l1.hip l1l1_dual_kernel: V consecutive filters of one (pixel, channel,
// image) system per thread, G = K / V threads a system.  The block-0 value of a system,
// sum_cs B[cs, cb] u0f[pix, cs, n], is the same for its G threads: lane j forms that of the wave's
// j-th system once and every thread picks its own system's from that lane.  The loop runs to a
// multiple of the wave so that all lanes take part in every exchange.
template <typename T, int V> __global__ void __launch_bounds__(kThreads) pdl1_dual_kernel(const Pdl1DualArgs<T> a) {
    const int G = a.K / V, Wf = a.W / 2 + 1, CN = a.Cb * a.N;
    const int64_t total = a.npix * CN * G;
    const int64_t total_pad = (total + kWave - 1) / kWave * kWave;
    const int lane = threadIdx.x & (kWave - 1);
    double acc[2] = {0.0, 0.0};
    const cx<T> zero = mk<T>(T(0), T(0));
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total_pad;
         t += (int64_t)gridDim.x * blockDim.x) {
        const bool valid = t < total;
        const int64_t t0 = t - lane;                                  // the wave's first thread: < total
        const int64_t tl = t0 + kWave - 1 < total ? t0 + kWave - 1 : total - 1;
        const int64_t sys0 = t0 / G;
        const int nsys = (int)(tl / G - sys0) + 1;                    // systems under this wave, <= 64
        const int64_t tv = valid ? t : tl;
        const int64_t sys = tv / G;
        const int lg = (int)(tv - sys * G);
        const int64_t pix = sys / CN;
        const int src = (int)(sys - sys0);
        cx<T> f = zero;
        if (lane < nsys) {
            const int64_t fsys = sys0 + lane, fpix = fsys / CN;       // the system this lane mixes for
            const int fcn = (int)(fsys - fpix * CN), fcb = fcn / a.N, fn = fcn - fcb * a.N;
            for (int cs = 0; cs < a.Cs; ++cs) {
                const cx<T> u = a.u0f[(fpix * a.Cs + cs) * a.N + fn];
                const T bv = a.b[cs * a.Cb + fcb];
                f = mk<T>(fma1(bv, u.re, f.re), fma1(bv, u.im, f.im));
            }
        }
        const cx<T> v0 = wave_pick(f, lane, src);
        if (valid) {
            const CxVec<T, V> su = *reinterpret_cast<const CxVec<T, V> *>(a.u1f + (int64_t)V * t);
            const CxVec<T, V> d = *reinterpret_cast<const CxVec<T, V> *>(a.df + pix * a.K + V * lg);
            double u2 = 0.0;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const cx<T> s = cmulc_add(su.v[e], d.v[e], v0);
                u2 += (double)s.re * (double)s.re + (double)s.im * (double)s.im;
            }
            acc[0] += parseval_weight((int)(pix % Wf), Wf, a.W) * u2;
        }
    }
    block_sum_store<2>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * 2);
}

template <typename T, int CB> void pdl1_launch_wave(hipStream_t st, const Pdl1SolveArgs<T> &a, int grid) {
    const size_t lds = sizeof(double) * kPdl1Scratch + sizeof(T) * (CB * CB + CB);
    hipLaunchKernelGGL((pdl1_solve_wave_kernel<T, CB>), dim3(grid), dim3(kThreads), lds, st, a);
}

}  // namespace

template <typename T> int launch_pdl1_solve(hipStream_t st, const Pdl1SolveArgs<T> &a, bool *wave_form) {
    SA_REQUIRE(a.Cb >= 1 && a.Cb <= kPdMaxCb, "pdl1_solve: 1 <= Cb <= 16");
    SA_REQUIRE(a.Cs >= 1, "pdl1_solve: Cs >= 1");
    SA_REQUIRE(a.z1f != a.xf && a.z0f != a.ax0f, "pdl1_solve: the spectra may not alias");
    const bool wave = !a.force_generic && pd_wave_form(a.K, a.Cb);
    int grid;
    if (wave) {
        grid = grid_for(a.npix * a.N * (a.K / 2));
        switch (a.Cb) {
        case 1: pdl1_launch_wave<T, 1>(st, a, grid); break;
        case 2: pdl1_launch_wave<T, 2>(st, a, grid); break;
        case 3: pdl1_launch_wave<T, 3>(st, a, grid); break;
        case 4: pdl1_launch_wave<T, 4>(st, a, grid); break;
        case 5: pdl1_launch_wave<T, 5>(st, a, grid); break;
        case 6: pdl1_launch_wave<T, 6>(st, a, grid); break;
        case 7: pdl1_launch_wave<T, 7>(st, a, grid); break;
        default: pdl1_launch_wave<T, 8>(st, a, grid); break;
        }
    } else {
        grid = grid_for(a.npix * a.N);
        hipLaunchKernelGGL((pdl1_solve_generic_kernel<T>), dim3(grid), dim3(kThreads), sizeof(double) * kPdl1Scratch, st, a);
    }
    SA_HIP(hipGetLastError());
    if (wave_form) *wave_form = wave;
    return grid;
}

template <typename T> int launch_pdl1_dual(hipStream_t st, const Pdl1DualArgs<T> &a) {
    SA_REQUIRE(a.Cb >= 1 && a.Cs >= 1, "pdl1_dual: Cb, Cs >= 1");
    const size_t lds = sizeof(double) * 2 * (kThreads / kWave);
    constexpr int V = 16 / sizeof(cx<T>);        // 2 in float32, 1 in float64
    const int64_t sys = a.npix * a.Cb * a.N;
    int grid;
    if (V == 2 && a.K % 2 == 0) {
        grid = grid_for(sys * (a.K / 2));
        hipLaunchKernelGGL((pdl1_dual_kernel<T, V>), dim3(grid), dim3(kThreads), lds, st, a);
    } else {
        grid = grid_for(sys * a.K);
        hipLaunchKernelGGL((pdl1_dual_kernel<T, 1>), dim3(grid), dim3(kThreads), lds, st, a);
    }
    SA_HIP(hipGetLastError());
    return grid;
}

#define SA_PDL1_INST(T)                                                                       \
    template int launch_pdl1_solve<T>(hipStream_t, const Pdl1SolveArgs<T> &, bool *);        \
    template int launch_pdl1_dual<T>(hipStream_t, const Pdl1DualArgs<T> &);
SA_PDL1_INST(float)
SA_PDL1_INST(double)

}  // namespace sporco_amd
