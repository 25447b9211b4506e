// csc_l1l1.hip -- the kernels of ConvL1L1Grd (csc_l1l1.h): l1l1_y0step, the signal-sized block of
// the two-block constraint with a soft-threshold prox, and l1l1_dual, the two dual-residual norms
// in one read-only pass.  float32 / float64, any H, W, N, K; Cd <= kL1MaxCd.
#include "csc_l1l1.h"
#include "csc_kernels_dev.h"

namespace sporco_amd {

namespace {

template <typename T>
__global__ void __launch_bounds__(kThreads) l1l1_y0step_kernel(const L1Y0Args<T> a, int64_t n, double *partials) {
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const T irho = T(1) / a.rho;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int nn = (int)(i % a.N);
        const int c = (int)((i / a.N) % a.C);
        const int64_t pix = i / ((int64_t)a.N * a.C);
        const int x = (int)(pix % a.W), h = (int)(pix / a.W);
        const T wv = a.w.ptr ? weight_at(a.w, h, x, c, nn, 0) : T(1);
        const T axnr = a.ax0nr[i], sv = a.s[i], yo = a.y0[i], uo = a.us * a.u0[i];
        const T ax = a.rlx == T(1) ? axnr : a.rlx * axnr + (T(1) - a.rlx) * (yo + sv);
        const T yn = soft(ax + uo - sv, irho * wv);
        const T un = uo + (ax - (yn + sv));
        a.y0[i] = yn;
        a.u0[i] = un;
        if (a.dy0) a.dy0[i] = yo - yn;
        const double r = (double)(axnr - (yn + sv));
        const double g = (double)(wv * (a.geval_y ? yn : axnr - sv));
        acc[0] += r * r;
        acc[1] += (double)axnr * (double)axnr;
        acc[2] += (double)yn * (double)yn;
        acc[3] += (double)un * (double)un;
        acc[4] += g < 0.0 ? -g : g;
    }
    block_sum_store<5>(acc, dyn_lds<double>(), partials + (int64_t)blockIdx.x * 5);
}

// V consecutive filters of one (pixel, image) system per thread, one load of V cx<T> each (CxVec: 16
// bytes for V = 2 in float32 and V = 1 in float64); G = K / V threads a system.
// The block-0 values of a system (Cd of dy0f, Cd of u0f) are the same for its G threads.  A wave's
// 64 threads lie in at most 64 consecutive systems: lane j loads the values of the wave's j-th system
// once, and every thread picks those of its own system from that lane.  The loop runs to a multiple
// of the wave so that all lanes take part in every exchange.
template <typename T, int V> __global__ void __launch_bounds__(kThreads) l1l1_dual_kernel(const L1DualArgs<T> a) {
    const int G = a.K / V, Wf = a.W / 2 + 1, Cd = a.Cd;
    const int64_t total = a.npix * a.CN * G;
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
        const int64_t pix = sys / a.CN;
        const int64_t fsys = sys0 + lane, fpix = fsys / a.CN;         // the system this lane fetches for
        const int fcn = (int)(fsys - fpix * a.CN);
        const int src = (int)(sys - sys0);
        CxVec<T, V> sd, su;
#pragma unroll
        for (int e = 0; e < V; ++e) sd.v[e] = su.v[e] = zero;
        if (valid) {
            sd = *reinterpret_cast<const CxVec<T, V> *>(a.dy1f + (int64_t)V * t);
            su = *reinterpret_cast<const CxVec<T, V> *>(a.u1f + (int64_t)V * t);
        }
        for (int c = 0; c < Cd; ++c) {
            cx<T> fd = zero, fu = zero;
            if (lane < nsys) {
                const int64_t o = (fpix * Cd + c) * a.CN + fcn;
                fd = a.dy0f[o];
                fu = a.u0f[o];
            }
            const cx<T> vd = wave_pick(fd, lane, src), vu = wave_pick(fu, lane, src);
            if (valid) {
                const CxVec<T, V> d = *reinterpret_cast<const CxVec<T, V> *>(a.df + (pix * Cd + c) * a.K + V * lg);
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    sd.v[e] = cmulc_add(sd.v[e], d.v[e], vd);
                    su.v[e] = cmulc_add(su.v[e], d.v[e], vu);
                }
            }
        }
        if (valid) {
            const double pw = parseval_weight((int)(pix % Wf), Wf, a.W);
            double d2 = 0.0, u2 = 0.0;
#pragma unroll
            for (int e = 0; e < V; ++e) {
                d2 += (double)sd.v[e].re * (double)sd.v[e].re + (double)sd.v[e].im * (double)sd.v[e].im;
                u2 += (double)su.v[e].re * (double)su.v[e].re + (double)su.v[e].im * (double)su.v[e].im;
            }
            acc[0] += pw * d2;
            acc[1] += pw * u2;
        }
    }
    block_sum_store<2>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * 2);
}

}  // namespace

template <typename T> int launch_l1l1_y0step(hipStream_t st, const L1Y0Args<T> &a, double *partials) {
    const int64_t n = (int64_t)a.H * a.W * a.C * a.N;
    const int grid = grid_for(n);
    hipLaunchKernelGGL((l1l1_y0step_kernel<T>), dim3(grid), dim3(kThreads), sizeof(double) * 5 * (kThreads / kWave), st,
                       a, n, partials);
    SA_HIP(hipGetLastError());
    return grid;
}

template <typename T> int launch_l1l1_dual(hipStream_t st, const L1DualArgs<T> &a) {
    SA_REQUIRE(a.Cd >= 1 && a.Cd <= kL1MaxCd, "l1l1_dual: 1 <= Cd <= 8");
    const size_t lds = sizeof(double) * 2 * (kThreads / kWave);
    constexpr int V = 16 / sizeof(cx<T>);        // 2 in float32, 1 in float64
    int grid;
    if (V == 2 && a.K % 2 == 0) {
        grid = grid_for(a.npix * a.CN * (a.K / 2));
        hipLaunchKernelGGL((l1l1_dual_kernel<T, V>), dim3(grid), dim3(kThreads), lds, st, a);
    } else {
        grid = grid_for(a.npix * a.CN * a.K);
        hipLaunchKernelGGL((l1l1_dual_kernel<T, 1>), dim3(grid), dim3(kThreads), lds, st, a);
    }
    SA_HIP(hipGetLastError());
    return grid;
}

#define SA_L1L1_INST(T)                                                                     \
    template int launch_l1l1_y0step<T>(hipStream_t, const L1Y0Args<T> &, double *);         \
    template int launch_l1l1_dual<T>(hipStream_t, const L1DualArgs<T> &);
SA_L1L1_INST(float)
SA_L1L1_INST(double)

}  // namespace sporco_amd
