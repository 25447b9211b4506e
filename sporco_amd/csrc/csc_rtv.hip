// csc_rtv.hip -- the kernels of ConvBPDNRecTV (csc_rtv.h): rtv_solve in the frequency domain,
// rtv_ystep / rtv_adjoint as spatial streaming passes, rtv_dual as a frequency-domain reduction.
// float32 / float64, any H, W >= 2, C, N, K.
#include "csc_rtv.h"
#include "csc_kernels_dev.h"

#include <algorithm>

namespace sporco_amd {

namespace {

constexpr int kRtvScratch = 5 * (kThreads / kWave);   // doubles of LDS for block_sum_store<5>

template <typename T> __device__ __forceinline__ T rtv_abs(T v) { return v < T(0) ? -v : v; }
template <typename T> __device__ __forceinline__ T rtv_sqrt(T v);
template <> __device__ __forceinline__ float rtv_sqrt<float>(float v) { return sqrtf(v); }
template <> __device__ __forceinline__ double rtv_sqrt<double>(double v) { return sqrt(v); }
// prox_l2's factor max(0, a - alpha) / a, 0 at a = 0 (sporco/prox/_l2.py prox_l2)
template <typename T> __device__ __forceinline__ T rtv_shrink(T nrm, T alpha) {
    const T b = nrm - alpha;
    return (nrm > T(0) && b > T(0)) ? b / nrm : T(0);
}

// What a (pixel, c, n) system needs beside its K filters.
template <typename T> struct RtvSys {
    cx<T> s, zd;      // Sf, Zyf - us Zuf
    T g, tau;         // sum |Df|^2, rho GHG
};

// the 2 x 2 system (diag(1, tau) B B^H + rho I) v = (s - p1; rho zd - tau p2)  (csc_rtv.h)
template <typename T>
__device__ __forceinline__ void rtv_solve2(const RtvSys<T> &y, T rho, cx<T> p1, cx<T> p2, T gw, T gww, cx<T> &v1,
                                           cx<T> &v2) {
    const cx<T> r1 = y.s - p1, r2 = cscale(y.zd, rho) - cscale(p2, y.tau);
    const T m11 = y.g + rho, m12 = gw, m21 = y.tau * gw, m22 = fma1(y.tau, gww, rho);
    const T idet = T(1) / (m11 * m22 - m12 * m21);
    v1 = cscale(cscale(r1, m22) - cscale(r2, m12), idet);
    v2 = cscale(cscale(r2, m11) - cscale(r1, m21), idet);
}

// K even and G = K / 2 a power of two <= 64: a lane owns two adjacent filters, G lanes a system, the
// sums over the filters are wave shuffles (the layout of ck_admm.hip sm_solve_wave_kernel).
template <typename T> __global__ void __launch_bounds__(kThreads) rtv_solve_wave_kernel(const RtvSolveArgs<T> a) {
    const int G = a.K >> 1, Wf = a.W / 2 + 1;
    const int64_t total = a.npix * a.CN * G;
    const int64_t total_pad = (total + kWave - 1) / kWave * kWave;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const T rho = a.rho, us = a.us, w0 = a.tvw[0];
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total_pad;
         t += (int64_t)gridDim.x * blockDim.x) {
        const bool valid = t < total;
        const int64_t grp = t / G;
        const int lg = (int)(t - grp * G);
        const int64_t pix = grp / a.CN;
        const cx<T> zero = mk<T>(T(0), T(0));
        cxpair<T> yu, d;
        yu.a = yu.b = d.a = d.b = zero;
        RtvSys<T> y;
        y.s = y.zd = zero;
        y.g = y.tau = T(0);
        T wa = T(0), wb = T(0);
        if (valid) {
            const cxpair<T> yf = *reinterpret_cast<const cxpair<T> *>(a.yf + 2 * t);
            const cxpair<T> uf = *reinterpret_cast<const cxpair<T> *>(a.uf + 2 * t);
            yu.a = yf.a - cscale(uf.a, us);
            yu.b = yf.b - cscale(uf.b, us);
            d = *reinterpret_cast<const cxpair<T> *>(a.df + pix * a.K + 2 * lg);
            y.s = a.sf[grp];
            y.zd = a.zyf[grp] - cscale(a.zuf[grp], us);
            y.g = a.gram[pix];
            y.tau = rho * (a.ghh[pix / Wf] + a.ghw[pix % Wf]);
            wa = a.uniform ? w0 : a.tvw[2 * lg];
            wb = a.uniform ? w0 : a.tvw[2 * lg + 1];
        }
        cx<T> p1 = cmul(d.a, yu.a) + cmul(d.b, yu.b);
        cx<T> ca, cb;     // x = yu + conj(d) c
        if (a.uniform) {
            for (int m = G >> 1; m > 0; m >>= 1) {
                p1.re += __shfl_xor(p1.re, m, kWave);
                p1.im += __shfl_xor(p1.im, m, kWave);
            }
            const T c = fma1(y.tau, w0 * w0, T(1));
            const cx<T> r = y.s + cscale(y.zd, rho * w0) - cscale(p1, c);
            ca = cb = cscale(r, T(1) / fma1(c, y.g, rho));
        } else {
            cx<T> p2 = cscale(cmul(d.a, yu.a), wa) + cscale(cmul(d.b, yu.b), wb);
            T gw = fma1(wa, cabs2(d.a), wb * cabs2(d.b)), gww = fma1(wa * wa, cabs2(d.a), wb * wb * cabs2(d.b));
            for (int m = G >> 1; m > 0; m >>= 1) {
                p1.re += __shfl_xor(p1.re, m, kWave);
                p1.im += __shfl_xor(p1.im, m, kWave);
                p2.re += __shfl_xor(p2.re, m, kWave);
                p2.im += __shfl_xor(p2.im, m, kWave);
                gw += __shfl_xor(gw, m, kWave);
                gww += __shfl_xor(gww, m, kWave);
            }
            cx<T> v1, v2;
            rtv_solve2(y, rho, p1, p2, gw, gww, v1, v2);
            ca = v1 + cscale(v2, wa);
            cb = v1 + cscale(v2, wb);
        }
        cxpair<T> x;
        x.a = yu.a + cmulc(d.a, ca);
        x.b = yu.b + cmulc(d.b, cb);
        if (valid) *reinterpret_cast<cxpair<T> *>(a.xf + 2 * t) = x;
        // Df.Xf and sum_m w_m Df_m Xf_m while the filters of the frequency are in registers
        cx<T> dx = cmul(d.a, x.a) + cmul(d.b, x.b);
        cx<T> dxw = cscale(cmul(d.a, x.a), wa) + cscale(cmul(d.b, x.b), wb);
        for (int m = G >> 1; m > 0; m >>= 1) {
            dx.re += __shfl_xor(dx.re, m, kWave);
            dx.im += __shfl_xor(dx.im, m, kWave);
            dxw.re += __shfl_xor(dxw.re, m, kWave);
            dxw.im += __shfl_xor(dxw.im, m, kWave);
        }
        if (valid && lg == 0) {
            a.rwf[grp] = dxw;
            if (a.want_obj) acc[0] += parseval_weight((int)(pix % Wf), Wf, a.W) * (double)cabs2(dx - y.s);
        }
        if (a.want_xrrs && valid) {
            // ax = conj(Df)(Df.x) + tau conj(w Df)(w Df . x) + rho x,  b = rho yu + conj(Df) Sf + rho conj(w Df) zd
            const cx<T> axa = cmulc(d.a, dx + cscale(dxw, y.tau * wa)) + cscale(x.a, rho);
            const cx<T> axb = cmulc(d.b, dx + cscale(dxw, y.tau * wb)) + cscale(x.b, rho);
            const cx<T> ba = cscale(yu.a, rho) + cmulc(d.a, y.s + cscale(y.zd, rho * wa));
            const cx<T> bb = cscale(yu.b, rho) + cmulc(d.b, y.s + cscale(y.zd, rho * wb));
            acc[1] += (double)cabs2(axa - ba) + (double)cabs2(axb - bb);
            acc[2] += (double)cabs2(axa) + (double)cabs2(axb);
            acc[3] += (double)cabs2(ba) + (double)cabs2(bb);
        }
    }
    block_sum_store<4>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * 4);
}

// Any K: one thread per (pixel, c, n) system, strided over its filters.
template <typename T> __global__ void __launch_bounds__(kThreads) rtv_solve_generic_kernel(const RtvSolveArgs<T> a) {
    const int Wf = a.W / 2 + 1;
    const int64_t total = a.npix * a.CN;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const T rho = a.rho, us = a.us, w0 = a.tvw[0];
    for (int64_t grp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; grp < total;
         grp += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = grp / a.CN;
        const cx<T> *d = a.df + pix * a.K, *yf = a.yf + grp * a.K, *uf = a.uf + grp * a.K;
        cx<T> *x = a.xf + grp * a.K;
        RtvSys<T> y;
        y.s = a.sf[grp];
        y.zd = a.zyf[grp] - cscale(a.zuf[grp], us);
        y.g = a.gram[pix];
        y.tau = rho * (a.ghh[pix / Wf] + a.ghw[pix % Wf]);
        auto wk = [&](int k) -> T { return a.uniform ? w0 : a.tvw[k]; };
        cx<T> p1 = mk<T>(T(0), T(0)), p2 = p1;
        T gw = T(0), gww = T(0);
        for (int k = 0; k < a.K; ++k) {
            const cx<T> dy = cmul(d[k], yf[k] - cscale(uf[k], us));
            const T w = wk(k), d2 = cabs2(d[k]);
            p1 = p1 + dy;
            p2 = p2 + cscale(dy, w);
            gw = fma1(w, d2, gw);
            gww = fma1(w * w, d2, gww);
        }
        cx<T> v1, v2;
        if (a.uniform) {
            const T c = fma1(y.tau, w0 * w0, T(1));
            const cx<T> r = y.s + cscale(y.zd, rho * w0) - cscale(p1, c);
            v1 = cscale(r, T(1) / fma1(c, y.g, rho));
            v2 = mk<T>(T(0), T(0));
        } else {
            rtv_solve2(y, rho, p1, p2, gw, gww, v1, v2);
        }
        cx<T> dx = mk<T>(T(0), T(0)), dxw = dx;
        double b2 = 0.0;
        for (int k = 0; k < a.K; ++k) {
            const cx<T> yu = yf[k] - cscale(uf[k], us);
            const T w = wk(k);
            const cx<T> xk = yu + cmulc(d[k], a.uniform ? v1 : v1 + cscale(v2, w));
            const cx<T> dxk = cmul(d[k], xk);
            dx = dx + dxk;
            dxw = dxw + cscale(dxk, w);
            if (a.want_xrrs) b2 += (double)cabs2(cscale(yu, rho) + cmulc(d[k], y.s + cscale(y.zd, rho * w)));
            x[k] = xk;
        }
        a.rwf[grp] = dxw;
        if (a.want_obj) acc[0] += parseval_weight((int)(pix % Wf), Wf, a.W) * (double)cabs2(dx - y.s);
        if (a.want_xrrs) {
            double d2 = 0.0, ax2 = 0.0;
            for (int k = 0; k < a.K; ++k) {
                const cx<T> yu = yf[k] - cscale(uf[k], us);
                const T w = wk(k);
                const cx<T> ax = cmulc(d[k], dx + cscale(dxw, y.tau * w)) + cscale(x[k], rho);
                const cx<T> b = cscale(yu, rho) + cmulc(d[k], y.s + cscale(y.zd, rho * w));
                d2 += (double)cabs2(ax - b);
                ax2 += (double)cabs2(ax);
            }
            acc[1] += d2;
            acc[2] += ax2;
            acc[3] += b2;
        }
    }
    block_sum_store<4>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * 4);
}

// The coefficient block: V elements of a pixel's filter axis per access.
template <typename T, int V>
__global__ void __launch_bounds__(kThreads) rtv_y0_kernel(const RtvYArgs<T> a, int64_t nvec) {
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const bool relax = a.rlx != T(1);
    const T rlx = a.rlx, rl1 = T(1) - a.rlx, us = a.us;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e0 = i * V;
        const Vec<T, V> xv = *reinterpret_cast<const Vec<T, V> *>(a.x + e0);
        const Vec<T, V> uv = *reinterpret_cast<const Vec<T, V> *>(a.u0 + e0);
        Vec<T, V> yv;
        if (relax) yv = *reinterpret_cast<const Vec<T, V> *>(a.y0 + e0);
        int64_t wbase = 0;
        int k0 = 0;
        if (a.wl1.ptr) {
            int64_t r = e0 / a.K;
            k0 = (int)(e0 - r * a.K);
            const int n = (int)(r % a.N);
            r /= a.N;
            const int c = (int)(r % a.C);
            r /= a.C;
            const int xx = (int)(r % a.W);
            const int64_t yy = r / a.W;
            wbase = yy * a.wl1.stride[0] + xx * a.wl1.stride[1] + c * a.wl1.stride[2] + n * a.wl1.stride[3];
        }
        Vec<T, V> yn, un;
        T sr = T(0), sa = T(0), sy = T(0), sl = T(0);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            // AXnr_0 = x, AX = rlx AXnr + (1 - rlx) Yprev (cbpdntv.py:1319-1339)
            const T ax = xv.v[j];
            const T axr = relax ? fma1(rlx, ax, rl1 * yv.v[j]) : ax;
            const T v = fma1(us, uv.v[j], axr);
            // y0 = prox_l1(AX_0 + U_0, (lmbda / rho) wl1), U_0 += AX_0 - y0
            const T w1 = a.wl1.ptr ? a.wl1.ptr[wbase + (k0 + j) * a.wl1.stride[4]] : T(1);
            const T m = rtv_abs(v) - a.thr_l1 * w1;
            const T yl = m > T(0) ? (v < T(0) ? -m : m) : T(0);
            yn.v[j] = yl;
            un.v[j] = v - yl;
            sr = fma1(ax - yl, ax - yl, sr);
            sa = fma1(ax, ax, sa);
            sy = fma1(yl, yl, sy);
            sl += rtv_abs(w1 * (a.geval_y ? yl : ax));
        }
        *reinterpret_cast<Vec<T, V> *>(a.y0 + e0) = yn;
        *reinterpret_cast<Vec<T, V> *>(a.u0 + e0) = un;
        acc[0] += (double)sr;
        acc[1] += (double)sa;
        acc[2] += (double)sy;
        acc[3] += (double)sl;
    }
    block_sum_store<5>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * 8);
}

// The gradient block: one thread per (pixel, n); the l2 norm of prox_l2 runs over the C channels and
// the two components (cbpdntv.py:1105-1106).  AXnr_1 = G_i rw is the stencil on the weighted
// reconstruction; every thread reads and writes y1 / u1 at its own pixel only.
template <typename T> __global__ void __launch_bounds__(kThreads) rtv_y1_kernel(const RtvYArgs<T> a, int row0) {
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const bool relax = a.rlx != T(1);
    const T rlx = a.rlx, rl1 = T(1) - a.rlx, us = a.us;
    const int64_t total = (int64_t)a.H * a.W * a.N;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int n = (int)(t % a.N);
        const int64_t px = t / a.N;
        const int xx = (int)(px % a.W), yy = (int)(px / a.W);
        const int64_t pxu = (int64_t)(yy == 0 ? a.H - 1 : yy - 1) * a.W + xx;     // predecessor along axis 0
        const int64_t pxl = (int64_t)yy * a.W + (xx == 0 ? a.W - 1 : xx - 1);     // ... along axis 1
        T s2 = T(0), g2 = T(0);
        for (int pass = 0; pass < 2; ++pass) {
            const T nrm = rtv_sqrt(s2);
            const T sc = rtv_shrink(nrm, a.thr_tv);
            T sr = T(0), sa = T(0), sy = T(0);
            for (int c = 0; c < a.C; ++c) {
                const int64_t idx = (px * a.C + c) * a.N + n;
                const T r = a.rw[idx];
                const T a0 = r - a.rw[(pxu * a.C + c) * a.N + n], a1 = r - a.rw[(pxl * a.C + c) * a.N + n];
                const Vec<T, 2> u = *reinterpret_cast<const Vec<T, 2> *>(a.u1 + 2 * idx);
                T x0 = a0, x1 = a1;
                if (relax) {
                    const Vec<T, 2> p = *reinterpret_cast<const Vec<T, 2> *>(a.y1 + 2 * idx);
                    x0 = fma1(rlx, a0, rl1 * p.v[0]);
                    x1 = fma1(rlx, a1, rl1 * p.v[1]);
                }
                const T v0 = fma1(us, u.v[0], x0), v1 = fma1(us, u.v[1], x1);
                if (pass == 0) {
                    s2 = fma1(v0, v0, fma1(v1, v1, s2));
                    g2 = fma1(a0, a0, fma1(a1, a1, g2));
                    continue;
                }
                // y1 = prox_l2((AX + U)_1, mu / rho), U_1 += AX_1 - y1
                Vec<T, 2> yn, un;
                yn.v[0] = sc * v0;
                yn.v[1] = sc * v1;
                un.v[0] = v0 - yn.v[0];
                un.v[1] = v1 - yn.v[1];
                *reinterpret_cast<Vec<T, 2> *>(a.y1 + 2 * idx) = yn;
                *reinterpret_cast<Vec<T, 2> *>(a.u1 + 2 * idx) = un;
                sr = fma1(a0 - yn.v[0], a0 - yn.v[0], fma1(a1 - yn.v[1], a1 - yn.v[1], sr));
                sa = fma1(a0, a0, fma1(a1, a1, sa));
                sy = fma1(yn.v[0], yn.v[0], fma1(yn.v[1], yn.v[1], sy));
            }
            if (pass == 1) {
                acc[0] += (double)sr;
                acc[1] += (double)sa;
                acc[2] += (double)sy;
                // (||y1|| of the pixel is the shrunk norm)
                acc[4] += (double)(a.geval_y ? sc * nrm : rtv_sqrt(g2));
            }
        }
    }
    block_sum_store<5>(acc, dyn_lds<double>(), a.partials + ((int64_t)row0 + blockIdx.x) * 8);
}

template <typename T>
__global__ void __launch_bounds__(kThreads) rtv_adjoint_kernel(const T *__restrict__ y1, const T *__restrict__ u1,
                                                               T *__restrict__ zy, T *__restrict__ zu, int H, int W,
                                                               int CN) {
    const int64_t total = (int64_t)H * W * CN;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int cn = (int)(t % CN);
        const int64_t px = t / CN;
        const int xx = (int)(px % W), yy = (int)(px / W);
        const int64_t sd = ((int64_t)(yy + 1 == H ? 0 : yy + 1) * W + xx) * CN + cn;     // successor along axis 0
        const int64_t sr = ((int64_t)yy * W + (xx + 1 == W ? 0 : xx + 1)) * CN + cn;     // ... along axis 1
        // sum_i G_i^T v_i, G_i^T v = v - (its successor along i)
        zy[t] = (y1[2 * t] - y1[2 * sd]) + (y1[2 * t + 1] - y1[2 * sr + 1]);
        zu[t] = (u1[2 * t] - u1[2 * sd]) + (u1[2 * t + 1] - u1[2 * sr + 1]);
    }
}

template <typename T> __global__ void __launch_bounds__(kThreads) rtv_dual_kernel(const RtvDualArgs<T> a) {
    const int Wf = a.W / 2 + 1;
    const int64_t total = a.npix * a.CN * a.K;
    double acc[2] = {0.0, 0.0};
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t grp = t / a.K;
        const int k = (int)(t - grp * a.K);
        const int64_t pix = grp / a.CN;
        const cx<T> wd = cscale(a.df[pix * a.K + k], a.tvw[k]);
        const cx<T> s = (a.yf[t] - a.yfp[t]) + cmulc(wd, a.zyf[grp] - a.zyfp[grp]);
        const cx<T> u = a.uf[t] + cmulc(wd, a.zuf[grp]);
        const double pw = parseval_weight((int)(pix % Wf), Wf, a.W);
        acc[0] += pw * (double)cabs2(s);
        acc[1] += pw * (double)cabs2(u);
    }
    block_sum_store<2>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * 4);
}

inline bool rtv_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace

template <typename T> int launch_rtv_solve(hipStream_t st, const RtvSolveArgs<T> &a) {
    const size_t lds = sizeof(double) * kRtvScratch;
    int grid;
    if (a.K % 2 == 0 && rtv_pow2(a.K / 2) && a.K / 2 <= kWave) {
        grid = grid_for(a.npix * a.CN * (a.K / 2));
        hipLaunchKernelGGL((rtv_solve_wave_kernel<T>), dim3(grid), dim3(kThreads), lds, st, a);
    } else {
        grid = grid_for(a.npix * a.CN);
        hipLaunchKernelGGL((rtv_solve_generic_kernel<T>), dim3(grid), dim3(kThreads), lds, st, a);
    }
    SA_HIP(hipGetLastError());
    return grid;
}

template <typename T> int launch_rtv_ystep(hipStream_t st, const RtvYArgs<T> &a) {
    const size_t lds = sizeof(double) * kRtvScratch;
    constexpr int full = 16 / (int)sizeof(T);
    const int64_t E = (int64_t)a.H * a.W * a.C * a.N * a.K;
    int g0;
    if (a.K % full == 0) {
        g0 = grid_for(E / full);
        hipLaunchKernelGGL((rtv_y0_kernel<T, full>), dim3(g0), dim3(kThreads), lds, st, a, E / full);
    } else {
        g0 = grid_for(E);
        hipLaunchKernelGGL((rtv_y0_kernel<T, 1>), dim3(g0), dim3(kThreads), lds, st, a, E);
    }
    SA_HIP(hipGetLastError());
    const int g1 = grid_for((int64_t)a.H * a.W * a.N);
    hipLaunchKernelGGL((rtv_y1_kernel<T>), dim3(g1), dim3(kThreads), lds, st, a, g0);
    SA_HIP(hipGetLastError());
    return g0 + g1;
}

template <typename T>
void launch_rtv_adjoint(hipStream_t st, const T *y1, const T *u1, T *zy, T *zu, int H, int W, int CN) {
    hipLaunchKernelGGL((rtv_adjoint_kernel<T>), dim3(grid_for((int64_t)H * W * CN)), dim3(kThreads), 0, st, y1, u1, zy,
                       zu, H, W, CN);
    SA_HIP(hipGetLastError());
}

template <typename T> int launch_rtv_dual(hipStream_t st, const RtvDualArgs<T> &a) {
    const int grid = grid_for(a.npix * a.CN * a.K);
    hipLaunchKernelGGL((rtv_dual_kernel<T>), dim3(grid), dim3(kThreads), sizeof(double) * kRtvScratch, st, a);
    SA_HIP(hipGetLastError());
    return grid;
}

#define SA_RTV_INST(T)                                                                  \
    template int launch_rtv_solve<T>(hipStream_t, const RtvSolveArgs<T> &);             \
    template int launch_rtv_ystep<T>(hipStream_t, const RtvYArgs<T> &);                 \
    template void launch_rtv_adjoint<T>(hipStream_t, const T *, const T *, T *, T *, int, int, int); \
    template int launch_rtv_dual<T>(hipStream_t, const RtvDualArgs<T> &);
SA_RTV_INST(float)
SA_RTV_INST(double)

}  // namespace sporco_amd
