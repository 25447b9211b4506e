// csc_spline.hip -- the kernels of csc_spline.h: spl_solve, dct_post, dct_pre (pointwise over pairs of rows of the
// half spectrum), spl_ystep, spl_permute (pointwise over pairs of columns of the image), spl_tables, spl_sumsq.
// float32 / float64, any H >= 1, W >= 2, any number of planes.
#include "csc_spline.h"
#include "csc_kernels_dev.h"

#include <algorithm>

namespace sporco_amd {

namespace {

// where sample n of an axis of length N goes: the even samples in order, the odd ones reversed behind them
__device__ __forceinline__ int spl_vidx(int n, int N) { return (n & 1) ? N - 1 - (n >> 1) : (n >> 1); }

template <typename T> __device__ __forceinline__ T spl_abs(T v) { return v < T(0) ? -v : v; }
// prox_l1: sign(v) max(0, |v| - alpha) (sporco/prox/_lp.py:144-183)
template <typename T> __device__ __forceinline__ T spl_soft(T v, T alpha) {
    const T b = spl_abs(v) - alpha;
    return b > T(0) ? (v < T(0) ? -b : b) : T(0);
}

template <typename T> __device__ __forceinline__ cx<T> spl_w(const SplTab<T> &t) { return mk<T>(t.wr, t.wi); }

// ---- the pair of stored rows {k1, kb = (H - k1) mod H} at the stored column k2 ---------------------------------
// c[0..3]: the coefficients (k1, k2), (k1, km), (kb, k2), (kb, km), km = W - k2; has_m: km is a column of its
// own (0 < k2 < km); has_b: kb is a row of its own (k1 != 0 and 2 k1 != H).
template <typename T> struct SplPair {
    int k1, kb, k2, km;
    bool has_b, has_m;
    SplTab<T> t1, tb, t2, tm;
    __device__ __forceinline__ void at(int k1_, int k2_, const SplSolveArgs<T> &a) {
        k1 = k1_;
        k2 = k2_;
        kb = k1 == 0 ? 0 : a.H - k1;
        km = a.W - k2;
        has_b = kb != k1;
        has_m = k2 > 0 && km > k2;
        t1 = a.th[k1];
        tb = a.th[kb];
        t2 = a.tw[k2];
        tm = a.tw[has_m ? km : k2];
    }
    // the unscaled coefficients Xu from va = Vh[k1, k2], vb = Vh[kb, k2]
    __device__ __forceinline__ void post(cx<T> va, cx<T> vb, T (&c)[4]) const {
        const cx<T> w1 = spl_w(t1), wb = spl_w(tb), w2 = spl_w(t2), wm = spl_w(tm);
        c[0] = T(2) * cmul(w1, cmul(w2, va) + cmulc(w2, cconj(vb))).re;
        c[1] = has_m ? T(2) * cmul(w1, cmul(wm, cconj(vb)) + cmulc(wm, va)).re : T(0);
        c[2] = has_b ? T(2) * cmul(wb, cmul(w2, vb) + cmulc(w2, cconj(va))).re : T(0);
        c[3] = (has_b && has_m) ? T(2) * cmul(wb, cmul(wm, cconj(va)) + cmulc(wm, vb)).re : T(0);
    }
    // ... and back: Vh[k1, k2], Vh[kb, k2] from the four Xu
    __device__ __forceinline__ void pre(const T (&c)[4], cx<T> &va, cx<T> &vb) const {
        const cx<T> w1 = spl_w(t1), wb = spl_w(tb), w2 = spl_w(t2);
        const T half = T(0.5);
        // Xu[., W - k2]: 0 at k2 = 0 (column W), the coefficient itself at 2 k2 = W
        const T m0 = has_m ? c[1] : (k2 == 0 ? T(0) : c[0]);
        const T m1 = has_m ? c[3] : (k2 == 0 ? T(0) : c[2]);
        const cx<T> za = cscale(cmulc(w2, mk<T>(c[0], -m0)), half);
        // Z[H - k1, k2]: row H is zero (k1 = 0), the row itself at 2 k1 = H
        cx<T> zb = mk<T>(T(0), T(0));
        if (has_b) zb = cscale(cmulc(w2, mk<T>(c[2], -m1)), half);
        else if (k1 != 0) zb = za;
        va = cscale(cmulc(w1, za + mul_mi(zb)), half);
        vb = cscale(cmulc(wb, zb + mul_mi(za)), half);
    }
    __device__ __forceinline__ T alpha(int j) const { return ((j & 2) ? tb.al : t1.al) + ((j & 1) ? tm.al : t2.al); }
    __device__ __forceinline__ T scale(int j) const { return ((j & 2) ? tb.s : t1.s) * ((j & 1) ? tm.s : t2.s); }
    __device__ __forceinline__ bool has(int j) const { return (!(j & 2) || has_b) && (!(j & 1) || has_m); }
    __device__ __forceinline__ int row(int j) const { return (j & 2) ? kb : k1; }
    __device__ __forceinline__ int col(int j) const { return (j & 1) ? km : k2; }
};

template <typename T, int V> __device__ __forceinline__ void spl_ld(const cx<T> *p, cx<T> (&v)[V]) {
    const CxVec<T, V> t = *reinterpret_cast<const CxVec<T, V> *>(p);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = t.v[j];
}
template <typename T, int V> __device__ __forceinline__ void spl_st(cx<T> *p, const cx<T> (&v)[V]) {
    CxVec<T, V> t;
#pragma unroll
    for (int j = 0; j < V; ++j) t.v[j] = v[j];
    *reinterpret_cast<CxVec<T, V> *>(p) = t;
}
template <typename T, int V> __device__ __forceinline__ void spl_ldr(const T *p, T (&v)[V]) {
    const Vec<T, V> t = *reinterpret_cast<const Vec<T, V> *>(p);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = t.v[j];
}
template <typename T, int V> __device__ __forceinline__ void spl_str(T *p, const T (&v)[V]) {
    Vec<T, V> t;
#pragma unroll
    for (int j = 0; j < V; ++j) t.v[j] = v[j];
    *reinterpret_cast<Vec<T, V> *>(p) = t;
}

// MODE 0: spl_solve (post-twiddle, Gamma, pre-twiddle, in place); 1: dct_post (wf -> xr); 2: dct_pre (xr -> wf).
// A thread takes V consecutive planes of one row pair and column (V divides P: one 16-byte access in float32
// for V = 2), workgroup b the items b, b + gridDim.x, ...: a fixed assignment, so the partial sums repeat.
template <typename T, int V, int MODE>
__global__ void __launch_bounds__(kThreads) spl_solve_kernel(const SplSolveArgs<T> a) {
    const int Hp = a.H / 2 + 1;
    const int64_t PG = a.P / V, n = (int64_t)Hp * a.Wf * PG;
    double acc[kSplSolveSums] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * kThreads + (int)threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const int64_t f = i / PG, p = (i - f * PG) * V;
        const int k1 = (int)(f / a.Wf), k2 = (int)(f - (int64_t)k1 * a.Wf);
        SplPair<T> pr;
        pr.at(k1, k2, a);
        cx<T> *pa = a.wf + ((int64_t)pr.k1 * a.Wf + k2) * a.P + p;
        cx<T> *pb = a.wf + ((int64_t)pr.kb * a.Wf + k2) * a.P + p;
        cx<T> va[V], vb[V];
        T c[V][4];
        if (MODE != 2) {
            spl_ld<T, V>(pa, va);
            if (pr.has_b) spl_ld<T, V>(pb, vb);
#pragma unroll
            for (int v = 0; v < V; ++v) pr.post(va[v], pr.has_b ? vb[v] : va[v], c[v]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                T t[V];
#pragma unroll
                for (int v = 0; v < V; ++v) t[v] = T(0);
                if (pr.has(j)) spl_ldr<T, V>(a.xr + ((int64_t)pr.row(j) * a.W + pr.col(j)) * a.P + p, t);
                const T sc = pr.scale(j);
#pragma unroll
                for (int v = 0; v < V; ++v) c[v][j] = t[v] / sc;
            }
        }
        if (MODE == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!pr.has(j)) continue;
                const T al = pr.alpha(j), sc = pr.scale(j);
                const T den = T(1) + a.lr * (al * al);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const T zu = c[v][j], xu = zu / den;
                    c[v][j] = xu;
                    if (a.want_reg || a.want_lsc) {
                        const T xh = xu * sc;
                        const double r = (double)(al * xh);
                        acc[0] += r * r;
                        if (a.want_lsc) {
                            const double ax = (double)(den * xh), b = (double)(zu * sc), d = ax - b;
                            acc[1] += d * d;
                            acc[2] += ax * ax;
                            acc[3] += b * b;
                        }
                    }
                }
            }
        }
        if (MODE == 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!pr.has(j)) continue;
                const T sc = pr.scale(j);
                T t[V];
#pragma unroll
                for (int v = 0; v < V; ++v) t[v] = c[v][j] * sc;
                spl_str<T, V>(a.xr + ((int64_t)pr.row(j) * a.W + pr.col(j)) * a.P + p, t);
            }
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v) pr.pre(c[v], va[v], vb[v]);
            spl_st<T, V>(pa, va);
            if (pr.has_b) spl_st<T, V>(pb, vb);
        }
    }
    if (MODE == 0) block_sum_store<kSplSolveSums>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * kSplSolveSums);
}

// ---- pointwise over the image: a thread takes V planes of the columns 2 j and 2 j + 1 of one row, whose
// permuted places are j and W - 1 - j: a wave reads and writes runs of adjacent elements on both sides ---------
template <typename T, int V> struct SplItem {
    int64_t n0, n1, p0, p1;      // offsets of the two columns in the natural and in the permuted array
    bool has1;
    __device__ __forceinline__ void at(int64_t i, int H, int W, int64_t P) {
        const int64_t PG = P / V, Wp = (W + 1) / 2;
        const int64_t f = i / PG, p = (i - f * PG) * V;
        const int h = (int)(f / Wp), j = (int)(f - (int64_t)h * Wp);
        const int vh = spl_vidx(h, H);
        has1 = 2 * j + 1 < W;
        n0 = ((int64_t)h * W + 2 * j) * P + p;
        n1 = n0 + P;
        p0 = ((int64_t)vh * W + j) * P + p;
        p1 = ((int64_t)vh * W + (W - 1 - j)) * P + p;
    }
};

template <typename T, int V>
__global__ void __launch_bounds__(kThreads) spl_ystep_kernel(const SplArgs<T> a) {
    const int64_t n = (int64_t)a.H * ((a.W + 1) / 2) * (a.P / V);
    const bool relax = a.rlx != T(1);
    const T rl1 = T(1) - a.rlx;
    double acc[kSplYstepSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * kThreads + (int)threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        SplItem<T, V> it;
        it.at(i, a.H, a.W, a.P);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (c == 1 && !it.has1) continue;
            const int64_t no = c ? it.n1 : it.n0, po = c ? it.p1 : it.p0;
            T x[V], y[V], u[V], s[V], wd[V], ry[V];
            spl_ldr<T, V>(a.xv + po, x);
            spl_ldr<T, V>(a.y + no, y);
            spl_ldr<T, V>(a.u + no, u);
            spl_ldr<T, V>(a.s + no, s);
            if (a.wdf) spl_ldr<T, V>(a.wdf + no, wd);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const T wdv = a.wdf ? wd[v] : a.wdf_s;
                const T uv = a.u_scale * u[v];
                const T ax = relax ? a.rlx * x[v] + rl1 * (y[v] + s[v]) : x[v];
                const T yn = spl_soft((ax - s[v]) + uv, wdv / a.rho);
                const T un = uv + ((ax - yn) - s[v]);
                const T xs = x[v] - s[v];
                const double r = (double)((x[v] - yn) - s[v]), dy = (double)(yn - y[v]);
                acc[0] += r * r;
                acc[1] += (double)x[v] * (double)x[v];
                acc[2] += (double)yn * (double)yn;
                acc[3] += dy * dy;
                acc[4] += (double)un * (double)un;
                acc[5] += (double)spl_abs(wdv * (a.geval_y ? yn : xs));
                y[v] = yn;
                u[v] = un;
                ry[v] = yn + s[v];
            }
            spl_str<T, V>(a.y + no, y);
            spl_str<T, V>(a.u + no, u);
            spl_str<T, V>(a.ry + po, ry);
            spl_str<T, V>(a.ru + po, u);
        }
    }
    block_sum_store<kSplYstepSums>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * kSplYstepSums);
}

template <typename T, int V>
__global__ void __launch_bounds__(kThreads)
    spl_permute_kernel(const T *src, const T *src2, T *dst, int H, int W, int64_t P, int inverse) {
    const int64_t n = (int64_t)H * ((W + 1) / 2) * (P / V);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + (int)threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        SplItem<T, V> it;
        it.at(i, H, W, P);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (c == 1 && !it.has1) continue;
            const int64_t no = c ? it.n1 : it.n0, po = c ? it.p1 : it.p0;
            T t[V], t2[V];
            spl_ldr<T, V>(src + (inverse ? po : no), t);
            if (src2) {
                spl_ldr<T, V>(src2 + (inverse ? po : no), t2);
#pragma unroll
                for (int v = 0; v < V; ++v) t[v] += t2[v];
            }
            spl_str<T, V>(dst + (inverse ? no : po), t);
        }
    }
}

template <typename T> __global__ void __launch_bounds__(kThreads) spl_sumsq_kernel(const T *s, int64_t n, double *partials) {
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * kThreads + (int)threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
        acc[0] += (double)s[i] * (double)s[i];
    block_sum_store<1>(acc, dyn_lds<double>(), partials + blockIdx.x);
}

// entry k of an axis of length N: w = exp(-i pi k / (2 N)), s = sqrt(1 / (4 N)) at k = 0, else sqrt(1 / (2 N)),
// alpha = -2 + 2 cos(pi k / N) (spline.py:163-171); formed in double
template <typename T>
__global__ void __launch_bounds__(kThreads) spl_tables_kernel(int H, int W, SplTab<T> *th, SplTab<T> *tw) {
    const double pi = 3.141592653589793238462643383279;
    for (int i = (int)(blockIdx.x * kThreads + threadIdx.x); i < H + W; i += (int)(gridDim.x * kThreads)) {
        const int N = i < H ? H : W, k = i < H ? i : i - H;
        const double ang = pi * (double)k / (2.0 * (double)N);
        SplTab<T> t;
        t.wr = (T)cos(ang);
        t.wi = (T)(-sin(ang));
        t.s = (T)sqrt((k == 0 ? 0.25 : 0.5) / (double)N);
        t.al = (T)(-2.0 + 2.0 * cos(pi * (double)k / (double)N));
        (i < H ? th : tw)[k] = t;
    }
}

// two planes per access in float32 where the planes pair up
template <typename T> int spl_v(int64_t P) { return (sizeof(T) == 4 && P % 2 == 0) ? 2 : 1; }

template <typename T> void spl_check(const SplSolveArgs<T> &a, const char *what) {
    SA_REQUIRE(a.H >= 1 && a.W >= 2 && a.Wf == a.W / 2 + 1 && a.P >= 1 && a.wf && a.th && a.tw, what);
    SA_REQUIRE((int64_t)a.H * a.W * a.P < (int64_t)1 << 40, "spline: array too large");
}

template <typename T, int MODE> void spl_launch_pairs(hipStream_t st, const SplSolveArgs<T> &a, int nb) {
    const size_t lds = MODE == 0 ? sizeof(double) * kSplSolveSums * (kThreads / kWave) : 0;
    if (spl_v<T>(a.P) == 2) {
        if constexpr (sizeof(T) == 4) hipLaunchKernelGGL((spl_solve_kernel<T, 2, MODE>), dim3(nb), dim3(kThreads), lds, st, a);
    } else {
        hipLaunchKernelGGL((spl_solve_kernel<T, 1, MODE>), dim3(nb), dim3(kThreads), lds, st, a);
    }
    SA_HIP(hipGetLastError());
}

int spl_blocks_for(int64_t items) {
    // about four workgroups a compute unit at the most
    return (int)std::min<int64_t>(kSplMaxBlocks, std::max<int64_t>(1, ceil_div(items, kThreads)));
}

}  // namespace

template <typename T> int spl_solve_blocks(const SplSolveArgs<T> &a) {
    return spl_blocks_for((int64_t)(a.H / 2 + 1) * a.Wf * (a.P / spl_v<T>(a.P)));
}

template <typename T> int launch_spl_solve(hipStream_t st, const SplSolveArgs<T> &a) {
    spl_check(a, "spl_solve: bad argument");
    SA_REQUIRE(a.partials != nullptr, "spl_solve: null argument");
    const int nb = spl_solve_blocks(a);
    spl_launch_pairs<T, 0>(st, a, nb);
    return nb;
}

template <typename T> void launch_dct_post(hipStream_t st, const SplSolveArgs<T> &a) {
    spl_check(a, "dct_post: bad argument");
    SA_REQUIRE(a.xr != nullptr, "dct_post: null argument");
    spl_launch_pairs<T, 1>(st, a, spl_solve_blocks(a));
}

template <typename T> void launch_dct_pre(hipStream_t st, const SplSolveArgs<T> &a) {
    spl_check(a, "dct_pre: bad argument");
    SA_REQUIRE(a.xr != nullptr, "dct_pre: null argument");
    spl_launch_pairs<T, 2>(st, a, spl_solve_blocks(a));
}

template <typename T> int spl_ystep_blocks(int H, int W, int64_t P) {
    return spl_blocks_for((int64_t)H * ((W + 1) / 2) * (P / spl_v<T>(P)));
}

template <typename T> int launch_spl_ystep(hipStream_t st, const SplArgs<T> &a) {
    SA_REQUIRE(a.s && a.xv && a.y && a.u && a.ry && a.ru && a.partials, "spl_ystep: null argument");
    SA_REQUIRE(a.H >= 1 && a.W >= 2 && a.P >= 1 && (int64_t)a.H * a.W * a.P < (int64_t)1 << 40 && a.rho > T(0),
               "spl_ystep: bad argument");
    const int nb = spl_ystep_blocks<T>(a.H, a.W, a.P);
    const size_t lds = sizeof(double) * kSplYstepSums * (kThreads / kWave);
    if (spl_v<T>(a.P) == 2) {
        if constexpr (sizeof(T) == 4) hipLaunchKernelGGL((spl_ystep_kernel<T, 2>), dim3(nb), dim3(kThreads), lds, st, a);
    } else {
        hipLaunchKernelGGL((spl_ystep_kernel<T, 1>), dim3(nb), dim3(kThreads), lds, st, a);
    }
    SA_HIP(hipGetLastError());
    return nb;
}

template <typename T>
void launch_spl_permute(hipStream_t st, const T *src, const T *src2, T *dst, int H, int W, int64_t P, bool inverse) {
    SA_REQUIRE(src && dst && src != dst && H >= 1 && W >= 2 && P >= 1 && (int64_t)H * W * P < (int64_t)1 << 40,
               "spl_permute: bad argument");
    const int nb = spl_ystep_blocks<T>(H, W, P);
    if (spl_v<T>(P) == 2) {
        if constexpr (sizeof(T) == 4)
            hipLaunchKernelGGL((spl_permute_kernel<T, 2>), dim3(nb), dim3(kThreads), 0, st, src, src2, dst, H, W, P,
                               inverse ? 1 : 0);
    } else {
        hipLaunchKernelGGL((spl_permute_kernel<T, 1>), dim3(nb), dim3(kThreads), 0, st, src, src2, dst, H, W, P,
                           inverse ? 1 : 0);
    }
    SA_HIP(hipGetLastError());
}

template <typename T> int launch_spl_sumsq(hipStream_t st, const T *s, int64_t n, double *partials) {
    SA_REQUIRE(s && partials && n >= 1, "spl_sumsq: bad argument");
    const int nb = spl_blocks_for(n);
    hipLaunchKernelGGL((spl_sumsq_kernel<T>), dim3(nb), dim3(kThreads), sizeof(double) * (kThreads / kWave), st, s, n,
                       partials);
    SA_HIP(hipGetLastError());
    return nb;
}

template <typename T> void launch_spl_tables(hipStream_t st, int H, int W, SplTab<T> *th, SplTab<T> *tw) {
    SA_REQUIRE(H >= 1 && W >= 2 && th && tw, "spl_tables: bad argument");
    hipLaunchKernelGGL((spl_tables_kernel<T>), dim3(grid_for(H + W)), dim3(kThreads), 0, st, H, W, th, tw);
    SA_HIP(hipGetLastError());
}

#define SA_SPL_INST(T)                                                                                      \
    template int spl_solve_blocks<T>(const SplSolveArgs<T> &);                                             \
    template int launch_spl_solve<T>(hipStream_t, const SplSolveArgs<T> &);                                \
    template void launch_dct_post<T>(hipStream_t, const SplSolveArgs<T> &);                                \
    template void launch_dct_pre<T>(hipStream_t, const SplSolveArgs<T> &);                                 \
    template int spl_ystep_blocks<T>(int, int, int64_t);                                                   \
    template int launch_spl_ystep<T>(hipStream_t, const SplArgs<T> &);                                     \
    template void launch_spl_permute<T>(hipStream_t, const T *, const T *, T *, int, int, int64_t, bool);  \
    template int launch_spl_sumsq<T>(hipStream_t, const T *, int64_t, double *);                           \
    template void launch_spl_tables<T>(hipStream_t, int, int, SplTab<T> *, SplTab<T> *);
SA_SPL_INST(float)
SA_SPL_INST(double)

}  // namespace sporco_amd
