// csc_tvdc.hip -- the kernels of csc_tvdc.h: tvdc_ystep, tvdc_adjoint (periodic stencils on the items, strips
// and row segments of TvdPlan), tvdc_solve, tvdc_dual and tvdc_setup (pointwise over the half spectrum).
// float32 / float64, any H, W >= 2, any number of planes; vector TV over up to kTvdMaxChannels channels.
#include "csc_tvdc.h"
#include "csc_kernels_dev.h"

#include <algorithm>

namespace sporco_amd {

namespace {

template <typename T> struct TvdcKArgs {
    TvdcArgs<T> a;
    TvdPlan pl;
};

template <typename T> __device__ __forceinline__ T tvdc_sqrt(T v);
template <> __device__ __forceinline__ float tvdc_sqrt<float>(float v) { return sqrtf(v); }
template <> __device__ __forceinline__ double tvdc_sqrt<double>(double v) { return sqrt(v); }
// prox_l2's factor max(0, a - alpha) / a, 0 at a = 0 (sporco/prox/_lp.py:284-290, zdivide)
template <typename T> __device__ __forceinline__ T tvdc_shrink(T nrm, T alpha) {
    const T b = nrm - alpha;
    return (nrm > T(0) && b > T(0)) ? b / nrm : T(0);
}
template <typename T> __device__ __forceinline__ T tvdc_abs(T v) { return v < T(0) ? -v : v; }
// prox_l1: sign(v) max(0, |v| - alpha) (sporco/prox/_lp.py:144-183)
template <typename T> __device__ __forceinline__ T tvdc_soft(T v, T alpha) {
    const T b = tvdc_abs(v) - alpha;
    return b > T(0) ? (v < T(0) ? -b : b) : T(0);
}

// The item of a thread: `cnt` elements of a row, `estr` apart, the first at e0 (csc_tvd.h).  Every element
// has a place in two kinds of row: the L = W P elements of a block of Y, U, dY, S or a weight (offset
// e0 + j estr) and the W NZ P elements of XH, RY, RU (offset xo[j], the first of its NZ planes).  Bit j of
// `first` / `last`: element j lies in column 0 / W - 1, where the periodic W-neighbour is at the other end.
template <typename T, int G, bool VTV, int NZ> struct TvdcItem {
    int64_t e0, estr, P, wrap, xwrap;
    int64_t xo[G];
    int cnt;
    unsigned first, last;
    bool ok;
    __device__ __forceinline__ void init(const TvdPlan &pl) {
        const int64_t i = (int64_t)blockIdx.x * kTvdThreads + (int)threadIdx.x;
        ok = i < pl.items;
        const int64_t is = ok ? i : 0;
        first = last = 0u;
        P = pl.P;
        wrap = pl.L;
        xwrap = pl.L * NZ;
        if (VTV) {
            const int64_t w = is / pl.N, n = is - w * pl.N;
            e0 = w * pl.P + n;
            estr = pl.N;
            cnt = pl.C;
            if (w == 0) first = ~0u;
            if (w == pl.W - 1) last = ~0u;
#pragma unroll
            for (int j = 0; j < G; ++j) xo[j] = w * pl.P * NZ + n + j * estr;
        } else {
            e0 = is * G;
            estr = 1;
            cnt = G;
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const int64_t w = (e0 + j) / pl.P;
                if (w == 0) first |= 1u << j;
                if (w == pl.W - 1) last |= 1u << j;
                xo[j] = w * pl.P * NZ + ((e0 + j) - w * pl.P);
            }
        }
    }
    __device__ __forceinline__ bool has(int j) const { return !VTV || j < cnt; }
    __device__ __forceinline__ bool is_first(int j) const { return (first >> j) & 1u; }
    __device__ __forceinline__ bool is_last(int j) const { return (last >> j) & 1u; }
    // the item's elements of a row of L elements starting at `row`
    __device__ __forceinline__ void load(const T *row, T (&v)[G]) const {
        if constexpr (!VTV) {
            const Vec<T, G> t = *reinterpret_cast<const Vec<T, G> *>(row + e0);
#pragma unroll
            for (int j = 0; j < G; ++j) v[j] = t.v[j];
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j) v[j] = j < cnt ? row[e0 + j * estr] : T(0);
        }
    }
    __device__ __forceinline__ void store(T *row, const T (&v)[G]) const {
        if constexpr (!VTV) {
            Vec<T, G> t;
#pragma unroll
            for (int j = 0; j < G; ++j) t.v[j] = v[j];
            *reinterpret_cast<Vec<T, G> *>(row + e0) = t;
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j)
                if (j < cnt) row[e0 + j * estr] = v[j];
        }
    }
    // ... and of a row of W NZ P elements (plane `z` of the NZ): one access where the row is not interleaved
    __device__ __forceinline__ void xload(const T *row, int z, T (&v)[G]) const {
        if constexpr (NZ == 1) {
            load(row, v);
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j) v[j] = has(j) ? row[xo[j] + z * P] : T(0);
        }
    }
    __device__ __forceinline__ void xstore(T *row, int z, const T (&v)[G]) const {
        if constexpr (NZ == 1) {
            store(row, v);
        } else {
#pragma unroll
            for (int j = 0; j < G; ++j)
                if (has(j)) row[xo[j] + z * P] = v[j];
        }
    }
    // the periodic left neighbours in a row of W NZ P elements
    __device__ __forceinline__ void xleft(const T *row, T (&l)[G]) const {
#pragma unroll
        for (int j = 0; j < G; ++j) l[j] = has(j) ? row[xo[j] - P * NZ + (is_first(j) ? xwrap : 0)] : T(0);
    }
    // the periodic right neighbours in a row of L elements
    __device__ __forceinline__ void right(const T *row, T (&r)[G]) const {
#pragma unroll
        for (int j = 0; j < G; ++j) r[j] = has(j) ? row[e0 + j * estr + P - (is_last(j) ? wrap : 0)] : T(0);
    }
};

template <int G, typename T> __device__ __forceinline__ void tvdc_zero(T (&v)[G]) {
#pragma unroll
    for (int j = 0; j < G; ++j) v[j] = T(0);
}

// relax_AX + ystep + ustep (admm.py:396-437; tvl2.py:613-619, tvl1.py:648-658) on the periodic gradient of X.
// A thread walks down the rows of its segment with the row above in registers; the first row of the image
// wraps to the last.
template <typename T, int G, bool VTV, bool L1>
__global__ void __launch_bounds__(kTvdThreads) tvdc_ystep_kernel(const TvdcKArgs<T> ka) {
    constexpr int NZ = L1 ? 2 : 1;
    const TvdcArgs<T> &a = ka.a;
    const TvdPlan &pl = ka.pl;
    TvdcItem<T, G, VTV, NZ> it;
    it.init(pl);
    const int ys = (int)blockIdx.y * pl.rows, ye = ys + pl.rows < pl.H ? ys + pl.rows : pl.H;
    const int64_t L = pl.L, E = L * pl.H, XL = L * NZ;
    const bool relax = a.rlx != T(1);
    const T rl1 = T(1) - a.rlx;
    const T irho = T(1) / a.rho;
    double acc[kTvdSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (it.ok) {
        T up[G], cur[G];
        it.xload(a.xh + (int64_t)(ys > 0 ? ys - 1 : pl.H - 1) * XL, 0, up);
        for (int y = ys; y < ye; ++y) {
            const int64_t ro = (int64_t)y * L;
            const T *xr = a.xh + (int64_t)y * XL;
            T l[G], a0[G], a1[G], y0[G], y1[G], u0[G], u1[G], d0[G], d1[G], wt[G];
            T hx[G], s[G], yd[G], ud[G], wd[G];
            it.xload(xr, 0, cur);
            it.xleft(xr, l);
            it.load(a.y + ro, y0);
            it.load(a.y + E + ro, y1);
            it.load(a.u + ro, u0);
            it.load(a.u + E + ro, u1);
            if (a.wtv) it.load(a.wtv + ro, wt);
            if (L1) {
                it.xload(xr, 1, hx);
                it.load(a.s + ro, s);
                it.load(a.y + 2 * E + ro, yd);
                it.load(a.u + 2 * E + ro, ud);
                if (a.wdf) it.load(a.wdf + ro, wd);
            }
            T n2[G], grp = T(0);
#pragma unroll
            for (int j = 0; j < G; ++j) {
                n2[j] = T(0);
                if (!it.has(j)) continue;
                a0[j] = cur[j] - up[j];
                a1[j] = cur[j] - l[j];
                // AX = rlx AXnr + (1 - rlx) (Y + c), v = AX + U (u0, u1, ud become v)
                const T x0 = relax ? a.rlx * a0[j] + rl1 * y0[j] : a0[j];
                const T x1 = relax ? a.rlx * a1[j] + rl1 * y1[j] : a1[j];
                u0[j] = x0 + a.u_scale * u0[j];
                u1[j] = x1 + a.u_scale * u1[j];
                n2[j] = u0[j] * u0[j] + u1[j] * u1[j];
                grp += n2[j];
                if (L1) {
                    const T xd = relax ? a.rlx * hx[j] + rl1 * (yd[j] + s[j]) : hx[j];
                    ud[j] = xd + a.u_scale * ud[j];
                }
            }
            T gsum = T(0);
#pragma unroll
            for (int j = 0; j < G; ++j) {
                d0[j] = d1[j] = T(0);
                if (!it.has(j)) continue;
                const T wtj = (!VTV && a.wtv) ? wt[j] : a.wtv_s;
                const T sc = tvdc_shrink(tvdc_sqrt(VTV ? grp : n2[j]), a.thr * wtj);
                const T yn0 = sc * u0[j], yn1 = sc * u1[j];
                d0[j] = yn0 - y0[j];
                d1[j] = yn1 - y1[j];
                u0[j] -= yn0;
                u1[j] -= yn1;
                y0[j] = yn0;
                y1[j] = yn1;
                const double r0 = (double)(a0[j] - yn0), r1 = (double)(a1[j] - yn1);
                double rr = r0 * r0 + r1 * r1;
                double ax2 = (double)a0[j] * (double)a0[j] + (double)a1[j] * (double)a1[j];
                double yy = (double)yn0 * (double)yn0 + (double)yn1 * (double)yn1;
                double uu = (double)u0[j] * (double)u0[j] + (double)u1[j] * (double)u1[j];
                if (L1) {
                    // the data block: Y_d = prox_l1(AX_d + U_d - S, Wdf / rho), U_d += AX_d - Y_d - S
                    const T wdj = a.wdf ? wd[j] : a.wdf_s;
                    const T vd = ud[j] - s[j];
                    const T ynd = tvdc_soft(vd, irho * wdj);
                    ud[j] = vd - ynd;
                    yd[j] = ynd;
                    const T xs = hx[j] - s[j];
                    const double rd = (double)(xs - ynd);
                    rr += rd * rd;
                    ax2 += (double)hx[j] * (double)hx[j];
                    yy += (double)ynd * (double)ynd;
                    uu += (double)ud[j] * (double)ud[j];
                    acc[5] += (double)tvdc_abs(wdj * (a.geval_y ? ynd : xs));
                }
                acc[0] += rr;
                acc[1] += ax2;
                acc[2] += yy;
                acc[4] += uu;
                const T g2 = a.geval_y ? yn0 * yn0 + yn1 * yn1 : a0[j] * a0[j] + a1[j] * a1[j];
                if (VTV) gsum += g2;
                else acc[3] += (double)(wtj * tvdc_sqrt(g2));
            }
            if (VTV) acc[3] += (double)(a.wtv_s * tvdc_sqrt(gsum));
            it.store(a.y + ro, y0);
            it.store(a.y + E + ro, y1);
            it.store(a.u + ro, u0);
            it.store(a.u + E + ro, u1);
            if (L1) {
                it.store(a.y + 2 * E + ro, yd);
                it.store(a.u + 2 * E + ro, ud);
            }
            if (a.dy) {
                it.store(a.dy + ro, d0);
                it.store(a.dy + E + ro, d1);
            }
#pragma unroll
            for (int j = 0; j < G; ++j) up[j] = cur[j];
        }
    }
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    block_sum_store<kTvdSums>(acc, dyn_lds<double>(), a.partials + blk * kTvdSums);
}

// RY = G^T Y_g (l1: and Y_d beside it), RU the same of U: (G^T v)[h, w] = (v_0[h, w] - v_0[h + 1, w]) +
// (v_1[h, w] - v_1[h, w + 1]), indices periodic.  A thread walks down its rows with block 0 of the current
// row in registers and reads the row below; the last row of the image wraps to the first.  l2: the same
// stencil on dY = Y - Yprev, differenced before it (csc_tvd.h), for the dual residual.
template <typename T, int G, bool VTV, bool L1>
__global__ void __launch_bounds__(kTvdThreads) tvdc_adjoint_kernel(const TvdcKArgs<T> ka) {
    constexpr int NZ = L1 ? 2 : 1;
    const TvdcArgs<T> &a = ka.a;
    const TvdPlan &pl = ka.pl;
    TvdcItem<T, G, VTV, NZ> it;
    it.init(pl);
    const int ys = (int)blockIdx.y * pl.rows, ye = ys + pl.rows < pl.H ? ys + pl.rows : pl.H;
    const int64_t L = pl.L, E = L * pl.H, XL = L * NZ;
    const bool want_dy = !L1 && a.dy != nullptr;
    double acc[kTvdSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (it.ok) {
        T y0[G], u0[G], d0[G];
        tvdc_zero<G>(d0);
        it.load(a.y + (int64_t)ys * L, y0);
        it.load(a.u + (int64_t)ys * L, u0);
        if (want_dy) it.load(a.dy + (int64_t)ys * L, d0);
        for (int y = ys; y < ye; ++y) {
            const int64_t ro = (int64_t)y * L, rn = (int64_t)(y + 1 < pl.H ? y + 1 : 0) * L;
            T yn[G], un[G], dn[G], y1[G], u1[G], d1[G], yr[G], ur[G], dr[G], gy[G], gu[G];
            tvdc_zero<G>(dn);
            tvdc_zero<G>(d1);
            tvdc_zero<G>(dr);
            it.load(a.y + rn, yn);
            it.load(a.u + rn, un);
            it.load(a.y + E + ro, y1);
            it.load(a.u + E + ro, u1);
            it.right(a.y + E + ro, yr);
            it.right(a.u + E + ro, ur);
            if (want_dy) {
                it.load(a.dy + rn, dn);
                it.load(a.dy + E + ro, d1);
                it.right(a.dy + E + ro, dr);
            }
#pragma unroll
            for (int j = 0; j < G; ++j) {
                gy[j] = gu[j] = T(0);
                if (!it.has(j)) continue;
                gy[j] = (y0[j] - yn[j]) + (y1[j] - yr[j]);
                gu[j] = (u0[j] - un[j]) + (u1[j] - ur[j]);
                if (!L1) {
                    const T gd = (d0[j] - dn[j]) + (d1[j] - dr[j]);
                    acc[0] += (double)gd * (double)gd;
                    acc[1] += (double)gu[j] * (double)gu[j];
                }
                y0[j] = yn[j];
                u0[j] = un[j];
                d0[j] = dn[j];
            }
            it.xstore(a.ry + (int64_t)y * XL, 0, gy);
            it.xstore(a.ru + (int64_t)y * XL, 0, gu);
            if (L1) {
                T yd[G], ud[G];
                it.load(a.y + 2 * E + ro, yd);
                it.load(a.u + 2 * E + ro, ud);
                it.xstore(a.ry + (int64_t)y * XL, 1, yd);
                it.xstore(a.ru + (int64_t)y * XL, 1, ud);
            }
        }
    }
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    block_sum_store<kTvdSums>(acc, dyn_lds<double>(), a.partials + blk * kTvdSums);
}

// ---- pointwise over the half spectrum -----------------------------------------------------------------
// A thread takes V consecutive planes of one frequency (V divides P: one 16-byte access in float32 for
// V = 2), workgroup b the groups b, b + gridDim.x, ...: a fixed assignment, so the partial sums repeat.
template <typename T, int V> struct TvdcFreq {
    int64_t hw, p;     // frequency h Wf + wf, first plane
    int h, wf;
    __device__ __forceinline__ void at(int64_t i, const TvdcSolveArgs<T> &a) {
        const int64_t e = i * V;
        hw = e / a.P;
        p = e - hw * a.P;
        h = (int)(hw / a.Wf);
        wf = (int)(hw - (int64_t)h * a.Wf);
    }
};
template <typename T, int V> __device__ __forceinline__ void tvdc_ld(const cx<T> *p, cx<T> (&v)[V]) {
    const CxVec<T, V> t = *reinterpret_cast<const CxVec<T, V> *>(p);
#pragma unroll
    for (int j = 0; j < V; ++j) v[j] = t.v[j];
}
template <typename T, int V> __device__ __forceinline__ void tvdc_st(cx<T> *p, const cx<T> (&v)[V]) {
    CxVec<T, V> t;
#pragma unroll
    for (int j = 0; j < V; ++j) t.v[j] = v[j];
    *reinterpret_cast<CxVec<T, V> *>(p) = t;
}
// Af and |Af|^2 of V planes: per plane (PA = P), or one value for all of them (PA = 1)
template <typename T, int V>
__device__ __forceinline__ void tvdc_ld_a(const TvdcSolveArgs<T> &a, const TvdcFreq<T, V> &f, bool want_af,
                                          cx<T> (&af)[V], T (&aha)[V]) {
    if (a.PA == 1) {
        const cx<T> t = want_af ? a.af[f.hw] : mk<T>(T(0), T(0));
        const T g = a.aha[f.hw];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            af[j] = t;
            aha[j] = g;
        }
    } else {
        if (want_af) tvdc_ld<T, V>(a.af + f.hw * a.P + f.p, af);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (!want_af) af[j] = mk<T>(T(0), T(0));
            aha[j] = a.aha[f.hw * a.P + f.p + j];
        }
    }
}

template <typename T, int V, bool L1>
__global__ void __launch_bounds__(kThreads) tvdc_solve_kernel(const TvdcSolveArgs<T> a) {
    constexpr int NZ = L1 ? 2 : 1;
    const int64_t n = (int64_t)a.H * a.Wf * a.P / V;
    const bool want_af = L1 || a.want_dfid;
    double acc[kTvdcSolveSums] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * kThreads + (int)threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        TvdcFreq<T, V> f;
        f.at(i, a);
        cx<T> z0[V], z1[V], bs[V], af[V], sf[V], xf[V], hxf[V];
        T aha[V];
        cx<T> *w0 = a.wf + f.hw * a.P * NZ + f.p;
        tvdc_ld<T, V>(w0, z0);
        if (L1) tvdc_ld<T, V>(w0 + a.P, z1);
        tvdc_ld<T, V>(a.ahsf + f.hw * a.P + f.p, bs);
        tvdc_ld_a<T, V>(a, f, want_af, af, aha);
        if (a.want_dfid) tvdc_ld<T, V>(a.sf + f.hw * a.P + f.p, sf);
        const T gh = a.ch[f.h] + a.cw[f.wf];
        const double pw = parseval_weight(f.wf, a.Wf, a.W);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            cx<T> b;
            T den;
            if (L1) {
                b = (bs[j] + z0[j]) + cmulc(af[j], z1[j]);
                den = aha[j] + gh;
            } else {
                b = bs[j] + cscale(z0[j], a.rho);
                den = aha[j] + a.rho * gh;
            }
            xf[j] = mk<T>(b.re / den, b.im / den);
            if (want_af) hxf[j] = cmul(af[j], xf[j]);
            if (a.want_dfid) {
                const cx<T> e = hxf[j] - sf[j];
                acc[0] += pw * ((double)e.re * (double)e.re + (double)e.im * (double)e.im);
            }
            if (a.want_lsc) {
                const cx<T> ax = cscale(xf[j], den), d = ax - b;
                acc[1] += (double)d.re * (double)d.re + (double)d.im * (double)d.im;
                acc[2] += (double)ax.re * (double)ax.re + (double)ax.im * (double)ax.im;
                acc[3] += (double)b.re * (double)b.re + (double)b.im * (double)b.im;
            }
        }
        tvdc_st<T, V>(w0, xf);
        if (L1) tvdc_st<T, V>(w0 + a.P, hxf);
    }
    block_sum_store<kTvdcSolveSums>(acc, dyn_lds<double>(), a.partials + (int64_t)blockIdx.x * kTvdcSolveSums);
}

// || A^T U ||^2 of the l1 problem by Parseval: A^T U = G^T U_g + H^T U_d, its spectrum wf_0 + conj(Af) wf_1
template <typename T, int V>
__global__ void __launch_bounds__(kThreads) tvdc_dual_kernel(const TvdcSolveArgs<T> a) {
    const int64_t n = (int64_t)a.H * a.Wf * a.P / V;
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * kThreads + (int)threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        TvdcFreq<T, V> f;
        f.at(i, a);
        cx<T> z0[V], z1[V], af[V];
        T aha[V];
        const cx<T> *w0 = a.wf + f.hw * a.P * 2 + f.p;
        tvdc_ld<T, V>(w0, z0);
        tvdc_ld<T, V>(w0 + a.P, z1);
        tvdc_ld_a<T, V>(a, f, true, af, aha);
        const double pw = parseval_weight(f.wf, a.Wf, a.W);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const cx<T> t = z0[j] + cmulc(af[j], z1[j]);
            acc[0] += pw * ((double)t.re * (double)t.re + (double)t.im * (double)t.im);
        }
    }
    block_sum_store<1>(acc, dyn_lds<double>(), a.partials + blockIdx.x);
}

template <typename T>
__global__ void __launch_bounds__(kThreads) tvdc_setup_kernel(const TvdcSolveArgs<T> a, T *aha, cx<T> *ahsf) {
    const int64_t nf = (int64_t)a.H * a.Wf, stride = (int64_t)gridDim.x * kThreads;
    const int64_t i0 = (int64_t)blockIdx.x * kThreads + (int)threadIdx.x;
    if (aha)
        for (int64_t i = i0; i < nf * a.PA; i += stride) aha[i] = cabs2(a.af[i]);
    if (ahsf)
        for (int64_t i = i0; i < nf * a.P; i += stride)
            ahsf[i] = cmulc(a.af[a.PA == 1 ? i / a.P : i], a.sf[i]);
}

// ch[k] = 2 - 2 cos(2 pi k / H), k < H, and cw[l] = 2 - 2 cos(2 pi l / W), l < Wf: |Gf_0|^2 and |Gf_1|^2 of
// the filters [1, -1] (sporco/signal.py:230-239), formed in double
template <typename T> __global__ void __launch_bounds__(kThreads) tvdc_tables_kernel(int H, int W, T *ch, T *cw) {
    const double two_pi = 6.283185307179586476925286766559;
    const int Wf = W / 2 + 1;
    for (int i = (int)(blockIdx.x * kThreads + threadIdx.x); i < H + Wf; i += (int)(gridDim.x * kThreads)) {
        if (i < H) ch[i] = (T)(2.0 - 2.0 * cos(two_pi * (double)i / (double)H));
        else cw[i - H] = (T)(2.0 - 2.0 * cos(two_pi * (double)(i - H) / (double)W));
    }
}

template <typename T> TvdcKArgs<T> tvdc_kargs(const TvdcArgs<T> &a, const TvdPlan &pl) {
    SA_REQUIRE(pl.H >= 2 && pl.W >= 2 && pl.L == (int64_t)pl.W * pl.P && pl.rows >= 1 &&
                   (int64_t)pl.rows * pl.nseg >= pl.H && (int64_t)(pl.nseg - 1) * pl.rows < pl.H &&
                   (int64_t)pl.strips * kTvdThreads >= pl.items && pl.nseg <= 65535,
               "tvdc: inconsistent plan");
    if (pl.vtv)
        SA_REQUIRE(pl.cnt == pl.C && pl.C <= pl.G && (int64_t)pl.C * pl.N == pl.P && pl.estr == pl.N &&
                       pl.items == (int64_t)pl.W * pl.N,
                   "tvdc: inconsistent vector TV plan");
    else
        SA_REQUIRE(pl.cnt == pl.G && pl.items * pl.G == pl.L && (size_t)pl.G * sizeof(T) <= 16,
                   "tvdc: inconsistent item width");
    TvdcKArgs<T> ka;
    ka.a = a;
    ka.pl = pl;
    return ka;
}

constexpr size_t kTvdcLds = sizeof(double) * kTvdSums * (kTvdThreads / kWave);

// the instantiation of a plan: G elements per item, planes independent or vector TV, two or three blocks
#define SA_TVDC_DISPATCH_L(KERNEL, L1)                                                                          \
    do {                                                                                                        \
        const dim3 grid((unsigned)pl.strips, (unsigned)pl.nseg), block(kTvdThreads);                            \
        if (pl.vtv) {                                                                                           \
            if (pl.G == 4) hipLaunchKernelGGL((KERNEL<T, 4, true, L1>), grid, block, kTvdcLds, st, ka);         \
            else hipLaunchKernelGGL((KERNEL<T, kTvdMaxChannels, true, L1>), grid, block, kTvdcLds, st, ka);     \
        } else if (pl.G == 4) {                                                                                 \
            if constexpr (sizeof(T) == 4) hipLaunchKernelGGL((KERNEL<T, 4, false, L1>), grid, block, kTvdcLds, st, ka); \
        } else if (pl.G == 2) {                                                                                 \
            hipLaunchKernelGGL((KERNEL<T, 2, false, L1>), grid, block, kTvdcLds, st, ka);                       \
        } else {                                                                                                \
            hipLaunchKernelGGL((KERNEL<T, 1, false, L1>), grid, block, kTvdcLds, st, ka);                       \
        }                                                                                                       \
        SA_HIP(hipGetLastError());                                                                              \
    } while (0)
#define SA_TVDC_DISPATCH(KERNEL)                    \
    do {                                            \
        if (l1) SA_TVDC_DISPATCH_L(KERNEL, true);   \
        else SA_TVDC_DISPATCH_L(KERNEL, false);     \
    } while (0)

template <typename T> void tvdc_check_spectrum(const TvdcSolveArgs<T> &a, const char *what) {
    SA_REQUIRE(a.H >= 2 && a.W >= 2 && a.Wf == a.W / 2 + 1 && a.P >= 1 && (a.PA == a.P || a.PA == 1) && a.af && a.partials,
               what);
    SA_REQUIRE((int64_t)a.H * a.Wf * a.P < (int64_t)1 << 40, "tvdc: spectrum too large");
}
// two planes per access in float32 where the planes pair up
template <typename T> int tvdc_solve_v(const TvdcSolveArgs<T> &a) { return (sizeof(T) == 4 && a.P % 2 == 0) ? 2 : 1; }

}  // namespace

template <typename T> void launch_tvdc_ystep(hipStream_t st, const TvdcArgs<T> &a, const TvdPlan &pl, bool l1) {
    SA_REQUIRE(a.xh && a.y && a.u && a.partials && (!l1 || a.s), "tvdc_ystep: null argument");
    SA_REQUIRE(!(l1 && a.dy), "tvdc_ystep: the l1 problem keeps no Y - Yprev");
    SA_REQUIRE(!(pl.vtv && a.wtv), "tvdc_ystep: vector TV takes a scalar TVWeight");
    const TvdcKArgs<T> ka = tvdc_kargs(a, pl);
    SA_TVDC_DISPATCH(tvdc_ystep_kernel);
}

template <typename T> void launch_tvdc_adjoint(hipStream_t st, const TvdcArgs<T> &a, const TvdPlan &pl, bool l1) {
    SA_REQUIRE(a.y && a.u && a.ry && a.ru && a.partials, "tvdc_adjoint: null argument");
    const TvdcKArgs<T> ka = tvdc_kargs(a, pl);
    SA_TVDC_DISPATCH(tvdc_adjoint_kernel);
}

template <typename T> int tvdc_solve_blocks(const TvdcSolveArgs<T> &a) {
    // about four workgroups a compute unit at the most
    return (int)std::min<int64_t>(1024, std::max<int64_t>(1, ceil_div((int64_t)a.H * a.Wf * a.P / tvdc_solve_v(a), kThreads)));
}

template <typename T> int launch_tvdc_solve(hipStream_t st, const TvdcSolveArgs<T> &a, bool l1) {
    tvdc_check_spectrum(a, "tvdc_solve: bad argument");
    SA_REQUIRE(a.wf && a.ahsf && a.aha && a.ch && a.cw && (!a.want_dfid || a.sf), "tvdc_solve: null argument");
    const int nb = tvdc_solve_blocks(a);
    const size_t lds = sizeof(double) * kTvdcSolveSums * (kThreads / kWave);
    if (tvdc_solve_v(a) == 2) {
        if constexpr (sizeof(T) == 4) {
            if (l1) hipLaunchKernelGGL((tvdc_solve_kernel<T, 2, true>), dim3(nb), dim3(kThreads), lds, st, a);
            else hipLaunchKernelGGL((tvdc_solve_kernel<T, 2, false>), dim3(nb), dim3(kThreads), lds, st, a);
        }
    } else {
        if (l1) hipLaunchKernelGGL((tvdc_solve_kernel<T, 1, true>), dim3(nb), dim3(kThreads), lds, st, a);
        else hipLaunchKernelGGL((tvdc_solve_kernel<T, 1, false>), dim3(nb), dim3(kThreads), lds, st, a);
    }
    SA_HIP(hipGetLastError());
    return nb;
}

template <typename T> int launch_tvdc_dual(hipStream_t st, const TvdcSolveArgs<T> &a) {
    tvdc_check_spectrum(a, "tvdc_dual: bad argument");
    SA_REQUIRE(a.wf && a.aha, "tvdc_dual: null argument");
    const int nb = tvdc_solve_blocks(a);
    const size_t lds = sizeof(double) * (kThreads / kWave);
    if (tvdc_solve_v(a) == 2) {
        if constexpr (sizeof(T) == 4) hipLaunchKernelGGL((tvdc_dual_kernel<T, 2>), dim3(nb), dim3(kThreads), lds, st, a);
    } else {
        hipLaunchKernelGGL((tvdc_dual_kernel<T, 1>), dim3(nb), dim3(kThreads), lds, st, a);
    }
    SA_HIP(hipGetLastError());
    return nb;
}

template <typename T> void launch_tvdc_setup(hipStream_t st, const TvdcSolveArgs<T> &a, T *aha, cx<T> *ahsf) {
    SA_REQUIRE(a.H >= 2 && a.W >= 2 && a.Wf == a.W / 2 + 1 && a.P >= 1 && (a.PA == a.P || a.PA == 1) && a.af &&
                   (!ahsf || a.sf),
               "tvdc_setup: bad argument");
    hipLaunchKernelGGL((tvdc_setup_kernel<T>), dim3(grid_for((int64_t)a.H * a.Wf * a.P)), dim3(kThreads), 0, st, a, aha,
                       ahsf);
    SA_HIP(hipGetLastError());
}

template <typename T> void launch_tvdc_tables(hipStream_t st, int H, int W, T *ch, T *cw) {
    SA_REQUIRE(H >= 2 && W >= 2 && ch && cw, "tvdc_tables: bad argument");
    hipLaunchKernelGGL((tvdc_tables_kernel<T>), dim3(grid_for(H + W / 2 + 1)), dim3(kThreads), 0, st, H, W, ch, cw);
    SA_HIP(hipGetLastError());
}

#define SA_TVDC_INST(T)                                                                                   \
    template void launch_tvdc_ystep<T>(hipStream_t, const TvdcArgs<T> &, const TvdPlan &, bool);         \
    template void launch_tvdc_adjoint<T>(hipStream_t, const TvdcArgs<T> &, const TvdPlan &, bool);       \
    template int tvdc_solve_blocks<T>(const TvdcSolveArgs<T> &);                                         \
    template int launch_tvdc_solve<T>(hipStream_t, const TvdcSolveArgs<T> &, bool);                      \
    template int launch_tvdc_dual<T>(hipStream_t, const TvdcSolveArgs<T> &);                             \
    template void launch_tvdc_setup<T>(hipStream_t, const TvdcSolveArgs<T> &, T *, cx<T> *);             \
    template void launch_tvdc_tables<T>(hipStream_t, int, int, T *, T *);
SA_TVDC_INST(float)
SA_TVDC_INST(double)

}  // namespace sporco_amd
