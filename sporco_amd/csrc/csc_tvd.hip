// csc_tvd.hip -- the kernels of csc_tvd.h: tvd_sweep, tvd_ystep, tvd_adjoint, their three-block forms
// tvl1_ystep, tvl1_adjoint (and the elementwise product of two device arrays).  float32 / float64, any H, W >= 2, any number of planes; vector TV over up to
// kTvdMaxChannels channels.
#include "csc_tvd.h"
#include "csc_kernels_dev.h"

#include <algorithm>

namespace sporco_amd {

TvdPlan tvd_plan(size_t elem_size, int H, int W, int64_t P, int C, bool vtv) {
    SA_REQUIRE(H >= 2 && W >= 2 && P >= 1, "tvd: H, W >= 2 and at least one plane");
    TvdPlan pl;
    pl.H = H;
    pl.W = W;
    pl.P = P;
    pl.L = (int64_t)W * P;
    SA_REQUIRE(pl.L * H < (int64_t)1 << 40, "tvd: array too large");
    pl.vtv = vtv ? 1 : 0;
    if (vtv) {
        SA_REQUIRE(C >= 1 && C <= kTvdMaxChannels && P % C == 0, "tvd: vector TV over 1 ... 8 channels, P = C N");
        pl.C = C;
        pl.N = (int)(P / C);
        pl.G = C <= 4 ? 4 : kTvdMaxChannels;
        pl.cnt = C;
        pl.estr = pl.N;
        pl.items = (int64_t)W * pl.N;
    } else {
        // the widest access that divides a row and still leaves a full strip of items
        int v = (int)(16 / elem_size);
        while (v > 1 && (pl.L % v != 0 || pl.L / v < kTvdThreads)) v >>= 1;
        pl.G = pl.cnt = v;
        pl.items = pl.L / v;
    }
    pl.strips = (int)ceil_div(pl.items, kTvdThreads);
    // about four workgroups a compute unit, a segment no shorter than kTvdMinRows rows
    const int64_t target = ceil_div(1024, pl.strips);
    pl.rows = (int)std::max<int64_t>(kTvdMinRows, ceil_div(H, target));
    pl.nseg = (int)ceil_div(H, pl.rows);
    SA_REQUIRE(pl.nseg <= 65535 && pl.strips < (1 << 30), "tvd: grid too large");
    return pl;
}

namespace {

template <typename T> struct TvdKArgs {
    TvdArgs<T> a;
    TvdPlan pl;
};

template <typename T> __device__ __forceinline__ T tvd_sqrt(T v);
template <> __device__ __forceinline__ float tvd_sqrt<float>(float v) { return sqrtf(v); }
template <> __device__ __forceinline__ double tvd_sqrt<double>(double v) { return sqrt(v); }
// prox_l2's factor max(0, a - alpha) / a, 0 at a = 0 (sporco/prox/_lp.py:284-290, zdivide)
template <typename T> __device__ __forceinline__ T tvd_shrink(T nrm, T alpha) {
    const T b = nrm - alpha;
    return (nrm > T(0) && b > T(0)) ? b / nrm : T(0);
}

// The item of a thread: `cnt` elements of a row, `estr` apart, the first at e0.  Bit j of `first` / `last`:
// element j lies in column 0 / W - 1 (for P < V the elements of an item are different columns).
template <typename T, int G, bool VTV> struct TvdItem {
    int64_t e0, estr;
    int cnt;
    unsigned first, last;
    bool ok;
    __device__ __forceinline__ void init(const TvdPlan &pl) {
        const int64_t i = (int64_t)blockIdx.x * kTvdThreads + (int)threadIdx.x;
        ok = i < pl.items;
        const int64_t is = ok ? i : 0;
        first = last = 0u;
        if (VTV) {
            const int64_t w = is / pl.N, n = is - w * pl.N;
            e0 = w * pl.P + n;
            estr = pl.N;
            cnt = pl.C;
            if (w == 0) first = ~0u;
            if (w == pl.W - 1) last = ~0u;
        } else {
            e0 = is * G;
            estr = 1;
            cnt = G;
#pragma unroll
            for (int j = 0; j < G; ++j) {
                const int64_t w = (e0 + j) / pl.P;
                if (w == 0) first |= 1u << j;
                if (w == pl.W - 1) last |= 1u << j;
            }
        }
    }
    __device__ __forceinline__ bool has(int j) const { return !VTV || j < cnt; }
    __device__ __forceinline__ bool is_first(int j) const { return (first >> j) & 1u; }
    __device__ __forceinline__ bool is_last(int j) const { return (last >> j) & 1u; }
    // the item's elements of the row starting at `row`
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
    // their W-neighbours: P elements before (0 in column 0) and, with RIGHT, after (0 in column W - 1)
    template <bool RIGHT> __device__ __forceinline__ void sides(const T *row, int64_t P, T (&l)[G], T (&r)[G]) const {
#pragma unroll
        for (int j = 0; j < G; ++j) {
            l[j] = r[j] = T(0);
            if (!has(j)) continue;
            const int64_t e = e0 + j * estr;
            if (!is_first(j)) l[j] = row[e - P];
            if (RIGHT && !is_last(j)) r[j] = row[e + P];
        }
    }
};

template <int G, typename T> __device__ __forceinline__ void tvd_zero(T (&v)[G]) {
#pragma unroll
    for (int j = 0; j < G; ++j) v[j] = T(0);
}

// P = A^T (Y - u_scale U) of a row from PD = A^T (Y - U) and Q = A^T U
template <typename T, int G, bool VTV>
__device__ __forceinline__ void tvd_load_p(const TvdArgs<T> &a, const TvdItem<T, G, VTV> &it, int64_t ro, T (&p)[G]) {
    it.load(a.pd + ro, p);
    if (a.u_scale != T(1)) {
        T q[G];
        it.load(a.q + ro, q);
        const T f = T(1) - a.u_scale;
#pragma unroll
        for (int j = 0; j < G; ++j) p[j] += f * q[j];
    }
}

template <typename T, int G, bool VTV>
__global__ void __launch_bounds__(kTvdThreads) tvd_sweep_kernel(const TvdKArgs<T> ka) {
    const TvdArgs<T> &a = ka.a;
    const TvdPlan &pl = ka.pl;
    TvdItem<T, G, VTV> it;
    it.init(pl);
    if (!it.ok) return;
    const int ys = (int)blockIdx.y * pl.rows, ye = ys + pl.rows < pl.H ? ys + pl.rows : pl.H;
    const int64_t L = pl.L;
    T up[G], cur[G], dn[G];
    tvd_zero<G>(up);
    if (ys > 0) it.load(a.xin + (int64_t)(ys - 1) * L, up);
    it.load(a.xin + (int64_t)ys * L, cur);
    for (int y = ys; y < ye; ++y) {
        const int64_t ro = (int64_t)y * L;
        tvd_zero<G>(dn);
        if (y + 1 < pl.H) it.load(a.xin + ro + L, dn);
        T l[G], r[G], p[G], s[G], wd[G], out[G];
        it.template sides<true>(a.xin + ro, pl.P, l, r);
        tvd_load_p<T, G, VTV>(a, it, ro, p);
        it.load(a.s + ro, s);
        if (a.wdf) it.load(a.wdf + ro, wd);
        const int nv = (y > 0 ? 1 : 0) + (y + 1 < pl.H ? 1 : 0);
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const T w = a.wdf ? wd[j] : a.wdf_s, w2 = w * w;
            const T lcw = (T)(nv + (it.is_first(j) ? 0 : 1) + (it.is_last(j) ? 0 : 1));
            const T xs = ((up[j] + dn[j]) + l[j]) + r[j];
            out[j] = (a.rho * (xs + p[j]) + w2 * s[j]) / (w2 + a.rho * lcw);
        }
        it.store(a.xout + ro, out);
#pragma unroll
        for (int j = 0; j < G; ++j) {
            up[j] = cur[j];
            cur[j] = dn[j];
        }
    }
}

template <typename T, int G, bool VTV, bool RES>
__global__ void __launch_bounds__(kTvdThreads) tvd_ystep_kernel(const TvdKArgs<T> ka) {
    const TvdArgs<T> &a = ka.a;
    const TvdPlan &pl = ka.pl;
    TvdItem<T, G, VTV> it;
    it.init(pl);
    const int ys = (int)blockIdx.y * pl.rows, ye = ys + pl.rows < pl.H ? ys + pl.rows : pl.H;
    const int64_t L = pl.L, E = L * pl.H;
    const bool relax = a.rlx != T(1);
    const T rl1 = T(1) - a.rlx;
    double acc[kTvdSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (it.ok) {
        T up[G], cur[G], dn[G];
        tvd_zero<G>(up);
        if (ys > 0) it.load(a.xin + (int64_t)(ys - 1) * L, up);
        it.load(a.xin + (int64_t)ys * L, cur);
        for (int y = ys; y < ye; ++y) {
            const int64_t ro = (int64_t)y * L;
            const bool top = y == 0, bottom = y + 1 == pl.H;
            tvd_zero<G>(dn);
            if (!bottom) it.load(a.xin + ro + L, dn);
            T l[G], r[G], p[G], s[G], wd[G], a0[G], a1[G];
            it.template sides<true>(a.xin + ro, pl.P, l, r);
            tvd_load_p<T, G, VTV>(a, it, ro, p);
            it.load(a.s + ro, s);
            if (a.wdf) it.load(a.wdf + ro, wd);
#pragma unroll
            for (int j = 0; j < G; ++j) {
                if (!it.has(j)) continue;
                const T w = a.wdf ? wd[j] : a.wdf_s, w2 = w * w;
                a0[j] = bottom ? T(0) : dn[j] - cur[j];
                a1[j] = it.is_last(j) ? T(0) : r[j] - cur[j];
                // A^T A X as the reference forms it: G_i^T of the forward differences
                const T ata = ((top ? T(0) : cur[j] - up[j]) - a0[j]) + ((it.is_first(j) ? T(0) : cur[j] - l[j]) - a1[j]);
                const T axv = a.rho * ata + w2 * cur[j], bv = w2 * s[j] + a.rho * p[j];
                const double d = (double)(axv - bv);
                acc[5] += d * d;
                acc[6] += (double)axv * (double)axv;
                acc[7] += (double)bv * (double)bv;
                if (!RES) {
                    const double f = (double)(w * (cur[j] - s[j]));
                    acc[3] += f * f;
                }
            }
            if (!RES) {
                T y0[G], y1[G], u0[G], u1[G], wt[G];
                it.load(a.y + ro, y0);
                it.load(a.y + E + ro, y1);
                it.load(a.u + ro, u0);
                it.load(a.u + E + ro, u1);
                if (a.wtv) it.load(a.wtv + ro, wt);
                T n2[G], grp = T(0);
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    n2[j] = T(0);
                    if (!it.has(j)) continue;
                    // AX = rlx AXnr + (1 - rlx) Y, v = AX + U (u0, u1 become v)
                    const T x0 = relax ? a.rlx * a0[j] + rl1 * y0[j] : a0[j];
                    const T x1 = relax ? a.rlx * a1[j] + rl1 * y1[j] : a1[j];
                    u0[j] = x0 + a.u_scale * u0[j];
                    u1[j] = x1 + a.u_scale * u1[j];
                    n2[j] = u0[j] * u0[j] + u1[j] * u1[j];
                    grp += n2[j];
                }
                T d0[G], d1[G], gsum = T(0);
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    d0[j] = d1[j] = T(0);
                    if (!it.has(j)) continue;
                    const T wtj = (!VTV && a.wtv) ? wt[j] : a.wtv_s;
                    const T sc = tvd_shrink(tvd_sqrt(VTV ? grp : n2[j]), a.thr * wtj);
                    const T yn0 = sc * u0[j], yn1 = sc * u1[j];
                    d0[j] = yn0 - y0[j];
                    d1[j] = yn1 - y1[j];
                    u0[j] -= yn0;
                    u1[j] -= yn1;
                    y0[j] = yn0;
                    y1[j] = yn1;
                    const double r0 = (double)(a0[j] - yn0), r1 = (double)(a1[j] - yn1);
                    acc[0] += r0 * r0 + r1 * r1;
                    acc[1] += (double)a0[j] * (double)a0[j] + (double)a1[j] * (double)a1[j];
                    acc[2] += (double)yn0 * (double)yn0 + (double)yn1 * (double)yn1;
                    const T g2 = a.geval_y ? yn0 * yn0 + yn1 * yn1 : a0[j] * a0[j] + a1[j] * a1[j];
                    if (VTV) gsum += g2;
                    else acc[4] += (double)(wtj * tvd_sqrt(g2));
                }
                if (VTV) acc[4] += (double)(a.wtv_s * tvd_sqrt(gsum));
                it.store(a.y + ro, y0);
                it.store(a.y + E + ro, y1);
                it.store(a.u + ro, u0);
                it.store(a.u + E + ro, u1);
                it.store(a.dy + ro, d0);
                it.store(a.dy + E + ro, d1);
            }
#pragma unroll
            for (int j = 0; j < G; ++j) {
                up[j] = cur[j];
                cur[j] = dn[j];
            }
        }
    }
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    block_sum_store<kTvdSums>(acc, dyn_lds<double>(), a.partials + blk * kTvdSums);
}

template <typename T, int G, bool VTV>
__global__ void __launch_bounds__(kTvdThreads) tvd_adjoint_kernel(const TvdKArgs<T> ka) {
    const TvdArgs<T> &a = ka.a;
    const TvdPlan &pl = ka.pl;
    TvdItem<T, G, VTV> it;
    it.init(pl);
    const int ys = (int)blockIdx.y * pl.rows, ye = ys + pl.rows < pl.H ? ys + pl.rows : pl.H;
    const int64_t L = pl.L, E = L * pl.H;
    double acc[kTvdSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (it.ok) {
        // block 0 of Y - U, U and dY in the row above (0 above the image)
        T zp[G], up[G], dp[G];
        tvd_zero<G>(zp);
        tvd_zero<G>(up);
        tvd_zero<G>(dp);
        if (ys > 0) {
            const int64_t rp = (int64_t)(ys - 1) * L;
            T t[G];
            it.load(a.y + rp, t);
            it.load(a.u + rp, up);
            it.load(a.dy + rp, dp);
#pragma unroll
            for (int j = 0; j < G; ++j) zp[j] = t[j] - up[j];
        }
        for (int y = ys; y < ye; ++y) {
            const int64_t ro = (int64_t)y * L;
            T y0[G], u0[G], d0[G], y1[G], u1[G], d1[G], yl[G], ul[G], dl[G], none[G];
            tvd_zero<G>(y0);
            tvd_zero<G>(u0);
            tvd_zero<G>(d0);
            if (y + 1 < pl.H) {      // (the last row of G_0 is zero: block 0 of that row does not enter)
                it.load(a.y + ro, y0);
                it.load(a.u + ro, u0);
                it.load(a.dy + ro, d0);
            }
            it.load(a.y + E + ro, y1);
            it.load(a.u + E + ro, u1);
            it.load(a.dy + E + ro, d1);
            it.template sides<false>(a.y + E + ro, pl.P, yl, none);
            it.template sides<false>(a.u + E + ro, pl.P, ul, none);
            it.template sides<false>(a.dy + E + ro, pl.P, dl, none);
            T pd[G], q[G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                pd[j] = q[j] = T(0);
                if (!it.has(j)) continue;
                const bool lastc = it.is_last(j);      // (... and the last column of G_1)
                const T y1c = lastc ? T(0) : y1[j], u1c = lastc ? T(0) : u1[j], d1c = lastc ? T(0) : d1[j];
                const T z0 = y0[j] - u0[j];
                pd[j] = (zp[j] - z0) + ((yl[j] - ul[j]) - (y1c - u1c));
                q[j] = (up[j] - u0[j]) + (ul[j] - u1c);
                const T sd = (dp[j] - d0[j]) + (dl[j] - d1c);
                acc[0] += (double)sd * (double)sd;
                acc[1] += (double)q[j] * (double)q[j];
                zp[j] = z0;
                up[j] = u0[j];
                dp[j] = d0[j];
            }
            it.store(a.pd + ro, pd);
            it.store(a.q + ro, q);
        }
    }
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    block_sum_store<kTvdSums>(acc, dyn_lds<double>(), a.partials + blk * kTvdSums);
}

template <typename T> __device__ __forceinline__ T tvd_abs(T v) { return v < T(0) ? -v : v; }
// prox_l1: sign(v) max(0, |v| - alpha) (sporco/prox/_lp.py:144-183)
template <typename T> __device__ __forceinline__ T tvd_soft(T v, T alpha) {
    const T b = tvd_abs(v) - alpha;
    return b > T(0) ? (v < T(0) ? -b : b) : T(0);
}

// tvd_ystep for the three-block constraint (G_0; G_1; I) x - y = (0; 0; s): the same row walk, the data
// block of Y and U at 2 E, no dY.
template <typename T, int G, bool VTV, bool RES>
__global__ void __launch_bounds__(kTvdThreads) tvl1_ystep_kernel(const TvdKArgs<T> ka) {
    const TvdArgs<T> &a = ka.a;
    const TvdPlan &pl = ka.pl;
    TvdItem<T, G, VTV> it;
    it.init(pl);
    const int ys = (int)blockIdx.y * pl.rows, ye = ys + pl.rows < pl.H ? ys + pl.rows : pl.H;
    const int64_t L = pl.L, E = L * pl.H;
    const bool relax = a.rlx != T(1);
    const T rl1 = T(1) - a.rlx;
    const T irho = T(1) / a.rho;
    double acc[kTvdSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (it.ok) {
        T up[G], cur[G], dn[G];
        tvd_zero<G>(up);
        if (ys > 0) it.load(a.xin + (int64_t)(ys - 1) * L, up);
        it.load(a.xin + (int64_t)ys * L, cur);
        for (int y = ys; y < ye; ++y) {
            const int64_t ro = (int64_t)y * L;
            const bool top = y == 0, bottom = y + 1 == pl.H;
            tvd_zero<G>(dn);
            if (!bottom) it.load(a.xin + ro + L, dn);
            T l[G], r[G], p[G], s[G], a0[G], a1[G];
            it.template sides<true>(a.xin + ro, pl.P, l, r);
            tvd_load_p<T, G, VTV>(a, it, ro, p);
            it.load(a.s + ro, s);
#pragma unroll
            for (int j = 0; j < G; ++j) {
                if (!it.has(j)) continue;
                a0[j] = bottom ? T(0) : dn[j] - cur[j];
                a1[j] = it.is_last(j) ? T(0) : r[j] - cur[j];
                // A^T A X = G^T G X + X against A^T (c + Y - U) = P + S
                const T ata = ((top ? T(0) : cur[j] - up[j]) - a0[j]) + ((it.is_first(j) ? T(0) : cur[j] - l[j]) - a1[j]);
                const T axv = ata + cur[j], bv = p[j] + s[j];
                const double d = (double)(axv - bv);
                acc[5] += d * d;
                acc[6] += (double)axv * (double)axv;
                acc[7] += (double)bv * (double)bv;
            }
            if (!RES) {
                T y0[G], y1[G], yd[G], u0[G], u1[G], ud[G], wt[G], wd[G];
                it.load(a.y + ro, y0);
                it.load(a.y + E + ro, y1);
                it.load(a.y + 2 * E + ro, yd);
                it.load(a.u + ro, u0);
                it.load(a.u + E + ro, u1);
                it.load(a.u + 2 * E + ro, ud);
                if (a.wtv) it.load(a.wtv + ro, wt);
                if (a.wdf) it.load(a.wdf + ro, wd);
                T n2[G], grp = T(0);
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    n2[j] = T(0);
                    if (!it.has(j)) continue;
                    // AX = rlx AXnr + (1 - rlx) (Y + c), v = AX + U (u0, u1, ud become v)
                    const T x0 = relax ? a.rlx * a0[j] + rl1 * y0[j] : a0[j];
                    const T x1 = relax ? a.rlx * a1[j] + rl1 * y1[j] : a1[j];
                    const T xd = relax ? a.rlx * cur[j] + rl1 * (yd[j] + s[j]) : cur[j];
                    u0[j] = x0 + a.u_scale * u0[j];
                    u1[j] = x1 + a.u_scale * u1[j];
                    ud[j] = xd + a.u_scale * ud[j];
                    n2[j] = u0[j] * u0[j] + u1[j] * u1[j];
                    grp += n2[j];
                }
                T gsum = T(0);
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    if (!it.has(j)) continue;
                    const T wtj = (!VTV && a.wtv) ? wt[j] : a.wtv_s;
                    const T wdj = a.wdf ? wd[j] : a.wdf_s;
                    const T sc = tvd_shrink(tvd_sqrt(VTV ? grp : n2[j]), a.thr * wtj);
                    const T yn0 = sc * u0[j], yn1 = sc * u1[j];
                    // the data block: Y_d = prox_l1(AX_d + U_d - S, Wdf / rho), U_d += AX_d - Y_d - S
                    const T vd = ud[j] - s[j];
                    const T ynd = tvd_soft(vd, irho * wdj);
                    u0[j] -= yn0;
                    u1[j] -= yn1;
                    ud[j] = vd - ynd;
                    y0[j] = yn0;
                    y1[j] = yn1;
                    yd[j] = ynd;
                    const T xs = cur[j] - s[j];
                    const double r0 = (double)(a0[j] - yn0), r1 = (double)(a1[j] - yn1), rd = (double)(xs - ynd);
                    acc[0] += (r0 * r0 + r1 * r1) + rd * rd;
                    acc[1] += ((double)a0[j] * (double)a0[j] + (double)a1[j] * (double)a1[j]) +
                              (double)cur[j] * (double)cur[j];
                    acc[2] += ((double)yn0 * (double)yn0 + (double)yn1 * (double)yn1) + (double)ynd * (double)ynd;
                    acc[3] += (double)tvd_abs(wdj * (a.geval_y ? ynd : xs));
                    const T g2 = a.geval_y ? yn0 * yn0 + yn1 * yn1 : a0[j] * a0[j] + a1[j] * a1[j];
                    if (VTV) gsum += g2;
                    else acc[4] += (double)(wtj * tvd_sqrt(g2));
                }
                if (VTV) acc[4] += (double)(a.wtv_s * tvd_sqrt(gsum));
                it.store(a.y + ro, y0);
                it.store(a.y + E + ro, y1);
                it.store(a.y + 2 * E + ro, yd);
                it.store(a.u + ro, u0);
                it.store(a.u + E + ro, u1);
                it.store(a.u + 2 * E + ro, ud);
            }
#pragma unroll
            for (int j = 0; j < G; ++j) {
                up[j] = cur[j];
                cur[j] = dn[j];
            }
        }
    }
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    block_sum_store<kTvdSums>(acc, dyn_lds<double>(), a.partials + blk * kTvdSums);
}

// tvd_adjoint with the identity block: PD = G^T (Y_g - U_g) + (Y_d - U_d), Q = G^T U_g + U_d, and the two
// norms of the dual residual (tvl1.py:362-372): sum Q^2 and sum U^2 over every entry of the three blocks
// (the last row of block 0 and the last column of block 1 do not enter the stencil but are part of U).
template <typename T, int G, bool VTV>
__global__ void __launch_bounds__(kTvdThreads) tvl1_adjoint_kernel(const TvdKArgs<T> ka) {
    const TvdArgs<T> &a = ka.a;
    const TvdPlan &pl = ka.pl;
    TvdItem<T, G, VTV> it;
    it.init(pl);
    const int ys = (int)blockIdx.y * pl.rows, ye = ys + pl.rows < pl.H ? ys + pl.rows : pl.H;
    const int64_t L = pl.L, E = L * pl.H;
    double acc[kTvdSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (it.ok) {
        // block 0 of Y - U and of U in the row above (0 above the image)
        T zp[G], up[G];
        tvd_zero<G>(zp);
        tvd_zero<G>(up);
        if (ys > 0) {
            const int64_t rp = (int64_t)(ys - 1) * L;
            T t[G];
            it.load(a.y + rp, t);
            it.load(a.u + rp, up);
#pragma unroll
            for (int j = 0; j < G; ++j) zp[j] = t[j] - up[j];
        }
        for (int y = ys; y < ye; ++y) {
            const int64_t ro = (int64_t)y * L;
            const bool bottom = y + 1 == pl.H;
            T y0[G], u0[G], y1[G], u1[G], yd[G], ud[G], yl[G], ul[G], none[G];
            tvd_zero<G>(y0);
            if (!bottom) it.load(a.y + ro, y0);
            it.load(a.u + ro, u0);
            it.load(a.y + E + ro, y1);
            it.load(a.u + E + ro, u1);
            it.load(a.y + 2 * E + ro, yd);
            it.load(a.u + 2 * E + ro, ud);
            it.template sides<false>(a.y + E + ro, pl.P, yl, none);
            it.template sides<false>(a.u + E + ro, pl.P, ul, none);
            T pd[G], q[G];
#pragma unroll
            for (int j = 0; j < G; ++j) {
                pd[j] = q[j] = T(0);
                if (!it.has(j)) continue;
                acc[1] += ((double)u0[j] * (double)u0[j] + (double)u1[j] * (double)u1[j]) + (double)ud[j] * (double)ud[j];
                const bool lastc = it.is_last(j);
                const T u0c = bottom ? T(0) : u0[j];      // (the last row of G_0 is zero ...)
                const T y1c = lastc ? T(0) : y1[j], u1c = lastc ? T(0) : u1[j];      // (... and the last column of G_1)
                const T z0 = y0[j] - u0c;
                pd[j] = ((zp[j] - z0) + ((yl[j] - ul[j]) - (y1c - u1c))) + (yd[j] - ud[j]);
                q[j] = ((up[j] - u0c) + (ul[j] - u1c)) + ud[j];
                acc[0] += (double)q[j] * (double)q[j];
                zp[j] = z0;
                up[j] = u0c;
            }
            it.store(a.pd + ro, pd);
            it.store(a.q + ro, q);
        }
    }
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    block_sum_store<kTvdSums>(acc, dyn_lds<double>(), a.partials + blk * kTvdSums);
}

// partials[block] = sum s^2 over the block's share of the n elements, in a fixed order
template <typename T>
__global__ void __launch_bounds__(kTvdThreads) tvl1_s2_kernel(const T *__restrict__ s, int64_t n, double *partials) {
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * kTvdThreads + (int)threadIdx.x; i < n; i += (int64_t)gridDim.x * kTvdThreads)
        acc[0] += (double)s[i] * (double)s[i];
    block_sum_store<1>(acc, dyn_lds<double>(), partials + blockIdx.x);
}

template <typename T>
__global__ void __launch_bounds__(kThreads) tvd_mul_kernel(const T *__restrict__ x, const T *__restrict__ y,
                                                           T *__restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = x[i] * y[i];
}

template <typename T> TvdKArgs<T> tvd_kargs(const TvdArgs<T> &a, const TvdPlan &pl) {
    SA_REQUIRE(pl.H >= 2 && pl.W >= 2 && pl.L == (int64_t)pl.W * pl.P && pl.rows >= 1 &&
                   (int64_t)pl.rows * pl.nseg >= pl.H && (int64_t)(pl.nseg - 1) * pl.rows < pl.H &&
                   (int64_t)pl.strips * kTvdThreads >= pl.items && pl.nseg <= 65535,
               "tvd: inconsistent plan");
    if (pl.vtv)
        SA_REQUIRE(pl.cnt == pl.C && pl.C <= pl.G && (int64_t)pl.C * pl.N == pl.P && pl.estr == pl.N &&
                       pl.items == (int64_t)pl.W * pl.N,
                   "tvd: inconsistent vector TV plan");
    else
        SA_REQUIRE(pl.cnt == pl.G && pl.items * pl.G == pl.L && (size_t)pl.G * sizeof(T) <= 16,
                   "tvd: inconsistent item width");
    TvdKArgs<T> ka;
    ka.a = a;
    ka.pl = pl;
    return ka;
}

constexpr size_t kTvdLds = sizeof(double) * kTvdSums * (kTvdThreads / kWave);

// the instantiation of a plan: G elements per item, planes independent or vector TV
#define SA_TVD_DISPATCH(KERNEL, ...)                                                                            \
    do {                                                                                                        \
        const dim3 grid((unsigned)pl.strips, (unsigned)pl.nseg), block(kTvdThreads);                            \
        if (pl.vtv) {                                                                                           \
            if (pl.G == 4) hipLaunchKernelGGL((KERNEL<T, 4, true, ##__VA_ARGS__>), grid, block, kTvdLds, st, ka);  \
            else hipLaunchKernelGGL((KERNEL<T, kTvdMaxChannels, true, ##__VA_ARGS__>), grid, block, kTvdLds, st, ka); \
        } else if (pl.G == 4) {                                                                                 \
            if constexpr (sizeof(T) == 4) hipLaunchKernelGGL((KERNEL<T, 4, false, ##__VA_ARGS__>), grid, block, kTvdLds, st, ka); \
        } else if (pl.G == 2) {                                                                                 \
            hipLaunchKernelGGL((KERNEL<T, 2, false, ##__VA_ARGS__>), grid, block, kTvdLds, st, ka);             \
        } else {                                                                                                \
            hipLaunchKernelGGL((KERNEL<T, 1, false, ##__VA_ARGS__>), grid, block, kTvdLds, st, ka);             \
        }                                                                                                       \
        SA_HIP(hipGetLastError());                                                                              \
    } while (0)

}  // namespace

template <typename T> void launch_tvd_sweep(hipStream_t st, const TvdArgs<T> &a, const TvdPlan &pl) {
    SA_REQUIRE(a.s && a.xin && a.xout && a.xin != a.xout && a.pd && a.q, "tvd_sweep: null argument");
    const TvdKArgs<T> ka = tvd_kargs(a, pl);
    SA_TVD_DISPATCH(tvd_sweep_kernel);
}

template <typename T> void launch_tvd_ystep(hipStream_t st, const TvdArgs<T> &a, const TvdPlan &pl, bool res_only) {
    SA_REQUIRE(a.s && a.xin && a.pd && a.q && a.partials, "tvd_ystep: null argument");
    SA_REQUIRE(res_only || (a.y && a.u && a.dy), "tvd_ystep: null argument");
    SA_REQUIRE(!(pl.vtv && a.wtv), "tvd_ystep: vector TV takes a scalar TVWeight");
    const TvdKArgs<T> ka = tvd_kargs(a, pl);
    if (res_only) SA_TVD_DISPATCH(tvd_ystep_kernel, true);
    else SA_TVD_DISPATCH(tvd_ystep_kernel, false);
}

template <typename T> void launch_tvd_adjoint(hipStream_t st, const TvdArgs<T> &a, const TvdPlan &pl) {
    SA_REQUIRE(a.y && a.u && a.dy && a.pd && a.q && a.partials, "tvd_adjoint: null argument");
    const TvdKArgs<T> ka = tvd_kargs(a, pl);
    SA_TVD_DISPATCH(tvd_adjoint_kernel);
}

template <typename T> void launch_tvl1_ystep(hipStream_t st, const TvdArgs<T> &a, const TvdPlan &pl, bool res_only) {
    SA_REQUIRE(a.s && a.xin && a.pd && a.q && a.partials, "tvl1_ystep: null argument");
    SA_REQUIRE(res_only || (a.y && a.u), "tvl1_ystep: null argument");
    SA_REQUIRE(!(pl.vtv && a.wtv), "tvl1_ystep: vector TV takes a scalar TVWeight");
    const TvdKArgs<T> ka = tvd_kargs(a, pl);
    if (res_only) SA_TVD_DISPATCH(tvl1_ystep_kernel, true);
    else SA_TVD_DISPATCH(tvl1_ystep_kernel, false);
}

template <typename T> void launch_tvl1_adjoint(hipStream_t st, const TvdArgs<T> &a, const TvdPlan &pl) {
    SA_REQUIRE(a.y && a.u && a.pd && a.q && a.partials, "tvl1_adjoint: null argument");
    const TvdKArgs<T> ka = tvd_kargs(a, pl);
    SA_TVD_DISPATCH(tvl1_adjoint_kernel);
}

template <typename T> void launch_tvl1_s2(hipStream_t st, const T *s, const TvdPlan &pl, double *partials) {
    SA_REQUIRE(s && partials && pl.blocks() >= 1 && pl.blocks() < ((int64_t)1 << 31), "tvl1_s2: bad argument");
    hipLaunchKernelGGL((tvl1_s2_kernel<T>), dim3((unsigned)pl.blocks()), dim3(kTvdThreads), kTvdLds, st, s,
                       pl.L * pl.H, partials);
    SA_HIP(hipGetLastError());
}

template <typename T> void launch_tvd_mul(hipStream_t st, const T *x, const T *y, T *out, int64_t n) {
    hipLaunchKernelGGL((tvd_mul_kernel<T>), dim3(grid_for(n)), dim3(kThreads), 0, st, x, y, out, n);
    SA_HIP(hipGetLastError());
}

#define SA_TVD_INST(T)                                                                                  \
    template void launch_tvd_sweep<T>(hipStream_t, const TvdArgs<T> &, const TvdPlan &);               \
    template void launch_tvd_ystep<T>(hipStream_t, const TvdArgs<T> &, const TvdPlan &, bool);         \
    template void launch_tvd_adjoint<T>(hipStream_t, const TvdArgs<T> &, const TvdPlan &);             \
    template void launch_tvl1_ystep<T>(hipStream_t, const TvdArgs<T> &, const TvdPlan &, bool);        \
    template void launch_tvl1_adjoint<T>(hipStream_t, const TvdArgs<T> &, const TvdPlan &);            \
    template void launch_tvl1_s2<T>(hipStream_t, const T *, const TvdPlan &, double *);                \
    template void launch_tvd_mul<T>(hipStream_t, const T *, const T *, T *, int64_t);
SA_TVD_INST(float)
SA_TVD_INST(double)

}  // namespace sporco_amd
