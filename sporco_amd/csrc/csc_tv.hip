// csc_tv.hip -- tv_ystep and tv_adjoint of ConvBPDNScalarTV / ConvBPDNVectorTV (csc_tv.h): two
// streaming launches per iteration, float32 / float64, any H, W, C, N; K up to 1024 accesses per
// pixel (K <= 4096 / 2048 with 16-byte accesses, K <= 1024 otherwise).
#include "csc_tv.h"
#include "csc_kernels_dev.h"

#include <algorithm>

namespace sporco_amd {

namespace {

constexpr int kTvThreads = 256;
constexpr int kTvItems = 4;       // items a thread owns at most (its row state lives in registers)
constexpr int kTvScratch = 24;    // doubles of LDS for the block reduction (5 x 4 waves)

template <typename T, int V> struct alignas(sizeof(T) * V) TvVec {
    T v[V];
};

template <typename T, int V> __device__ __forceinline__ TvVec<T, V> tv_load(const T *p) {
    return *reinterpret_cast<const TvVec<T, V> *>(p);
}
template <typename T, int V> __device__ __forceinline__ void tv_store(T *p, const TvVec<T, V> &v) {
    *reinterpret_cast<TvVec<T, V> *>(p) = v;
}
template <typename T> __device__ __forceinline__ T tv_abs(T v) { return v < T(0) ? -v : v; }
template <typename T> __device__ __forceinline__ T tv_sqrt(T v);
template <> __device__ __forceinline__ float tv_sqrt<float>(float v) { return sqrtf(v); }
template <> __device__ __forceinline__ double tv_sqrt<double>(double v) { return sqrt(v); }
// prox_l2's factor max(0, a - alpha) / a, 0 at a = 0 (sporco/prox/_l2.py prox_l2)
template <typename T> __device__ __forceinline__ T tv_shrink(T nrm, T alpha) {
    const T b = nrm - alpha;
    return (nrm > T(0) && b > T(0)) ? b / nrm : T(0);
}

template <typename T> struct TvKArgs {
    TvArgs<T> a;
    int TW, rows, kv, shfl;
};

// Where the items of a thread lie: item i of the strip is access (i mod kv) of column (i / kv).
template <typename T, int V, int NI> struct TvItems {
    int64_t col[NI];    // element offset of the item inside a row of the array
    int64_t left[NI];   // ... of its x-predecessor (tv_ystep) / x-successor (tv_adjoint)
    int64_t wcol[NI];   // the same for the L1-weight array (without the row term)
    bool ok[NI];
    bool first[NI];     // access 0 of its pixel
    T w[NI][V];         // Wtv of its filters
    __device__ __forceinline__ void init(const TvKArgs<T> &ka, int x0, int cn, bool successor) {
        const TvArgs<T> &a = ka.a;
        const int items = ka.TW * ka.kv, CN = a.C * a.N;
        const int ci = cn / a.N, ni = cn - ci * a.N;
#pragma unroll
        for (int r = 0; r < NI; ++r) {
            const int i = (int)threadIdx.x + r * kTvThreads;
            const int j = i / ka.kv, k0 = (i - j * ka.kv) * V, gx = x0 + j;
            ok[r] = i < items && gx < a.W;
            first[r] = k0 == 0;
            const int gxs = ok[r] ? gx : 0;
            const int nb = successor ? (gxs + 1 == a.W ? 0 : gxs + 1) : (gxs == 0 ? a.W - 1 : gxs - 1);
            const int ks = ok[r] ? k0 : 0;
            col[r] = ((int64_t)gxs * CN + cn) * a.K + ks;
            left[r] = ((int64_t)nb * CN + cn) * a.K + ks;
            wcol[r] = gxs * a.wl1.stride[1] + ci * a.wl1.stride[2] + ni * a.wl1.stride[3] + ks * a.wl1.stride[4];
#pragma unroll
            for (int e = 0; e < V; ++e) w[r][e] = a.tvw[ks + e];
        }
    }
};

// sum of (s0, s1) over the kv items of a pixel, the same value in every one of them
template <typename T, int NI>
__device__ __forceinline__ void tv_pixel_sum(T (&s0)[NI], T (&s1)[NI], const TvKArgs<T> &ka, T *red) {
    if (ka.shfl) {
        // kv a power of two <= 64: the items of a pixel are kv neighbouring lanes
#pragma unroll
        for (int r = 0; r < NI; ++r)
            for (int m = 1; m < ka.kv && r * kTvThreads < ka.TW * ka.kv; m <<= 1) {
                s0[r] += __shfl_xor(s0[r], m, kWave);
                s1[r] += __shfl_xor(s1[r], m, kWave);
            }
        return;
    }
    const int items = ka.TW * ka.kv;
#pragma unroll
    for (int r = 0; r < NI; ++r) {
        const int i = (int)threadIdx.x + r * kTvThreads;
        if (i < items) {
            red[2 * i] = s0[r];
            red[2 * i + 1] = s1[r];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < NI; ++r) {
        const int i = (int)threadIdx.x + r * kTvThreads;
        if (i < items) {
            const T *src = red + 2 * (size_t)((i / ka.kv) * ka.kv);
            T t0 = T(0), t1 = T(0);
            for (int t = 0; t < ka.kv; ++t) {
                t0 += src[2 * t];
                t1 += src[2 * t + 1];
            }
            s0[r] = t0;
            s1[r] = t1;
        }
    }
}

// One workgroup: a strip of TW columns of one image (c, n), all K filters, the rows of one segment.
// MODE 0: scalar TV (one shrink factor for the whole array, from a.gn2), 1: vector TV, 2: the pass
// before MODE 0 that sums ||(AX + U)_{0,1}||^2 and writes nothing else
template <typename T, int V, int NI, int MODE>
__global__ void __launch_bounds__(kTvThreads) tv_ystep_kernel(const TvKArgs<T> ka) {
    const TvArgs<T> &a = ka.a;
    double *scratch = dyn_lds<double>();
    T *red = reinterpret_cast<T *>(scratch + kTvScratch);   // 2 buffers x (items, 2)
    const int x0 = blockIdx.z * ka.TW, ys = blockIdx.y * ka.rows;
    const int ye = ys + ka.rows < a.H ? ys + ka.rows : a.H;
    const int cn = blockIdx.x;
    const int64_t row = (int64_t)a.W * a.C * a.N * a.K, E = row * a.H;
    const int nitem = (ka.TW * ka.kv + kTvThreads - 1) / kTvThreads;
    const bool relax = a.rlx != T(1);
    const T rlx = a.rlx, rl1 = T(1) - a.rlx, us = a.u_scale;
    // scalar TV: prox_l2 of the reference's y step has no axis (cbpdntv.py:319), the norm is the
    // one of the whole array of gradient blocks
    const T gsc = MODE == 0 ? tv_shrink(tv_sqrt((T)*a.gn2), a.thr_tv) : T(0);
    TvItems<T, V, NI> it;
    it.init(ka, x0, cn, false);

    TvVec<T, V> xp[NI];     // the row above
    {
        const int64_t rp = (int64_t)(ys == 0 ? a.H - 1 : ys - 1) * row;
#pragma unroll
        for (int r = 0; r < NI; ++r)
            if (r < nitem && it.ok[r]) xp[r] = tv_load<T, V>(a.x + rp + it.col[r]);
    }
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int y = ys; y < ye; ++y) {
        const int64_t ro = (int64_t)y * row;
        TvVec<T, V> v0[NI], v1[NI], g0[NI], g1[NI];
        T s0[NI], s1[NI];
#pragma unroll
        for (int r = 0; r < NI; ++r) {
            s0[r] = s1[r] = T(0);
            if (!(r < nitem && it.ok[r])) continue;
            const int64_t o = ro + it.col[r];
            const TvVec<T, V> xc = tv_load<T, V>(a.x + o), xl = tv_load<T, V>(a.x + ro + it.left[r]);
            const TvVec<T, V> u0 = tv_load<T, V>(a.u + o), u1 = tv_load<T, V>(a.u + E + o),
                              uL = tv_load<T, V>(a.u + 2 * E + o);
            TvVec<T, V> p0, p1, pL;
            if (relax) {
                p0 = tv_load<T, V>(a.y + o);
                p1 = tv_load<T, V>(a.y + E + o);
                pL = tv_load<T, V>(a.y + 2 * E + o);
            }
            TvVec<T, V> yL, nuL;
            T sr = T(0), sa = T(0), sy = T(0), sl = T(0), st = T(0);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                // AXnr = (Wtv G_0 x, Wtv G_1 x, x), AX = rlx AXnr + (1 - rlx) Yprev (cbpdntv.py:542-559)
                const T a0 = it.w[r][e] * (xc.v[e] - xp[r].v[e]), a1 = it.w[r][e] * (xc.v[e] - xl.v[e]);
                const T aL = xc.v[e];
                g0[r].v[e] = a0;
                g1[r].v[e] = a1;
                const T x0v = relax ? fma1(rlx, a0, rl1 * p0.v[e]) : a0;
                const T x1v = relax ? fma1(rlx, a1, rl1 * p1.v[e]) : a1;
                const T xLv = relax ? fma1(rlx, aL, rl1 * pL.v[e]) : aL;
                v0[r].v[e] = fma1(us, u0.v[e], x0v);
                v1[r].v[e] = fma1(us, u1.v[e], x1v);
                const T n2 = fma1(v0[r].v[e], v0[r].v[e], v1[r].v[e] * v1[r].v[e]);
                if (MODE == 2) {
                    sr += n2;
                    continue;
                }
                const T vL = fma1(us, uL.v[e], xLv);
                // Y_L = prox_l1(AX_L + U_L, (lmbda / rho) wl1), U_L += AX_L - Y_L
                T w1 = T(1);
                if (a.wl1.ptr) w1 = a.wl1.ptr[y * a.wl1.stride[0] + it.wcol[r] + e * a.wl1.stride[4]];
                const T m = tv_abs(vL) - a.thr_l1 * w1;
                const T yl = m > T(0) ? (vL < T(0) ? -m : m) : T(0);
                yL.v[e] = yl;
                nuL.v[e] = vL - yl;
                sr = fma1(aL - yl, aL - yl, sr);
                sa = fma1(aL, aL, sa);
                sy = fma1(yl, yl, sy);
                sl += tv_abs(w1 * (a.geval_y ? yl : aL));
                if (MODE == 1) {
                    s0[r] += n2;
                    s1[r] = fma1(a0, a0, fma1(a1, a1, s1[r]));
                } else {
                    // Y_{0,1} = prox_l2((AX + U)_{0,1}, mu / rho)
                    const T sc = gsc;
                    const T y0 = sc * v0[r].v[e], y1 = sc * v1[r].v[e];
                    sr = fma1(a0 - y0, a0 - y0, fma1(a1 - y1, a1 - y1, sr));
                    sa = fma1(a0, a0, fma1(a1, a1, sa));
                    sy = fma1(y0, y0, fma1(y1, y1, sy));
                    st += a.geval_y ? tv_sqrt(fma1(y0, y0, y1 * y1)) : tv_sqrt(fma1(a0, a0, a1 * a1));
                    g0[r].v[e] = y0;
                    g1[r].v[e] = y1;
                    v0[r].v[e] -= y0;
                    v1[r].v[e] -= y1;
                }
            }
            xp[r] = xc;
            if (MODE == 2) {
                acc[0] += (double)sr;
                continue;
            }
            tv_store<T, V>(a.y + 2 * E + o, yL);
            tv_store<T, V>(a.u + 2 * E + o, nuL);
            if (MODE == 0) {
                tv_store<T, V>(a.y + o, g0[r]);
                tv_store<T, V>(a.y + E + o, g1[r]);
                tv_store<T, V>(a.u + o, v0[r]);
                tv_store<T, V>(a.u + E + o, v1[r]);
            }
            acc[0] += (double)sr;
            acc[1] += (double)sa;
            acc[2] += (double)sy;
            acc[3] += (double)sl;
            acc[4] += (double)st;
        }
        if (MODE == 1) {
            // ... over the two components and all K filters of the pixel
            tv_pixel_sum<T, NI>(s0, s1, ka, red + (size_t)(y & 1) * 2 * ka.TW * ka.kv);
#pragma unroll
            for (int r = 0; r < NI; ++r) {
                if (!(r < nitem && it.ok[r])) continue;
                const int64_t o = ro + it.col[r];
                const T nrm = tv_sqrt(s0[r]);
                const T sc = tv_shrink(nrm, a.thr_tv);
                T sr = T(0), sa = T(0), sy = T(0);
                TvVec<T, V> y0, y1, n0, n1;
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const T a0 = g0[r].v[e], a1 = g1[r].v[e];
                    y0.v[e] = sc * v0[r].v[e];
                    y1.v[e] = sc * v1[r].v[e];
                    n0.v[e] = v0[r].v[e] - y0.v[e];
                    n1.v[e] = v1[r].v[e] - y1.v[e];
                    sr = fma1(a0 - y0.v[e], a0 - y0.v[e], fma1(a1 - y1.v[e], a1 - y1.v[e], sr));
                    sa = fma1(a0, a0, fma1(a1, a1, sa));
                    sy = fma1(y0.v[e], y0.v[e], fma1(y1.v[e], y1.v[e], sy));
                }
                tv_store<T, V>(a.y + o, y0);
                tv_store<T, V>(a.y + E + o, y1);
                tv_store<T, V>(a.u + o, n0);
                tv_store<T, V>(a.u + E + o, n1);
                acc[0] += (double)sr;
                acc[1] += (double)sa;
                acc[2] += (double)sy;
                // (||Y_{0,1}|| of the pixel is the shrunk norm; one item of the pixel counts it)
                if (it.first[r]) acc[4] += (double)(a.geval_y ? sc * nrm : tv_sqrt(s1[r]));
            }
        }
    }
    __syncthreads();
    const int64_t blk = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    block_sum_store<5>(acc, scratch, a.partials + blk * 8);
}

template <typename T, int V, int NI>
__global__ void __launch_bounds__(kTvThreads) tv_adjoint_kernel(const TvKArgs<T> ka) {
    const TvArgs<T> &a = ka.a;
    double *scratch = dyn_lds<double>();
    const int x0 = blockIdx.z * ka.TW, ys = blockIdx.y * ka.rows;
    const int ye = ys + ka.rows < a.H ? ys + ka.rows : a.H;
    const int cn = blockIdx.x;
    const int64_t row = (int64_t)a.W * a.C * a.N * a.K, E = row * a.H;
    const int nitem = (ka.TW * ka.kv + kTvThreads - 1) / kTvThreads;
    const T us = a.u_scale;
    TvItems<T, V, NI> it;
    it.init(ka, x0, cn, true);

    TvVec<T, V> yc[NI], uc[NI];     // block 0 of the current row
#pragma unroll
    for (int r = 0; r < NI; ++r)
        if (r < nitem && it.ok[r]) {
            yc[r] = tv_load<T, V>(a.y + (int64_t)ys * row + it.col[r]);
            uc[r] = tv_load<T, V>(a.u + (int64_t)ys * row + it.col[r]);
        }
    double acc[2] = {0.0, 0.0};
    for (int y = ys; y < ye; ++y) {
        const int64_t ro = (int64_t)y * row, rn = (int64_t)(y + 1 == a.H ? 0 : y + 1) * row;
#pragma unroll
        for (int r = 0; r < NI; ++r) {
            if (!(r < nitem && it.ok[r])) continue;
            const int64_t o = ro + it.col[r], on = rn + it.col[r], ox = ro + it.left[r];
            const TvVec<T, V> yn = tv_load<T, V>(a.y + on), y1 = tv_load<T, V>(a.y + E + o),
                              y1r = tv_load<T, V>(a.y + E + ox), yL = tv_load<T, V>(a.y + 2 * E + o);
            const TvVec<T, V> un = tv_load<T, V>(a.u + on), u1 = tv_load<T, V>(a.u + E + o),
                              u1r = tv_load<T, V>(a.u + E + ox), uL = tv_load<T, V>(a.u + 2 * E + o);
            const TvVec<T, V> po = tv_load<T, V>(a.p + o);
            TvVec<T, V> p, q;
            T ss = T(0), sq = T(0);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                // A^T v = v_L + Wtv sum_i G_i^T v_i, G_i^T v = v - (its successor along i)
                p.v[e] = fma1(it.w[r][e], (yc[r].v[e] - yn.v[e]) + (y1.v[e] - y1r.v[e]), yL.v[e]);
                q.v[e] = us * fma1(it.w[r][e], (uc[r].v[e] - un.v[e]) + (u1.v[e] - u1r.v[e]), uL.v[e]);
                const T d = p.v[e] - po.v[e];
                ss = fma1(d, d, ss);
                sq = fma1(q.v[e], q.v[e], sq);
            }
            tv_store<T, V>(a.p + o, p);
            tv_store<T, V>(a.q + o, q);
            acc[0] += (double)ss;
            acc[1] += (double)sq;
            yc[r] = yn;
            uc[r] = un;
        }
    }
    const int64_t blk = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    block_sum_store<2>(acc, scratch, a.partials + blk * 8);
}

// The reference's x step with one TVWeight per filter (csc_tv.h launch_tv_sm_ref): one thread per
// (pixel, c, n) system, in place on the spectrum of A^T (Y - U).
template <typename T> __global__ void __launch_bounds__(kTvThreads) tv_sm_ref_kernel(const TvSmArgs<T> a) {
    const int64_t total = a.npix * a.CN;
    const int Wf = a.W / 2 + 1;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const T rho = a.rho;
    for (int64_t grp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; grp < total;
         grp += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = grp / a.CN;
        const cx<T> *d = a.df + pix * a.K;
        cx<T> *x = a.xf + grp * a.K;
        const cx<T> s = a.sf[grp];
        const T gh = grad_gh(a.g, pix, Wf);
        auto diag = [&](int k) -> T { return a.g.mu * (grad_w(a.g, k) * gh) + rho; };
        T gram = T(0);
        for (int k = 0; k < a.K; ++k) gram += cabs2(d[k]);
        // t = <c, b>, c = Df / (<Df, conj Df> + diag), b = conj(Df) Sf + rho yuf
        cx<T> t = mk<T>(T(0), T(0));
        double b2 = 0.0;
        for (int k = 0; k < a.K; ++k) {
            const cx<T> b = cmulc(d[k], s) + cscale(x[k], rho);
            t = t + cscale(cmul(d[k], b), T(1) / (gram + diag(k)));
            b2 += (double)cabs2(b);
        }
        cx<T> dx = mk<T>(T(0), T(0));
        for (int k = 0; k < a.K; ++k) {
            const cx<T> b = cmulc(d[k], s) + cscale(x[k], rho);
            const cx<T> xk = cscale(b - cmulc(d[k], t), T(1) / diag(k));
            dx = dx + cmul(d[k], xk);
            x[k] = xk;
        }
        if (a.want_obj) acc[0] += parseval_weight((int)(pix % Wf), Wf, a.W) * (double)cabs2(dx - s);
        if (a.want_xrrs) {
            double d2 = 0.0, ax2 = 0.0;
            for (int k = 0; k < a.K; ++k) {
                const cx<T> xk = x[k];
                const cx<T> b = cscale(xk, diag(k)) + cmulc(d[k], t);
                const cx<T> ax = cmulc(d[k], dx) + cscale(xk, diag(k));
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

template <typename T> TvKArgs<T> tv_kargs(const TvArgs<T> &a, const TvPlan &pl) {
    TvKArgs<T> ka;
    ka.a = a;
    ka.TW = pl.TW;
    ka.rows = pl.rows;
    ka.kv = pl.kv;
    ka.shfl = pl.kv <= kWave && (pl.kv & (pl.kv - 1)) == 0;
    SA_REQUIRE(pl.nseg <= 65535 && ceil_div(a.W, pl.TW) <= 65535, "TV kernels: grid too large");
    SA_REQUIRE(pl.TW * pl.kv <= kTvThreads * kTvItems && pl.kv * pl.vec == a.K, "TV kernels: plan does not fit");
    return ka;
}

size_t tv_lds_bytes(const TvPlan &pl, size_t elem, bool vtv) {
    return sizeof(double) * kTvScratch + (vtv ? elem * 4 * (size_t)pl.TW * pl.kv : 0);
}

}  // namespace

template <typename T> TvPlan tv_plan(int H, int W, int CN, int K) {
    TvPlan pl;
    constexpr int full = 16 / (int)sizeof(T);
    pl.vec = K % full == 0 ? full : 1;
    pl.kv = K / pl.vec;
    SA_REQUIRE(pl.kv <= kTvThreads * kTvItems,
               "TV regularisation: too many filters for one workgroup (K <= 1024, or 4096 / 2048 in "
               "multiples of 4 / 2 for float32 / float64)");
    // two items per thread where the filter count allows it: the loads of a row in flight per
    // thread stay within the registers of four workgroups per compute unit
    pl.TW = 64;
    while (pl.TW > 1 && ((int64_t)pl.TW * pl.kv > 2 * kTvThreads || pl.TW / 2 >= W)) pl.TW >>= 1;
    // row segments: enough workgroups to fill the device, each paying one extra row
    const int64_t strips = ceil_div(W, pl.TW) * CN;
    int64_t nseg = std::min<int64_t>(ceil_div(2048, strips), std::max<int64_t>(1, H / 16));
    nseg = std::max<int64_t>(1, std::min<int64_t>(nseg, H));
    pl.rows = (int)ceil_div(H, nseg);
    pl.nseg = (int)ceil_div(H, pl.rows);
    pl.blocks = strips * pl.nseg;
    return pl;
}

// the kernel instantiation of a plan: accesses of V elements, NI items per thread
#define SA_TV_DISPATCH(KERNEL, ...)                                                                     \
    do {                                                                                                \
        const int ni = (int)ceil_div((int64_t)pl.TW * pl.kv, kTvThreads);                               \
        if (pl.vec == full) {                                                                           \
            if (ni <= 1) hipLaunchKernelGGL((KERNEL<T, full, 1, ##__VA_ARGS__>), grid, dim3(kTvThreads), lds, st, ka);      \
            else if (ni <= 2) hipLaunchKernelGGL((KERNEL<T, full, 2, ##__VA_ARGS__>), grid, dim3(kTvThreads), lds, st, ka); \
            else hipLaunchKernelGGL((KERNEL<T, full, kTvItems, ##__VA_ARGS__>), grid, dim3(kTvThreads), lds, st, ka);       \
        } else {                                                                                        \
            if (ni <= 1) hipLaunchKernelGGL((KERNEL<T, 1, 1, ##__VA_ARGS__>), grid, dim3(kTvThreads), lds, st, ka);         \
            else if (ni <= 2) hipLaunchKernelGGL((KERNEL<T, 1, 2, ##__VA_ARGS__>), grid, dim3(kTvThreads), lds, st, ka);    \
            else hipLaunchKernelGGL((KERNEL<T, 1, kTvItems, ##__VA_ARGS__>), grid, dim3(kTvThreads), lds, st, ka);          \
        }                                                                                               \
    } while (0)

template <typename T> int64_t launch_tv_ystep(hipStream_t st, const TvArgs<T> &a, const TvPlan &pl) {
    const TvKArgs<T> ka = tv_kargs(a, pl);
    constexpr int full = 16 / (int)sizeof(T);
    const dim3 grid((unsigned)(a.C * a.N), (unsigned)pl.nseg, (unsigned)ceil_div(a.W, pl.TW));
    const size_t lds = tv_lds_bytes(pl, sizeof(T), a.vector_tv);
    if (a.vector_tv) SA_TV_DISPATCH(tv_ystep_kernel, 1);
    else if (a.norm_pass) SA_TV_DISPATCH(tv_ystep_kernel, 2);
    else SA_TV_DISPATCH(tv_ystep_kernel, 0);
    SA_HIP(hipGetLastError());
    return pl.blocks;
}

template <typename T> int64_t launch_tv_adjoint(hipStream_t st, const TvArgs<T> &a, const TvPlan &pl) {
    const TvKArgs<T> ka = tv_kargs(a, pl);
    constexpr int full = 16 / (int)sizeof(T);
    const dim3 grid((unsigned)(a.C * a.N), (unsigned)pl.nseg, (unsigned)ceil_div(a.W, pl.TW));
    const size_t lds = tv_lds_bytes(pl, sizeof(T), false);
    SA_TV_DISPATCH(tv_adjoint_kernel);
    SA_HIP(hipGetLastError());
    return pl.blocks;
}

template <typename T> int launch_tv_sm_ref(hipStream_t st, const TvSmArgs<T> &a) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(a.npix * a.CN, kTvThreads), kMaxPartialBlocks));
    hipLaunchKernelGGL((tv_sm_ref_kernel<T>), dim3(grid), dim3(kTvThreads), sizeof(double) * kTvScratch, st, a);
    SA_HIP(hipGetLastError());
    return grid;
}

#define SA_TV_INST(T)                                                                     \
    template TvPlan tv_plan<T>(int, int, int, int);                                        \
    template int64_t launch_tv_ystep<T>(hipStream_t, const TvArgs<T> &, const TvPlan &);  \
    template int launch_tv_sm_ref<T>(hipStream_t, const TvSmArgs<T> &);                   \
    template int64_t launch_tv_adjoint<T>(hipStream_t, const TvArgs<T> &, const TvPlan &);
SA_TV_INST(float)
SA_TV_INST(double)

}  // namespace sporco_amd
