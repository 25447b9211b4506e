// csc_pgm_bpdn.hip -- the kernels of csc_pgm_bpdn.h: bpdn_pgm_step, bpdn_pgm_ystep.
// float32 / float64, 1 <= M, N <= kBpdnMaxDim, any K >= 1.  Compiled with -ffp-contract=off (Makefile): the two
// product forms must round alike, every fused multiply-add here is spelled out.
#include "csc_pgm_bpdn.h"
#include "csc_bpdn_product.h"
#include "csc_kernels_dev.h"

#include <algorithm>

namespace sporco_amd {

namespace {

template <typename T> __device__ __forceinline__ T pb_abs(T v) { return v < T(0) ? -v : v; }
// prox_l1: sign(v) max(0, |v| - alpha) (sporco/prox/_lp.py:144-183)
template <typename T> __device__ __forceinline__ T pb_soft(T v, T alpha) {
    const T b = pb_abs(v) - alpha;
    return b > T(0) ? (v < T(0) ? -b : b) : T(0);
}

// two LDS tiles of R = max(M4, N4) rows: ty holds Y, then X' (Cauchy: G); tr holds R = w (D Y - S)
template <typename T, int KB> struct PbGeom {
    static constexpr int LDB = KB == 32 ? 48 : 16;
    static constexpr int NCT = KB / 16;
    int M, N, M4, N4, M16, N16, R;
    T *ty, *tr;
    double *scratch;
    __device__ __forceinline__ PbGeom(int M_, int N_) : M(M_), N(N_) {
        M4 = (M + 3) & ~3;
        N4 = (N + 3) & ~3;
        M16 = (M + 15) & ~15;
        N16 = (N + 15) & ~15;
        R = M4 > N4 ? M4 : N4;
        ty = dyn_lds<T>();
        tr = ty + R * LDB;
        scratch = reinterpret_cast<double *>(tr + R * LDB);
    }
    // rows [r0, r1) of a tile <- 0 (the padding of the k range; no later store touches it)
    __device__ __forceinline__ void zero_rows(T *t, int r0, int r1) const {
        for (int idx = (int)threadIdx.x; idx < (r1 - r0) * LDB; idx += kThreads) t[r0 * LDB + idx] = T(0);
    }
};

// the prox phase of one element: X' from (Y, G), stored, with its sums
template <typename T>
__device__ __forceinline__ T pb_prox_elem(const PgmBpdnArgs<T> &a, int64_t off, T y, T gv, T invL, T thr,
                                          double (&acc)[kPgmBpdnSums]) {
    const T w = a.wl1 ? a.wl1[off] : a.wl1_s;
    T xn;
    if (a.revert) {
        xn = a.xprv[off];
    } else {
        xn = pb_soft(y - invL * gv, thr * w);
        if (a.nonneg && xn < T(0)) xn = T(0);
        if (a.zz) a.zz[off] = xn;
    }
    a.x[off] = xn;
    const double d = (double)(xn - y), dr = (double)(xn - (a.yprv ? a.yprv[off] : y));
    acc[PGMB_DXG] += d * (double)gv;
    acc[PGMB_DXY2] += d * d;
    acc[PGMB_L1] += (double)pb_abs(w * xn);
    acc[PGMB_X2] += (double)xn * (double)xn;
    acc[PGMB_RS2] += dr * dr;
    return xn;
}

template <typename T, int KB, int FORM>
__global__ void __launch_bounds__(kThreads) bpdn_pgm_step_kernel(const PgmBpdnArgs<T> a) {
    using G = PbGeom<T, KB>;
    const G g(a.M, a.N);
    const int64_t nblk = (a.K + KB - 1) / KB;
    const bool grad = (a.phase & PGMB_PHASE_GRAD) != 0, prox = (a.phase & PGMB_PHASE_PROX) != 0;
    const T invL = T(1) / a.L, thr = a.lmbda / a.L;
    g.zero_rows(g.ty, g.M, g.M4);
    g.zero_rows(g.tr, g.N, g.N4);
    double acc[kPgmBpdnSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t c0 = blk * KB;
        if (grad) {
            // 1. the Y tile, zero beyond the last column
            for (int idx = (int)threadIdx.x; idx < g.M * KB; idx += kThreads) {
                const int i = idx / KB, j = idx % KB;
                const int64_t col = c0 + j, off = (int64_t)i * a.K + col;
                T yv = T(0);
                if (col < a.K) {
                    if (a.ymode == PGMB_Y_LOAD) {
                        yv = a.y[off];
                    } else {
                        const T xp = a.xprv[off];
                        if (a.ymode == PGMB_Y_MOMENTUM) {
                            yv = xp + a.beta * (xp - a.x[off]);
                        } else {
                            T zv = a.z[off];
                            if (a.z_update) {
                                zv = zv + a.zc * (xp - a.yprv[off]);
                                a.z[off] = zv;
                            }
                            yv = (a.tk * xp + a.tt * zv) / a.TT;
                        }
                        a.y[off] = yv;
                    }
                }
                g.ty[i * G::LDB + j] = yv;
            }
            __syncthreads();
            // 2. R = w (D Y - S), f(Y)
            bpdn_product<T, G::NCT, FORM>(a.dtk, g.N16, g.M4, g.ty, G::LDB, [&](int i, int j, T v) {
                const int64_t col = c0 + j;
                if (i < g.N) {
                    T r = T(0);
                    if (col < a.K) {
                        const int64_t off = (int64_t)i * a.K + col;
                        const T e = v - a.s[off], w = a.w ? a.w[off] : a.w_s;
                        r = w * e;
                        acc[PGMB_FY] += (double)w * ((double)e * (double)e);
                    }
                    g.tr[i * G::LDB + j] = r;
                }
            });
            __syncthreads();
            // 3. G = D^T R; both phases: the prox step in the epilogue, X' over Y in LDS
            bpdn_product<T, G::NCT, FORM>(a.dk, g.M16, g.N4, g.tr, G::LDB, [&](int i, int j, T v) {
                const int64_t col = c0 + j;
                if (i < g.M && col < a.K) {
                    const int64_t off = (int64_t)i * a.K + col;
                    acc[PGMB_G2] += (double)v * (double)v;
                    if (a.g) {
                        if (a.bb) {
                            const double dg = (double)(v - a.g[off]), dx = (double)(a.xprv[off] - a.x[off]);
                            acc[PGMB_BBXG] += dx * dg;
                            acc[PGMB_BBG2] += dg * dg;
                        }
                        a.g[off] = v;
                    }
                    if (prox)
                        g.ty[i * G::LDB + j] = pb_prox_elem(a, off, g.ty[i * G::LDB + j], v, invL, thr, acc);
                    else if (a.cauchy)
                        g.ty[i * G::LDB + j] = v;
                }
            });
            __syncthreads();
        } else {
            // the prox phase alone: Y and G from global memory
            for (int idx = (int)threadIdx.x; idx < g.M * KB; idx += kThreads) {
                const int i = idx / KB, j = idx % KB;
                const int64_t col = c0 + j, off = (int64_t)i * a.K + col;
                T xn = T(0);
                if (col < a.K) xn = pb_prox_elem(a, off, a.y[off], a.g[off], invL, thr, acc);
                g.ty[i * G::LDB + j] = xn;
            }
            __syncthreads();
        }
        if (prox || a.cauchy) {
            // 4. F(X') (the gradient phase of the Cauchy rule: || D G ||^2)
            bpdn_product<T, G::NCT, FORM>(a.dtk, g.N16, g.M4, g.ty, G::LDB, [&](int i, int j, T v) {
                const int64_t col = c0 + j;
                if (i < g.N && col < a.K) {
                    if (prox) {
                        const int64_t off = (int64_t)i * a.K + col;
                        const T e = v - a.s[off], w = a.w ? a.w[off] : a.w_s;
                        acc[PGMB_FX] += (double)w * ((double)e * (double)e);
                    } else {
                        acc[PGMB_DG2] += (double)v * (double)v;
                    }
                }
            });
            __syncthreads();
        }
    }
    block_sum_store<kPgmBpdnSums>(acc, g.scratch, a.partials + (int64_t)blockIdx.x * kPgmBpdnSums);
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
    bpdn_pgm_ystep_kernel(const T *x, const T *xprv, const T *zz, T *y, T beta, T gamma, int64_t n, double *partials) {
    double acc[1] = {0.0};
    for (int64_t off = (int64_t)blockIdx.x * kThreads + threadIdx.x; off < n; off += (int64_t)gridDim.x * kThreads) {
        const T xv = x[off];
        T yv = xv;
        if (zz) yv = yv + gamma * (zz[off] - xv);
        yv = yv + beta * (xv - xprv[off]);
        y[off] = yv;
        const double d = (double)(xv - yv);
        acc[0] += d * d;
    }
    block_sum_store<1>(acc, dyn_lds<double>(), partials + blockIdx.x);
}

template <auto KERNEL, typename A> void pb_launch(int nb, size_t lds, hipStream_t st, const A &a) {
    static PerDeviceOnce attr_set;
    if (attr_set.first())
        SA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   160 * 1024));
    hipLaunchKernelGGL(KERNEL, dim3(nb), dim3(kThreads), lds, st, a);
    SA_HIP(hipGetLastError());
}

// whether the launch uses the matrix instruction: float32 on the device, unless the plain form is asked for
template <typename T> constexpr bool pb_has_mfma() {
#ifdef SPORCO_AMD_HOSTSIM
    return false;
#else
    return sizeof(T) == 4;
#endif
}

}  // namespace

template <typename T> int launch_bpdn_pgm_step(hipStream_t st, const PgmBpdnArgs<T> &a) {
    const char *what = "bpdn_pgm_step: bad argument";
    SA_REQUIRE(a.M >= 1 && a.M <= kBpdnMaxDim && a.N >= 1 && a.N <= kBpdnMaxDim && a.K >= 1 &&
                   a.K < (int64_t)1 << 31 && a.KB == bpdn_kb<T>(a.M, a.N),
               what);
    SA_REQUIRE(pgm_bpdn_lds_bytes<T>(a.M, a.N) <= (size_t)160 * 1024, what);
    SA_REQUIRE(a.form == BPDN_FORM_PLAIN || a.form == BPDN_FORM_MFMA, what);
    const bool grad = (a.phase & PGMB_PHASE_GRAD) != 0, prox = (a.phase & PGMB_PHASE_PROX) != 0;
    SA_REQUIRE((grad || prox) && (a.phase & ~(PGMB_PHASE_GRAD | PGMB_PHASE_PROX)) == 0, what);
    SA_REQUIRE(a.ymode == PGMB_Y_LOAD || a.ymode == PGMB_Y_MOMENTUM || a.ymode == PGMB_Y_ROBUST, what);
    SA_REQUIRE(a.dk && a.dtk && a.s && a.y && a.partials, "bpdn_pgm_step: null argument");
    SA_REQUIRE(a.L > T(0), "bpdn_pgm_step: L must be positive");
    if (grad) {
        SA_REQUIRE(a.ymode == PGMB_Y_LOAD || (a.xprv && a.x), "bpdn_pgm_step: null argument");
        SA_REQUIRE(a.ymode != PGMB_Y_ROBUST || (a.z && a.TT != T(0) && (!a.z_update || a.yprv)),
                   "bpdn_pgm_step: null argument");
        SA_REQUIRE(!a.bb || (a.g && a.xprv && a.x), "bpdn_pgm_step: null argument");
        SA_REQUIRE(!(a.cauchy && prox), "bpdn_pgm_step: the Cauchy sums belong to a gradient phase alone");
    } else {
        SA_REQUIRE(a.g != nullptr, "bpdn_pgm_step: a prox phase alone reads G");
        SA_REQUIRE(!a.cauchy && !a.bb, what);
    }
    if (prox) SA_REQUIRE(a.x && (!a.revert || a.xprv), "bpdn_pgm_step: null argument");
    const int nb = bpdn_blocks(a.K, a.KB);
    const size_t lds = pgm_bpdn_lds_bytes<T>(a.M, a.N);
    const bool mf = a.form == BPDN_FORM_MFMA;
    if (mf) SA_REQUIRE(pb_has_mfma<T>(), "bpdn_pgm_step: the matrix form exists in float32 on the device only");
    if (a.KB == 32) {
        if constexpr (pb_has_mfma<T>()) {
            if (mf) pb_launch<&bpdn_pgm_step_kernel<T, 32, BPDN_FORM_MFMA>>(nb, lds, st, a);
        }
        if (!mf) pb_launch<&bpdn_pgm_step_kernel<T, 32, BPDN_FORM_PLAIN>>(nb, lds, st, a);
    } else {
        if constexpr (pb_has_mfma<T>()) {
            if (mf) pb_launch<&bpdn_pgm_step_kernel<T, 16, BPDN_FORM_MFMA>>(nb, lds, st, a);
        }
        if (!mf) pb_launch<&bpdn_pgm_step_kernel<T, 16, BPDN_FORM_PLAIN>>(nb, lds, st, a);
    }
    return nb;
}

template <typename T>
int launch_bpdn_pgm_ystep(hipStream_t st, const T *x, const T *xprv, const T *zz, T *y, T beta, T gamma, int64_t n,
                          double *partials) {
    SA_REQUIRE(x && xprv && y && partials && n >= 1, "bpdn_pgm_ystep: null argument");
    const int64_t want = (n + kThreads - 1) / kThreads;
    const int nb = (int)(want < kBpdnMaxBlocks ? want : kBpdnMaxBlocks);
    hipLaunchKernelGGL((bpdn_pgm_ystep_kernel<T>), dim3(nb), dim3(kThreads), sizeof(double) * (kThreads / kWave), st, x,
                       xprv, zz, y, beta, gamma, n, partials);
    SA_HIP(hipGetLastError());
    return nb;
}

#define SA_PGM_BPDN_INST(T)                                                                                  \
    template int launch_bpdn_pgm_step<T>(hipStream_t, const PgmBpdnArgs<T> &);                              \
    template int launch_bpdn_pgm_ystep<T>(hipStream_t, const T *, const T *, const T *, T *, T, T, int64_t, double *);
SA_PGM_BPDN_INST(float)
SA_PGM_BPDN_INST(double)

}  // namespace sporco_amd
