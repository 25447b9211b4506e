// csc_bpdn.hip -- the kernels of csc_bpdn.h: bpdn_dts, bpdn_iter (and its projection mode), bpdn_joint_rows,
// bpdn_joint_apply, bpdn_lsc, bpdn_proj_cols.
// float32 / float64, 1 <= M, N <= kBpdnMaxDim, any K >= 1.  Compiled with -ffp-contract=off (Makefile): the two
// product forms must round alike, every fused multiply-add here is spelled out.
#include "csc_bpdn.h"
#include "csc_bpdn_product.h"
#include "csc_kernels_dev.h"

#include <algorithm>

namespace sporco_amd {

namespace {

template <typename T> __device__ __forceinline__ T bp_abs(T v) { return v < T(0) ? -v : v; }
// prox_l1: sign(v) max(0, |v| - alpha) (sporco/prox/_lp.py:144-183)
template <typename T> __device__ __forceinline__ T bp_soft(T v, T alpha) {
    const T b = bp_abs(v) - alpha;
    return b > T(0) ? (v < T(0) ? -b : b) : T(0);
}

template <typename T, int KB> struct BpGeom {
    static constexpr int LDB = KB == 32 ? 48 : 16;
    static constexpr int NCT = KB / 16;
    int M, N, M4, N4, M16, N16, R;
    T *tb, *tx;
    double *scratch;
    __device__ __forceinline__ BpGeom(int M_, int N_) : M(M_), N(N_) {
        M4 = (M + 3) & ~3;
        N4 = (N + 3) & ~3;
        M16 = (M + 15) & ~15;
        N16 = (N + 15) & ~15;
        R = M4 > N4 ? M4 : N4;
        tb = dyn_lds<T>();
        tx = tb + R * LDB;
        scratch = reinterpret_cast<double *>(tx + R * LDB);
    }
    // rows [r0, r1) of a tile <- 0 (the padding of the k range; no later store touches it)
    __device__ __forceinline__ void zero_rows(T *t, int r0, int r1) const {
        for (int idx = (int)threadIdx.x; idx < (r1 - r0) * LDB; idx += kThreads) t[r0 * LDB + idx] = T(0);
    }
};

// ---- the column search of the projection mode (csc_bpdn.h) ----
// Thread t works for column t / LPC of the tile with the rows t % LPC, + LPC, ...: LPC = 256 / KB lanes that lie side
// by side in one wave, so an xor shuffle by a mask below LPC stays inside the group.
template <int KB> struct BpCols {
    static constexpr int LPC = kThreads / KB;
    static_assert(LPC >= 1 && LPC <= kWave && (LPC & (LPC - 1)) == 0 && KB <= kBpdnSums * 4, "one wave holds whole groups");
};
// the sum over a group, the same bits in each of its lanes (every level adds the same two values in both partners)
template <int LPC, typename V> __device__ __forceinline__ V bp_group_sum(V v) {
#pragma unroll
    for (int m = LPC / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}
// whether any group of the wave still says so (f is uniform over a group)
template <int LPC> __device__ __forceinline__ bool bp_wave_any(bool f) {
    int v = f ? 1 : 0;
#pragma unroll
    for (int m = kWave / 2; m >= LPC; m >>= 1) v |= __shfl_xor(v, m, kWave);
    return v != 0;
}
// tau >= 0 of this thread's column of the (M, KB) tile t: sum_i max(|t_ij| - tau, 0) = gamma, 0 where the column lies
// inside the ball.  Every thread of the workgroup calls it; the tile is only read.
template <typename T, int KB> __device__ __forceinline__ double bp_col_tau(const T *t, int M, double gamma) {
    constexpr int LDB = BpGeom<T, KB>::LDB, LPC = BpCols<KB>::LPC;
    const T *col = t + (int)threadIdx.x / LPC;
    const int q = (int)threadIdx.x % LPC;
    double s = 0.0;
    for (int i = q; i < M; i += LPC) s += (double)bp_abs(col[i * LDB]);
    s = bp_group_sum<LPC>(s);
    int n = M;
    bool live = s > gamma;      // (a NaN sum: the column is left as it is)
    double tau = live ? (s - gamma) / (double)n : 0.0;
    // each pass that does not end the search takes at least one entry out of the active set: at most M passes follow
    for (int pass = 0; pass < M; ++pass) {
        if (!bp_wave_any<LPC>(live)) break;
        double s2 = 0.0;
        int n2 = 0;
        if (live) {
            for (int i = q; i < M; i += LPC) {
                const double v = (double)bp_abs(col[i * LDB]);
                if (v > tau) {
                    s2 += v;
                    ++n2;
                }
            }
        }
        s2 = bp_group_sum<LPC>(s2);
        n2 = bp_group_sum<LPC>(n2);
        if (live) {
            // the set reproduces itself: tau is its threshold.  Nothing above tau (gamma = 0 with equal magnitudes, an
            // infinite or NaN threshold): tau stands and zeroes the column.
            if (n2 == n || n2 == 0) {
                live = false;
            } else {
                n = n2;
                tau = (s2 - gamma) / (double)n2;
            }
        }
    }
    return tau;
}

// what the y and u steps leave of one element
template <typename T>
__device__ __forceinline__ void bp_ustep_sums(const BpdnArgs<T> &a, T x, T y, T uv, T ax, T yn, T w, T &un,
                                              double (&acc)[kBpdnSums]) {
    un = uv + (ax - yn);
    const double r = (double)(x - yn), dy = (double)(yn - y);
    acc[BPDN_R2] += r * r;
    acc[BPDN_X2] += (double)x * (double)x;
    acc[BPDN_Y2] += (double)yn * (double)yn;
    acc[BPDN_S2] += dy * dy;
    acc[BPDN_U2] += (double)un * (double)un;
    acc[BPDN_L1] += (double)bp_abs(w * (a.geval_y ? yn : x));
}

// sum (D V - S)^2 over the block's columns, V the (M, KB) tile tv
template <typename T, int KB, int FORM>
__device__ __forceinline__ void bp_dfid(const BpdnArgs<T> &a, const BpGeom<T, KB> &g, const T *tv, int64_t c0, double &dfid) {
    bpdn_product<T, BpGeom<T, KB>::NCT, FORM>(a.dtk, g.N16, g.M4, tv, BpGeom<T, KB>::LDB, [&](int i, int j, T v) {
        const int64_t col = c0 + j;
        if (i < g.N && col < a.K) {
            const double d = (double)(v - a.s[(int64_t)i * a.K + col]);
            dfid += d * d;
        }
    });
}

// this thread's rows t, t + 256 of the tile: sums of squares over the block's columns, in column order
template <typename T, int KB>
__device__ __forceinline__ void bp_row_sums(const BpGeom<T, KB> &g, const T *t, double (&racc)[2]) {
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int row = (int)threadIdx.x + rr * kThreads;
        if (row < g.M) {
            double s = 0.0;
            for (int j = 0; j < KB; ++j) {
                const double v = (double)t[row * BpGeom<T, KB>::LDB + j];
                s += v * v;
            }
            racc[rr] += s;
        }
    }
}
template <typename T, int KB>
__device__ __forceinline__ void bp_row_store(const BpGeom<T, KB> &g, const double (&racc)[2], double *rowp) {
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {
        const int row = (int)threadIdx.x + rr * kThreads;
        if (row < g.M) rowp[(int64_t)blockIdx.x * g.M + row] = racc[rr];
    }
}

// The projection mode's share of a column block, X in tx and B (no longer needed) in tb:
//     V = relax(X, Y) + U -> tb; tau_j by the column search -> scratch; Y' = soft(V, tau_j) [max(., 0)]; u step and sums;
//     the variable of DFid -> tb, that of Cnstr -> tx; DFid; sum (proj_l1(g) - g)^2 by a second search on tx.
// Y and U of the block are read a second time where BPDN's y step reads them once (they were read for B a moment ago).
template <typename T, int KB, int FORM>
__device__ __forceinline__ void bp_proj_block(const BpdnArgs<T> &a, const BpGeom<T, KB> &g, int64_t c0, bool relax, T rl1,
                                              double (&acc)[kBpdnSums]) {
    using G = BpGeom<T, KB>;
    constexpr int LPC = BpCols<KB>::LPC;
    for (int idx = (int)threadIdx.x; idx < g.M * KB; idx += kThreads) {
        const int i = idx / KB, j = idx % KB;
        const int64_t col = c0 + j, off = (int64_t)i * a.K + col;
        T v = T(0);
        if (col < a.K) {
            const T x = g.tx[i * G::LDB + j];
            const T ax = relax ? a.rlx * x + rl1 * a.y[off] : x;
            v = ax + a.u_scale * a.u[off];
        }
        g.tb[i * G::LDB + j] = v;
    }
    __syncthreads();
    const double tau = bp_col_tau<T, KB>(g.tb, g.M, a.gamma);
    if ((int)threadIdx.x % LPC == 0) g.scratch[(int)threadIdx.x / LPC] = tau;
    __syncthreads();
    for (int idx = (int)threadIdx.x; idx < g.M * KB; idx += kThreads) {
        const int i = idx / KB, j = idx % KB;
        const int64_t col = c0 + j, off = (int64_t)i * a.K + col;
        T keep = T(0), gkeep = T(0);
        if (col < a.K) {
            const T x = g.tx[i * G::LDB + j], y = a.y[off], uv = a.u_scale * a.u[off];
            const T ax = relax ? a.rlx * x + rl1 * y : x;
            const T z = bp_soft(g.tb[i * G::LDB + j], (T)g.scratch[j]);
            const T yn = (a.nonneg && z < T(0)) ? T(0) : z;      // (the reference clips after projecting)
            T un;
            bp_ustep_sums(a, x, y, uv, ax, yn, T(0), un, acc);
            a.y[off] = yn;
            a.u[off] = un;
            if (a.want_x) a.x[off] = x;
            keep = a.feval_x ? x : yn;
            gkeep = a.geval_y ? yn : x;
        }
        g.tb[i * G::LDB + j] = keep;
        g.tx[i * G::LDB + j] = gkeep;
    }
    __syncthreads();
    bp_dfid<T, KB, FORM>(a, g, g.tb, c0, acc[BPDN_DFID]);
    {
        const T t2 = (T)bp_col_tau<T, KB>(g.tx, g.M, a.gamma);
        const T *col = g.tx + (int)threadIdx.x / LPC;
        for (int i = (int)threadIdx.x % LPC; i < g.M; i += LPC) {
            const T gv = col[i * G::LDB];
            const double d = (double)(bp_soft(gv, t2) - gv);
            acc[BPDN_CNSTR] += d * d;
        }
    }
    __syncthreads();
}

// one iteration; PROJ: the projection mode (csc_bpdn.h)
template <typename T, int KB, int FORM, bool PROJ> __device__ __forceinline__ void bp_iter_body(const BpdnArgs<T> &a) {
    using G = BpGeom<T, KB>;
    const G g(a.M, a.N);
    const int64_t nblk = (a.K + KB - 1) / KB;
    const bool relax = a.rlx != T(1);
    const T rl1 = T(1) - a.rlx;
    g.zero_rows(g.tb, g.M, g.M4);
    g.zero_rows(g.tx, g.M, g.M4);
    double acc[kBpdnSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double racc[2] = {0.0, 0.0}, raccx[2] = {0.0, 0.0};
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t c0 = blk * KB;
        // B = D^T S + rho (Y - U), zero beyond the last column
        for (int idx = (int)threadIdx.x; idx < g.M * KB; idx += kThreads) {
            const int i = idx / KB, j = idx % KB;
            const int64_t col = c0 + j, off = (int64_t)i * a.K + col;
            T b = T(0);
            if (col < a.K) {
                b = a.dts[off] + a.rho * (a.y[off] - a.u_scale * a.u[off]);
                if (a.bsave) a.bsave[off] = b;
            }
            g.tb[i * G::LDB + j] = b;
        }
        __syncthreads();
        bpdn_product<T, G::NCT, FORM>(a.pk, g.M16, g.M4, g.tb, G::LDB, [&](int i, int j, T v) {
            if (i < g.M) g.tx[i * G::LDB + j] = v;
        });
        __syncthreads();
        if constexpr (PROJ) {
            bp_proj_block<T, KB, FORM>(a, g, c0, relax, rl1, acc);
            continue;
        }
        for (int idx = (int)threadIdx.x; idx < g.M * KB; idx += kThreads) {
            const int i = idx / KB, j = idx % KB;
            const int64_t col = c0 + j, off = (int64_t)i * a.K + col;
            T keep = T(0);
            if (col < a.K) {
                const T x = g.tx[i * G::LDB + j], y = a.y[off], uv = a.u_scale * a.u[off];
                const T w = a.wl1 ? a.wl1[off] : a.wl1_s;
                const T ax = relax ? a.rlx * x + rl1 * y : x;
                const T z = bp_soft(ax + uv, a.lr * w);
                if (a.joint) {
                    a.z[off] = z;
                    a.x[off] = x;
                    keep = z;
                } else {
                    const T yn = (a.nonneg && z < T(0)) ? T(0) : z;
                    T un;
                    bp_ustep_sums(a, x, y, uv, ax, yn, w, un, acc);
                    a.y[off] = yn;
                    a.u[off] = un;
                    if (a.want_x) a.x[off] = x;
                    keep = a.feval_x ? x : yn;
                }
            }
            g.tb[i * G::LDB + j] = keep;
        }
        __syncthreads();
        if (a.joint) {
            bp_row_sums<T, KB>(g, g.tb, racc);
            if (a.rowpx) bp_row_sums<T, KB>(g, g.tx, raccx);
        } else {
            bp_dfid<T, KB, FORM>(a, g, g.tb, c0, acc[BPDN_DFID]);
        }
        __syncthreads();
    }
    if (a.joint) {
        bp_row_store<T, KB>(g, racc, a.rowp);
        if (a.rowpx) bp_row_store<T, KB>(g, raccx, a.rowpx);
    } else {
        block_sum_store<kBpdnSums>(acc, g.scratch, a.partials + (int64_t)blockIdx.x * kBpdnSums);
    }
}
template <typename T, int KB, int FORM> __global__ void __launch_bounds__(kThreads) bpdn_iter_kernel(const BpdnArgs<T> a) {
    bp_iter_body<T, KB, FORM, false>(a);
}
template <typename T, int KB, int FORM> __global__ void __launch_bounds__(kThreads) bpdn_iter_proj_kernel(const BpdnArgs<T> a) {
    bp_iter_body<T, KB, FORM, true>(a);
}

template <typename T, int KB, int FORM>
__global__ void __launch_bounds__(kThreads) bpdn_joint_apply_kernel(const BpdnArgs<T> a) {
    using G = BpGeom<T, KB>;
    const G g(a.M, a.N);
    const int64_t nblk = (a.K + KB - 1) / KB;
    const bool relax = a.rlx != T(1);
    const T rl1 = T(1) - a.rlx;
    g.zero_rows(g.tb, g.M, g.M4);
    g.zero_rows(g.tx, g.M, g.M4);
    double acc[kBpdnSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double racc[2] = {0.0, 0.0};
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t c0 = blk * KB;
        for (int idx = (int)threadIdx.x; idx < g.M * KB; idx += kThreads) {
            const int i = idx / KB, j = idx % KB;
            const int64_t col = c0 + j, off = (int64_t)i * a.K + col;
            T keep = T(0), ykeep = T(0);
            if (col < a.K) {
                const T x = a.x[off], y = a.y[off], uv = a.u_scale * a.u[off];
                const T w = a.wl1 ? a.wl1[off] : a.wl1_s;
                const T ax = relax ? a.rlx * x + rl1 * y : x;
                const T zs = a.rowf[i] * a.z[off];
                const T yn = (a.nonneg && zs < T(0)) ? T(0) : zs;
                T un;
                bp_ustep_sums(a, x, y, uv, ax, yn, w, un, acc);
                a.y[off] = yn;
                a.u[off] = un;
                keep = a.feval_x ? x : yn;
                ykeep = yn;
            }
            g.tb[i * G::LDB + j] = keep;
            g.tx[i * G::LDB + j] = ykeep;
        }
        __syncthreads();
        bp_row_sums<T, KB>(g, g.tx, racc);
        bp_dfid<T, KB, FORM>(a, g, g.tb, c0, acc[BPDN_DFID]);
        __syncthreads();
    }
    bp_row_store<T, KB>(g, racc, a.rowp);
    block_sum_store<kBpdnSums>(acc, g.scratch, a.partials + (int64_t)blockIdx.x * kBpdnSums);
}

template <typename T, int KB, int FORM> __global__ void __launch_bounds__(kThreads) bpdn_dts_kernel(const BpdnArgs<T> a) {
    using G = BpGeom<T, KB>;
    const G g(a.M, a.N);
    const int64_t nblk = (a.K + KB - 1) / KB;
    g.zero_rows(g.tb, g.N, g.N4);
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t c0 = blk * KB;
        for (int idx = (int)threadIdx.x; idx < g.N * KB; idx += kThreads) {
            const int i = idx / KB, j = idx % KB;
            const int64_t col = c0 + j;
            g.tb[i * G::LDB + j] = col < a.K ? a.s[(int64_t)i * a.K + col] : T(0);
        }
        __syncthreads();
        bpdn_product<T, G::NCT, FORM>(a.dk, g.M16, g.N4, g.tb, G::LDB, [&](int i, int j, T v) {
            const int64_t col = c0 + j;
            if (i < g.M && col < a.K) a.dts[(int64_t)i * a.K + col] = v;
        });
        __syncthreads();
    }
}

template <typename T, int KB, int FORM> __global__ void __launch_bounds__(kThreads) bpdn_lsc_kernel(const BpdnArgs<T> a) {
    using G = BpGeom<T, KB>;
    const G g(a.M, a.N);
    const int64_t nblk = (a.K + KB - 1) / KB;
    g.zero_rows(g.tb, g.M, g.M4);
    g.zero_rows(g.tx, g.N, g.N4);
    double acc[kBpdnLscSums] = {0.0, 0.0, 0.0};
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t c0 = blk * KB;
        for (int idx = (int)threadIdx.x; idx < g.M * KB; idx += kThreads) {
            const int i = idx / KB, j = idx % KB;
            const int64_t col = c0 + j;
            g.tb[i * G::LDB + j] = col < a.K ? a.x[(int64_t)i * a.K + col] : T(0);
        }
        __syncthreads();
        bpdn_product<T, G::NCT, FORM>(a.dtk, g.N16, g.M4, g.tb, G::LDB, [&](int i, int j, T v) {
            if (i < g.N) g.tx[i * G::LDB + j] = v;
        });
        __syncthreads();
        bpdn_product<T, G::NCT, FORM>(a.dk, g.M16, g.N4, g.tx, G::LDB, [&](int i, int j, T v) {
            const int64_t col = c0 + j;
            if (i < g.M && col < a.K) {
                const T ax = v + a.c * g.tb[i * G::LDB + j];
                const T b = a.bsave[(int64_t)i * a.K + col];
                const double d = (double)(ax - b);
                acc[0] += d * d;
                acc[1] += (double)ax * (double)ax;
                acc[2] += (double)b * (double)b;
            }
        });
        __syncthreads();
    }
    block_sum_store<kBpdnLscSums>(acc, g.scratch, a.partials + (int64_t)blockIdx.x * kBpdnLscSums);
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
    bpdn_joint_rows_kernel(const double *rowp, int nb, int M, int mode, T mr, T *rowf, double *out, int slot) {
    double acc[1] = {0.0};
    for (int m = (int)threadIdx.x; m < M; m += kThreads) {
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += rowp[(int64_t)b * M + m];
        if (mode == 0) {
            // prox_l2 (sporco/prox/_lp.py:284-290): max(0, a - alpha) / a, zero at a zero row
            const T nrm = (T)sqrt(s);
            const T d = nrm - mr;
            rowf[m] = nrm == T(0) ? T(0) : (d > T(0) ? d : T(0)) / nrm;
        } else {
            acc[0] += sqrt(s);
        }
    }
    if (mode != 0) block_sum_store<1>(acc, dyn_lds<double>(), out + slot);
}

// proj_l1 of the columns of a plain array: tiles in, the column search, soft threshold, tiles out
template <typename T> struct BpdnColsArgs {
    const T *v = nullptr;
    T *out = nullptr;
    int M = 1;
    int64_t K = 1;
    double gamma = 0.0;
};
template <typename T, int KB> __global__ void __launch_bounds__(kThreads) bpdn_proj_cols_kernel(const BpdnColsArgs<T> a) {
    using G = BpGeom<T, KB>;
    constexpr int LPC = BpCols<KB>::LPC;
    const G g(a.M, 1);
    const int64_t nblk = (a.K + KB - 1) / KB;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t c0 = blk * KB;
        for (int idx = (int)threadIdx.x; idx < g.M * KB; idx += kThreads) {
            const int i = idx / KB, j = idx % KB;
            const int64_t col = c0 + j;
            g.tb[i * G::LDB + j] = col < a.K ? a.v[(int64_t)i * a.K + col] : T(0);
        }
        __syncthreads();
        const double tau = bp_col_tau<T, KB>(g.tb, g.M, a.gamma);
        if ((int)threadIdx.x % LPC == 0) g.scratch[(int)threadIdx.x / LPC] = tau;
        __syncthreads();
        for (int idx = (int)threadIdx.x; idx < g.M * KB; idx += kThreads) {
            const int i = idx / KB, j = idx % KB;
            const int64_t col = c0 + j;
            if (col < a.K) a.out[(int64_t)i * a.K + col] = bp_soft(g.tb[i * G::LDB + j], (T)g.scratch[j]);
        }
        __syncthreads();
    }
}

template <auto KERNEL, typename A> void bp_launch(int nb, size_t lds, hipStream_t st, const A &a) {
    static PerDeviceOnce attr_set;
    if (attr_set.first())
        SA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   160 * 1024));
    hipLaunchKernelGGL(KERNEL, dim3(nb), dim3(kThreads), lds, st, a);
    SA_HIP(hipGetLastError());
}

template <typename T> void bp_check(const BpdnArgs<T> &a, const char *what) {
    SA_REQUIRE(a.M >= 1 && a.M <= kBpdnMaxDim && a.N >= 1 && a.N <= kBpdnMaxDim && a.K >= 1 &&
                   a.K < (int64_t)1 << 31 && a.KB == bpdn_kb<T>(a.M, a.N),
               what);
    SA_REQUIRE(bpdn_lds_bytes<T>(a.M, a.N) <= (size_t)160 * 1024, what);
    SA_REQUIRE(a.form == BPDN_FORM_PLAIN || a.form == BPDN_FORM_MFMA, what);
}

// whether the launch uses the matrix instruction: float32 on the device, unless the plain form is asked for
template <typename T> constexpr bool bp_has_mfma() {
#ifdef SPORCO_AMD_HOSTSIM
    return false;
#else
    return sizeof(T) == 4;
#endif
}

#define SA_BP_DISPATCH(KERNEL, a, nb)                                                                              \
    do {                                                                                                           \
        const size_t lds_ = bpdn_lds_bytes<T>((a).M, (a).N);                                                       \
        const bool mf_ = (a).form == BPDN_FORM_MFMA;                                                               \
        if (mf_) SA_REQUIRE(bp_has_mfma<T>(), "bpdn: the matrix form exists in float32 on the device only");        \
        if ((a).KB == 32) {                                                                                        \
            if constexpr (bp_has_mfma<T>()) {                                                                      \
                if (mf_) bp_launch<&KERNEL<T, 32, BPDN_FORM_MFMA>>(nb, lds_, st, a);                                \
            }                                                                                                      \
            if (!mf_) bp_launch<&KERNEL<T, 32, BPDN_FORM_PLAIN>>(nb, lds_, st, a);                                  \
        } else {                                                                                                   \
            if constexpr (bp_has_mfma<T>()) {                                                                      \
                if (mf_) bp_launch<&KERNEL<T, 16, BPDN_FORM_MFMA>>(nb, lds_, st, a);                                \
            }                                                                                                      \
            if (!mf_) bp_launch<&KERNEL<T, 16, BPDN_FORM_PLAIN>>(nb, lds_, st, a);                                  \
        }                                                                                                          \
    } while (0)

}  // namespace

template <typename T> void launch_bpdn_dts(hipStream_t st, const BpdnArgs<T> &a) {
    bp_check(a, "bpdn_dts: bad argument");
    SA_REQUIRE(a.dk && a.s && a.dts, "bpdn_dts: null argument");
    const int nb = bpdn_blocks(a.K, a.KB);
    SA_BP_DISPATCH(bpdn_dts_kernel, a, nb);
}

template <typename T> int launch_bpdn_iter(hipStream_t st, const BpdnArgs<T> &a) {
    bp_check(a, "bpdn_iter: bad argument");
    SA_REQUIRE(a.pk && a.dtk && a.s && a.dts && a.x && a.y && a.u && a.rho > T(0), "bpdn_iter: null argument");
    SA_REQUIRE(a.joint ? (a.z && a.rowp) : (a.partials != nullptr), "bpdn_iter: null argument");
    const int nb = bpdn_blocks(a.K, a.KB);
    if (a.proj_l1) {
        SA_REQUIRE(!a.joint && a.gamma >= 0.0, "bpdn_iter: the projection mode takes gamma >= 0 and no joint term");
        SA_BP_DISPATCH(bpdn_iter_proj_kernel, a, nb);
    } else {
        SA_BP_DISPATCH(bpdn_iter_kernel, a, nb);
    }
    return nb;
}

template <typename T> int launch_bpdn_proj_cols(hipStream_t st, const T *v, T *out, int M, int64_t K, double gamma) {
    SA_REQUIRE(v && out && M >= 1 && M <= kBpdnMaxDim && K >= 1 && K < (int64_t)1 << 31 && gamma >= 0.0,
               "bpdn_proj_cols: bad argument");
    BpdnColsArgs<T> a;
    a.v = v;
    a.out = out;
    a.M = M;
    a.K = K;
    a.gamma = gamma;
    const int KB = bpdn_kb<T>(M, 1), nb = bpdn_blocks(K, KB);
    const size_t lds = bpdn_lds_bytes<T>(M, 1);
    if (KB == 32)
        bp_launch<&bpdn_proj_cols_kernel<T, 32>>(nb, lds, st, a);
    else
        bp_launch<&bpdn_proj_cols_kernel<T, 16>>(nb, lds, st, a);
    return nb;
}

template <typename T> int launch_bpdn_joint_apply(hipStream_t st, const BpdnArgs<T> &a) {
    bp_check(a, "bpdn_joint_apply: bad argument");
    SA_REQUIRE(a.dtk && a.s && a.x && a.y && a.u && a.z && a.rowf && a.rowp && a.partials, "bpdn_joint_apply: null argument");
    const int nb = bpdn_blocks(a.K, a.KB);
    SA_BP_DISPATCH(bpdn_joint_apply_kernel, a, nb);
    return nb;
}

template <typename T> int launch_bpdn_lsc(hipStream_t st, const BpdnArgs<T> &a) {
    bp_check(a, "bpdn_lsc: bad argument");
    SA_REQUIRE(a.dk && a.dtk && a.x && a.bsave && a.partials, "bpdn_lsc: null argument");
    const int nb = bpdn_blocks(a.K, a.KB);
    SA_BP_DISPATCH(bpdn_lsc_kernel, a, nb);
    return nb;
}

template <typename T>
void launch_bpdn_joint_rows(hipStream_t st, const double *rowp, int nb, int M, int mode, T mr, T *rowf, double *out,
                            int slot) {
    SA_REQUIRE(rowp && nb >= 1 && nb <= kBpdnMaxBlocks && M >= 1 && M <= kBpdnMaxDim, "bpdn_joint_rows: bad argument");
    SA_REQUIRE(mode == 0 ? rowf != nullptr : (out != nullptr && slot >= 0 && slot < kOutSlots),
               "bpdn_joint_rows: null argument");
    hipLaunchKernelGGL((bpdn_joint_rows_kernel<T>), dim3(1), dim3(kThreads), sizeof(double) * (kThreads / kWave), st, rowp,
                       nb, M, mode, mr, rowf, out, slot);
    SA_HIP(hipGetLastError());
}

#define SA_BPDN_INST(T)                                                                                     \
    template void launch_bpdn_dts<T>(hipStream_t, const BpdnArgs<T> &);                                    \
    template int launch_bpdn_iter<T>(hipStream_t, const BpdnArgs<T> &);                                    \
    template int launch_bpdn_joint_apply<T>(hipStream_t, const BpdnArgs<T> &);                             \
    template int launch_bpdn_lsc<T>(hipStream_t, const BpdnArgs<T> &);                                     \
    template int launch_bpdn_proj_cols<T>(hipStream_t, const T *, T *, int, int64_t, double);              \
    template void launch_bpdn_joint_rows<T>(hipStream_t, const double *, int, int, int, T, T *, double *, int);
SA_BPDN_INST(float)
SA_BPDN_INST(double)

}  // namespace sporco_amd
