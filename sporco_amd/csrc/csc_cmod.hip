// csc_cmod.hip -- the kernels of csc_cmod.h: cmod_gram, cmod_gram_reduce, cmod_rhs, cmod_iter, cmod_dfid.
// float32 / float64, 1 <= M, N <= kCmodMaxDim, any K >= 1.  Compiled with -ffp-contract=off (Makefile): the two
// product forms must round alike, every fused multiply-add here is spelled out.
#include "csc_cmod.h"
#include "csc_bpdn_product.h"
#include "csc_kernels_dev.h"
#include "csc_cmod_cols.h"

namespace sporco_amd {

namespace {

// grid (output block, slab).  LDS: ta [64][kCmodLd] rows of [Z; S], tb [64][kCmodLd] rows of Z.
template <typename T, int FORM> __global__ void __launch_bounds__(kThreads) cmod_gram_kernel(const CmodGramArgs<T> a) {
    constexpr int NCT = kCmodBlk / 16;
    const CmodPlan &p = a.p;
    const int rb = (int)blockIdx.x / p.CB, cb = (int)blockIdx.x % p.CB;
    const int split = (int)blockIdx.y;
    const int64_t k_lo = (int64_t)split * p.slab;
    const int64_t k_hi = k_lo + p.slab < a.K ? k_lo + p.slab : a.K;
    T *ta = dyn_lds<T>();
    T *tb = ta + kCmodBlk * kCmodLd;
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
    const int lc = lane & 15, lh = lane >> 4;
    // staging: thread t takes column t & 31 of rows t >> 5, + 8, ...
    const int sc = (int)threadIdx.x & (kCmodKS - 1), sr0 = (int)threadIdx.x / kCmodKS;
#ifndef SPORCO_AMD_HOSTSIM
    sa_floatx4 c[NCT];
    if constexpr (FORM == BPDN_FORM_MFMA) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) c[ct] = sa_floatx4{0.f, 0.f, 0.f, 0.f};
    }
#endif
    T acc[NCT][4];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[ct][r] = T(0);
    for (int64_t kb = k_lo; kb < k_hi; kb += kCmodKS) {
        const int64_t col = kb + sc;
        const bool col_ok = col < k_hi;
        for (int r = sr0; r < kCmodBlk; r += kThreads / kCmodKS) {
            const int gr = rb * kCmodBlk + r;      // row of [Z (M16 rows); S (N16 rows)]
            T va = T(0);
            if (col_ok) {
                if (gr < a.M) va = a.z[(int64_t)gr * a.K + col];
                else if (gr >= p.M16 && gr - p.M16 < a.N) va = a.s[(int64_t)(gr - p.M16) * a.K + col];
            }
            ta[r * kCmodLd + sc] = va;
            const int gc = cb * kCmodBlk + r;      // row of Z
            tb[r * kCmodLd + sc] = (col_ok && gc < a.M) ? a.z[(int64_t)gc * a.K + col] : T(0);
        }
        __syncthreads();
#ifndef SPORCO_AMD_HOSTSIM
        if constexpr (FORM == BPDN_FORM_MFMA) {
            // A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]; D: column l & 15, rows 4 (l >> 4) + r
            const T *ap = ta + (16 * wave + lc) * kCmodLd + lh;
            const T *bp = tb + lc * kCmodLd + lh;
#pragma unroll
            for (int k0 = 0; k0 < kCmodKS; k0 += 4) {
                const float av = ap[k0];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) c[ct] = sa_mfma_f32_16x16x4(av, bp[16 * ct * kCmodLd + k0], c[ct]);
            }
        } else
#endif
        {
            const T *ap = ta + (16 * wave + 4 * lh) * kCmodLd;
            const T *bp = tb + lc * kCmodLd;
            for (int k = 0; k < kCmodKS; ++k) {
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const T bv = bp[16 * ct * kCmodLd + k];
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[ct][r] = fma1(ap[r * kCmodLd + k], bv, acc[ct][r]);
                }
            }
        }
        __syncthreads();
    }
#ifndef SPORCO_AMD_HOSTSIM
    if constexpr (FORM == BPDN_FORM_MFMA) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
            acc[ct][0] = c[ct].x;
            acc[ct][1] = c[ct].y;
            acc[ct][2] = c[ct].z;
            acc[ct][3] = c[ct].w;
        }
    }
#endif
    // every element of the padded block is written: the reduction reads no stale value
    const int ldp = p.CB * kCmodBlk;
    T *dst = a.part + (int64_t)split * p.RB * kCmodBlk * ldp;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = rb * kCmodBlk + 16 * wave + 4 * lh + r, colo = cb * kCmodBlk + 16 * ct + lc;
            dst[(int64_t)row * ldp + colo] = acc[ct][r];
        }
}

// one thread per element of the (M + N, M) result
template <typename T> __global__ void __launch_bounds__(kThreads) cmod_gram_reduce_kernel(const CmodGramArgs<T> a) {
    const CmodPlan &p = a.p;
    const int total = (a.M + a.N) * a.M;
    const int ldp = p.CB * kCmodBlk;
    const int64_t plane = (int64_t)p.RB * kCmodBlk * ldp;
    for (int idx = (int)(blockIdx.x * kThreads + threadIdx.x); idx < total; idx += (int)gridDim.x * kThreads) {
        const int row = idx / a.M, m = idx % a.M;
        const int prow = row < a.M ? row : p.M16 + (row - a.M);
        const T *src = a.part + (int64_t)prow * ldp + m;
        double s = 0.0;
        for (int sp = 0; sp < p.nsplit; ++sp) s += (double)src[sp * plane];
        if (row < a.M) {
            a.g[(int64_t)row * a.M + m] = s;
        } else {
            const int n = row - a.M;
            a.sztd[(int64_t)n * a.M + m] = s;
            a.sztk[(int64_t)m * p.N16 + n] = (T)s;
        }
    }
}

template <typename T> __global__ void __launch_bounds__(kThreads) cmod_rhs_kernel(const CmodArgs<T> a) {
    const int N16 = (a.N + 15) & ~15;
    const int total = a.M * N16;
    for (int idx = (int)(blockIdx.x * kThreads + threadIdx.x); idx < total; idx += (int)gridDim.x * kThreads) {
        if (idx % N16 < a.N) a.bk[idx] = a.sztk[idx] + a.rho * (a.yk[idx] - a.u_scale * a.uk[idx]);
    }
}

// one workgroup per 16 columns of the dictionary
template <typename T, int FORM> __global__ void __launch_bounds__(kThreads) cmod_iter_kernel(const CmodArgs<T> a) {
    const int M = a.M, N = a.N;
    const int M4 = (M + 3) & ~3, N16 = (N + 15) & ~15;
    const int R = M4 > N16 ? M4 : N16;
    T *tq = dyn_lds<T>();                  // [M4][16] Q[:, block]; then [N][16] AX + U and G
    T *tx = tq + R * 16;                   // [N16][16] X
    double *cs = reinterpret_cast<double *>(tx + N16 * 16);
    double *scratch = cs + 256;
    const int j0 = 16 * (int)blockIdx.x;
    const bool relax = a.rlx != T(1);
    const T rl1 = T(1) - a.rlx;
    for (int idx = (int)threadIdx.x; idx < M4 * 16; idx += kThreads) {
        const int k = idx >> 4, j = idx & 15;
        tq[idx] = (k < M && j0 + j < M) ? a.q[(int64_t)k * M + j0 + j] : T(0);
    }
    __syncthreads();
    bpdn_product<T, 1, FORM>(a.bk, N16, M4, tq, 16, [&](int i, int j, T v) { tx[i * 16 + j] = v; });
    __syncthreads();
    // thread t: column t & 15 of rows t >> 4, + 16, ...
    const int c = (int)threadIdx.x & 15, m = j0 + c;
    const bool col_ok = m < M;
    T *tv = tq;
    for (int n = (int)threadIdx.x >> 4; n < N; n += 16) {
        T v = T(0);
        if (col_ok) {
            const int off = m * N16 + n;
            const T x = tx[n * 16 + c], y = a.yk[off], uv = a.u_scale * a.uk[off];
            const T ax = relax ? a.rlx * x + rl1 * y : x;
            v = ax + uv;
        }
        tv[n * 16 + c] = v;
    }
    __syncthreads();
    T mean, nrm;
    cm_col_stats(tv, N, a.zero_mean, cs, mean, nrm);
    double acc[kCmodSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int n = (int)threadIdx.x >> 4; n < N; n += 16) {
        T g = T(0);
        if (col_ok) {
            const int off = m * N16 + n;
            const T x = tx[n * 16 + c], y = a.yk[off], uv = a.u_scale * a.uk[off];
            const T ax = relax ? a.rlx * x + rl1 * y : x;
            const T yn = (tv[n * 16 + c] - mean) / nrm;
            const T un = uv + (ax - yn);
            const double r = (double)(x - yn), dy = (double)(yn - y);
            acc[CMOD_R2] += r * r;
            acc[CMOD_X2] += (double)x * (double)x;
            acc[CMOD_Y2] += (double)yn * (double)yn;
            acc[CMOD_S2] += dy * dy;
            acc[CMOD_U2] += (double)un * (double)un;
            a.xk[off] = x;
            a.yk[off] = yn;
            a.uk[off] = un;
            g = a.geval_y ? yn : x;
        }
        tx[n * 16 + c] = g;      // (this thread's own elements)
    }
    __syncthreads();
    // Cnstr: || Pcn(G) - G ||^2
    cm_col_stats(tx, N, a.zero_mean, cs, mean, nrm);
    if (col_ok) {
        for (int n = (int)threadIdx.x >> 4; n < N; n += 16) {
            const T g = tx[n * 16 + c];
            const double d = (double)((g - mean) / nrm - g);
            acc[CMOD_CNSTR] += d * d;
        }
    }
    block_sum_store<kCmodSums>(acc, scratch, a.partials + (int64_t)blockIdx.x * kCmodSums);
}

// sum (F Z - S)^2 over the block's columns; a workgroup loops over column blocks of KB
template <typename T, int KB, int FORM> __global__ void __launch_bounds__(kThreads) cmod_dfid_kernel(const CmodDfidArgs<T> a) {
    constexpr int LDB = KB == 32 ? 48 : 16;
    const int M = a.M, N = a.N;
    const int M4 = (M + 3) & ~3, N16 = (N + 15) & ~15;
    T *tz = dyn_lds<T>();
    double *scratch = reinterpret_cast<double *>(tz + M4 * LDB);
    const int64_t nblk = (a.K + KB - 1) / KB;
    for (int idx = (int)threadIdx.x; idx < (M4 - M) * LDB; idx += kThreads) tz[M * LDB + idx] = T(0);
    double acc[1] = {0.0};
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t c0 = blk * KB;
        for (int idx = (int)threadIdx.x; idx < M * KB; idx += kThreads) {
            const int i = idx / KB, j = idx % KB;
            const int64_t col = c0 + j;
            tz[i * LDB + j] = col < a.K ? a.z[(int64_t)i * a.K + col] : T(0);
        }
        __syncthreads();
        bpdn_product<T, KB / 16, FORM>(a.fk, N16, M4, tz, LDB, [&](int i, int j, T v) {
            const int64_t col = c0 + j;
            if (i < N && col < a.K) {
                const int64_t off = (int64_t)i * a.K + col;
                const double d = (double)(a.s ? v - a.s[off] : v);
                acc[0] += (double)(a.w ? a.w[off] : a.w_s) * (d * d);
            }
        });
        __syncthreads();
    }
    block_sum_store<1>(acc, scratch, a.partials + (int64_t)blockIdx.x * a.stride);
}

template <auto KERNEL, typename A> void cm_launch(dim3 grid, size_t lds, hipStream_t st, const A &a) {
    static PerDeviceOnce attr_set;
    if (attr_set.first())
        SA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   160 * 1024));
    hipLaunchKernelGGL(KERNEL, grid, dim3(kThreads), lds, st, a);
    SA_HIP(hipGetLastError());
}

// whether the launch may use the matrix instruction: float32 on the device
template <typename T> constexpr bool cm_has_mfma() {
#ifdef SPORCO_AMD_HOSTSIM
    return false;
#else
    return sizeof(T) == 4;
#endif
}

template <typename T> void cm_check_form(int form, const char *what) {
    SA_REQUIRE(form == BPDN_FORM_PLAIN || form == BPDN_FORM_MFMA, what);
    if (form == BPDN_FORM_MFMA) SA_REQUIRE(cm_has_mfma<T>(), "cmod: the matrix form exists in float32 on the device only");
}

inline bool cm_dims_ok(int M, int N) { return M >= 1 && M <= kCmodMaxDim && N >= 1 && N <= kCmodMaxDim; }

}  // namespace

template <typename T> int launch_cmod_gram(hipStream_t st, const CmodGramArgs<T> &a) {
    SA_REQUIRE(cm_dims_ok(a.M, a.N) && a.K >= 1 && a.K < (int64_t)1 << 31, "cmod_gram: bad argument");
    SA_REQUIRE(a.z && a.s && a.part, "cmod_gram: null argument");
    const CmodPlan ref = cmod_plan(a.N, a.M, a.K);
    SA_REQUIRE(a.p.slab == ref.slab && a.p.nsplit == ref.nsplit && a.p.RB == ref.RB && a.p.CB == ref.CB &&
                   a.p.M16 == ref.M16 && a.p.N16 == ref.N16,
               "cmod_gram: the plan is not that of the problem");
    cm_check_form<T>(a.form, "cmod_gram: bad form");
    const dim3 grid(a.p.RB * a.p.CB, a.p.nsplit);
    const size_t lds = cmod_gram_lds_bytes<T>();
    if constexpr (cm_has_mfma<T>()) {
        if (a.form == BPDN_FORM_MFMA) cm_launch<&cmod_gram_kernel<T, BPDN_FORM_MFMA>>(grid, lds, st, a);
    }
    if (a.form == BPDN_FORM_PLAIN) cm_launch<&cmod_gram_kernel<T, BPDN_FORM_PLAIN>>(grid, lds, st, a);
    return (int)(grid.x * grid.y);
}

template <typename T> void launch_cmod_gram_reduce(hipStream_t st, const CmodGramArgs<T> &a) {
    SA_REQUIRE(cm_dims_ok(a.M, a.N) && a.part && a.g && a.sztd && a.sztk, "cmod_gram_reduce: bad argument");
    const int total = (a.M + a.N) * a.M;
    const int nb = (total + kThreads - 1) / kThreads;
    hipLaunchKernelGGL((cmod_gram_reduce_kernel<T>), dim3(nb < 1024 ? nb : 1024), dim3(kThreads), 0, st, a);
    SA_HIP(hipGetLastError());
}

template <typename T> void launch_cmod_rhs(hipStream_t st, const CmodArgs<T> &a) {
    SA_REQUIRE(cm_dims_ok(a.M, a.N) && a.sztk && a.bk && a.yk && a.uk, "cmod_rhs: bad argument");
    const int total = a.M * bpdn_up(a.N, 16);
    const int nb = (total + kThreads - 1) / kThreads;
    hipLaunchKernelGGL((cmod_rhs_kernel<T>), dim3(nb < 1024 ? nb : 1024), dim3(kThreads), 0, st, a);
    SA_HIP(hipGetLastError());
}

template <typename T> int launch_cmod_iter(hipStream_t st, const CmodArgs<T> &a) {
    SA_REQUIRE(cm_dims_ok(a.M, a.N) && a.q && a.bk && a.xk && a.yk && a.uk && a.partials && a.rho > T(0),
               "cmod_iter: bad argument");
    cm_check_form<T>(a.form, "cmod_iter: bad form");
    const size_t lds = cmod_iter_lds_bytes<T>(a.N, a.M);
    SA_REQUIRE(lds <= (size_t)160 * 1024, "cmod_iter: the tiles do not fit in LDS");
    const int nb = bpdn_up(a.M, 16) / 16;
    if constexpr (cm_has_mfma<T>()) {
        if (a.form == BPDN_FORM_MFMA) cm_launch<&cmod_iter_kernel<T, BPDN_FORM_MFMA>>(dim3(nb), lds, st, a);
    }
    if (a.form == BPDN_FORM_PLAIN) cm_launch<&cmod_iter_kernel<T, BPDN_FORM_PLAIN>>(dim3(nb), lds, st, a);
    return nb;
}

template <typename T> int launch_cmod_dfid(hipStream_t st, const CmodDfidArgs<T> &a) {
    SA_REQUIRE(cm_dims_ok(a.M, a.N) && a.K >= 1 && a.K < (int64_t)1 << 31 && a.KB == bpdn_kb<T>(a.M, a.N),
               "cmod_dfid: bad argument");
    SA_REQUIRE(a.fk && a.z && a.partials && a.stride >= 1, "cmod_dfid: null argument");
    cm_check_form<T>(a.form, "cmod_dfid: bad form");
    const size_t lds = bpdn_lds_bytes<T>(a.M, a.N);
    SA_REQUIRE(lds <= (size_t)160 * 1024, "cmod_dfid: the tile does not fit in LDS");
    const int nb = bpdn_blocks(a.K, a.KB);
    const bool mf = a.form == BPDN_FORM_MFMA;
    if (a.KB == 32) {
        if constexpr (cm_has_mfma<T>()) {
            if (mf) cm_launch<&cmod_dfid_kernel<T, 32, BPDN_FORM_MFMA>>(dim3(nb), lds, st, a);
        }
        if (!mf) cm_launch<&cmod_dfid_kernel<T, 32, BPDN_FORM_PLAIN>>(dim3(nb), lds, st, a);
    } else {
        if constexpr (cm_has_mfma<T>()) {
            if (mf) cm_launch<&cmod_dfid_kernel<T, 16, BPDN_FORM_MFMA>>(dim3(nb), lds, st, a);
        }
        if (!mf) cm_launch<&cmod_dfid_kernel<T, 16, BPDN_FORM_PLAIN>>(dim3(nb), lds, st, a);
    }
    return nb;
}

#define SA_CMOD_INST(T)                                                                \
    template int launch_cmod_gram<T>(hipStream_t, const CmodGramArgs<T> &);            \
    template void launch_cmod_gram_reduce<T>(hipStream_t, const CmodGramArgs<T> &);    \
    template void launch_cmod_rhs<T>(hipStream_t, const CmodArgs<T> &);                \
    template int launch_cmod_iter<T>(hipStream_t, const CmodArgs<T> &);                \
    template int launch_cmod_dfid<T>(hipStream_t, const CmodDfidArgs<T> &);
SA_CMOD_INST(float)
SA_CMOD_INST(double)

}  // namespace sporco_amd
