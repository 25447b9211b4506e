// csc_rpca.hip -- the kernels of csc_rpca.h: rpca_gram, rpca_gram_reduce, rpca_iter, rpca_sumsq.
// float32 / float64, 1 <= min(R, C) <= kRpcaMaxDim, any long side with R C < 2^31.  Compiled with -ffp-contract=off
// (Makefile): the two product forms of rpca_iter must round alike, every fused multiply-add here is spelled out.
#include "csc_rpca.h"
#include "csc_bpdn_product.h"
#include "csc_kernels_dev.h"

namespace sporco_amd {

namespace {

// V at element `off`, in the working precision
template <typename T>
__device__ __forceinline__ T rp_v(const T *s, const T *y, const T *u, T u_scale, int mode, int64_t off) {
    const T sv = s[off];
    if (mode == RPCA_V_S) return sv;
    const T d = sv - y[off];
    if (mode == RPCA_V_SY) return d;
    return d - u_scale * u[off];
}

// grid (output block, slab).  LDS: ta [64][kRpcaLd] the lines of the block's rows, tb the lines of its columns
// (a diagonal block: tb is ta).
template <typename T, int FORM> __global__ void __launch_bounds__(kThreads) rpca_gram_kernel(const RpcaGramArgs<T> a) {
    constexpr int NCT = kRpcaBlk / 16;
    const RpcaPlan &p = a.p;
    const int rb = (int)blockIdx.x / p.NB, cb = (int)blockIdx.x % p.NB;
    const int split = (int)blockIdx.y;
    const int64_t k_lo = (int64_t)split * p.slab;
    const int64_t k_hi = k_lo + p.slab < p.L ? k_lo + p.slab : p.L;
    const int64_t sl = p.tall ? p.n : 1, si = p.tall ? 1 : p.L;
    double *ta = dyn_lds<double>();
    double *tb = rb == cb ? ta : ta + kRpcaBlk * kRpcaLd;
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
    const int lc = lane & 15, lh = lane >> 4;
#ifndef SPORCO_AMD_HOSTSIM
    sa_doublex4 c[NCT];
    if constexpr (FORM == BPDN_FORM_MFMA) {
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) c[ct] = sa_doublex4{0.0, 0.0, 0.0, 0.0};
    }
#endif
    double acc[NCT][4];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[ct][r] = 0.0;
    for (int64_t kb = k_lo; kb < k_hi; kb += kRpcaKS) {
        // consecutive threads along the axis that is contiguous in memory
        for (int idx = (int)threadIdx.x; idx < kRpcaBlk * kRpcaKS; idx += kThreads) {
            const int r = p.tall ? idx % kRpcaBlk : idx / kRpcaKS;
            const int kk = p.tall ? idx / kRpcaBlk : idx % kRpcaKS;
            const int64_t l = kb + kk;
            const bool l_ok = l < k_hi;
            const int ia = rb * kRpcaBlk + r;
            ta[r * kRpcaLd + kk] =
                (l_ok && ia < p.n) ? (double)rp_v(a.s, a.y, a.u, a.u_scale, a.mode, l * sl + ia * si) : 0.0;
            if (rb != cb) {
                const int ib = cb * kRpcaBlk + r;
                tb[r * kRpcaLd + kk] =
                    (l_ok && ib < p.n) ? (double)rp_v(a.s, a.y, a.u, a.u_scale, a.mode, l * sl + ib * si) : 0.0;
            }
        }
        __syncthreads();
#ifndef SPORCO_AMD_HOSTSIM
        if constexpr (FORM == BPDN_FORM_MFMA) {
            // A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]; D: column l & 15, rows (l >> 4) + 4 r
            const double *ap = ta + (16 * wave + lc) * kRpcaLd + lh;
            const double *bp = tb + lc * kRpcaLd + lh;
#pragma unroll
            for (int k0 = 0; k0 < kRpcaKS; k0 += 4) {
                const double av = ap[k0];
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) c[ct] = sa_mfma_f64_16x16x4(av, bp[16 * ct * kRpcaLd + k0], c[ct]);
            }
        } else
#endif
        {
            const double *ap = ta + (16 * wave + lh) * kRpcaLd;
            const double *bp = tb + lc * kRpcaLd;
            for (int k = 0; k < kRpcaKS; ++k) {
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) {
                    const double bv = bp[16 * ct * kRpcaLd + k];
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[ct][r] = fma1(ap[4 * r * kRpcaLd + k], bv, acc[ct][r]);
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
    const int ldp = p.NB * kRpcaBlk;
    double *dst = a.part + (int64_t)split * ldp * ldp;
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = rb * kRpcaBlk + 16 * wave + lh + 4 * r, col = cb * kRpcaBlk + 16 * ct + lc;
            dst[(int64_t)row * ldp + col] = acc[ct][r];
        }
}

// one thread per element of G
template <typename T> __global__ void __launch_bounds__(kThreads) rpca_gram_reduce_kernel(const RpcaGramArgs<T> a) {
    const RpcaPlan &p = a.p;
    const int total = p.n * p.n;
    const int ldp = p.NB * kRpcaBlk;
    const int64_t plane = (int64_t)ldp * ldp;
    for (int idx = (int)(blockIdx.x * kThreads + threadIdx.x); idx < total; idx += (int)gridDim.x * kThreads) {
        const int i = idx / p.n, j = idx % p.n;
        const double *src = a.part + (int64_t)i * ldp + j;
        double s = 0.0;
        for (int sp = 0; sp < p.nsplit; ++sp) s += src[sp * plane];
        a.g[idx] = s;
    }
}

template <typename T> __device__ __forceinline__ T rp_abs(T v) { return v < T(0) ? -v : v; }

// a workgroup loops over blocks of KB positions of the long axis
template <typename T, int KB, int FORM> __global__ void __launch_bounds__(kThreads) rpca_iter_kernel(const RpcaIterArgs<T> a) {
    constexpr int LDB = KB == 32 ? 48 : 16;
    const RpcaPlan &p = a.p;
    const int n = p.n, n4 = p.n4;
    const int64_t sl = p.tall ? n : 1, si = p.tall ? 1 : p.L;
    T *tv = dyn_lds<T>();                  // [n4][LDB] the block of V
    T *tx = tv + n4 * LDB;                 // [n16][LDB] the block of X
    double *scratch = reinterpret_cast<double *>(tx + p.n16 * LDB);
    const bool relax = a.rlx != T(1);
    const T rl1 = T(1) - a.rlx;
    const int64_t nblk = (p.L + KB - 1) / KB;
    double acc[kRpcaSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t l0 = blk * KB;
        // (the product of the previous block has been read out of tx by every thread that gets here; tv is free)
        for (int idx = (int)threadIdx.x; idx < n4 * KB; idx += kThreads) {
            const int i = p.tall ? idx % n4 : idx / KB;
            const int j = p.tall ? idx / n4 : idx % KB;
            const int64_t l = l0 + j;
            T v = T(0);
            if (i < n && l < p.L)
                v = a.apply ? a.s[l * sl + i * si]
                            : rp_v<T>(a.s, a.y, a.u, a.u_scale, RPCA_V_SYU, l * sl + i * si);
            tv[i * LDB + j] = v;
        }
        __syncthreads();
        bpdn_product<T, KB / 16, FORM>(a.tk, p.n16, n4, tv, LDB, [&](int i, int j, T v) { tx[i * LDB + j] = v; });
        __syncthreads();
        for (int idx = (int)threadIdx.x; idx < n * KB; idx += kThreads) {
            const int i = p.tall ? idx % n : idx / KB;
            const int j = p.tall ? idx / n : idx % KB;
            const int64_t l = l0 + j;
            if (l >= p.L) continue;
            const int64_t off = l * sl + i * si;
            const T x = tx[i * LDB + j];
            if (a.apply) {
                a.x[off] = x;
                continue;
            }
            const T s = a.s[off], y = a.y[off], uv = a.u_scale * a.u[off];
            const T ax = relax ? a.rlx * x - rl1 * (y - s) : x;
            const T v = (s - ax) - uv;
            const T m = rp_abs(v) - a.thr;
            const T yn = m > T(0) ? (v < T(0) ? -m : m) : T(0);
            const T un = uv + ((ax + yn) - s);
            const double r = (double)((x + yn) - s), dy = (double)(yn - y);
            acc[RPCA_R2] += r * r;
            acc[RPCA_S2] += dy * dy;
            acc[RPCA_X2] += (double)x * (double)x;
            acc[RPCA_Y2] += (double)yn * (double)yn;
            acc[RPCA_U2] += (double)un * (double)un;
            acc[RPCA_L1Y] += (double)rp_abs(yn);
            acc[RPCA_L1SX] += (double)rp_abs(s - x);
            a.x[off] = x;
            a.y[off] = yn;
            a.u[off] = un;
        }
        __syncthreads();      // (tx is read out before the next block's product writes it)
    }
    if (!a.apply) block_sum_store<kRpcaSums>(acc, scratch, a.partials + (int64_t)blockIdx.x * kRpcaSums);
}

template <typename T> __global__ void __launch_bounds__(kThreads) rpca_sumsq_kernel(const T *v, int64_t count, double *partials) {
    double *scratch = dyn_lds<double>();
    double acc[1] = {0.0};
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < count; idx += (int64_t)gridDim.x * kThreads) {
        const double d = (double)v[idx];
        acc[0] += d * d;
    }
    block_sum_store<1>(acc, scratch, partials + blockIdx.x);
}

template <auto KERNEL, typename A> void rp_launch(dim3 grid, size_t lds, hipStream_t st, const A &a) {
    static PerDeviceOnce attr_set;
    if (attr_set.first())
        SA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   160 * 1024));
    hipLaunchKernelGGL(KERNEL, grid, dim3(kThreads), lds, st, a);
    SA_HIP(hipGetLastError());
}

// whether a launch may use a matrix instruction: rpca_gram's is float64 for both dtypes, rpca_iter's float32
constexpr bool rp_on_device() {
#ifdef SPORCO_AMD_HOSTSIM
    return false;
#else
    return true;
#endif
}
template <typename T> constexpr bool rp_iter_has_mfma() { return rp_on_device() && sizeof(T) == 4; }

template <typename T> bool rp_plan_ok(const RpcaPlan &p) {
    if (p.n < 1 || p.n > kRpcaMaxDim || p.L < p.n || p.L * p.n >= (int64_t)1 << 31) return false;
    if (!p.tall && p.L == p.n) return false;      // (a square problem is tall)
    const RpcaPlan ref = p.tall ? rpca_plan<T>((int)p.L, p.n) : rpca_plan<T>(p.n, (int)p.L);
    return p.n4 == ref.n4 && p.n16 == ref.n16 && p.NB == ref.NB && p.nsplit == ref.nsplit && p.slab == ref.slab &&
           p.KB == ref.KB && p.nb_iter == ref.nb_iter;
}

}  // namespace

template <typename T> int launch_rpca_gram(hipStream_t st, const RpcaGramArgs<T> &a) {
    SA_REQUIRE(rp_plan_ok<T>(a.p), "rpca_gram: the plan is not that of a problem served");
    SA_REQUIRE(a.mode == RPCA_V_SYU || a.mode == RPCA_V_SY || a.mode == RPCA_V_S, "rpca_gram: bad mode");
    SA_REQUIRE(a.s && a.part && (a.mode == RPCA_V_S || a.y) && (a.mode != RPCA_V_SYU || a.u), "rpca_gram: null argument");
    SA_REQUIRE(a.form == BPDN_FORM_PLAIN || a.form == BPDN_FORM_MFMA, "rpca_gram: bad form");
    if (a.form == BPDN_FORM_MFMA) SA_REQUIRE(rp_on_device(), "rpca_gram: the matrix form exists on the device only");
    const dim3 grid(a.p.NB * a.p.NB, a.p.nsplit);
    const size_t lds = rpca_gram_lds_bytes();
    if constexpr (rp_on_device()) {
        if (a.form == BPDN_FORM_MFMA) rp_launch<&rpca_gram_kernel<T, BPDN_FORM_MFMA>>(grid, lds, st, a);
    }
    if (a.form == BPDN_FORM_PLAIN) rp_launch<&rpca_gram_kernel<T, BPDN_FORM_PLAIN>>(grid, lds, st, a);
    return (int)(grid.x * grid.y);
}

template <typename T> void launch_rpca_gram_reduce(hipStream_t st, const RpcaGramArgs<T> &a) {
    SA_REQUIRE(rp_plan_ok<T>(a.p) && a.part && a.g, "rpca_gram_reduce: bad argument");
    const int total = a.p.n * a.p.n;
    const int nb = (total + kThreads - 1) / kThreads;
    hipLaunchKernelGGL((rpca_gram_reduce_kernel<T>), dim3(nb < 1024 ? nb : 1024), dim3(kThreads), 0, st, a);
    SA_HIP(hipGetLastError());
}

template <typename T> int launch_rpca_iter(hipStream_t st, const RpcaIterArgs<T> &a) {
    SA_REQUIRE(rp_plan_ok<T>(a.p), "rpca_iter: the plan is not that of a problem served");
    SA_REQUIRE(a.s && a.x && a.tk, "rpca_iter: null argument");
    if (!a.apply) SA_REQUIRE(a.y && a.u && a.partials && a.thr >= T(0), "rpca_iter: bad argument");
    SA_REQUIRE(a.form == BPDN_FORM_PLAIN || a.form == BPDN_FORM_MFMA, "rpca_iter: bad form");
    if (a.form == BPDN_FORM_MFMA)
        SA_REQUIRE(rp_iter_has_mfma<T>(), "rpca_iter: the matrix form exists in float32 on the device only");
    const size_t lds = rpca_iter_lds_bytes<T>(a.p);
    SA_REQUIRE(lds <= (size_t)160 * 1024, "rpca_iter: the tiles do not fit in LDS");
    const int nb = a.p.nb_iter;
    const bool mf = a.form == BPDN_FORM_MFMA;
    if (a.p.KB == 32) {
        if constexpr (rp_iter_has_mfma<T>()) {
            if (mf) rp_launch<&rpca_iter_kernel<T, 32, BPDN_FORM_MFMA>>(dim3(nb), lds, st, a);
        }
        if (!mf) rp_launch<&rpca_iter_kernel<T, 32, BPDN_FORM_PLAIN>>(dim3(nb), lds, st, a);
    } else {
        if constexpr (rp_iter_has_mfma<T>()) {
            if (mf) rp_launch<&rpca_iter_kernel<T, 16, BPDN_FORM_MFMA>>(dim3(nb), lds, st, a);
        }
        if (!mf) rp_launch<&rpca_iter_kernel<T, 16, BPDN_FORM_PLAIN>>(dim3(nb), lds, st, a);
    }
    return nb;
}

template <typename T> int launch_rpca_sumsq(hipStream_t st, const T *v, int64_t count, double *partials) {
    SA_REQUIRE(v && partials && count >= 1, "rpca_sumsq: bad argument");
    const int64_t want = (count + kThreads - 1) / kThreads;
    const int nb = (int)(want < 1024 ? want : 1024);
    hipLaunchKernelGGL((rpca_sumsq_kernel<T>), dim3(nb), dim3(kThreads), sizeof(double) * 4, st, v, count, partials);
    SA_HIP(hipGetLastError());
    return nb;
}

#define SA_RPCA_INST(T)                                                                \
    template int launch_rpca_gram<T>(hipStream_t, const RpcaGramArgs<T> &);            \
    template void launch_rpca_gram_reduce<T>(hipStream_t, const RpcaGramArgs<T> &);    \
    template int launch_rpca_iter<T>(hipStream_t, const RpcaIterArgs<T> &);            \
    template int launch_rpca_sumsq<T>(hipStream_t, const T *, int64_t, double *);
SA_RPCA_INST(float)
SA_RPCA_INST(double)

}  // namespace sporco_amd
