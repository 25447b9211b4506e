// csc_pgm_cmod.hip -- the kernels of csc_pgm_cmod.h: cmod_pgm_grad, cmod_pgm_reduce, cmod_pgm_prox, cmod_pgm_yrobust.
// float32 / float64, 1 <= M, N <= kCmodMaxDim, any K >= 1.  Compiled with -ffp-contract=off (Makefile): the two
// product forms must round alike, every fused multiply-add here is spelled out.
#include "csc_pgm_cmod.h"
#include "csc_kernels_dev.h"
#include "csc_cmod_cols.h"

namespace sporco_amd {

namespace {

// grid (row block, slab).  LDS: tz [M16][kCmodLd] the Z tile, tr [32][kCmodLd] the tile of R = w (Y Z - S).
// CTW: the 16-column tiles of G a wave accumulates (tiles wave, wave + 4, ...), both row halves of each.
template <typename T, int FORM, int CTW>
__global__ void __launch_bounds__(kThreads) cmod_pgm_grad_kernel(const PgmCmodGradArgs<T> a) {
    constexpr int RH = kPgmCmodRows / 16;
    const PgmCmodPlan &p = a.p;
    const int M = a.M, N = a.N, M4 = p.M4, M16 = p.M16, N16 = p.N16;
    const int row0 = (int)blockIdx.x * kPgmCmodRows, split = (int)blockIdx.y;
    const int64_t k_lo = (int64_t)split * p.slab;
    const int64_t k_hi = k_lo + p.slab < a.K ? k_lo + p.slab : a.K;
    T *tz = dyn_lds<T>();
    T *tr = tz + M16 * kCmodLd;
    double *scratch = reinterpret_cast<double *>(tr + kPgmCmodRows * kCmodLd);
    const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
    const int lc = lane & 15, lh = lane >> 4;
    const int nct = M16 / 16;
    // which row halves of the block exist (N16 is a multiple of 16, the block of 32)
    bool live[RH];
#pragma unroll
    for (int rh = 0; rh < RH; ++rh) live[rh] = row0 + 16 * rh < N16;
    // the residual tile of this wave: row half wave >> 1, column half wave & 1
    const int prh = wave >> 1, pch = wave & 1;
    const bool plive = row0 + 16 * prh < N16;
    // staging: thread t takes column t & 31 of rows t >> 5, + 8, ...
    const int sc = (int)threadIdx.x & (kCmodKS - 1), sr0 = (int)threadIdx.x / kCmodKS;
#ifndef SPORCO_AMD_HOSTSIM
    sa_floatx4 c[CTW][RH];
    if constexpr (FORM == BPDN_FORM_MFMA) {
#pragma unroll
        for (int i = 0; i < CTW; ++i)
#pragma unroll
            for (int rh = 0; rh < RH; ++rh) c[i][rh] = sa_floatx4{0.f, 0.f, 0.f, 0.f};
    }
#endif
    // (the matrix form keeps its sums in c alone)
    constexpr int ACT = FORM == BPDN_FORM_MFMA ? 1 : CTW;
    T acc[ACT][RH][4];
#pragma unroll
    for (int i = 0; i < ACT; ++i)
#pragma unroll
        for (int rh = 0; rh < RH; ++rh)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][rh][r] = T(0);
    // rows M .. M16 of the Z tile stay zero: no staging store touches them
    for (int idx = (int)threadIdx.x; idx < (M16 - M) * kCmodLd; idx += kThreads) tz[M * kCmodLd + idx] = T(0);
    double fy[1] = {0.0};
    for (int64_t kb = k_lo; kb < k_hi; kb += kCmodKS) {
        {
            const int64_t col = kb + sc;
            const bool col_ok = col < k_hi;
            for (int r = sr0; r < M; r += kThreads / kCmodKS)
                tz[r * kCmodLd + sc] = col_ok ? a.z[(int64_t)r * a.K + col] : T(0);
        }
        __syncthreads();
        // r = Y_blk . Ztile, k over the M4 rows of the tile
        {
            T ra[4] = {T(0), T(0), T(0), T(0)};
            if (plive) {
#ifndef SPORCO_AMD_HOSTSIM
                if constexpr (FORM == BPDN_FORM_MFMA) {
                    // A[i = l & 15][k = l >> 4] = Y, B[k = l >> 4][j = l & 15] = Ztile
                    sa_floatx4 cr = sa_floatx4{0.f, 0.f, 0.f, 0.f};
                    const T *ap = a.yk + (int64_t)lh * N16 + row0 + 16 * prh + lc;
                    const T *bp = tz + lh * kCmodLd + 16 * pch + lc;
                    for (int k0 = 0; k0 < M4; k0 += 4)
                        cr = sa_mfma_f32_16x16x4(ap[(int64_t)k0 * N16], bp[k0 * kCmodLd], cr);
                    ra[0] = cr.x;
                    ra[1] = cr.y;
                    ra[2] = cr.z;
                    ra[3] = cr.w;
                } else
#endif
                {
                    const T *ap = a.yk + row0 + 16 * prh + 4 * lh;
                    const T *bp = tz + 16 * pch + lc;
                    for (int k = 0; k < M4; ++k) {
                        const Vec<T, 4> av = *reinterpret_cast<const Vec<T, 4> *>(ap + (int64_t)k * N16);
                        const T bv = bp[k * kCmodLd];
#pragma unroll
                        for (int r = 0; r < 4; ++r) ra[r] = fma1(av.v[r], bv, ra[r]);
                    }
                }
            }
            const int64_t col = kb + 16 * pch + lc;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int lr = 16 * prh + 4 * lh + r, n = row0 + lr;
                T rv = T(0);
                if (n < N && col < k_hi) {
                    const int64_t off = (int64_t)n * a.K + col;
                    const T e = ra[r] - a.s[off], w = a.w ? a.w[off] : a.w_s;
                    rv = w * e;
                    fy[0] += (double)w * ((double)e * (double)e);
                }
                tr[lr * kCmodLd + 16 * pch + lc] = rv;
            }
        }
        __syncthreads();
        // G_blk += R . Ztile^T, k over the kCmodKS columns of the step
#ifndef SPORCO_AMD_HOSTSIM
        if constexpr (FORM == BPDN_FORM_MFMA) {
            // A[i = l & 15][k = l >> 4] = R, B[k = l >> 4][j = l & 15] = Ztile^T; D: column l & 15, rows 4 (l >> 4) + r
            const T *ap = tr + lc * kCmodLd + lh;
            const T *bp = tz + lc * kCmodLd + lh;
#pragma unroll
            for (int k0 = 0; k0 < kCmodKS; k0 += 4) {
                float av[RH];
#pragma unroll
                for (int rh = 0; rh < RH; ++rh) av[rh] = ap[16 * rh * kCmodLd + k0];
#pragma unroll
                for (int i = 0; i < CTW; ++i) {
                    const int ct = wave + 4 * i;
                    if (ct < nct) {
                        const float bv = bp[16 * ct * kCmodLd + k0];
#pragma unroll
                        for (int rh = 0; rh < RH; ++rh)
                            if (live[rh]) c[i][rh] = sa_mfma_f32_16x16x4(av[rh], bv, c[i][rh]);
                    }
                }
            }
        } else
#endif
        {
            const T *ap = tr + 4 * lh * kCmodLd;
            const T *bp = tz + lc * kCmodLd;
            for (int k = 0; k < kCmodKS; ++k) {
#pragma unroll
                for (int i = 0; i < CTW; ++i) {
                    const int ct = wave + 4 * i;
                    if (ct < nct) {
                        const T bv = bp[16 * ct * kCmodLd + k];
#pragma unroll
                        for (int rh = 0; rh < RH; ++rh)
                            if (live[rh]) {
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                    acc[i][rh][r] = fma1(ap[(16 * rh + r) * kCmodLd + k], bv, acc[i][rh][r]);
                            }
                    }
                }
            }
        }
        __syncthreads();
    }
    const auto sum_of = [&](int i, int rh, int r) -> T {
#ifndef SPORCO_AMD_HOSTSIM
        if constexpr (FORM == BPDN_FORM_MFMA) return c[i][rh][r];
        else
#endif
            return acc[i][rh][r];
    };
    // every element of the block's part of the padded plane [M16][N16] is written: the reduction reads no stale value
    T *dst = a.part + (int64_t)split * M16 * N16;
#pragma unroll
    for (int i = 0; i < CTW; ++i) {
        const int ct = wave + 4 * i;
        if (ct < nct) {
#pragma unroll
            for (int rh = 0; rh < RH; ++rh)
                if (live[rh]) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        dst[(int64_t)(16 * ct + lc) * N16 + row0 + 16 * rh + 4 * lh + r] = sum_of(i, rh, r);
                }
        }
    }
    block_sum_store<1>(fy, scratch,
                       a.partials + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * a.stride + PGMC_FY);
}

// one thread per element of the k-major G; workgroup b leaves its sums in row b of the table
template <typename T> __global__ void __launch_bounds__(kThreads) cmod_pgm_reduce_kernel(const PgmCmodGradArgs<T> a) {
    const PgmCmodPlan &p = a.p;
    const int total = a.M * p.N16;
    const int64_t plane = (int64_t)p.M16 * p.N16;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int idx = (int)(blockIdx.x * kThreads + threadIdx.x); idx < total; idx += (int)gridDim.x * kThreads) {
        if (idx % p.N16 >= a.N) continue;
        double s = 0.0;
        for (int sp = 0; sp < p.nsplit; ++sp) s += (double)a.part[sp * plane + idx];
        const T gv = (T)s;
        acc[0] += (double)gv * (double)gv;
        if (a.bb) {
            const double dg = (double)(gv - a.gk[idx]), dx = (double)(a.xprvk[idx] - a.xoldk[idx]);
            acc[1] += dx * dg;
            acc[2] += dg * dg;
        }
        a.gk[idx] = gv;
    }
    double *dst = a.partials + (int64_t)blockIdx.x * a.stride;
    double *scratch = dyn_lds<double>();
    const double g2[1] = {acc[0]};
    block_sum_store<1>(g2, scratch, dst + PGMC_G2);
    __syncthreads();
    const double bb[2] = {acc[1], acc[2]};
    block_sum_store<2>(bb, scratch, dst + PGMC_BBXG);
}

// one workgroup per 16 columns of the dictionary
template <typename T> __global__ void __launch_bounds__(kThreads) cmod_pgm_prox_kernel(const PgmCmodProxArgs<T> a) {
    const int M = a.M, N = a.N;
    const int N16 = (N + 15) & ~15;
    T *tv = dyn_lds<T>();                  // [N][16] V = Y - G / L; then X'
    double *cs = reinterpret_cast<double *>(tv + N16 * 16);
    double *scratch = cs + 256;
    const int j0 = 16 * (int)blockIdx.x;
    const T invL = T(1) / a.L;
    // thread t: column t & 15 of rows t >> 4, + 16, ...
    const int c = (int)threadIdx.x & 15, m = j0 + c;
    const bool col_ok = m < M;
    T mean = T(0), nrm = T(1);
    if (!a.revert) {
        for (int n = (int)threadIdx.x >> 4; n < N; n += 16) {
            T v = T(0);
            if (col_ok) {
                const int off = m * N16 + n;
                v = a.yk[off] - invL * a.gk[off];
                if (a.nonneg && v < T(0)) v = T(0);
            }
            tv[n * 16 + c] = v;
        }
        __syncthreads();
        cm_col_stats(tv, N, a.zero_mean, cs, mean, nrm);
    }
    double dxg = 0.0, dxy2 = 0.0, rs2 = 0.0, cns = 0.0;
    for (int n = (int)threadIdx.x >> 4; n < N; n += 16) {
        T xn = T(0);
        if (col_ok) {
            const int off = m * N16 + n;
            const T y = a.yk[off], gv = a.gk[off], xp = a.xprvk[off];
            T yn;
            if (a.revert) {
                xn = xp;
                yn = xn + a.gamma * (a.zzk_in[off] - xn);
            } else {
                xn = (tv[n * 16 + c] - mean) / nrm;
                if (a.zzk) a.zzk[off] = xn;
                yn = xn;
            }
            yn = yn + a.beta * (xn - xp);
            a.xk[off] = xn;
            if (a.ynextk) a.ynextk[off] = yn;
            const double d = (double)(xn - y), dr = (double)(xn - (a.rs_ynext ? yn : a.yprvk ? a.yprvk[off] : y));
            dxg += d * (double)gv;
            dxy2 += d * d;
            rs2 += dr * dr;
        }
        tv[n * 16 + c] = xn;      // (this thread's own elements)
    }
    __syncthreads();
    // Cnstr: || Pcn(X') - X' ||^2 (X' is not negative under NonNegCoef: the clip of Pcn changes nothing)
    cm_col_stats(tv, N, a.zero_mean, cs, mean, nrm);
    if (col_ok) {
        for (int n = (int)threadIdx.x >> 4; n < N; n += 16) {
            T xv = tv[n * 16 + c];
            if (a.nonneg && xv < T(0)) xv = T(0);
            const double d = (double)((xv - mean) / nrm - tv[n * 16 + c]);
            cns += d * d;
        }
    }
    double *dst = a.partials + (int64_t)blockIdx.x * a.stride;
    const double s3[3] = {dxg, dxy2, cns};
    block_sum_store<3>(s3, scratch, dst + PGMC_DXG);
    __syncthreads();
    const double s1[1] = {rs2};
    block_sum_store<1>(s1, scratch, dst + PGMC_RS2);
}

template <typename T>
__global__ void __launch_bounds__(kThreads)
    cmod_pgm_yrobust_kernel(const T *xprv, const T *yprv, T *z, T *y, T tk, T tt, T TT, T zc, int z_update, int n) {
    for (int off = (int)(blockIdx.x * kThreads + threadIdx.x); off < n; off += (int)gridDim.x * kThreads) {
        const T xp = xprv[off];
        T zv = z[off];
        if (z_update) {
            zv = zv + zc * (xp - yprv[off]);
            z[off] = zv;
        }
        y[off] = (tk * xp + tt * zv) / TT;
    }
}

template <auto KERNEL, typename A> void pc_launch(dim3 grid, size_t lds, hipStream_t st, const A &a) {
    static PerDeviceOnce attr_set;
    if (attr_set.first())
        SA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   160 * 1024));
    hipLaunchKernelGGL(KERNEL, grid, dim3(kThreads), lds, st, a);
    SA_HIP(hipGetLastError());
}

// whether the launch may use the matrix instruction: float32 on the device
template <typename T> constexpr bool pc_has_mfma() {
#ifdef SPORCO_AMD_HOSTSIM
    return false;
#else
    return sizeof(T) == 4;
#endif
}

inline bool pc_dims_ok(int M, int N) { return M >= 1 && M <= kCmodMaxDim && N >= 1 && N <= kCmodMaxDim; }

template <typename T> bool pc_plan_ok(const PgmCmodGradArgs<T> &a) {
    const PgmCmodPlan ref = pgm_cmod_plan(a.N, a.M, a.K);
    return a.p.slab == ref.slab && a.p.nsplit == ref.nsplit && a.p.NRB == ref.NRB && a.p.M16 == ref.M16 &&
           a.p.N16 == ref.N16 && a.p.M4 == ref.M4 && a.p.ctw == ref.ctw;
}

template <typename T, int FORM> void pc_launch_grad(dim3 grid, size_t lds, hipStream_t st, const PgmCmodGradArgs<T> &a) {
    switch (a.p.ctw) {
    case 1: pc_launch<&cmod_pgm_grad_kernel<T, FORM, 1>>(grid, lds, st, a); break;
    case 2: pc_launch<&cmod_pgm_grad_kernel<T, FORM, 2>>(grid, lds, st, a); break;
    case 4: pc_launch<&cmod_pgm_grad_kernel<T, FORM, 4>>(grid, lds, st, a); break;
    default: pc_launch<&cmod_pgm_grad_kernel<T, FORM, 8>>(grid, lds, st, a); break;
    }
}

}  // namespace

template <typename T> int launch_cmod_pgm_grad(hipStream_t st, const PgmCmodGradArgs<T> &a) {
    SA_REQUIRE(pc_dims_ok(a.M, a.N) && a.K >= 1 && a.K < (int64_t)1 << 31, "cmod_pgm_grad: bad argument");
    SA_REQUIRE(a.z && a.s && a.yk && a.part && a.partials && a.stride > PGMC_FY, "cmod_pgm_grad: null argument");
    SA_REQUIRE(pc_plan_ok(a), "cmod_pgm_grad: the plan is not that of the problem");
    SA_REQUIRE(a.form == BPDN_FORM_PLAIN || a.form == BPDN_FORM_MFMA, "cmod_pgm_grad: bad form");
    const size_t lds = pgm_cmod_grad_lds_bytes<T>(a.M);
    SA_REQUIRE(lds <= (size_t)160 * 1024, "cmod_pgm_grad: the tiles do not fit in LDS");
    const dim3 grid(a.p.NRB, a.p.nsplit);
    if (a.form == BPDN_FORM_MFMA) {
        SA_REQUIRE(pc_has_mfma<T>(), "cmod_pgm_grad: the matrix form exists in float32 on the device only");
        if constexpr (pc_has_mfma<T>()) pc_launch_grad<T, BPDN_FORM_MFMA>(grid, lds, st, a);
    } else {
        pc_launch_grad<T, BPDN_FORM_PLAIN>(grid, lds, st, a);
    }
    return (int)(grid.x * grid.y);
}

template <typename T> int launch_cmod_pgm_reduce(hipStream_t st, const PgmCmodGradArgs<T> &a) {
    SA_REQUIRE(pc_dims_ok(a.M, a.N) && a.part && a.gk && a.partials && a.stride > PGMC_BBG2,
               "cmod_pgm_reduce: bad argument");
    SA_REQUIRE(pc_plan_ok(a), "cmod_pgm_reduce: the plan is not that of the problem");
    SA_REQUIRE(!a.bb || (a.xprvk && a.xoldk), "cmod_pgm_reduce: null argument");
    static_assert(kThreads == 256, "pgm_cmod_reduce_blocks counts workgroups of 256 threads");
    const int nb = pgm_cmod_reduce_blocks(a.M, a.p.N16);
    hipLaunchKernelGGL((cmod_pgm_reduce_kernel<T>), dim3(nb), dim3(kThreads), sizeof(double) * 2 * (kThreads / kWave), st,
                       a);
    SA_HIP(hipGetLastError());
    return nb;
}

template <typename T> int launch_cmod_pgm_prox(hipStream_t st, const PgmCmodProxArgs<T> &a) {
    SA_REQUIRE(pc_dims_ok(a.M, a.N) && a.yk && a.gk && a.xprvk && a.xk && a.partials && a.stride > PGMC_RS2,
               "cmod_pgm_prox: null argument");
    SA_REQUIRE(a.L > T(0), "cmod_pgm_prox: L must be positive");
    SA_REQUIRE(!(a.zero_mean && a.nonneg), "cmod_pgm_prox: ZeroMean and NonNegCoef exclude each other");
    SA_REQUIRE(!a.revert || a.zzk_in, "cmod_pgm_prox: a revert reads ZZ");
    const size_t lds = pgm_cmod_prox_lds_bytes<T>(a.N);
    SA_REQUIRE(lds <= (size_t)160 * 1024, "cmod_pgm_prox: the tile does not fit in LDS");
    const int nb = bpdn_up(a.M, 16) / 16;
    pc_launch<&cmod_pgm_prox_kernel<T>>(dim3(nb), lds, st, a);
    return nb;
}

template <typename T>
void launch_cmod_pgm_yrobust(hipStream_t st, const T *xprv, const T *yprv, T *z, T *y, T tk, T tt, T TT, T zc, int z_update,
                             int n) {
    SA_REQUIRE(xprv && z && y && n >= 1 && TT != T(0) && (!z_update || yprv), "cmod_pgm_yrobust: bad argument");
    const int nb = (n + kThreads - 1) / kThreads;
    hipLaunchKernelGGL((cmod_pgm_yrobust_kernel<T>), dim3(nb < 1024 ? nb : 1024), dim3(kThreads), 0, st, xprv, yprv, z, y, tk,
                       tt, TT, zc, z_update, n);
    SA_HIP(hipGetLastError());
}

#define SA_PGM_CMOD_INST(T)                                                                 \
    template int launch_cmod_pgm_grad<T>(hipStream_t, const PgmCmodGradArgs<T> &);          \
    template int launch_cmod_pgm_reduce<T>(hipStream_t, const PgmCmodGradArgs<T> &);        \
    template int launch_cmod_pgm_prox<T>(hipStream_t, const PgmCmodProxArgs<T> &);          \
    template void launch_cmod_pgm_yrobust<T>(hipStream_t, const T *, const T *, T *, T *, T, T, T, T, int, int);
SA_PGM_CMOD_INST(float)
SA_PGM_CMOD_INST(double)

}  // namespace sporco_amd
