// csc_fused_kernels.inc -- the register-resident column kernels of the ADMM X-step (csc_fused.h; see
// csc_fused.hip for the method) and their launchers, included by csc_fused.hip (the dispatch, the
// host tables and the powers of two) and by csc_fused_mr.hip / csc_fused_mr2.hip (the mixed-radix
// heights).
#include "csc_fused.h"

#include "csc_fused_body.h"
#include "regfft.h"

#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <utility>

namespace sporco_amd {

namespace {

using namespace regfft;

template <int N1, int NW, int LP, int KC, bool GRAD, bool KRT = false, bool PER_TILE = false,
          int DBG = 0>
// (compile-time K: four waves per SIMD, i.e. at most 128 registers -- at 8 waves per workgroup that is
// the difference between two workgroups on a CU and one, and the GradReg form at H = 256 sat at 130)
__global__ void __launch_bounds__(NW * 64) SA_MIN_WAVES_PER_SIMD(KC == 64 ? 4 : 1)
fused_cols_kernel(const FusedColsArgs<float> a) {
    constexpr bool PERSIST = NW == 16 && KC == 64;   // (run-time K: scalar registers are short)
    constexpr int AOFF = 0;
    SA_ARGS_PTR_T(FusedColsArgs<float>) afix = nullptr;
    (void)afix;
#include "csc_fused_body.inc"
}

// Dual residual of the mask-decoupled X-step (cbpdn.py:1814-1818): the forward half of the column
// pass on the row spectra of u1 -- load the tile, FFT-N1, twiddle, exchange, FFT-NW -- and then, per
// frequency f, sum_k |conj(Df[f][k]) u0f[f] + u1f[f][k]|^2 instead of a solve; nothing is written
// back (one read pass over the spectrum).  partials[tile] carries the Parseval weight of wf.
// N1: rows per thread -- 32, or a mixed-radix length (16 waves, LP = 1; the second exchange group partly
// filled, as in csc_fused_body.inc)
template <int NW, int LP, int KC, int N1 = 32>
__global__ void __launch_bounds__(NW * 64) cols_dualres_kernel(const FusedColsArgs<float> a) {
    constexpr bool MR = mr_length(N1);
    static_assert(!MR || (NW == 16 && LP == 1), "mixed-radix heights: 16 waves, one line per group");
    constexpr int H = N1 * NW, J = MR ? (N1 > NW ? 2 : 1) : N1 / NW;
    constexpr int LBW = ilog2(NW);
    constexpr int FP = LP * NW, Q = J / LP;
    static_assert(J % LP == 0, "lines per group must divide the lines per thread");
    const int tid = threadIdx.x;
    const int k = tid & 63;
    const int w = sa_readfirstlane(tid >> 6);
    const int K = KC ? KC : (a.Ks ? a.Ks : a.K);
    const bool kv = KC == 64 ? true : k < a.K;
    f2 *LA = dyn_lds<f2>();
    double *scratch = reinterpret_cast<double *>(LA + FP * NW * 64);
    const cf zero = mk<float>(0.f, 0.f);
    const int ko = (w * K + k) * (int)sizeof(cf);
    const int Wf = a.W / 2 + 1;
    const int64_t ntiles = (int64_t)Wf * a.CN;
    int token = 0;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int wf = (int)(tile / a.CN);
        const BufRsrc Tb = make_rsrc(a.t + tile * H * K, (uint32_t)(H * K * sizeof(cf)));
        const BufRsrc Db = make_rsrc(a.dft + (int64_t)wf * H * K, (uint32_t)(H * K * sizeof(cf)));
        const cf *S = a.sft + tile * H + w;
        const cf *twA = a.twA + w * N1;
        cf v[N1];
#pragma unroll
        for (int h1 = 0; h1 < N1; ++h1)
            v[h1] = kv ? buf_load_cf(Tb, ko, NW * h1 * K * (int)sizeof(cf)) : zero;
        dif1<N1, false>(v, 0);
        reg_fence<N1>(v, 0, token);
#pragma unroll
        for (int i = 1; i < N1; ++i) v[i] = cmul(v[i], twA[i]);
        reg_fence<N1>(v, 0, token);
        float acc = 0.f;
        static_for<Q>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            const bool lv = !MR || q * FP + w < N1;      // (this wave's line of the group exists)
#pragma unroll
            for (int fl = 0; fl < FP; ++fl) {
                if (q * FP + fl >= N1) continue;
                const cf x = v[pos1<N1>(q * FP + fl)];
                f2 t;
                t.x = x.re;
                t.y = x.im;
                LA[(fl * NW + w) * 64 + k] = t;
            }
            __syncthreads();
            if (lv) {
            cf u[FP];
#pragma unroll
            for (int jl = 0; jl < LP; ++jl) {
#pragma unroll
                for (int h2 = 0; h2 < NW; ++h2) {
                    const f2 t = LA[((w + NW * jl) * NW + h2) * 64 + k];
                    u[NW * jl + h2] = mk<float>(t.x, t.y);
                }
                dif<NW, false>(u, NW * jl);     // u[NW jl + i] = X[f1 + N1 brev(i)], f1 = w + NW j
            }
#pragma unroll
            for (int jl = 0; jl < LP; ++jl) {
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    const int fo = NW * (q * LP + jl) + N1 * brev(i, LBW);   // f - w
                    const cf d = kv ? buf_load_cf_cached(Db, ko, fo * K * (int)sizeof(cf)) : zero;
                    cf s0;
                    sa_uload2(reinterpret_cast<const float *>(S + fo), s0.re, s0.im);
                    const cf val = cmulc(d, s0) + u[NW * jl + i];
                    acc += kv ? cabs2(val) : 0.f;
                }
            }
            }   // lv
            __syncthreads();     // the exchange buffer is reused by the next group / tile
        });
        const double pw = (wf == 0 || ((a.W & 1) == 0 && wf == Wf - 1)) ? 1.0 : 2.0;
        double ac[1] = {(double)acc * pw};
        block_sum_store<1>(ac, scratch, a.partials + tile);
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// 64 < K <= 256 (csc_fused.h FusedSlabArgs): the column pass of NH = ceil(K / 64) slabs of 64
// filters as ONE launch.  The NH slab workgroups of a tile run side by side on
// different CUs, keep their 64-filter slab of the spectrum in registers, and exchange only
// the partial inner products through `qpart` (written through, flagged per (tile, slab) with
// the launch's sequence number): two X-sized passes.  The grid is persistent
// and never larger than the device holds at once (one 16-wave / two 8-wave workgroups per
// CU): partners are consecutive workgroup indices and walk the same tiles in the same order,
// so whoever waits, waits for a workgroup that is resident.  A poll that does not complete
// (2^22 rounds) raises `*coop_err` instead of hanging the device.
// ---------------------------------------------------------------------------
// PGM: the gradient step of the fused FISTA iteration for K > 64 instead (csc_pgm.h pgm_grad_ifft):
// the input rows are the spectrum Yf itself (no forward transform), the per-row coefficient is
// -(sum_k Df Yf - Sf) / L, the output goes to a.c.t, and partials[tile] = sum |sum_k Df Yf - Sf|^2.
// N1: rows per thread -- 32, or a mixed-radix length (16 waves, LP = 1: the second exchange group partly
// filled, as in csc_fused_body.inc; not with PGM)
template <int NW, int LP, int KS, bool GRAD, bool PGM = false, int N1 = 32>
__global__ void __launch_bounds__(NW * 64) cols_slab_coop_kernel(const FusedSlabArgs<float> aa) {
    static_assert(!(GRAD && PGM), "one or the other");
    constexpr bool MR = mr_length(N1);
    static_assert(!MR || (NW == 16 && LP == 1 && !PGM), "mixed-radix heights: 16 waves, one line per group, ADMM");
    constexpr int H = N1 * NW, J = MR ? (N1 > NW ? 2 : 1) : N1 / NW;
    constexpr int LBW = ilog2(NW);
    constexpr int FP = LP * NW, Q = J / LP, CPL = NW / 4, NCH = LP * CPL;
    static_assert(MR || Q * FP == N1, "a thread holds N1 spectrum rows");
    constexpr int NU = Q * FP;          // slots of the spectrum rows of a thread (>= N1)
    const int tid = threadIdx.x;
    const int k = tid & 63;
    const int w = sa_readfirstlane(tid >> 6);
    const int K = KS ? KS : aa.c.K;
    const int NH = (K + 63) / 64;
    const int slab = blockIdx.x % NH, pair = blockIdx.x / NH, npairs = gridDim.x / NH;
    const bool kv = KS == 128 ? true : slab * 64 + k < K;   // the last slab may be partial
    const cf zero = mk<float>(0.f, 0.f);
    const int xcd = pair & 7;          // (virtual: the residue of the row frequencies it walks)
    const int ko = (w * K + slab * 64 + k) * (int)sizeof(cf);
    f2 *L = dyn_lds<f2>();
    double *scratch = reinterpret_cast<double *>(L + FP * NW * 64);
    int token = 0;
    if (aa.c.ctl && aa.c.ctl->stop) return;     // (every workgroup of the launch sees the same value)
    {   // groups start a fraction of a tile's time apart (the partners of a group together)
        const int ph = (pair >> 3) % aa.c.stagger_groups;
        for (int i = 0; i < ph * aa.c.stagger_sleeps; ++i) __builtin_amdgcn_s_sleep(127);
    }
    // the partial sums this wave needs in phase 2, one row per lane: lane l < 32 holds row
    // r = l of slab 0 (+ 2, ...), lane l >= 32 the same row of slab 1 (+ 3, ...)
    const int rl = k & 31;
    const int fo_lane = NW * (rl / NW) + N1 * brev(rl % NW, LBW);
    // (mixed-radix heights: the line w + NW (rl / NW) may not exist -- its lanes hold zeros)
    const bool row_ok = !MR || (rl < NU && w + NW * (rl / NW) < N1);
    bool gave_up = false;

    for (int slot = pair >> 3;; slot += npairs >> 3) {
    SA_ARGS_PTR_T(FusedSlabArgs<float>) ap = sa_args_reload<true>(aa);
    const int Wf = ap->c.W / 2 + 1, CN = ap->c.CN;
    if (slot >= ((Wf + 7) / 8) * CN) break;
    const int wf = (slot / CN) * 8 + xcd;
    if (wf >= Wf) break;
    const int tile = wf * CN + slot % CN;
    const AdmmCtl *ctl = ap->c.ctl;
    const float rho = ctl ? ctl->rho_f : ap->c.rho;
    const uint32_t tbytes = (uint32_t)(H * K * sizeof(cf));
    const BufRsrc Tb = make_rsrc(ap->c.t + (int64_t)tile * H * K, tbytes);
    const BufRsrc Db = make_rsrc(ap->c.dft + (int64_t)wf * H * K, tbytes);
    const cf *twA = ap->c.twA + w * N1;
    const cf *twB = ap->c.twB + w * (J * NW);
    const cf *S = ap->c.sft + (int64_t)tile * H + w;
    const float *G = PGM ? nullptr : (GRAD ? ap->c.g1t : ap->c.gramt) + (int64_t)wf * H + w;
    const float *GH = ap->c.ghh + w;
    cf *qp = ap->qpart + (int64_t)tile * NH * H + w;      // [slab][f]
    // where this lane publishes: lane 16 e (+ 8) -> Re (Im) of row N1 brev(e, 2) 2^(LBW - 2) + ...
    float *pub = reinterpret_cast<float *>(qp + (int64_t)slab * H) +
                 2 * (N1 * (brev(k >> 4, 2) << (LBW - 2))) + ((k >> 3) & 1);
    unsigned *flags = ap->coop_flags + (int64_t)tile * NH;
    const unsigned seq = ap->coop_seq;
    float rg = 0.f, ak = 0.f, bk = 0.f, gw = 0.f;
    if constexpr (GRAD) {
        gw = sa_uload(ap->c.ghw + wf);
        ak = ap->c.mu * ((ap->c.wg && kv) ? ap->c.wg[slab * 64 + k] : 1.f);
        bk = ak * gw + rho;
    }

    // ---- phase 1: FFT along H, this slab's share of sum_k Df yuf ------------------------
    cf uall[NU];                       // the slab's spectrum rows: group q in [q FP, (q + 1) FP)
    if constexpr (MR) {
#pragma unroll
        for (int i = 0; i < NU; ++i) uall[i] = zero;
    }
    if constexpr (PGM) {
        // the iterate is already a spectrum: rows f = w + NW j + N1 brev(i) of Yf, and the slab's
        // share of sum_k Df Yf
        const BufRsrc Yb = make_rsrc(ap->pgm_yf + (int64_t)tile * H * K, tbytes);
        static_for<Q>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
#pragma unroll
            for (int jl = 0; jl < LP; ++jl) {
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    const int fo = NW * (q * LP + jl) + N1 * brev(i, LBW);
                    uall[q * FP + NW * jl + i] = kv ? buf_load_cf(Yb, ko, fo * K * (int)sizeof(cf)) : zero;
                }
            }
            static_for<NCH>([&](auto gc) {
                constexpr int g = decltype(gc)::value;
                constexpr int jl = g / CPL, c = g % CPL, j = q * LP + jl;
                float red[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int fo = NW * j + N1 * brev(4 * c + e, LBW);
                    const cf d = kv ? buf_load_cf_cached(Db, ko, fo * K * (int)sizeof(cf)) : zero;
                    const cf p = cmul(d, uall[q * FP + NW * jl + 4 * c + e]);
                    red[2 * e] = p.re;
                    red[2 * e + 1] = p.im;
                }
                const float tot = reduce8_across_lanes(red, k);
                constexpr int fo_c = NW * j + N1 * brev(c, LBW - 2);
                if ((k & 7) == 0) sa_store_agent(pub + 2 * fo_c, tot);
            });
        });
    } else {
        cf v[N1];
#pragma unroll
        for (int h1 = 0; h1 < N1; ++h1)
            v[h1] = kv ? buf_load_cf(Tb, ko, NW * h1 * K * (int)sizeof(cf)) : zero;
        dif1<N1, false>(v, 0);
        reg_fence<N1>(v, 0, token);
#pragma unroll
        for (int i = 1; i < N1; ++i) {
            cf tw;
            sa_uload2(reinterpret_cast<const float *>(twA + i), tw.re, tw.im);
            v[i] = cmul(v[i], tw);
        }
        reg_fence<N1>(v, 0, token);
        static_for<Q>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            const bool lv = !MR || q * FP + w < N1;      // (this wave's line of the group exists)
#pragma unroll
            for (int fl = 0; fl < FP; ++fl) {
                if (q * FP + fl >= N1) continue;
                const cf x = v[pos1<N1>(q * FP + fl)];
                f2 t;
                t.x = x.re;
                t.y = x.im;
                L[(fl * NW + w) * 64 + k] = t;
            }
            cf dn[4];
            auto prefetch = [&](auto gc) {
                constexpr int g = decltype(gc)::value;
                constexpr int jl = g / CPL, c = g % CPL, j = q * LP + jl;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int fo = NW * j + N1 * brev(4 * c + e, LBW);
                    dn[e] = kv ? buf_load_cf_cached(Db, ko, fo * K * (int)sizeof(cf)) : zero;
                }
            };
            if (lv) prefetch(std::integral_constant<int, 0>{});
            __syncthreads();
            if (lv) {
#pragma unroll
            for (int jl = 0; jl < LP; ++jl) {
#pragma unroll
                for (int h2 = 0; h2 < NW; ++h2) {
                    const f2 t = L[((w + NW * jl) * NW + h2) * 64 + k];
                    uall[q * FP + NW * jl + h2] = mk<float>(t.x, t.y);
                }
            }
            }
            if (q + 1 < Q) __syncthreads();
            if (lv) {
            static_for<NCH>([&](auto gc) {
                constexpr int g = decltype(gc)::value;
                constexpr int jl = g / CPL, c = g % CPL, j = q * LP + jl;
                if constexpr (c == 0) dif<NW, false>(uall, q * FP + NW * jl);
                cf d[4];
                float red[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = dn[e];
                if constexpr (g + 1 < NCH) prefetch(std::integral_constant<int, g + 1>{});
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    cf p = cmul(d[e], uall[q * FP + NW * jl + 4 * c + e]);
                    if constexpr (GRAD) {
                        const int fo = NW * j + N1 * brev(4 * c + e, LBW);
                        p = cscale(p, sa_rcp(ak * sa_uload(GH + fo) + bk));
                    }
                    red[2 * e] = p.re;
                    red[2 * e + 1] = p.im;
                }
                const float tot = reduce8_across_lanes(red, k);
                // lane 16 e holds Re, lane 16 e + 8 holds Im of the slab's partial sum for row
                // fo(e) = NW j + N1 brev(4 c + e): one store by those eight lanes
                constexpr int fo_c = NW * j + N1 * brev(c, LBW - 2);
                if ((k & 7) == 0) sa_store_agent(pub + 2 * fo_c, tot);
            });
            }   // lv
        });
    }
    // ---- publish, and wait for the other slabs of this tile ------------------------------
    sa_wait_stores();
    __syncthreads();
    if (tid == 0) sa_store_agent(flags + slab, seq);
    // what phase 2 needs besides the sums, requested before the wait: per row (one row per
    // lane, as the sums below) Sf and the Sherman-Morrison denominator; the first rows of Df
    float s_re, s_im, g_l, gh_l = 0.f;
    if (row_ok) {
        const f2 t = *reinterpret_cast<const f2 *>(S + fo_lane);
        s_re = t.x;
        s_im = t.y;
        g_l = PGM ? 0.f : G[fo_lane];
        if constexpr (GRAD) gh_l = GH[fo_lane];
    } else {
        s_re = s_im = 0.f;
        g_l = 1.f;
    }
    cf dn[4];
    auto prefetch_d = [&](auto nc) {
        constexpr int n = decltype(nc)::value;
        constexpr int q = n / NCH, g = n % NCH, jl = g / CPL, c = g % CPL, j = q * LP + jl;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int fo = NW * j + N1 * brev(4 * c + e, LBW);
            dn[e] = kv ? buf_load_cf_cached(Db, ko, fo * K * (int)sizeof(cf)) : zero;
        }
    };
    if (!MR || w < N1) prefetch_d(std::integral_constant<int, 0>{});
    if (tid < NH && tid != slab && !gave_up) {
        int polls = 0;
        while (sa_load_agent(flags + tid) != seq) {
            sa_spin_pause();
            if (++polls > (1 << 22)) {
                *ap->coop_err = 1;
                gave_up = true;      // (no further waiting in this launch: the result is void anyway)
                break;
            }
        }
    }
    __syncthreads();
    float qre = 0.f, qim = 0.f;
    for (int sl = 0; sl < NH; sl += 2) {
        const int mine = sl + (k >> 5);
        if (mine < NH && row_ok) {
            float a0, b0;
            sa_load_agent2(reinterpret_cast<const float *>(qp + (int64_t)mine * H + fo_lane), a0, b0);
            qre += a0;
            qim += b0;
        }
    }
    qre += __shfl_xor(qre, 32, 64);
    qim += __shfl_xor(qim, 32, 64);
    // the Sherman-Morrison coefficient of this lane's row (both halves of the wave hold it)
    cf coef_l;
    float obj_l;
    if constexpr (PGM) {
        const cf r = mk<float>(qre - s_re, qim - s_im);        // e_y = sum_k Df Yf - Sf
        coef_l = cscale(r, -ap->pgm_inv_L);
        obj_l = k < 32 ? cabs2(r) : 0.f;
        if (ap->pgm_ey && slab == 0 && k < 32) ap->pgm_ey[(int64_t)tile * H + w + fo_lane] = r;
    } else {
        if constexpr (GRAD)
            coef_l = cscale(mk<float>(s_re - rho * qre, s_im - rho * qim), sa_rcp(g_l));
        else
            coef_l = cscale(mk<float>(s_re - qre, s_im - qim), sa_rcp(g_l + rho));
        obj_l = k < 32 ? cabs2(coef_l) : 0.f;
    }

    // ---- phase 2: Sherman-Morrison with the complete sums, IFFT along H --------------------
    static_for<Q * NCH>([&](auto nc) {
        constexpr int n = decltype(nc)::value;
        constexpr int q = n / NCH, g = n % NCH, jl = g / CPL, c = g % CPL, j = q * LP + jl;
        const bool lv = !MR || q * FP + w < N1;          // (this wave's line of the group exists)
        // (the operand prefetch runs one chunk ahead: chunk n + 1 is requested when ITS line exists)
        constexpr int qn = (n + 1) / NCH;
        const bool lvn = !MR || qn * FP + w < N1;
        cf d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = dn[e];
        if constexpr (n + 1 < Q * NCH) {
            if (lvn) prefetch_d(std::integral_constant<int, n + 1>{});
        }
        if (lv) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = NW * j + 4 * c + e;        // the lane that holds this row's values
            const cf coef = mk<float>(sa_readlane(coef_l.re, r), sa_readlane(coef_l.im, r));
            cf &ue = uall[q * FP + NW * jl + 4 * c + e];
            if constexpr (GRAD) {
                const float gh = sa_readlane(gh_l, r);
                const cf xn = cscale(cscale(ue, rho) + cmulc(d[e], coef), sa_rcp(ak * gh + bk));
                rg += (gh + gw) * cabs2(xn);
                ue = xn;
            } else {
                // (product first, then the sum: the four-instruction cmulc_add measured 2 % slower
                // here -- 7.22 against 7.08 ms at 1024 x 1024, profiles/r06s_config3_ab.txt)
                ue = ue + cmulc(d[e], coef);
            }
        }
        if constexpr (c == CPL - 1) {
            dit<NW, true>(uall, q * FP + NW * jl);
#pragma unroll
            for (int h2 = 1; h2 < NW; ++h2) {
                cf tw;
                sa_uload2(reinterpret_cast<const float *>(twB + NW * j + h2), tw.re, tw.im);
                uall[q * FP + NW * jl + h2] = cmulc(tw, uall[q * FP + NW * jl + h2]);
            }
        }
        }   // lv
        if constexpr (g == NCH - 1) {
            {
                float &rg_ = rg;
                int &tk_ = token;
                SA_VGPR_FENCE3(rg_, tk_, tk_);
            }
            if (lv) {
#pragma unroll
            for (int jl2 = 0; jl2 < LP; ++jl2) {
#pragma unroll
                for (int h2 = 0; h2 < NW; ++h2) {
                    f2 t;
                    t.x = uall[q * FP + NW * jl2 + h2].re;
                    t.y = uall[q * FP + NW * jl2 + h2].im;
                    L[((w + NW * jl2) * NW + h2) * 64 + k] = t;
                }
            }
            }
            __syncthreads();
            // (back into the group's own registers: rows h1 = pos(q FP + fl) of the last stage)
#pragma unroll
            for (int fl = 0; fl < FP; ++fl) {
                if (q * FP + fl >= N1) continue;
                const f2 t = L[(fl * NW + w) * 64 + k];
                uall[q * FP + fl] = mk<float>(t.x, t.y);
            }
            if (q + 1 < Q) __syncthreads();
        }
    });
    cf v[N1];
#pragma unroll
    for (int i = 0; i < N1; ++i) v[pos1<N1>(i)] = uall[i];
    reg_fence<N1>(v, 0, token);
    dit1<N1, true>(v, 0);
#pragma unroll
    for (int h1 = 0; h1 < N1; ++h1)
        if (kv) buf_store_cf(Tb, ko, NW * h1 * K * (int)sizeof(cf), v[h1]);

    // every slab computes the same |coef|^2: slab 0 reports it
    const double pw = (wf == 0 || ((ap->c.W & 1) == 0 && wf == Wf - 1)) ? 1.0 : 2.0;
    if constexpr (GRAD) {
        const float wk = (ap->c.wg && kv) ? ap->c.wg[slab * 64 + k] : 1.f;
        double acc[2] = {slab == 0 ? (double)obj_l * pw : 0.0, kv ? (double)(rg * wk) * pw : 0.0};
        block_sum_store<2>(acc, scratch, ap->c.partials + 2 * ((int64_t)tile * NH + slab));
    } else if constexpr (PGM) {
        double acc[1] = {(double)obj_l};
        if (slab == 0) block_sum_store<1>(acc, scratch, ap->c.partials + tile);
    } else {
        double acc[1] = {(double)obj_l * pw * (double)rho * (double)rho};
        if (slab == 0) block_sum_store<1>(acc, scratch, ap->c.partials + tile);
    }
    __syncthreads();      // (scratch and the exchange buffer are reused by the next tile)
    }
}


// ---------------------------------------------------------------------------
// Launchers: one per kernel family, templated on the column shape -- <NW, 32> for the powers of
// two H = 32 NW (NW = 4, 8, 16; LP = 16 / NW lines per exchange group), <16, N1> for the
// mixed-radix heights H = 16 N1 (regfft.h SA_MR_LENGTHS; LP = 1).  csc_fused.hip switches over the
// shapes; the mixed-radix instantiations live in csc_fused_mr.hip and csc_fused_mr2.hip.
// ---------------------------------------------------------------------------

// Workgroups of a persistent launch: as many as the device holds at once (16-wave
// workgroups: one per CU; 8-wave ones: two), a multiple of 8 so that the XCD of a workgroup
// is blockIdx % 8 for every slot it walks.
int64_t persistent_grid(int NW) {
    const int cus = current_device_cus();
    if (NW != 16) return INT64_MAX;      // (the 8-wave kernel takes one tile per workgroup)
    return std::max<int64_t>(8, cus / 8 * 8);
}

template <int NW, int N1, int KC, bool GRAD, bool KRT = false, bool PER_TILE = false>
void fused_cols_variant(hipStream_t st, const FusedColsArgs<float> &a) {
    constexpr int LP = 16 / NW;
    const int64_t all = ceil_div(a.W / 2 + 1, 8) * 8 * a.CN;   // see the tile mapping in the kernel
    launch_lds<&fused_cols_kernel<N1, NW, LP, KC, GRAD, KRT, PER_TILE>>(
        dim3((unsigned)std::min<int64_t>(all, persistent_grid(KC == 64 ? NW : 0))), dim3(NW * 64),
        fused_lds_bytes(NW, LP), st, a);
}
// tail: the kernel owns the first 64 of a.K > 64 filters (FusedColsArgs::Kv)
template <int NW, int N1, int KC> void fused_cols_kc(hipStream_t st, const FusedColsArgs<float> &a, bool tail) {
    const bool grad = a.g1t != nullptr;
    if constexpr (!mr_length(N1)) {
        if (a.per_tile) return fused_cols_variant<NW, N1, KC, false, false, true>(st, a);
        if constexpr (KC == 64) {
            if (tail && grad) return fused_cols_variant<NW, N1, 64, true, true>(st, a);
        }
    }
    // (coef_out on a K <= 64 system: the instantiation that stores the multipliers -- the
    // mask-decoupled X-step reads D x = Sf - rho coef off them, api_maskdcpl.inc)
    if (grad) fused_cols_variant<NW, N1, KC, true>(st, a);
    else if (tail || a.coef_out) fused_cols_variant<NW, N1, KC, false, true>(st, a);
    else fused_cols_variant<NW, N1, KC, false>(st, a);
}

// Workgroups of the cooperating slab pass: NH per tile side by side, as many groups as the device
// holds at once with one workgroup per CU (a multiple of 8 groups: the residue of the row
// frequencies a group walks stays fixed).
template <int NW, int N1, int KS, bool GRAD, bool PGM>
void cols_slab_variant(hipStream_t st, const FusedSlabArgs<float> &a) {
    constexpr int LP = 16 / NW;
    const int cus = current_device_cus();
    const int NH = (int)ceil_div(a.c.K, 64);
    int groups = (cus / NH) & ~7;
#ifdef SPORCO_AMD_HOSTSIM
    groups = 8;
    hostsim::set_coop(NH);     // (the CPU test simulator runs the NH partners side by side)
#endif
    SA_REQUIRE(groups >= 8, "too few compute units for cooperating slab workgroups");
    const int64_t slots = ceil_div(a.c.W / 2 + 1, 8) * a.c.CN;
    if ((int64_t)(groups >> 3) > slots) groups = (int)slots * 8;
    launch_lds<&cols_slab_coop_kernel<NW, LP, KS, GRAD, PGM, N1>>(dim3((unsigned)(groups * NH)), dim3(NW * 64),
                                                                 fused_lds_bytes(NW, LP), st, a);
}
template <int NW, int N1, int KS> void cols_slab_ks(hipStream_t st, const FusedSlabArgs<float> &a, bool pgm) {
    if constexpr (!mr_length(N1)) {
        if (pgm) return cols_slab_variant<NW, N1, KS, false, true>(st, a);
    }
    if (a.c.g1t) cols_slab_variant<NW, N1, KS, true, false>(st, a);
    else cols_slab_variant<NW, N1, KS, false, false>(st, a);
}

}  // namespace

// The column pass with K <= 64 (launch_fused_cols)
template <int NW, int N1> void fused_cols_launch(hipStream_t st, const FusedColsArgs<float> &a) {
    const bool tail = !a.per_tile && a.Kv == 64 && a.K > 64;
    SA_REQUIRE(!(a.per_tile && a.g1t), "per-tile operands do not combine with the gradient term");
    // mixed-radix heights: the plain system, the gradient term, or the multipliers stored (mask
    // decoupling); no per-tile operands, no tail -- the API layer keeps everything else on the generic chain
    SA_REQUIRE(!regfft::mr_length(N1) || (!a.per_tile && !tail && !(a.coef_out && a.g1t)),
               "mixed-radix heights: the plain and the gradient-regularised column pass only");
    if (a.K == 64 || tail) fused_cols_kc<NW, N1, 64>(st, a, tail);
    else fused_cols_kc<NW, N1, 0>(st, a, tail);
}

// The dual residual (launch_cols_dualres)
template <int NW, int N1> void cols_dualres_launch(hipStream_t st, const FusedColsArgs<float> &a) {
    constexpr int LP = 16 / NW;
    const int64_t ntiles = (int64_t)(a.W / 2 + 1) * a.CN;
    // (one 16-wave workgroup fills a CU; two 8-wave, four 4-wave ones share it)
    const dim3 grid((unsigned)std::min<int64_t>(ntiles, (int64_t)current_device_cus() * LP)), block(NW * 64);
    if (a.K == 64 && (a.Ks == 0 || a.Ks == 64))
        launch_lds<&cols_dualres_kernel<NW, LP, 64, N1>>(grid, block, fused_lds_bytes(NW, LP), st, a);
    else
        launch_lds<&cols_dualres_kernel<NW, LP, 0, N1>>(grid, block, fused_lds_bytes(NW, LP), st, a);
}

// The cooperating slab pass with 64 < K <= 256: the ADMM column pass (launch_cols_slab_coop), or with
// `pgm` the gradient step of the fused FISTA iteration (launch_pgm_grad_slabs)
template <int NW, int N1> void cols_slab_launch(hipStream_t st, const FusedSlabArgs<float> &a, bool pgm) {
    // mixed-radix heights: a run-time row stride only, and no FISTA form
    if constexpr (regfft::mr_length(N1)) {
        SA_REQUIRE(!pgm, "mixed-radix heights: no cooperating slab form of the FISTA gradient step");
    } else {
        if (a.c.K == 128) return cols_slab_ks<NW, N1, 128>(st, a, pgm);
    }
    cols_slab_ks<NW, N1, 0>(st, a, pgm);
}

// The mixed-radix launchers: instantiated in csc_fused_mr.hip (SA_MR_LENGTHS_LO) and
// csc_fused_mr2.hip (SA_MR_LENGTHS_HI), two translation units that compile side by side.
#define SA_FUSED_LAUNCHERS(DECL, n)                                                                \
    DECL void fused_cols_launch<16, n>(hipStream_t, const FusedColsArgs<float> &);               \
    DECL void cols_dualres_launch<16, n>(hipStream_t, const FusedColsArgs<float> &);             \
    DECL void cols_slab_launch<16, n>(hipStream_t, const FusedSlabArgs<float> &, bool);
#define SA_FUSED_EXTERN(n) SA_FUSED_LAUNCHERS(extern template, n)
SA_MR_LENGTHS(SA_FUSED_EXTERN)
#undef SA_FUSED_EXTERN

}  // namespace sporco_amd
