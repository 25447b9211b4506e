// csc_fused.hip -- register-resident column FFT + Sherman-Morrison + column IFFT.
//
// One workgroup of NW waves owns one (wf, cn) tile: all H = N1 * NW points of all K <= 64
// filters -- H = 32 NW on NW = 4, 8 or 16 waves (H = 128, 256, 512), or H = 16 N1 on 16 waves for
// the mixed-radix N1 = 10 ... 30 (H = 160 ... 480; regfft.h SA_MR_LENGTHS).  A tile is 256 KiB of
// complex64 at 512 x 64, which is why it lives in the 512 KiB vector register file and
// not in the 160 KiB LDS.  Lane = filter k, so every global access of a wave
// is one contiguous K*8-byte row and the K-length inner product of
// linalg.solvedbi_sm (sporco/linalg.py:232-297) is a cross-lane reduction.
//
// The length-H transform is split H = N1 x NW (Cooley-Tukey):
//   forward   wave w holds rows h = NW*h1 + w:   DIF FFT-N1 over h1 in registers,
//             twiddle W_H^(w*f1), exchange through LDS so that wave w' holds the lines
//             f1 = w' + NW*j x all NW h2, DIF FFT-NW over h2  ->  X[f1 + N1*f2]
//   solve     per frequency f: q = sum_k Df*yuf (transposing wave reduction),
//             xf = yuf + conj(Df) * (Sf - q) / (sum_k |Df|^2 + rho)
//   inverse   the mirror image (DIT FFT-NW, conj twiddle, LDS exchange, DIT FFT-N1),
//             landing on the rows the wave loaded, stored in place.
// LDS is used only for the two exchanges, a group of 16 lines at a time (LP = 16 / NW lines of NW
// points per wave: 128 KiB at 16 waves).  Forward FFTs are decimation-in-frequency (natural in,
// digit-reversed out), inverse ones decimation-in-time (digit-reversed in, natural
// out), so no reordering pass exists anywhere.
//
// This file: the host tables, the predicates, the public launchers' switch over the column shapes,
// and the small kernels around the column pass.  The column kernels and the per-shape launchers are
// in csc_fused_kernels.inc; their mixed-radix instantiations in csc_fused_mr.hip / csc_fused_mr2.hip.
#include "csc_fused_kernels.inc"

namespace sporco_amd {

namespace {

// g1t[wf][h] = 1 + sum_k |Df|^2 / (mu wg_k (ghh[h] + ghw[wf]) + rho): the Sherman-Morrison
// denominator of linalg.solvedbd_sm_c (linalg.py:346-366), refreshed when rho changes.
// One wave per (wf, h) row of the tile-major Df, lane = filter.
__global__ void __launch_bounds__(256) grad_g1_kernel(const FusedColsArgs<float> a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nrows = (int64_t)(a.W / 2 + 1) * a.H;
    if (row >= nrows) return;
    const int wf = (int)(row / a.H), h = (int)(row % a.H);
    const float gh = a.ghh[h], gw = a.ghw[wf];
    float s = 0.f;
    const int Ks = a.Ks ? a.Ks : a.K;
    for (int k = lane; k < a.K; k += 64) {
        const float ak = a.mu * (a.wg ? a.wg[k] : 1.f);
        const float dd = ak * gh + (ak * gw + a.rho);
        s += cabs2(a.dft[row * Ks + k]) / dd;
    }
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) a.g1t_out[row] = 1.f + s;
}

template <typename E>
__global__ void __launch_bounds__(256) permute_ab_kernel(const E *__restrict__ in,
                                                         E *__restrict__ out, int64_t A, int64_t B,
                                                         int64_t C, int64_t Cin, int64_t Cout) {
    const int64_t n = A * B * C;
    for (int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; o < n;
         o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = o % C, ba = o / C;
        const int64_t aa = ba % A, bb = ba / A;
        out[ba * Cout + c] = in[(aa * B + bb) * Cin + c];
    }
}

}  // namespace

template <typename E>
void launch_permute_ab(hipStream_t st, const E *in, E *out, int64_t A, int64_t B, int64_t C,
                       int64_t in_stride, int64_t out_stride) {
    const int64_t n = A * B * C;
    if (n <= 0) return;
    int64_t g = ceil_div(n, 256);
    if (g > 8192) g = 8192;
    hipLaunchKernelGGL((permute_ab_kernel<E>), dim3((unsigned)g), dim3(256), 0, st, in, out, A, B, C,
                       in_stride ? in_stride : C, out_stride ? out_stride : C);
    SA_HIP(hipGetLastError());
}

bool fused_mr_height(int H) { return H % 16 == 0 && regfft::mr_length(H / 16); }
// (the second table has (lines per wave) x 16 entries for each of the 16 waves)
int fused_twiddle_count(int H) { return fused_mr_height(H) ? (H > 256 ? 512 : 256) : H; }

template <typename T> void fused_twiddles(int H, int, cx<T> *twA, cx<T> *twB) {
    // H = N1 x NW: 32 rows per thread on H / 32 waves, or H / 16 = 10 ... 30 rows on 16 waves
    const bool mr = fused_mr_height(H);
    const int NW = mr ? 16 : H / 32, N1 = H / NW;
    // (mixed-radix heights: two stage-2 lines per wave, the second one only while w + 16 < N1; the
    // second table has J NW = 32 entries per wave -- fused_twiddle_count(H) in all)
    const int J = mr ? (N1 > NW ? 2 : 1) : N1 / NW;
    const double two_pi = 6.283185307179586476925286766559;
    for (int w = 0; w < NW; ++w) {
        for (int i = 0; i < N1; ++i) {
            const double ang = -two_pi * (double)(w * regfft::line_rev(N1, i)) / (double)H;
            twA[w * N1 + i] = mk<T>((T)std::cos(ang), (T)std::sin(ang));
        }
        for (int j = 0; j < J; ++j)
            for (int h2 = 0; h2 < NW; ++h2) {
                const double ang = -two_pi * (double)((w + NW * j) * h2) / (double)H;
                twB[w * (J * NW) + NW * j + h2] = mk<T>((T)std::cos(ang), (T)std::sin(ang));
            }
    }
}
template void fused_twiddles<float>(int, int, cx<float> *, cx<float> *);
template void fused_twiddles<double>(int, int, cx<double> *, cx<double> *);

template <> bool fused_cols_supported<float>(int H, int K) {
    return (fused_pow2_height(H) || fused_mr_height(H)) && K >= 1 && K <= 64;
}
template <> bool fused_cols_supported<double>(int, int) { return false; }

template <> int64_t launch_fused_cols<float>(hipStream_t st, const FusedColsArgs<float> &a_in) {
    SA_REQUIRE(fused_cols_supported<float>(a_in.H, a_in.Kv ? a_in.Kv : a_in.K),
               "shape not handled by the fused column kernel");
    FusedColsArgs<float> a = a_in;
    // start-up stagger of the persistent workgroups: 4 phase groups 2 x 8128 cycles apart (about a
    // fifth of a tile's time each): measured 1.13 -> 1.06 ms at 512 x 512, K = 64, N = 32
    // (profiles/r02_fused_cols_notes.md)
    a.stagger_groups = kColsStaggerGroups;
    a.stagger_sleeps = kColsStaggerSleeps;
    regfft::with_line_shape(a.H, [&](auto nw, auto n1) { fused_cols_launch<nw.value, n1.value>(st, a); });
    SA_HIP(hipGetLastError());
    return (int64_t)(a.W / 2 + 1) * a.CN;
}
template <> int64_t launch_fused_cols<double>(hipStream_t, const FusedColsArgs<double> &) {
    throw Error(-1, "the fused column kernel is float32 only");
}

template <> int64_t launch_cols_dualres<float>(hipStream_t st, const FusedColsArgs<float> &a) {
    SA_REQUIRE(fused_cols_supported<float>(a.H, a.K), "shape not handled by the fused column kernel");
    regfft::with_line_shape(a.H, [&](auto nw, auto n1) { cols_dualres_launch<nw.value, n1.value>(st, a); });
    SA_HIP(hipGetLastError());
    return (int64_t)(a.W / 2 + 1) * a.CN;
}
template <> int64_t launch_cols_dualres<double>(hipStream_t, const FusedColsArgs<double> &) {
    throw Error(-1, "the fused column kernel is float32 only");
}
__global__ void __launch_bounds__(256) gram_rows_kernel(const cf *__restrict__ z,
                                                        float *__restrict__ out, int64_t nrows,
                                                        int K) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += cabs2(z[row * K + k]);
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) out[row] = s;
}
template <> void launch_gram_rows<float>(hipStream_t st, const cx<float> *z, float *out,
                                         int64_t nrows, int K) {
    hipLaunchKernelGGL(gram_rows_kernel, dim3((unsigned)ceil_div(nrows, 4)), dim3(256), 0, st, z, out,
                       nrows, K);
    SA_HIP(hipGetLastError());
}
template <> void launch_gram_rows<double>(hipStream_t, const cx<double> *, double *, int64_t, int) {
    throw Error(-1, "the fused column kernel is float32 only");
}
template <> void launch_grad_g1<float>(hipStream_t st, const FusedColsArgs<float> &a) {
    const int64_t nrows = (int64_t)(a.W / 2 + 1) * a.H;
    hipLaunchKernelGGL(grad_g1_kernel, dim3((unsigned)ceil_div(nrows, 4)), dim3(256), 0, st, a);
    SA_HIP(hipGetLastError());
}
template <> void launch_grad_g1<double>(hipStream_t, const FusedColsArgs<double> &) {
    throw Error(-1, "the fused column kernel is float32 only");
}
// ---------------------------------------------------------------------------
// a few more than 64 filters: the column pass of the filters >= Kv (csc_fused.h)
// ---------------------------------------------------------------------------
// sft_eff[tile][f] = sft[tile][f] - sum_{k >= Kv} dft[wf][f][k] t[tile][f][k]
// (gradient-regularised system, a.g1t set: - rho sum_{k >= Kv} dft t / dd_k, with
// dd_k = mu wg_k (ghh[f] + ghw[wf]) + rho as in the column kernel)
__global__ void __launch_bounds__(256) tail_inner_kernel(const FusedColsArgs<float> a,
                                                         const cf *__restrict__ sft,
                                                         cf *__restrict__ sft_eff, int64_t ntiles) {
    const int H = a.H, K = a.K, Kv = a.Kv, Ks = a.Ks ? a.Ks : a.K;
    const bool grad = a.g1t != nullptr;
    const int64_t total = ntiles * H;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t tile = i / H;
        const int f = (int)(i - tile * H);
        const int64_t wf = tile / a.CN;
        const cf *d = a.dft + (wf * H + f) * Ks, *x = a.t + i * Ks;
        const float gh = grad ? a.ghh[f] + a.ghw[wf] : 0.f;
        cf q = mk<float>(0.f, 0.f);
        for (int k = Kv; k < K; ++k) {
            cf p = cmul(d[k], x[k]);
            if (grad) p = cscale(p, a.rho / (a.mu * (a.wg ? a.wg[k] : 1.f) * gh + a.rho));
            q = q + p;
        }
        sft_eff[i] = sft[i] - q;
    }
}

// t[tile][f][k] += conj(dft[wf][f][k]) coef[tile][f] for k >= Kv; one workgroup per tile,
// thread = column frequency.  Gradient-regularised system: t = (rho t + conj(dft) coef) / dd_k,
// and the tail's share of the gradient term is added to the tile's second partial.
__global__ void __launch_bounds__(512) tail_update_kernel(const FusedColsArgs<float> a) {
    const int H = a.H, K = a.K, Kv = a.Kv, Ks = a.Ks ? a.Ks : a.K;
    const bool grad = a.g1t != nullptr;
    const int64_t tile = blockIdx.x;
    const int64_t wf = tile / a.CN;
    const int Wf = a.W / 2 + 1;
    double acc[1] = {0.0};
    for (int f = threadIdx.x; f < H; f += blockDim.x) {
        const int64_t row = tile * H + f;
        const cf cf_ = a.coef_out[row];
        const cf *d = a.dft + (wf * H + f) * Ks;
        cf *x = a.t + row * Ks;
        const float gh = grad ? a.ghh[f] + a.ghw[wf] : 0.f;
        for (int k = Kv; k < K; ++k) {
            if (grad) {
                const float wk = a.wg ? a.wg[k] : 1.f;
                const cf xn = cscale(cscale(x[k], a.rho) + cmulc(d[k], cf_),
                                     1.f / (a.mu * wk * gh + a.rho));
                x[k] = xn;
                acc[0] += (double)(gh * wk * cabs2(xn));
            } else {
                x[k] = x[k] + cmulc(d[k], cf_);
            }
        }
    }
    if (grad) {
        double *scratch = dyn_lds<double>();
        block_sum_store<1>(acc, scratch, scratch + 12);   // (thread 0 writes, thread 0 reads)
        if (threadIdx.x == 0) {
            const double pw = (wf == 0 || ((a.W & 1) == 0 && wf == Wf - 1)) ? 1.0 : 2.0;
            a.partials[2 * tile + 1] += scratch[12] * pw;
        }
    }
}

template <> void launch_tail_inner<float>(hipStream_t st, const FusedColsArgs<float> &a,
                                          const cx<float> *sft, cx<float> *sft_eff) {
    const int64_t ntiles = (int64_t)(a.W / 2 + 1) * a.CN;
    const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(ntiles * a.H, 256), 65535);
    hipLaunchKernelGGL(tail_inner_kernel, dim3(grid), dim3(256), 0, st, a, sft, sft_eff, ntiles);
    SA_HIP(hipGetLastError());
}
template <> void launch_tail_update<float>(hipStream_t st, const FusedColsArgs<float> &a) {
    const int64_t ntiles = (int64_t)(a.W / 2 + 1) * a.CN;
    hipLaunchKernelGGL(tail_update_kernel, dim3((unsigned)ntiles), dim3(a.H), sizeof(double) * 16, st, a);
    SA_HIP(hipGetLastError());
}
template <> void launch_tail_inner<double>(hipStream_t, const FusedColsArgs<double> &,
                                           const cx<double> *, cx<double> *) {
    throw Error(-1, "the fused column kernel is float32 only");
}
template <> void launch_tail_update<double>(hipStream_t, const FusedColsArgs<double> &) {
    throw Error(-1, "the fused column kernel is float32 only");
}

template <> bool fused_slabs_supported<float>(int H, int K) {
    return (fused_pow2_height(H) || fused_mr_height(H)) && K > 64 && K <= 256 && K % 2 == 0;
}
template <> bool fused_slabs_supported<double>(int, int) { return false; }

template <> int64_t launch_cols_slab_coop<float>(hipStream_t st, const FusedSlabArgs<float> &a_in) {
    SA_REQUIRE(fused_slabs_supported<float>(a_in.c.H, a_in.c.K), "shape not handled by the slab column kernels");
    SA_REQUIRE(a_in.coop_flags && a_in.coop_err, "the cooperating slab kernel needs its flag buffers");
    FusedSlabArgs<float> a = a_in;
    a.c.stagger_groups = kColsStaggerGroups;
    a.c.stagger_sleeps = kColsStaggerSleeps;
    regfft::with_line_shape(a.c.H, [&](auto nw, auto n1) { cols_slab_launch<nw.value, n1.value>(st, a, false); });
    SA_HIP(hipGetLastError());
    return (int64_t)(a.c.W / 2 + 1) * a.c.CN;
}
template <> int64_t launch_cols_slab_coop<double>(hipStream_t, const FusedSlabArgs<double> &) {
    throw Error(-1, "the fused column kernels are float32 only");
}

template <> int64_t launch_pgm_grad_slabs<float>(hipStream_t st, const FusedSlabArgs<float> &a_in) {
    SA_REQUIRE(fused_slabs_supported<float>(a_in.c.H, a_in.c.K), "shape not handled by the slab column kernels");
    SA_REQUIRE(a_in.coop_flags && a_in.coop_err && a_in.pgm_yf, "the cooperating slab kernel needs its buffers");
    FusedSlabArgs<float> a = a_in;
    a.c.stagger_groups = 1;
    a.c.stagger_sleeps = 0;
    regfft::with_line_shape(a.c.H, [&](auto nw, auto n1) { cols_slab_launch<nw.value, n1.value>(st, a, true); });
    SA_HIP(hipGetLastError());
    return (int64_t)(a.c.W / 2 + 1) * a.c.CN;
}
template <> int64_t launch_pgm_grad_slabs<double>(hipStream_t, const FusedSlabArgs<double> &) {
    throw Error(-1, "the fused column kernels are float32 only");
}

template void launch_permute_ab<float>(hipStream_t, const float *, float *, int64_t, int64_t, int64_t,
                                       int64_t, int64_t);
template void launch_permute_ab<double>(hipStream_t, const double *, double *, int64_t, int64_t,
                                        int64_t, int64_t, int64_t);
template void launch_permute_ab<cx<float>>(hipStream_t, const cx<float> *, cx<float> *, int64_t,
                                           int64_t, int64_t, int64_t, int64_t);
template void launch_permute_ab<cx<double>>(hipStream_t, const cx<double> *, cx<double> *, int64_t,
                                            int64_t, int64_t, int64_t, int64_t);

}  // namespace sporco_amd

