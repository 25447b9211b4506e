// csc_pgm.hip -- the column passes of the fused PGM iteration (csc_pgm.h): the launchers' switch
// over the column shapes, and the small kernels of the K > 64 forms.  The column kernels and the
// per-shape launchers are in csc_pgm_body.inc.
#include "csc_pgm_body.inc"

namespace sporco_amd {

namespace {

// K > 64: the objective sums from the slabs' shares of sum_k Df Xf' (see csc_pgm.h)
__global__ void __launch_bounds__(256) pgm_stats_slabs_kernel(const PgmColsArgs<float> a, int NH,
                                                              double *partials2) {
    const int tile = blockIdx.x, Wf = a.W / 2 + 1, wf = tile / a.CN;
    const cf *qp = a.qpart + (int64_t)tile * NH * a.H;
    const cf *S = a.sft + (int64_t)tile * a.H;
    const cf *EY = a.ey ? a.ey + (int64_t)tile * a.H : nullptr;
    double fs = 0.0, lin = 0.0;
    for (int f = threadIdx.x; f < a.H; f += blockDim.x) {
        cf ex = mk<float>(0.f, 0.f);
        for (int sl = 0; sl < NH; ++sl) ex = ex + qp[(int64_t)sl * a.H + f];
        ex = ex - S[f];
        fs += (double)cabs2(ex);
        if (EY) {
            const cf ey = EY[f];
            lin += (double)((ex.re - ey.re) * ey.re + (ex.im - ey.im) * ey.im);
        }
    }
    const double pw = (wf == 0 || ((a.W & 1) == 0 && wf == Wf - 1)) ? 1.0 : 2.0;
    double acc[3] = {fs * pw, fs, lin};
    block_sum_store<3>(acc, dyn_lds<double>(), partials2 + (int64_t)tile * 3);
}

// K > 64, between the two passes: r = sum_slab qpart - sf per frequency of a tile, and the sums
// of the one-pass kernel per tile
__global__ void __launch_bounds__(256) ccmod_resid_sum_kernel(const CcmodTiledArgs<float> a, int NH) {
    const int tile = blockIdx.x, Wf = a.W / 2 + 1, wf = tile / a.CN;
    const cf *qp = a.qpart + (int64_t)tile * NH * a.H;
    const cf *S = a.sft + (int64_t)tile * a.H;
    cf *R = a.rbuf + (int64_t)tile * a.H;
    double r2 = 0.0, q2 = 0.0;
    for (int f = threadIdx.x; f < a.H; f += blockDim.x) {
        cf q = mk<float>(0.f, 0.f);
        for (int sl = 0; sl < NH; ++sl) q = q + qp[(int64_t)sl * a.H + f];
        const cf r = q - S[f];
        R[f] = r;
        r2 += (double)cabs2(r);
        q2 += (double)cabs2(q);
    }
    const double pw = (wf == 0 || ((a.W & 1) == 0 && wf == Wf - 1)) ? 1.0 : 2.0;
    double accd[4] = {r2, r2 * pw, q2, 0.0};
    block_sum_store<4>(accd, dyn_lds<double>(), a.partials + (int64_t)tile * 4);
}

__global__ void __launch_bounds__(256) sum_groups_kernel(const cf *__restrict__ part,
                                                         cf *__restrict__ out, int64_t n, int G) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        cf s = part[i];
        for (int g = 1; g < G; ++g) s = s + part[(int64_t)g * n + i];
        out[i] = s;
    }
}

}  // namespace

void launch_ccmod_resid_sum(hipStream_t st, const CcmodTiledArgs<float> &a, int slabs) {
    const int64_t ntiles = (int64_t)(a.W / 2 + 1) * a.CN;
    hipLaunchKernelGGL(ccmod_resid_sum_kernel, dim3((unsigned)ntiles), dim3(256), sizeof(double) * 4 * 16, st, a,
                       slabs);
}

// heights of the column kernels: 128, 256, 512 with 1 <= K <= kmax, the mixed-radix ones with K <= 64
static bool pgm_shape_ok(int H, int K, int kmax) {
    return K >= 1 && (fused_mr_height(H) ? K <= 64 : fused_pow2_height(H) && K <= kmax);
}

template <> int64_t launch_pgm_grad_ifft<float>(hipStream_t st, const PgmColsArgs<float> &a) {
    SA_REQUIRE(pgm_shape_ok(a.H, a.K, 64), "shape not handled by the fused PGM kernels");
    regfft::with_line_shape(a.H, [&](auto nw, auto n1) { pgm_grad_launch<nw.value, n1.value>(st, a); });
    SA_HIP(hipGetLastError());
    return (int64_t)(a.W / 2 + 1) * a.CN;
}
template <> int64_t launch_pgm_grad_ifft<double>(hipStream_t, const PgmColsArgs<double> &) {
    throw Error(-1, "the fused PGM kernels are float32 only");
}

template <> int64_t launch_pgm_stats_slabs<float>(hipStream_t st, const PgmColsArgs<float> &a,
                                                  double *partials2) {
    const int64_t ntiles = (int64_t)(a.W / 2 + 1) * a.CN;
    hipLaunchKernelGGL(pgm_stats_slabs_kernel, dim3((unsigned)ntiles), dim3(256), sizeof(double) * 3 * 4,
                       st, a, (int)ceil_div(a.K, 64), partials2);
    SA_HIP(hipGetLastError());
    return ntiles;
}
template <> int64_t launch_pgm_stats_slabs<double>(hipStream_t, const PgmColsArgs<double> &, double *) {
    throw Error(-1, "the fused FISTA kernels are float32 only");
}

template <> int64_t launch_pgm_fft_momentum<float>(hipStream_t st, const PgmColsArgs<float> &a) {
    SA_REQUIRE(pgm_shape_ok(a.H, a.K, 256), "shape not handled by the fused PGM kernels");
    SA_REQUIRE(a.K <= 64 || !a.want_stats || a.qpart, "K > 64 with statistics needs qpart");
    SA_REQUIRE(!a.ey || a.want_stats, "the backtracking sums need want_stats");
    regfft::with_line_shape(a.H, [&](auto nw, auto n1) { pgm_mom_launch<nw.value, n1.value>(st, a, false); });
    SA_HIP(hipGetLastError());
    return (int64_t)(a.W / 2 + 1) * a.CN * ceil_div(a.K, 64);
}
template <> int64_t launch_pgm_fft_momentum<double>(hipStream_t, const PgmColsArgs<double> &) {
    throw Error(-1, "the fused PGM kernels are float32 only");
}

template <> int64_t launch_cols_fft<float>(hipStream_t st, const PgmColsArgs<float> &a) {
    SA_REQUIRE(pgm_shape_ok(a.H, a.K, 256), "shape not handled by the fused column kernels");
    regfft::with_line_shape(a.H, [&](auto nw, auto n1) { pgm_mom_launch<nw.value, n1.value>(st, a, true); });
    SA_HIP(hipGetLastError());
    return (int64_t)(a.W / 2 + 1) * a.CN;
}
template <> int64_t launch_cols_fft<double>(hipStream_t, const PgmColsArgs<double> &) {
    throw Error(-1, "the fused column kernels are float32 only");
}

template <> bool ccmod_tiled_supported<float>(int H, int K) { return pgm_shape_ok(H, K, 256); }
template <> bool ccmod_tiled_supported<double>(int, int) { return false; }

template <> int64_t launch_ccmod_grad_tiled<float>(hipStream_t st, const CcmodTiledArgs<float> &a) {
    SA_REQUIRE(ccmod_tiled_supported<float>(a.H, a.K), "shape not handled by the tiled D-step kernel");
    const int64_t rows =
        regfft::with_line_shape(a.H, [&](auto nw, auto n1) { return ccmod_tiled_launch<nw.value, n1.value>(st, a); });
    SA_HIP(hipGetLastError());
    return rows;
}
template <> int64_t launch_ccmod_grad_tiled<double>(hipStream_t, const CcmodTiledArgs<double> &) {
    throw Error(-1, "the tiled D-step kernel is float32 only");
}

template <>
void launch_sum_groups<float>(hipStream_t st, const cx<float> *part, cx<float> *out, int64_t n, int G) {
    int64_t grid = ceil_div(n, 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(sum_groups_kernel, dim3((unsigned)grid), dim3(256), 0, st, part, out, n, G);
    SA_HIP(hipGetLastError());
}
template <>
void launch_sum_groups<double>(hipStream_t, const cx<double> *, cx<double> *, int64_t, int) {
    throw Error(-1, "float32 only");
}

}  // namespace sporco_amd
