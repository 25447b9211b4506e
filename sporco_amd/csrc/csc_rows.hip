// csc_rows.hip -- the register-resident row passes of the fused ADMM iteration (csc_rows.h): host
// tables, the one-launch solve, and the launchers' switch over the line shapes.  The kernels and
// the per-shape launchers are in csc_rows_body.inc.
#include "csc_rows_body.inc"

namespace sporco_amd {

// points per thread of a supported line length: 32 for the powers of two, W / 16 for the
// mixed-radix lengths (regfft.h SA_MR_LENGTHS)
static int rows_n1(int W) { return rows_mr_width(W) ? W / 16 : kN1; }

bool rows_mr_width(int W) { return W % 16 == 0 && regfft::mr_length(W / 16); }
template <> bool rows_supported<float>(int W, int K) {
    return (W == 128 || W == 256 || W == 512 || rows_mr_width(W)) && K >= 2 && K % 2 == 0;
}
template <> bool rows_supported<double>(int, int) { return false; }
template <> bool rows_joint_supported<float>(int W, int C, int K) {
    return rows_supported<float>(W, K) && C >= 1 && C <= 4 && K % 32 == 0;
}
template <> bool rows_joint_supported<double>(int, int, int) { return false; }

template <typename T> void rows_twiddles(int W, cx<T> *twA) {
    const int N1 = rows_n1(W), NW = W / N1;
    const double two_pi = 6.283185307179586476925286766559;
    for (int w = 0; w < NW; ++w)
        for (int i = 0; i < N1; ++i) {
            const double ang = -two_pi * (double)(w * regfft::line_rev(N1, i)) / (double)W;
            twA[w * N1 + i] = mk<T>((T)std::cos(ang), (T)std::sin(ang));
        }
}
template void rows_twiddles<float>(int, cx<float> *);
template void rows_twiddles<double>(int, cx<double> *);

// ---- the one-launch solve ---------------------------------------------------------------------
template <> bool admm_persist_supported<float>(int H, int W, int K) {
    return H == W && (W == 128 || W == 256) && K >= 2 && K % 2 == 0 && K <= 64;
}
template <> bool admm_persist_supported<double>(int, int, int) { return false; }

static int persist_cus() { return current_device_cus(); }
template <> int admm_persist_grid<float>(int H, int W, int K, int CN) {
    (void)W;
    // one workgroup per CU at most, a multiple of 8 (the column pass gives workgroup b the row
    // frequencies = b mod 8), and no more than the larger pass has tiles
#ifdef SPORCO_AMD_HOSTSIM
    int g = 8;      // (the CPU test simulator runs the whole grid side by side: hostsim::set_coop)
#else
    int g = persist_cus() & ~7;
#endif
    const int64_t row_tiles = (int64_t)H * (((int64_t)CN * K + 127) / 128);
    const int64_t col_tiles = (int64_t)(W / 2 + 1) * CN;
    const int64_t most = std::max(row_tiles, (col_tiles + 7) / 8 * 8);
    if (g > most) g = (int)((most + 7) / 8 * 8);
    return g < 8 ? 8 : g;
}
template <> int admm_persist_grid<double>(int, int, int, int) { return 0; }

template <int NW, int LP> static size_t persist_prepare() {
    const size_t lds = std::max<size_t>(std::max(rows_lds_bytes(NW), fused_lds_bytes(NW, LP)),
                                        sizeof(double) * (7 * kFinalizeThreads + 16));
    static PerDeviceOnce attr_set;
    if (attr_set.first()) {
        SA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&admm_persist_kernel<NW, LP>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    }
    return lds;
}
template <int NW, int LP>
static void launch_persist_inst(hipStream_t st, const AdmmPersistArgs<float> &a, int grid) {
    const size_t lds = persist_prepare<NW, LP>();
#ifdef SPORCO_AMD_HOSTSIM
    hostsim::set_coop(grid);
#endif
    hipLaunchKernelGGL((admm_persist_kernel<NW, LP>), dim3((unsigned)grid), dim3(NW * 64), lds, st, a);
    SA_HIP(hipGetLastError());
}
// The grid barrier inside the one-launch solve needs every workgroup resident at once: what the
// device can hold of this kernel (registers, LDS) times its CUs must cover the grid -- asked of
// the runtime here, before the solve commits to the form, rather than found out by a barrier that
// times out.  (Work of OTHER streams or processes on the device can still starve it: the form is
// opt-in, for exclusive use of a device, and a timed-out barrier comes back as SPORCO_AMD_EHIP.)
template <> bool admm_persist_resident<float>(int H, int W, int K, int CN) {
#ifdef SPORCO_AMD_HOSTSIM
    (void)H; (void)W; (void)K; (void)CN;
    return true;
#else
    if (!admm_persist_supported<float>(H, W, K)) return false;
    const int grid = admm_persist_grid<float>(H, W, K, CN);
    int per_cu = 0;
    if (W == 128) {
        const size_t lds = persist_prepare<4, 4>();
        SA_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per_cu, reinterpret_cast<const void *>(&admm_persist_kernel<4, 4>), 4 * 64, lds));
    } else {
        const size_t lds = persist_prepare<8, 2>();
        SA_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per_cu, reinterpret_cast<const void *>(&admm_persist_kernel<8, 2>), 8 * 64, lds));
    }
    return (int64_t)per_cu * current_device_cus() >= grid;
#endif
}
template <> bool admm_persist_resident<double>(int, int, int, int) { return false; }

template <> void launch_admm_persist<float>(hipStream_t st, const AdmmPersistArgs<float> &a, int grid) {
    const RowsFwdArgs<float> &f = a.iter[0].fwd;
    SA_REQUIRE(admm_persist_supported<float>(f.H, f.W, f.K), "shape not handled by the one-launch solve");
    SA_REQUIRE(grid >= 8 && grid % 8 == 0 && grid <= std::max(8, persist_cus()), "grid of the one-launch solve");
    if (f.W == 128) launch_persist_inst<4, 4>(st, a, grid);
    else launch_persist_inst<8, 2>(st, a, grid);
}
template <> void launch_admm_persist<double>(hipStream_t, const AdmmPersistArgs<double> &, int) {
    throw Error(-1, "the one-launch solve is float32 only");
}

// ams_bits[(h * CN + cn) * NW + w], bit n1 = (mask(h, NW n1 + w, c, n) != 0)
__global__ void __launch_bounds__(256) ams_pack_kernel(Weight<float> m, uint32_t *bits, int H, int W,
                                                       int C, int N, int NW) {
    const int64_t total = (int64_t)H * C * N * NW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int w = (int)(i % NW);
        const int cn = (int)((i / NW) % (C * N));
        const int h = (int)(i / ((int64_t)NW * C * N));
        const int c = cn / N, n = cn % N;
        uint32_t b = 0u;
        for (int n1 = 0; n1 < W / NW; ++n1) {
            const int x = NW * n1 + w;
            const float v = m.ptr[h * m.stride[0] + x * m.stride[1] + c * m.stride[2] + n * m.stride[3]];
            if (v != 0.f) b |= 1u << n1;
        }
        bits[i] = b;
    }
}

template <> void launch_ams_pack<float>(hipStream_t st, const Weight<float> &mask, uint32_t *bits,
                                        int H, int W, int C, int N) {
    const int NW = rows_mr_width(W) ? 16 : W / kN1;     // (waves of the row kernels: one word per wave)
    const int64_t total = (int64_t)H * C * N * NW;
    hipLaunchKernelGGL(ams_pack_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(total, 256), 65535)),
                       dim3(256), 0, st, mask, bits, H, W, C, N, NW);
    SA_HIP(hipGetLastError());
}
template <> void launch_ams_pack<double>(hipStream_t, const Weight<double> &, uint32_t *, int, int,
                                         int, int) {
    throw Error(-1, "the fused row kernels are float32 only");
}

template <> void launch_rows_fwd<float>(hipStream_t st, const RowsFwdArgs<float> &a) {
    SA_REQUIRE(rows_supported<float>(a.W, a.K), "shape not handled by the fused row kernels");
    SA_REQUIRE(a.H <= 65535, "too many rows for one launch");
    SA_REQUIRE(!(a.v && a.y_bcast), "the broadcast row pass has no V form");
    regfft::with_line_shape(a.W, [&](auto nw, auto n1) { rows_fwd_launch<nw.value, n1.value>(st, a); });
    SA_HIP(hipGetLastError());
}
template <> void launch_rows_fwd<double>(hipStream_t, const RowsFwdArgs<double> &) {
    throw Error(-1, "the fused row kernels are float32 only");
}

template <> int64_t launch_rows_inv_post<float>(hipStream_t st, const RowsPostArgs<float> &a) {
    SA_REQUIRE(rows_supported<float>(a.W, a.K), "shape not handled by the fused row kernels");
    SA_REQUIRE(a.H <= 65535, "too many rows for one launch");
    const int64_t tiles =
        regfft::with_line_shape(a.W, [&](auto nw, auto n1) { return rows_inv_post_launch<nw.value, n1.value>(st, a); });
    SA_HIP(hipGetLastError());
    return tiles;
}
template <> int64_t launch_rows_inv_post<double>(hipStream_t, const RowsPostArgs<double> &) {
    throw Error(-1, "the fused row kernels are float32 only");
}

template <> int64_t launch_rows_inv_prox_fwd<float>(hipStream_t st, const RowsProxArgs<float> &a) {
    SA_REQUIRE(rows_supported<float>(a.W, a.K), "shape not handled by the fused row kernels");
    SA_REQUIRE(a.H <= 65535, "too many rows for one launch");
    const int64_t tiles =
        regfft::with_line_shape(a.W, [&](auto nw, auto n1) { return rows_inv_prox_fwd_launch<nw.value, n1.value>(st, a); });
    SA_HIP(hipGetLastError());
    return tiles;
}
template <> int64_t launch_rows_inv_prox_fwd<double>(hipStream_t, const RowsProxArgs<double> &) {
    throw Error(-1, "the fused row kernels are float32 only");
}

}  // namespace sporco_amd
