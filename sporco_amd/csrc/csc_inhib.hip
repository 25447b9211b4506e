// csc_inhib.hip -- inhibition-weight update of ConvBPDNInhib (csc_inhib.h): one launch per
// iteration, float32 / float64, any H, W, C, N, K, window lengths up to the image extents.
#include "csc_inhib.h"

#include <algorithm>

namespace sporco_amd {

namespace {

constexpr int kInhibThreads = 256;
constexpr size_t kInhibLdsSoft = 64 * 1024;    // two workgroups per compute unit
constexpr size_t kInhibLdsHard = 160 * 1024;   // the LDS of a gfx950 compute unit
constexpr int kInhibScratch = 16;              // doubles of LDS for the block reduction (3 x 4 waves)

template <typename T> struct InhibKArgs {
    InhibArgs<T> a;
    int TW, rows, kt_log2;
};

template <typename T> __device__ __forceinline__ T absv(T v) { return v < T(0) ? -v : v; }

// One workgroup: a strip of TW columns of one image (c, n), all K filters, the rows of one segment.
// It walks down the rows; `R` keeps the last nth rows of the tap sums along W, so every row of X is
// read once per strip (plus the ntw - 1 halo columns) and c comes out one row per step.
template <typename T> __global__ void __launch_bounds__(kInhibThreads) inhib_update_kernel(const InhibKArgs<T> ka) {
    const InhibArgs<T> &a = ka.a;
    const int TW = ka.TW, K = a.K, WW = TW + a.ntw - 1, nth = a.nth, ntw = a.ntw;
    // origin of the taps: tap t acts at offset t - n / 2; the halo before a strip is n - 1 - n / 2
    const int bh = nth - 1 - nth / 2, bw = ntw - 1 - ntw / 2;
    double *scratch = dyn_lds<double>();
    T *A = reinterpret_cast<T *>(scratch + kInhibScratch);   // (WW, K)       |X| of one row, with halo
    T *R = A + (size_t)WW * K;                               // (nth, TW, K)  ring: tap sums along W
    T *Cb = R + (size_t)nth * TW * K;                        // (TW, K)       c = h (*) |X| of the output row
    // the taps and the grouping tables, read in the inner loops: copies in LDS (a dependent chain
    // of loads from global memory per element otherwise)
    T *taps_h = Cb + (size_t)TW * K, *taps_w = taps_h + nth;
    T *row_v = taps_w + ntw, *col_v = row_v + a.nnz, *col_sum = col_v + a.nnz;
    int *row_ptr = reinterpret_cast<int *>(col_sum + (a.nnz ? K : 0)), *row_k = row_ptr + a.Ng + 1;
    int *col_ptr = row_k + a.nnz, *col_g = col_ptr + K + 1;

    const int tid = threadIdx.x;
    const int KT = 1 << ka.kt_log2, TX = kInhibThreads >> ka.kt_log2;
    const int tk = tid & (KT - 1), tx = tid >> ka.kt_log2;
    // (the image index runs fastest over the grid: workgroups in flight together then read the
    // C N K contiguous values of the same pixels, one DRAM page instead of C N scattered ones)
    const int x0 = blockIdx.z * TW, ys = blockIdx.y * ka.rows;
    const int ye = ys + ka.rows < a.H ? ys + ka.rows : a.H;
    const int cn = blockIdx.x, ci = cn / a.N, ni = cn - ci * a.N;
    const int CN = a.C * a.N;
    const bool lateral = a.wml != nullptr;
    const T s = a.smooth, s1 = T(1) - a.smooth;

    for (int i = tid; i < nth; i += kInhibThreads) taps_h[i] = a.taps_h[i];
    for (int i = tid; i < ntw; i += kInhibThreads) taps_w[i] = a.taps_w[i];
    if (lateral) {
        // (InhibArgs: the value tables and the index tables are each one contiguous array)
        for (int i = tid; i < 2 * a.nnz + K; i += kInhibThreads) row_v[i] = a.row_v[i];
        for (int i = tid; i < a.Ng + 1 + 2 * a.nnz + K + 1; i += kInhibThreads) row_ptr[i] = a.row_ptr[i];
    }
    double acc[3] = {0.0, 0.0, 0.0};
    const int nload = (ye - ys) + nth - 1;
    int slot = 0;
    for (int i = 0; i < nload; ++i) {
        int yin = ys - bh + i;
        yin = yin < 0 ? yin + a.H : yin;
        while (yin >= a.H) yin -= a.H;
        for (int px = tx; px < WW; px += TX) {
            int gx = x0 - bw + px;
            gx = gx < 0 ? gx + a.W : gx;
            while (gx >= a.W) gx -= a.W;
            const T *src = a.x + (((int64_t)yin * a.W + gx) * CN + cn) * K;
            T *dst = A + (size_t)px * K;
            for (int k = tk; k < K; k += KT) dst[k] = absv(src[k]);
        }
        __syncthreads();
        for (int j = tx; j < TW; j += TX)
            for (int k = tk; k < K; k += KT) {
                const T *row = A + (size_t)(j + ntw - 1) * K + k;
                T v = T(0);
                for (int t = 0; t < ntw; ++t) v = fma1(taps_w[t], row[-(int64_t)t * K], v);
                R[((size_t)slot * TW + j) * K + k] = v;
            }
        __syncthreads();
        if (i >= nth - 1) {
            // input row i is output row gy + nth / 2: tap t of the sum along H meets ring slot (slot - t)
            const int gy = ys + i - (nth - 1);
            auto colsum = [&](int j, int k) {
                T v = T(0);
                int sl = slot;
                for (int t = 0; t < nth; ++t) {
                    v = fma1(taps_h[t], R[((size_t)sl * TW + j) * K + k], v);
                    sl = sl == 0 ? nth - 1 : sl - 1;
                }
                return v;
            };
            if (lateral) {
                for (int j = tx; j < TW; j += TX)
                    for (int k = tk; k < K; k += KT) Cb[(size_t)j * K + k] = colsum(j, k);
                __syncthreads();
            }
            for (int j = tx; j < TW; j += TX) {
                const int gx = x0 + j;
                if (gx >= a.W) break;
                const int64_t base = (((int64_t)gy * a.W + gx) * CN + cn) * K;
                const int64_t wbase = gy * a.w0.stride[0] + gx * a.w0.stride[1] + ci * a.w0.stride[2] +
                                      ni * a.w0.stride[3];
                const T *cj = Cb + (size_t)j * K;
                for (int k = tk; k < K; k += KT) {
                    const int64_t off = base + k;
                    const T c = lateral ? cj[k] : colsum(j, k);
                    const T gv = absv(a.g[off]);
                    const T w0 = a.w0.ptr ? a.w0.ptr[wbase + k * a.w0.stride[4]] : T(1);
                    T thr = a.lmbda * w0;
                    acc[0] += (double)(absv(w0) * gv);
                    if (lateral) {
                        // sum_g Wg[g, k] (sum_n Wg[g, n] c_n) - (sum_g Wg[g, k]) c_k, zero entries skipped
                        T lat = -(col_sum[k] * c);
                        for (int e = col_ptr[k]; e < col_ptr[k + 1]; ++e) {
                            const int g = col_g[e];
                            T pg = T(0);
                            for (int f = row_ptr[g]; f < row_ptr[g + 1]; ++f) pg = fma1(row_v[f], cj[row_k[f]], pg);
                            lat = fma1(col_v[e], pg, lat);
                        }
                        const T wl = fma1(s, a.wml[off], s1 * lat);
                        a.wml[off] = wl;
                        thr = fma1(a.mu, wl, thr);
                        acc[1] += (double)(absv(wl) * gv);
                    }
                    if (a.wms) {
                        const T sf = fma1(-a.h0, absv(a.x[off]), c);
                        const T ws = fma1(s, a.wms[off], s1 * sf);
                        a.wms[off] = ws;
                        thr = fma1(a.gamma, ws, thr);
                        acc[2] += (double)(absv(ws) * gv);
                    }
                    a.t[off] = thr;
                }
            }
        }
        slot = slot + 1 == nth ? 0 : slot + 1;
    }
    __syncthreads();
    const int64_t blk = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    block_sum_store<3>(acc, scratch, a.partials + blk * 4);
}

template <typename T> struct InhibInitArgs {
    T *t;
    Weight<T> w0;
    T lmbda;
    Dims5 d;
};

template <typename T> __global__ void __launch_bounds__(kInhibThreads) inhib_init_kernel(const InhibInitArgs<T> a) {
    const int64_t P = (int64_t)a.d.C * a.d.N * a.d.K, E = (int64_t)a.d.H * a.d.W * P;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < E; i += (int64_t)gridDim.x * blockDim.x) {
        T w = T(1);
        if (a.w0.ptr) {
            const int k = (int)(i % a.d.K);
            int64_t r = i / a.d.K;
            const int n = (int)(r % a.d.N);
            r /= a.d.N;
            const int c = (int)(r % a.d.C);
            r /= a.d.C;
            const int x = (int)(r % a.d.W), y = (int)(r / a.d.W);
            w = a.w0.ptr[y * a.w0.stride[0] + x * a.w0.stride[1] + c * a.w0.stride[2] + n * a.w0.stride[3] +
                         k * a.w0.stride[4]];
        }
        a.t[i] = a.lmbda * w;
    }
}

int log2_floor(int v) {
    int l = 0;
    while ((2 << l) <= v) ++l;
    return l;
}

}  // namespace

template <typename T> InhibPlan inhib_plan(int H, int W, int CN, int K, int nth, int ntw, int Ng, int nnz) {
    SA_REQUIRE(nth >= 1 && ntw >= 1 && nth <= H && ntw <= W, "inhibition window: 1 <= taps <= image extent on each axis");
    // (the taps; with a grouping matrix its tables: 2 nnz + K values, Ng + 1 + 2 nnz + K + 1 indices)
    const size_t tables = sizeof(T) * ((size_t)nth + ntw) +
                          (nnz ? sizeof(T) * (2 * (size_t)nnz + K) + sizeof(int) * ((size_t)Ng + 2 * (size_t)nnz + K + 2) : 0);
    auto bytes = [&](int tw) {
        return sizeof(double) * kInhibScratch + tables +
               sizeof(T) * (size_t)K * ((size_t)(tw + ntw - 1) + (size_t)nth * tw + tw);
    };
    // the widest strip whose rows keep the 256 threads busy (<= 8 elements each) and whose ring fits
    // the LDS share of two workgroups per compute unit; a long window or many filters: a narrower
    // strip, then the whole LDS
    InhibPlan pl;
    bool found = false;
    const size_t budgets[2] = {kInhibLdsSoft, kInhibLdsHard};
    for (int b = 0; b < 2 && !found; ++b)
        for (int tw = 64; tw >= 1 && !found; tw >>= 1) {
            if (tw > 1 && ((int64_t)tw * K > 2048 || tw / 2 >= W)) continue;
            if (bytes(tw) > budgets[b]) continue;
            pl.TW = tw;
            found = true;
        }
    SA_REQUIRE(found, "inhibition window times filter count too large for the LDS of a compute unit");
    pl.kt_log2 = std::min(6, log2_floor(K));
    pl.lds = bytes(pl.TW);
    // row segments: enough workgroups to fill the device, each paying nth - 1 warm-up rows
    const int64_t strips = ceil_div(W, pl.TW) * CN;
    int64_t nseg = std::min<int64_t>(ceil_div(2048, strips), std::max<int64_t>(1, H / (4 * (int64_t)nth)));
    nseg = std::max<int64_t>(1, std::min<int64_t>(nseg, H));
    pl.rows = (int)ceil_div(H, nseg);
    pl.nseg = (int)ceil_div(H, pl.rows);
    pl.blocks = strips * pl.nseg;
    return pl;
}

template <typename T> int64_t launch_inhib_update(hipStream_t st, const InhibArgs<T> &a, const InhibPlan &pl) {
    InhibKArgs<T> ka;
    ka.a = a;
    ka.TW = pl.TW;
    ka.rows = pl.rows;
    ka.kt_log2 = pl.kt_log2;
    const int64_t gz = (int64_t)a.C * a.N;
    SA_REQUIRE(pl.nseg <= 65535 && ceil_div(a.W, pl.TW) <= 65535, "inhibition update: grid too large");
    SA_REQUIRE(pl.lds <= kInhibLdsHard, "inhibition update: strip does not fit the LDS");
    static PerDeviceOnce attr_set;
    if (attr_set.first())
        SA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&inhib_update_kernel<T>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)kInhibLdsHard));
    const dim3 grid((unsigned)gz, (unsigned)pl.nseg, (unsigned)ceil_div(a.W, pl.TW));
    hipLaunchKernelGGL(inhib_update_kernel<T>, grid, dim3(kInhibThreads), pl.lds, st, ka);
    SA_HIP(hipGetLastError());
    return pl.blocks;
}

template <typename T> void launch_inhib_init(hipStream_t st, T *t, Weight<T> w0, T lmbda, Dims5 d) {
    InhibInitArgs<T> ia{t, w0, lmbda, d};
    const int64_t E = (int64_t)d.H * d.W * d.C * d.N * d.K;
    const int grid = (int)std::min<int64_t>(std::max<int64_t>(ceil_div(E, kInhibThreads), 1), 4096);
    hipLaunchKernelGGL(inhib_init_kernel<T>, dim3(grid), dim3(kInhibThreads), 0, st, ia);
    SA_HIP(hipGetLastError());
}

#define SA_INHIB_INST(T)                                                                              \
    template InhibPlan inhib_plan<T>(int, int, int, int, int, int, int, int);                            \
    template int64_t launch_inhib_update<T>(hipStream_t, const InhibArgs<T> &, const InhibPlan &);    \
    template void launch_inhib_init<T>(hipStream_t, T *, Weight<T>, T, Dims5);
SA_INHIB_INST(float)
SA_INHIB_INST(double)

}  // namespace sporco_amd
