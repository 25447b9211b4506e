// csc_inhib.h -- the inhibition-weight update of ConvBPDNInhib (sporco/admm/cbpdnin.py:294-352) as
// one kernel: windowed circular convolution of |X| per coefficient map, mixing across the filter
// axis through the grouping matrix, temporal smoothing, the new thresholds and the three
// regulariser sums.
//
// The reference convolves with two FFT round trips over all maps.  Its window is the outer product
// of two short tap vectors, so the convolution is two tap sums on a tile held in LDS; no transform.
//
// Layout: the coefficient arrays are (H, W, C, N, K) with the filter index fastest, so a pixel of
// one image is a contiguous run of K values and neighbouring pixels lie C N K apart.  One workgroup
// owns a strip of TW columns of one image (c, n) with all K filters and walks down the rows of a
// row segment:
//   load   |X| of one row of the strip plus ntw - 1 halo columns (wrapped at the border)   global -> LDS
//   rows   tap sum along W into slot (row mod nth) of a ring of nth rows                   LDS -> LDS
//   cols   c = tap sum along H over the ring: one output row per step                      LDS -> registers / LDS
//   final  lat, self, smoothing, thresholds T, the three sums     global reads of the weights and G, writes
// Every row of X is read once per strip (the first nth - 1 rows of a segment twice); all K values of
// a pixel are in the workgroup, so the group mixing needs no second pass over X.
#pragma once

#include "csc_kernels.h"

namespace sporco_amd {

template <typename T> struct InhibArgs {
    const T *x = nullptr;    // X of this iteration
    const T *g = nullptr;    // the variable of the regulariser sums (Y, or X)
    T *wml = nullptr;        // lateral weights, updated in place (null: no lateral term)
    T *wms = nullptr;        // self weights, updated in place (null: no self term)
    T *t = nullptr;          // thresholds lmbda w0 + mu wml + gamma wms (the handle's L1-weight array)
    Weight<T> w0;            // L1Weight
    const T *taps_h = nullptr, *taps_w = nullptr;
    int nth = 1, ntw = 1;
    // Wg by group (entries of row g: filters row_k, values row_v) and by filter (entries of column
    // k: groups col_g, values col_v), zero entries left out; col_sum[k] = sum_g Wg[g, k].
    // Two contiguous device arrays: indices {row_ptr (Ng + 1), row_k (nnz), col_ptr (K + 1), col_g
    // (nnz)} and values {row_v (nnz), col_v (nnz), col_sum (K)} -- the kernel copies each in one go.
    const int *row_ptr = nullptr, *row_k = nullptr, *col_ptr = nullptr, *col_g = nullptr;
    const T *row_v = nullptr, *col_v = nullptr, *col_sum = nullptr;
    int Ng = 0, nnz = 0;
    T lmbda = T(0), mu = T(0), gamma = T(0), smooth = T(0);
    T h0 = T(0);             // the window's value at the origin, taps_h[nth / 2] * taps_w[ntw / 2]
    int H = 1, W = 1, C = 1, N = 1, K = 1;
    double *partials = nullptr;   // 4 doubles per workgroup: sum |w0 G|, sum |wml G|, sum |wms G|, unused
};

// Strip width, row segments and thread split of a launch (chosen from the LDS the ring needs).
struct InhibPlan {
    int TW = 1, rows = 1, nseg = 1;   // columns of a strip; rows per segment; segments
    int kt_log2 = 0;                  // 256 threads = KT (filters) x 256 / KT (columns), powers of two
    size_t lds = 0;
    int64_t blocks = 0;
};
template <typename T> InhibPlan inhib_plan(int H, int W, int CN, int K, int nth, int ntw, int Ng, int nnz);

// Returns the number of workgroups (rows of `partials` written).
template <typename T> int64_t launch_inhib_update(hipStream_t st, const InhibArgs<T> &a, const InhibPlan &pl);

// t[i] = lmbda * w0(i) over the whole array
template <typename T> void launch_inhib_init(hipStream_t st, T *t, Weight<T> w0, T lmbda, Dims5 d);

}  // namespace sporco_amd
