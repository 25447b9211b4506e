// csc_cmod_cols.h -- the column statistics of the constraint-set projection of the dense dictionary updates, shared by
// csc_cmod.hip and csc_pgm_cmod.hip (device code).  A workgroup of kThreads = 256 threads holds a tile of 16 dictionary
// columns, [N][16]; thread t owns column t & 15 of rows t >> 4, + 16, ...
#pragma once

#include "csc_kernels_dev.h"

namespace sporco_amd {

// the sum of `v` over the 16 threads of a column (threads t with the same t & 15), in the order of t >> 4
__device__ __forceinline__ double cm_col_sum(double v, double *cs) {
    cs[threadIdx.x] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += cs[q * 16 + ((int)threadIdx.x & 15)];
    __syncthreads();
    return s;
}

// mean (zero_mean) and norm of the thread's column of the tile `t` ([N][16]), as Pcn wants them
// (cmod.py:286-342): mean = sum / N, norm = sqrt(sum (v - mean)^2) with 0 replaced by 1
template <typename T>
__device__ __forceinline__ void cm_col_stats(const T *t, int N, int zero_mean, double *cs, T &mean, T &nrm) {
    const int c = (int)threadIdx.x & 15;
    mean = T(0);
    if (zero_mean) {
        double s = 0.0;
        for (int n = (int)threadIdx.x >> 4; n < N; n += 16) s += (double)t[n * 16 + c];
        mean = (T)(cm_col_sum(s, cs) / (double)N);
    }
    double ss = 0.0;
    for (int n = (int)threadIdx.x >> 4; n < N; n += 16) {
        const double d = (double)(t[n * 16 + c] - mean);
        ss += d * d;
    }
    nrm = (T)sqrt(cm_col_sum(ss, cs));
    if (nrm == T(0)) nrm = T(1);
}

}  // namespace sporco_amd
