// csc_ball.h -- projection onto l2 balls, one ball per plane of an array whose planes are interleaved
// in memory: the block-0 step of ConvMinL1InL2Ball (sporco/admm/cbpdn.py:1830-2060),
//     minimise sum_m || x_m ||_1   such that   || sum_m d_m * x_m - s_k ||_2 <= epsilon   for every k,
// on the two-block constraint [D; I] x - [y0; y1] = [s; 0] of ConvBPDNMaskDcpl, and prox.proj_l2
// (sporco/prox/_lp.py:334-340) on a plain array.
//
// The array is viewed as (outer, C, inner); the norm is taken over C for each (outer, inner) pair, a
// "plane".  Block 0 is laid out (H, W, Cs, N): outer = 1, C = H W, inner = Cs N, so element i belongs to
// plane i % inner.  No element can be written before its plane's norm is known, hence two passes over
// the data with a launch boundary between them:
//     ball_norms    reads, writes one partial sum pair per (tile, plane)
//     ball_totals   sums the tiles' partials of each plane in a fixed order (a few kilobytes)
//     ball_y0step   reads again, scales, writes y0 and u0, forms the iteration's sums
// A tile is `cols` column groups (V consecutive planes each: one 16-byte access where inner is a multiple
// of V) by `RT` values of the C index; thread (row, col) of a tile's workgroup walks the C index in steps
// of `rows` and so never leaves its V planes.  A workgroup's sums over its rows go through a fixed-shape
// LDS tree, the tiles of a plane through one wave in a fixed order: no floating-point atomics, and two
// runs of the same problem agree bit for bit.  inner = 1 (a single plane per outer index) is folded: V
// consecutive values of C are loaded at once and their sums added in lane order.
#pragma once

#include "csc_kernels.h"

namespace sporco_amd {

// How (outer, C, inner) is cut into tiles (ball_geom); the same geometry serves both passes.
struct BallGeom {
    int V = 1;          // elements per access: 16 / sizeof(T), 8 / sizeof(T) or 1
    int fold = 0;       // inner == 1: the V elements of an access are V values of C of ONE plane
    int64_t outer = 1;
    int64_t Cv = 1;     // values of the C index a thread steps over (C, or C / V when folded)
    int64_t G = 1;      // column groups per value of C (inner / V; 1 when folded)
    int64_t planes = 1; // planes per outer index (inner)
    int cols = 1;       // column groups per tile (<= 256)
    int rows = 1;       // values of C a workgroup covers per step (256 / cols)
    int CB = 1;         // tiles across the column groups
    int RB = 1;         // tiles along C: the partial sums per plane
    int64_t RT = 1;     // values of C per tile (a multiple of rows)
    __host__ __device__ int64_t ntiles() const { return outer * CB * RB; }
    __host__ __device__ int64_t nplanes() const { return outer * planes; }
    // doubles of workspace: the partials (ntiles x planes-per-tile pairs), then the totals (a pair a plane)
    __host__ __device__ int64_t partial_doubles() const { return outer * RB * planes * 2; }
    __host__ __device__ int64_t workspace_doubles() const { return partial_doubles() + nplanes() * 2; }
};
BallGeom ball_geom(size_t elem_size, int64_t outer, int64_t C, int64_t inner);

// The step on block 0 given ax0nr = D x (left in the spatial domain by the x step's inverse transform):
//     ax = rlx ax0nr + (1 - rlx)(y0 + s)           (plainly ax0nr when rlx == 1, as md_y0step)
//     v  = ax + us u0 - s
//     y0 = sigma_p v,   sigma_p = 1 if d_p <= eps else eps / d_p,   d_p = || v ||_2 over plane p
//     u0 = us u0 + ax - (y0 + s)
// (d_p = 0 gives sigma_p = 1 and y0 = 0: the reference's zdivide.)  With u0 == s == nullptr ("plain"):
// y0 = sigma_p ax0nr, nothing else read or written -- prox.proj_l2.
template <typename T> struct BallArgs {
    const T *ax0nr = nullptr;
    T *y0 = nullptr;
    T *u0 = nullptr;
    const T *s = nullptr;
    double eps = 0.0;
    T rlx = T(1), us = T(1);
    int geval_y = 0;
    double *ws = nullptr;       // BallGeom::workspace_doubles() doubles
};

// Pass 1 (+ the per-plane totals): per plane, in double, sum v^2 and sum (ax0nr - s)^2 -- the second is
// what the constraint measure needs when it is evaluated at D x - s (AuxVarObj off).
template <typename T> void launch_ball_norms(hipStream_t st, const BallArgs<T> &a, const BallGeom &g);
void launch_ball_totals(hipStream_t st, double *ws, const BallGeom &g);
// Pass 2.  partials (5 a workgroup, md_y0step's slots and order): |ax0nr - y0 - s|^2, |ax0nr|^2, |y0|^2,
// |u0|^2 (all new values) and the constraint measure sum_p max(g_p - eps, 0)^2 with g_p the plane norm
// of ax0nr - s, or of the new y0 with geval_y: the square of the reference's || proj_l2(g0) - g0 ||
// (cbpdn.py:2034-2040).  ball_iter finalizes that fifth sum into SPORCO_AMD_OUT_DFID, which the class
// has no other use for (its objective has no data fidelity term).  Returns the number of workgroups
// (<= kMaxPartialBlocks).
template <typename T> int launch_ball_y0step(hipStream_t st, const BallArgs<T> &a, const BallGeom &g, double *partials);

}  // namespace sporco_amd
