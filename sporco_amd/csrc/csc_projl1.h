// csc_projl1.h -- Euclidean projection onto l1 balls, one ball per set of an array whose sets are
// interleaved in memory: the y step of ConvBPDNProjL1 (sporco/admm/cbpdn.py:1220-1395),
//     minimise (1/2) || sum_m d_m * x_m - s ||^2   such that   sum_m || x_m ||_1 <= gamma   per image,
// and prox.proj_l1 (sporco/prox/_l1proj.py) on a plain array.
//
// The array is viewed as (outer, P, inner): element i belongs to set (i / inner) % P, and the norm of a
// set runs over its outer and inner indices.  The coefficient array (H, W, C, N, M) has outer = H W C,
// P = N, inner = M: one ball per image.  (csc_ball.h is the other geometry: the norm over the middle.)
//
// For a set v with || v ||_1 > gamma the projection is sign(v) max(|v| - tau, 0), tau the root of
//     f(t) = s(t) - t c(t) - gamma,   c(t) = #{ |v_i| > t },   s(t) = sum_{|v_i| > t} |v_i|,
// a convex, decreasing, piecewise linear function.  No sort: a SEARCH PASS streams the array once and
// forms c and s at kCand candidate thresholds per set (and the maximum); projl1_decide then keeps, per
// set, the largest candidate L with f >= 0 and the smallest R with f < 0 (the maximum serves as the first
// R), and places the next candidates between the Newton step from L or R -- a tangent of a convex
// function, so (s - gamma) / c lies at or below tau from either side -- and the secant of L and R, which
// lies at or above it.  The search ends on INTEGERS: when c(L) = c(R) no magnitude lies in (t_L, t_R], f
// is linear there, and tau = (s(L) - gamma) / c(L) exactly; likewise when the count at a Newton step
// equals the count at the point it was taken from.  The counts travel as doubles (exact below 2^53).
// Sums are formed in double, a workgroup's through a fixed tree and the tiles of a set in a fixed order:
// no floating-point atomics, and two runs agree bit for bit.  A set inside its ball (s(0) <= gamma) has
// tau = 0 and is passed through unchanged; gamma = 0 gives tau = the maximum, hence zeros.
//
// The launch sequence of a search is fixed (projl1_search: init, then `passes` x (pass, decide), then the
// count of sets still searching); a set that has converged makes its workgroups return at once.  The
// apply kernel does nothing while a set is still searching: the caller reads the count with the
// iteration's sums and enqueues further passes.
#pragma once

#include "csc_kernels.h"

namespace sporco_amd {

constexpr int kProjL1Cand = 8;                     // candidate thresholds per set and pass
constexpr int kProjL1Part = 2 * kProjL1Cand + 1;   // per tile: s and c per candidate, the maximum
// per-set state (doubles)
enum ProjL1State {
    PL_STATUS = 0,      // 0 searching, 1 outside its ball (tau > 0 found), 2 inside (tau = 0)
    PL_TAU,
    PL_TL, PL_CL, PL_SL,        // the lower bracket point: f >= 0
    PL_TR, PL_CR, PL_SR,        // the upper bracket point: f < 0
    PL_Q0,              // the count at the point candidate 0 is the Newton step of; -1: none
    PL_PASSES,          // search passes this set took in the current search
    PL_HINT,            // tau of the previous search of this set (0: none): where the first pass looks
    PL_STATE_COUNT = 12
};

struct ProjL1Geom {
    int V = 1;              // elements per access: 16 / sizeof(T), 8 / sizeof(T) or 1
    int64_t outer = 1, P = 1, inner = 1;
    int64_t G = 1;          // accesses per (outer index, set): inner / V
    int64_t Q = 1;          // accesses per set: outer * G
    int64_t QT = 1;         // accesses per tile (a multiple of the workgroup size)
    int RB = 1;             // tiles per set
    __host__ __device__ int64_t ntiles() const { return P * RB; }
    // doubles of workspace: the state and candidates of every set, the tiles' partials, the counter
    __host__ __device__ int64_t state_doubles() const { return P * (PL_STATE_COUNT + kProjL1Cand); }
    __host__ __device__ int64_t workspace_doubles() const { return state_doubles() + ntiles() * kProjL1Part + 2; }
};
// (P = 1: the whole array is one set, and (outer, inner) is re-cut so that accesses are 16 bytes wherever
// the element count allows)
// (keep: the caller's kernels read the outer index -- NoBndryCross -- so the cut stays as given)
ProjL1Geom projl1_geom(size_t elem_size, int64_t outer, int64_t P, int64_t inner, bool keep = false);

// v = ax + us u with ax = rlx x + (1 - rlx) y (plainly x when rlx == 1); u == nullptr ("plain"): v = x.
template <typename T> struct ProjL1Args {
    const T *x = nullptr;
    T *y = nullptr;         // search: read when rlx != 1; apply: read and written
    T *u = nullptr;
    T *out = nullptr;       // plain apply: the projection of x
    double gamma = 0.0;
    T rlx = T(1), us = T(1);
    uint32_t flags = 0;     // F_NONNEG | F_NOBNDRY (apply)
    Dims5 d{1, 1, 1, 1, 1};
    int dH = 1, dW = 1;
    double *ws = nullptr;   // ProjL1Geom::workspace_doubles() doubles; the state part persists between calls
};

// Forget the thresholds of earlier searches (a new workspace, or a new problem in it).
void projl1_reset(hipStream_t st, double *ws, const ProjL1Geom &g);
// init + `passes` x (pass, decide) + count.  restart = false: continue a search (no init).
template <typename T>
void launch_projl1_search(hipStream_t st, const ProjL1Args<T> &a, const ProjL1Geom &g, int passes, bool restart);
// The y step and the dual step in one pass (modelled on ball_y0step): y = shrink(v, tau_n), then
// NonNegCoef / NoBndryCross as GenericConvBPDN.ystep applies them, u = v - y; partials (8 a workgroup, the
// slots and order of the staged statistics): |x - y|^2, |y - y_prev|^2, |x|^2, |y|^2, |u|^2.  Plain:
// out = shrink(x, tau_n).  Does nothing while a set is still searching.  Returns the number of workgroups.
template <typename T> int launch_projl1_apply(hipStream_t st, const ProjL1Args<T> &a, const ProjL1Geom &g, double *partials);
// sum_n sum_i min(|x_i|, tau_n)^2 over the sets outside their balls, after a search on x alone: the
// square of || proj(x) - x ||.  One partial a workgroup.
template <typename T> int launch_projl1_cnstr(hipStream_t st, const ProjL1Args<T> &a, const ProjL1Geom &g, double *partials);
// ws + state_doubles() + ntiles * kProjL1Part: [0] sets still searching, [1] the most passes a set took
__host__ __device__ inline double *projl1_counter(double *ws, const ProjL1Geom &g) { return ws + g.state_doubles() + g.ntiles() * kProjL1Part; }

}  // namespace sporco_amd
