// csc_projl1.hip -- the kernels of csc_projl1.h: projl1_init, projl1_pass, projl1_decide, projl1_count,
// projl1_apply, projl1_cnstr.  float32 / float64, any (outer, P, inner).
#include "csc_projl1.h"
#include "csc_kernels_dev.h"

#include <algorithm>
#include <cmath>

namespace sporco_amd {

ProjL1Geom projl1_geom(size_t elem_size, int64_t outer, int64_t P, int64_t inner, bool keep) {
    ProjL1Geom g;
    if (P == 1 && !keep) {       // one set: any cut of the flat array serves
        const int64_t n = outer * inner;
        inner = 1;
        while (inner < 1024 && n % (inner * 2) == 0) inner *= 2;
        outer = n / inner;
    }
    g.outer = outer;
    g.P = P;
    g.inner = inner;
    const int vmax = (int)(16 / elem_size);
    g.V = 1;
    for (int v = vmax; v > 1; v /= 2)
        if (inner % v == 0) {
            g.V = v;
            break;
        }
    g.G = inner / g.V;
    g.Q = outer * g.G;
    // about sixteen accesses a thread, at most about two thousand tiles in all
    const int64_t cap = std::max<int64_t>(1, 2048 / P);
    const int64_t rb = std::min<int64_t>(std::max<int64_t>(1, ceil_div(g.Q, (int64_t)kThreads * 16)), cap);
    g.QT = ceil_div(ceil_div(g.Q, rb), kThreads) * kThreads;
    g.RB = (int)ceil_div(g.Q, g.QT);
    return g;
}

namespace {

enum ProjL1Mode { PL_PLAIN = 0, PL_ADMM = 1, PL_ADMM_RLX = 2 };

__device__ __forceinline__ double *pl_state(double *ws, int64_t set) { return ws + set * (PL_STATE_COUNT + kProjL1Cand); }
__device__ __forceinline__ double *pl_cand(double *ws, int64_t set) { return pl_state(ws, set) + PL_STATE_COUNT; }
__device__ __forceinline__ double *pl_part(double *ws, const ProjL1Geom &g, int64_t tile) {
    return ws + g.state_doubles() + tile * kProjL1Part;
}

// ax and v of one element: the same instructions in the search and in the apply pass
template <typename T, int MODE> __device__ __forceinline__ void pl_elem(T x, T yo, T uo, T rlx, T &ax, T &v) {
    if (MODE == PL_PLAIN) {
        ax = x;
        v = x;
    } else {
        ax = MODE == PL_ADMM_RLX ? fma1(rlx, x, (T(1) - rlx) * yo) : x;
        v = ax + uo;
    }
}

template <typename T, int V> __device__ __forceinline__ Vec<T, V> pl_load(const T *p, int64_t e) {
    return *reinterpret_cast<const Vec<T, V> *>(p + e);
}

// The accesses q = q0, q0 + kThreads, ... < q1 of set `set` that a thread walks: (o, gi) with q = o G + gi,
// stepped without a division.
struct PlWalk {
    int64_t q, q1, o, gi, so, sg;
    __device__ __forceinline__ PlWalk(const ProjL1Geom &g, int rb) {
        q = (int64_t)rb * g.QT + (int)threadIdx.x;
        q1 = std::min<int64_t>((int64_t)(rb + 1) * g.QT, g.Q);
        o = q / g.G;
        gi = q - o * g.G;
        so = kThreads / g.G;
        sg = kThreads - so * g.G;
    }
    __device__ __forceinline__ bool more() const { return q < q1; }
    __device__ __forceinline__ int64_t elem(const ProjL1Geom &g, int64_t set) const {
        return ((o * g.P + set) * g.G + gi) * g.V;
    }
    __device__ __forceinline__ void next(const ProjL1Geom &g) {
        q += kThreads;
        o += so;
        gi += sg;
        if (gi >= g.G) {
            gi -= g.G;
            ++o;
        }
    }
};

// first candidates of a search: 0 (the l1 norm and the count of non-zeros), and points about the
// threshold the previous search of this set found
__global__ void __launch_bounds__(kThreads) projl1_init_kernel(double *ws, const ProjL1Geom g) {
    const int64_t set = (int64_t)blockIdx.x * kThreads + (int)threadIdx.x;
    if (set >= g.P) return;
    double *s = pl_state(ws, set), *c = pl_cand(ws, set);
    const double hint = s[PL_HINT];
    s[PL_STATUS] = 0.0;
    s[PL_TAU] = 0.0;
    s[PL_TL] = -1.0;        // (no lower point yet)
    s[PL_CL] = s[PL_SL] = 0.0;
    s[PL_TR] = -1.0;        // (no upper point yet: the maximum, once known)
    s[PL_CR] = s[PL_SR] = 0.0;
    s[PL_Q0] = -1.0;
    s[PL_PASSES] = 0.0;
    const double mult[kProjL1Cand - 1] = {0.9, 0.97, 0.99, 1.0, 1.01, 1.03, 1.1};
    c[0] = 0.0;
    for (int j = 1; j < kProjL1Cand; ++j) c[j] = hint > 0.0 ? hint * mult[j - 1] : HUGE_VAL;
}

__global__ void __launch_bounds__(kThreads) projl1_reset_kernel(double *ws, const ProjL1Geom g) {
    const int64_t set = (int64_t)blockIdx.x * kThreads + (int)threadIdx.x;
    if (set < g.P) pl_state(ws, set)[PL_HINT] = 0.0;
}

template <typename T, int V, int MODE>
__global__ void __launch_bounds__(kThreads) projl1_pass_kernel(const ProjL1Args<T> a, const ProjL1Geom g) {
    constexpr int J = kProjL1Cand;
    const int64_t tile = blockIdx.x;
    const int64_t set = tile / g.RB;
    const int rb = (int)(tile - set * g.RB);
    if (pl_state(a.ws, set)[PL_STATUS] != 0.0) return;     // (the same for the whole workgroup)
    double t[J], acc[2 * J];
    const double *cand = pl_cand(a.ws, set);
#pragma unroll
    for (int j = 0; j < J; ++j) {
        t[j] = cand[j];
        acc[j] = acc[J + j] = 0.0;
    }
    double mx = 0.0;
    for (PlWalk w(g, rb); w.more(); w.next(g)) {
        const int64_t e = w.elem(g, set);
        const Vec<T, V> xx = pl_load<T, V>(a.x, e);
        Vec<T, V> xy = xx, xu = xx;
        if (MODE != PL_PLAIN) xu = pl_load<T, V>(a.u, e);
        if (MODE == PL_ADMM_RLX) xy = pl_load<T, V>(a.y, e);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            T ax, v;
            pl_elem<T, MODE>(xx.v[i], xy.v[i], a.us * xu.v[i], a.rlx, ax, v);
            const double m = (double)(v < T(0) ? -v : v);
            mx = m > mx ? m : mx;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const bool in = m > t[j];
                acc[j] += in ? m : 0.0;
                acc[J + j] += in ? 1.0 : 0.0;
            }
        }
    }
    double *sh = dyn_lds<double>();         // 2 J sums a wave, then the maxima
    double *dst = pl_part(a.ws, g, tile);
    block_sum_store<2 * J>(acc, sh, dst);
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) {
        const double o = __shfl_xor(mx, m, kWave);
        mx = o > mx ? o : mx;
    }
    const int nwave = kThreads / kWave;
    double *shm = sh + 2 * J * nwave;
    if (((int)threadIdx.x & (kWave - 1)) == 0) shm[(int)threadIdx.x / kWave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m2 = shm[0];
        for (int wv = 1; wv < nwave; ++wv) m2 = shm[wv] > m2 ? shm[wv] : m2;
        dst[2 * J] = m2;
    }
}

// One wave a set: lane l adds the partials of tiles l, l + 64, ..., then the xor tree; lane 0 moves the
// bracket and places the next candidates (csc_projl1.h).
__global__ void __launch_bounds__(kThreads) projl1_decide_kernel(double *ws, const ProjL1Geom g, double gamma) {
    constexpr int J = kProjL1Cand;
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int64_t set = (int64_t)blockIdx.x * (kThreads / kWave) + (int)threadIdx.x / kWave;
    const bool valid = set < g.P;
    double *st = pl_state(ws, valid ? set : 0), *cand = pl_cand(ws, valid ? set : 0);
    bool live = false;
    if (valid) live = st[PL_STATUS] == 0.0;     // (a wave past the last set reads nothing)
    double tot[2 * J], mx = 0.0;
#pragma unroll
    for (int j = 0; j < 2 * J; ++j) tot[j] = 0.0;
    if (live) {
        for (int rb = lane; rb < g.RB; rb += kWave) {
            const double *src = pl_part(ws, g, set * g.RB + rb);
#pragma unroll
            for (int j = 0; j < 2 * J; ++j) tot[j] += src[j];
            mx = src[2 * J] > mx ? src[2 * J] : mx;
        }
    }
#pragma unroll
    for (int j = 0; j < 2 * J; ++j) tot[j] = wave_sum(tot[j]);
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) {
        const double o = __shfl_xor(mx, m, kWave);
        mx = o > mx ? o : mx;
    }
    if (!live || lane != 0) return;
    const double passes = st[PL_PASSES] + 1.0;
    st[PL_PASSES] = passes;
    if (passes == 1.0) {
        // candidate 0 is t = 0: tot[0] is the l1 norm
        if (tot[0] <= gamma) {
            st[PL_STATUS] = 2.0;
            st[PL_TAU] = 0.0;
            st[PL_HINT] = 0.0;
            return;
        }
        if (gamma <= 0.0) {
            st[PL_STATUS] = 1.0;
            st[PL_TAU] = mx;
            st[PL_HINT] = 0.0;
            return;
        }
        st[PL_TR] = mx;         // f(max) = -gamma < 0 with c = 0, s = 0
        st[PL_CR] = st[PL_SR] = 0.0;
    }
    double tL = st[PL_TL], cL = st[PL_CL], sL = st[PL_SL], tR = st[PL_TR], cR = st[PL_CR], sR = st[PL_SR];
    const double q0 = st[PL_Q0];
    double tau = -1.0;
    // the count at a Newton step equals the count where it was taken: the step is the root
    if (q0 >= 0.0 && (int64_t)tot[J] == (int64_t)q0) tau = cand[0];
    for (int j = 0; j < J; ++j) {
        const double tj = cand[j];
        if (!(tj < HUGE_VAL)) continue;
        const double f = tot[j] - tj * tot[J + j] - gamma;
        if (f >= 0.0) {
            if (tj > tL) {
                tL = tj;
                sL = tot[j];
                cL = tot[J + j];
            }
        } else if (tj < tR) {
            tR = tj;
            sR = tot[j];
            cR = tot[J + j];
        }
    }
    // (f(0) > 0 was established in the first pass, so a lower point exists and c(L) >= 1)
    const double nL = (sL - gamma) / cL;
    if (tau < 0.0 && (int64_t)cL == (int64_t)cR) tau = nL;     // nothing lies in (t_L, t_R]: f is linear there
    if (tau < 0.0 && !(nL > tL)) tau = tL;                     // f(t_L) = 0: the step from L stays at L
    if (tau >= 0.0) {
        st[PL_STATUS] = 1.0;
        st[PL_TAU] = tau;
        st[PL_HINT] = tau;
        return;
    }
    double lo = nL, qlo = cL;
    if (cR > 0.0) {
        const double nR = (sR - gamma) / cR;
        if (nR > lo) {
            lo = nR;
            qlo = cR;
        }
    }
    if (lo < tL) lo = tL;
    const double fL = sL - tL * cL - gamma, fR = sR - tR * cR - gamma;
    double hi = tL + fL * (tR - tL) / (fL - fR);
    if (!(hi < tR)) hi = tR;
    if (!(hi > lo)) hi = tR;
    st[PL_TL] = tL;
    st[PL_CL] = cL;
    st[PL_SL] = sL;
    st[PL_TR] = tR;
    st[PL_CR] = cR;
    st[PL_SR] = sR;
    st[PL_Q0] = lo > tL ? qlo : -1.0;
    for (int j = 0; j < J; ++j) cand[j] = lo + (hi - lo) * ((double)j / (double)(J - 1));
}

// [0] the sets still searching, [1] the most passes a set took
__global__ void __launch_bounds__(kThreads) projl1_count_kernel(double *ws, const ProjL1Geom g) {
    double acc[1] = {0.0};
    double mp = 0.0;
    for (int64_t set = (int)threadIdx.x; set < g.P; set += kThreads) {
        const double *s = pl_state(ws, set);
        acc[0] += s[PL_STATUS] == 0.0 ? 1.0 : 0.0;
        mp = s[PL_PASSES] > mp ? s[PL_PASSES] : mp;
    }
    double *sh = dyn_lds<double>();
    double *cnt = projl1_counter(ws, g);
    block_sum_store<1>(acc, sh, cnt);
    double *shm = sh + kThreads / kWave;
    shm[(int)threadIdx.x] = mp;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m2 = 0.0;
        for (int i = 0; i < kThreads; ++i) m2 = shm[i] > m2 ? shm[i] : m2;
        cnt[1] = m2;
    }
}

template <typename T, int V, int MODE>
__global__ void __launch_bounds__(kThreads) projl1_apply_kernel(const ProjL1Args<T> a, const ProjL1Geom g, double *partials) {
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const bool ready = projl1_counter(a.ws, g)[0] == 0.0;   // (no set is still searching)
    const int64_t ntiles = g.ntiles();
    const bool nonneg = a.flags & F_NONNEG, nob = a.flags & F_NOBNDRY;
    for (int64_t tile = blockIdx.x; ready && tile < ntiles; tile += gridDim.x) {
        const int64_t set = tile / g.RB;
        const int rb = (int)(tile - set * g.RB);
        const double *st = pl_state(a.ws, set);
        const bool inside = st[PL_STATUS] == 2.0;
        const T tau = (T)st[PL_TAU];
        for (PlWalk w(g, rb); w.more(); w.next(g)) {
            const int64_t e = w.elem(g, set);
            const Vec<T, V> xx = pl_load<T, V>(a.x, e);
            Vec<T, V> xy = xx, xu = xx, yn, un;
            if (MODE != PL_PLAIN) {
                xu = pl_load<T, V>(a.u, e);
                xy = pl_load<T, V>(a.y, e);
            }
            bool kill = false;
            if (MODE != PL_PLAIN && nob) {
                // (outer = H W C: the pixel of this access)
                const int64_t pix = w.o / a.d.C;
                kill = in_bndry((int)(pix / a.d.W), (int)(pix % a.d.W), a.d.H, a.d.W, a.dH, a.dW);
            }
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const T uo = a.us * xu.v[i];
                T ax, v;
                pl_elem<T, MODE>(xx.v[i], xy.v[i], uo, a.rlx, ax, v);
                T y = inside ? v : soft(v, tau);
                if (MODE != PL_PLAIN) {
                    if (nonneg && y < T(0)) y = T(0);
                    if (kill) y = T(0);
                    un.v[i] = uo + ax - y;
                    const double dr = (double)(xx.v[i] - y), ds = (double)(y - xy.v[i]);
                    acc[0] += dr * dr;
                    acc[1] += ds * ds;
                    acc[2] += (double)xx.v[i] * (double)xx.v[i];
                    acc[3] += (double)y * (double)y;
                    acc[4] += (double)un.v[i] * (double)un.v[i];
                }
                yn.v[i] = y;
            }
            if (MODE == PL_PLAIN) {
                *reinterpret_cast<Vec<T, V> *>(a.out + e) = yn;
            } else {
                *reinterpret_cast<Vec<T, V> *>(a.y + e) = yn;
                *reinterpret_cast<Vec<T, V> *>(a.u + e) = un;
            }
        }
    }
    block_sum_store<8>(acc, dyn_lds<double>(), partials + (int64_t)blockIdx.x * 8);
}

template <typename T, int V, int MODE>
__global__ void __launch_bounds__(kThreads) projl1_cnstr_kernel(const ProjL1Args<T> a, const ProjL1Geom g, double *partials) {
    double acc[1] = {0.0};
    const bool ready = projl1_counter(a.ws, g)[0] == 0.0;
    const int64_t ntiles = g.ntiles();
    for (int64_t tile = blockIdx.x; ready && tile < ntiles; tile += gridDim.x) {
        const int64_t set = tile / g.RB;
        const int rb = (int)(tile - set * g.RB);
        const double *st = pl_state(a.ws, set);
        if (st[PL_STATUS] != 1.0) continue;     // (inside its ball: proj(x) = x)
        const T tau = (T)st[PL_TAU];
        for (PlWalk w(g, rb); w.more(); w.next(g)) {
            const Vec<T, V> xx = pl_load<T, V>(a.x, w.elem(g, set));
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const T v = xx.v[i];
                const double d = (double)(v - soft(v, tau));
                acc[0] += d * d;
            }
        }
    }
    block_sum_store<1>(acc, dyn_lds<double>(), partials + (int64_t)blockIdx.x);
}

template <typename T> int pl_mode(const ProjL1Args<T> &a) {
    if (!a.u) return PL_PLAIN;
    SA_REQUIRE(a.y, "projl1: y and u go together");
    return a.rlx == T(1) ? PL_ADMM : PL_ADMM_RLX;
}

void pl_check(const ProjL1Geom &g) {
    SA_REQUIRE(g.outer >= 1 && g.P >= 1 && g.inner >= 1 && g.V >= 1 && g.G * g.V == g.inner && g.Q == g.outer * g.G &&
                   g.QT >= kThreads && g.QT % kThreads == 0 && g.RB >= 1 && (int64_t)g.RB * g.QT >= g.Q &&
                   (int64_t)(g.RB - 1) * g.QT < g.Q,
               "projl1: inconsistent geometry");
    SA_REQUIRE(g.ntiles() < (int64_t)1 << 31, "projl1: too many sets for one launch");
}

#define SA_PL_MODES(KERNEL, VV, ...)                                                              \
    switch (mode) {                                                                               \
    case PL_PLAIN: hipLaunchKernelGGL((KERNEL<T, VV, PL_PLAIN>), __VA_ARGS__); break;             \
    case PL_ADMM: hipLaunchKernelGGL((KERNEL<T, VV, PL_ADMM>), __VA_ARGS__); break;               \
    default: hipLaunchKernelGGL((KERNEL<T, VV, PL_ADMM_RLX>), __VA_ARGS__); break;                \
    }
#define SA_PL_DISPATCH(KERNEL, ...)                                                               \
    do {                                                                                          \
        constexpr int VM = (int)(16 / sizeof(T));                                                 \
        if (g.V == VM) {                                                                          \
            SA_PL_MODES(KERNEL, VM, __VA_ARGS__)                                                  \
        } else if (VM == 4 && g.V == 2) {                                                         \
            SA_PL_MODES(KERNEL, 2, __VA_ARGS__)                                                   \
        } else {                                                                                  \
            SA_REQUIRE(g.V == 1, "projl1: bad vector width");                                     \
            SA_PL_MODES(KERNEL, 1, __VA_ARGS__)                                                   \
        }                                                                                         \
    } while (0)

}  // namespace

void projl1_reset(hipStream_t st, double *ws, const ProjL1Geom &g) {
    hipLaunchKernelGGL(projl1_reset_kernel, dim3((unsigned)ceil_div(g.P, kThreads)), dim3(kThreads), 0, st, ws, g);
    SA_HIP(hipGetLastError());
}

template <typename T>
void launch_projl1_search(hipStream_t st, const ProjL1Args<T> &a, const ProjL1Geom &g, int passes, bool restart) {
    pl_check(g);
    SA_REQUIRE(a.x && a.ws && a.gamma >= 0.0 && passes >= 1, "projl1_search: bad argument");
    const int mode = pl_mode(a);
    const int64_t gset = ceil_div(g.P, kThreads), gwave = ceil_div(g.P, kThreads / kWave);
    SA_REQUIRE(gwave < (int64_t)1 << 31, "projl1: too many sets for one launch");
    if (restart) hipLaunchKernelGGL(projl1_init_kernel, dim3((unsigned)gset), dim3(kThreads), 0, st, a.ws, g);
    const size_t lds = sizeof(double) * (2 * kProjL1Cand + 1) * (kThreads / kWave);
    for (int k = 0; k < passes; ++k) {
        SA_PL_DISPATCH(projl1_pass_kernel, dim3((unsigned)g.ntiles()), dim3(kThreads), lds, st, a, g);
        hipLaunchKernelGGL(projl1_decide_kernel, dim3((unsigned)gwave), dim3(kThreads), 0, st, a.ws, g, a.gamma);
    }
    hipLaunchKernelGGL(projl1_count_kernel, dim3(1), dim3(kThreads), sizeof(double) * (kThreads + kThreads / kWave), st,
                       a.ws, g);
    SA_HIP(hipGetLastError());
}

template <typename T> int launch_projl1_apply(hipStream_t st, const ProjL1Args<T> &a, const ProjL1Geom &g, double *partials) {
    pl_check(g);
    SA_REQUIRE(a.x && a.ws && partials, "projl1_apply: null argument");
    const int mode = pl_mode(a);
    SA_REQUIRE(mode == PL_PLAIN ? a.out != nullptr : true, "projl1_apply: no output array");
    SA_REQUIRE(mode == PL_PLAIN || !(a.flags & F_NOBNDRY) || g.outer == (int64_t)a.d.H * a.d.W * a.d.C,
               "projl1_apply: NoBndryCross needs the coefficient array's geometry");
    const int grid = (int)std::min<int64_t>(g.ntiles(), kMaxPartialBlocks);
    const size_t lds = sizeof(double) * 8 * (kThreads / kWave);
    SA_PL_DISPATCH(projl1_apply_kernel, dim3(grid), dim3(kThreads), lds, st, a, g, partials);
    SA_HIP(hipGetLastError());
    return grid;
}

template <typename T> int launch_projl1_cnstr(hipStream_t st, const ProjL1Args<T> &a, const ProjL1Geom &g, double *partials) {
    pl_check(g);
    SA_REQUIRE(a.x && a.ws && partials && !a.u, "projl1_cnstr: bad argument");
    const int mode = PL_PLAIN;
    const int grid = (int)std::min<int64_t>(g.ntiles(), kMaxPartialBlocks);
    const size_t lds = sizeof(double) * (kThreads / kWave);
    SA_PL_DISPATCH(projl1_cnstr_kernel, dim3(grid), dim3(kThreads), lds, st, a, g, partials);
    SA_HIP(hipGetLastError());
    return grid;
}

#define SA_PL_INST(T)                                                                                       \
    template void launch_projl1_search<T>(hipStream_t, const ProjL1Args<T> &, const ProjL1Geom &, int, bool); \
    template int launch_projl1_apply<T>(hipStream_t, const ProjL1Args<T> &, const ProjL1Geom &, double *);   \
    template int launch_projl1_cnstr<T>(hipStream_t, const ProjL1Args<T> &, const ProjL1Geom &, double *);
SA_PL_INST(float)
SA_PL_INST(double)

}  // namespace sporco_amd
