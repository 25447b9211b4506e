// csc_ball.hip -- the kernels of csc_ball.h: ball_norms, ball_totals, ball_y0step.  float32 / float64,
// any (outer, C, inner).
#include "csc_ball.h"
#include "csc_kernels_dev.h"

#include <algorithm>

namespace sporco_amd {

BallGeom ball_geom(size_t elem_size, int64_t outer, int64_t C, int64_t inner) {
    BallGeom g;
    g.outer = outer;
    g.planes = inner;
    const int vmax = (int)(16 / elem_size);
    g.V = 1;
    for (int v = vmax; v > 1; v /= 2)
        if (inner % v == 0) {
            g.V = v;
            break;
        }
    g.Cv = C;
    g.G = inner / g.V;
    if (inner == 1 && C % vmax == 0) {      // one plane per outer index: vector along C
        g.V = vmax;
        g.fold = 1;
        g.Cv = C / vmax;
        g.G = 1;
    }
    g.cols = (int)std::min<int64_t>(g.G, kThreads);
    g.rows = kThreads / g.cols;
    g.CB = (int)ceil_div(g.G, g.cols);
    // about four steps a thread, at most about a thousand tiles (four workgroups a compute unit)
    const int64_t cap = std::max<int64_t>(1, 1024 / (outer * g.CB));
    int64_t rb = std::min<int64_t>(std::max<int64_t>(1, ceil_div(g.Cv, (int64_t)g.rows * 4)), cap);
    g.RT = ceil_div(ceil_div(g.Cv, rb), g.rows) * g.rows;
    g.RB = (int)ceil_div(g.Cv, g.RT);
    return g;
}

namespace {

enum BallMode { BALL_PLAIN = 0, BALL_ADMM = 1, BALL_ADMM_RLX = 2 };

// where a thread stands in a tile
struct BallPos {
    int64_t o, cg;      // outer index, column group
    int64_t r0, r1;     // its values of the C index: r0, r0 + rows, ... < r1
    int rb;
    bool active;
};
__device__ __forceinline__ BallPos ball_pos(const BallGeom &g, int64_t tile) {
    BallPos p;
    p.rb = (int)(tile % g.RB);
    const int64_t t2 = tile / g.RB;
    const int cb = (int)(t2 % g.CB);
    p.o = t2 / g.CB;
    const int col = (int)threadIdx.x % g.cols, row = (int)threadIdx.x / g.cols;
    p.cg = (int64_t)cb * g.cols + col;
    p.active = row < g.rows && p.cg < g.G;
    p.r0 = (int64_t)p.rb * g.RT + row;
    p.r1 = std::min<int64_t>((int64_t)(p.rb + 1) * g.RT, g.Cv);
    return p;
}

// ax and v of one element (the same instructions in both passes: the norm is that of the v scaled)
template <typename T, int MODE> __device__ __forceinline__ void ball_elem(T axnr, T yo, T uo, T sv, T rlx, T &ax, T &v) {
    if (MODE == BALL_PLAIN) {
        ax = axnr;
        v = axnr;
    } else {
        ax = MODE == BALL_ADMM_RLX ? fma1(rlx, axnr, (T(1) - rlx) * (yo + sv)) : axnr;
        v = (ax + uo) - sv;
    }
}

template <typename T, int V> __device__ __forceinline__ Vec<T, V> ball_load(const T *p, int64_t e) {
    return *reinterpret_cast<const Vec<T, V> *>(p + e);
}

template <typename T, int V, int MODE>
__global__ void __launch_bounds__(kThreads) ball_norms_kernel(const BallArgs<T> a, const BallGeom g) {
    constexpr int NA = 2 * V;
    double *sh = dyn_lds<double>();                 // kThreads * NA doubles
    const BallPos p = ball_pos(g, (int64_t)blockIdx.x);
    double acc[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) acc[j] = 0.0;
    if (p.active) {
        for (int64_t r = p.r0; r < p.r1; r += g.rows) {
            const int64_t e = ((p.o * g.Cv + r) * g.G + p.cg) * V;
            const Vec<T, V> xa = ball_load<T, V>(a.ax0nr, e);
            Vec<T, V> xy = xa, xu = xa, xs = xa;
            if (MODE != BALL_PLAIN) {
                xu = ball_load<T, V>(a.u0, e);
                xs = ball_load<T, V>(a.s, e);
            }
            if (MODE == BALL_ADMM_RLX) xy = ball_load<T, V>(a.y0, e);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                T ax, v;
                ball_elem<T, MODE>(xa.v[j], xy.v[j], a.us * xu.v[j], xs.v[j], a.rlx, ax, v);
                acc[2 * j] += (double)v * (double)v;
                if (MODE != BALL_PLAIN) {
                    const double q = (double)(xa.v[j] - xs.v[j]);
                    acc[2 * j + 1] += q * q;
                }
            }
        }
    }
    // the rows of each column: a tree of fixed shape in LDS (row r takes row r + w)
    const int col = (int)threadIdx.x % g.cols, row = (int)threadIdx.x / g.cols;
#pragma unroll
    for (int j = 0; j < NA; ++j) sh[(int)threadIdx.x * NA + j] = acc[j];
    __syncthreads();
    int w = 1;
    while (w < g.rows) w <<= 1;
    for (w >>= 1; w > 0; w >>= 1) {
        if (row < w && row + w < g.rows) {
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                acc[j] += sh[((row + w) * g.cols + col) * NA + j];
                sh[(int)threadIdx.x * NA + j] = acc[j];
            }
        }
        __syncthreads();
    }
    if (row == 0 && p.cg < g.G) {
        double *dst = a.ws + ((p.o * g.RB + p.rb) * g.planes) * 2;
        if (g.fold) {
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                s0 += acc[2 * j];
                s1 += acc[2 * j + 1];
            }
            dst[0] = s0;
            dst[1] = s1;
        } else {
#pragma unroll
            for (int j = 0; j < NA; ++j) dst[p.cg * NA + j] = acc[j];
        }
    }
}

// One wave a plane: lane l adds the partials of tiles l, l + 64, ..., then the xor tree.
__global__ void __launch_bounds__(kThreads) ball_totals_kernel(const double *part, double *totals, const BallGeom g) {
    const int lane = (int)threadIdx.x & (kWave - 1);
    const int64_t plane = (int64_t)blockIdx.x * (kThreads / kWave) + (int)threadIdx.x / kWave;
    const bool valid = plane < g.nplanes();
    double s0 = 0.0, s1 = 0.0;
    if (valid) {
        const int64_t o = plane / g.planes, j = plane % g.planes;
        for (int rb = lane; rb < g.RB; rb += kWave) {
            const double *src = part + ((o * g.RB + rb) * g.planes + j) * 2;
            s0 += src[0];
            s1 += src[1];
        }
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if (valid && lane == 0) {
        totals[plane * 2] = s0;
        totals[plane * 2 + 1] = s1;
    }
}

template <typename T, int V, int MODE>
__global__ void __launch_bounds__(kThreads) ball_y0step_kernel(const BallArgs<T> a, const BallGeom g, double *partials) {
    const double *totals = a.ws + g.partial_doubles();
    const int row = (int)threadIdx.x / g.cols;
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t ntiles = g.ntiles();
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const BallPos p = ball_pos(g, tile);
        if (!p.active) continue;
        T sig[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const int64_t plane = g.fold ? p.o : p.o * g.planes + p.cg * V + j;
            const double d = sqrt(totals[plane * 2]);
            const double sg = d <= a.eps ? 1.0 : a.eps / d;
            sig[j] = (T)sg;
            // the constraint measure: once a plane, by the thread that heads its column in the first tile
            if (p.rb == 0 && row == 0 && (!g.fold || j == 0)) {
                const double gp = (MODE == BALL_PLAIN) ? d : (a.geval_y ? sg * d : sqrt(totals[plane * 2 + 1]));
                const double ex = gp > a.eps ? gp - a.eps : 0.0;
                acc[4] += ex * ex;
            }
        }
        for (int64_t r = p.r0; r < p.r1; r += g.rows) {
            const int64_t e = ((p.o * g.Cv + r) * g.G + p.cg) * V;
            const Vec<T, V> xa = ball_load<T, V>(a.ax0nr, e);
            Vec<T, V> xy = xa, xu = xa, xs = xa;
            if (MODE != BALL_PLAIN) {
                xu = ball_load<T, V>(a.u0, e);
                xs = ball_load<T, V>(a.s, e);
            }
            if (MODE == BALL_ADMM_RLX) xy = ball_load<T, V>(a.y0, e);
            Vec<T, V> yn, un;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const T uo = a.us * xu.v[j];
                T ax, v;
                ball_elem<T, MODE>(xa.v[j], xy.v[j], uo, xs.v[j], a.rlx, ax, v);
                yn.v[j] = sig[j] * v;
                acc[2] += (double)yn.v[j] * (double)yn.v[j];
                if (MODE != BALL_PLAIN) {
                    un.v[j] = uo + (ax - (yn.v[j] + xs.v[j]));
                    const double rr = (double)(xa.v[j] - (yn.v[j] + xs.v[j]));
                    acc[0] += rr * rr;
                    acc[1] += (double)xa.v[j] * (double)xa.v[j];
                    acc[3] += (double)un.v[j] * (double)un.v[j];
                }
            }
            *reinterpret_cast<Vec<T, V> *>(a.y0 + e) = yn;
            if (MODE != BALL_PLAIN) *reinterpret_cast<Vec<T, V> *>(a.u0 + e) = un;
        }
    }
    block_sum_store<5>(acc, dyn_lds<double>(), partials + (int64_t)blockIdx.x * 5);
}

template <typename T> int ball_mode(const BallArgs<T> &a) {
    if (!a.u0 && !a.s) return BALL_PLAIN;
    SA_REQUIRE(a.u0 && a.s, "ball: u0 and s go together");
    return a.rlx == T(1) ? BALL_ADMM : BALL_ADMM_RLX;
}

void ball_check(const BallGeom &g) {
    SA_REQUIRE(g.outer >= 1 && g.Cv >= 1 && g.G >= 1 && g.cols >= 1 && g.cols * g.rows <= kThreads && g.RB >= 1 &&
                   g.RT >= 1 && (int64_t)g.RB * g.RT >= g.Cv && (int64_t)g.CB * g.cols >= g.G,
               "ball: inconsistent geometry");
    SA_REQUIRE(g.ntiles() < (int64_t)1 << 31, "ball: too many planes for one launch");
}

// the instantiation for (V, mode): V in {16, 8, 4 bytes} / sizeof(T)
#define SA_BALL_MODES(KERNEL, VV, ...)                                                             \
    switch (mode) {                                                                                \
    case BALL_PLAIN: hipLaunchKernelGGL((KERNEL<T, VV, BALL_PLAIN>), __VA_ARGS__); break;          \
    case BALL_ADMM: hipLaunchKernelGGL((KERNEL<T, VV, BALL_ADMM>), __VA_ARGS__); break;            \
    default: hipLaunchKernelGGL((KERNEL<T, VV, BALL_ADMM_RLX>), __VA_ARGS__); break;               \
    }
#define SA_BALL_DISPATCH(KERNEL, ...)                                                              \
    do {                                                                                           \
        constexpr int VM = (int)(16 / sizeof(T));                                                  \
        if (g.V == VM) {                                                                           \
            SA_BALL_MODES(KERNEL, VM, __VA_ARGS__)                                                 \
        } else if (VM == 4 && g.V == 2) {                                                          \
            SA_BALL_MODES(KERNEL, 2, __VA_ARGS__)                                                  \
        } else {                                                                                   \
            SA_REQUIRE(g.V == 1, "ball: bad vector width");                                        \
            SA_BALL_MODES(KERNEL, 1, __VA_ARGS__)                                                  \
        }                                                                                          \
    } while (0)

}  // namespace

template <typename T> void launch_ball_norms(hipStream_t st, const BallArgs<T> &a, const BallGeom &g) {
    ball_check(g);
    SA_REQUIRE(a.ax0nr && a.ws, "ball_norms: null argument");
    const int mode = ball_mode(a);
    const size_t lds = sizeof(double) * kThreads * 2 * g.V;
    SA_BALL_DISPATCH(ball_norms_kernel, dim3((unsigned)g.ntiles()), dim3(kThreads), lds, st, a, g);
    SA_HIP(hipGetLastError());
}

void launch_ball_totals(hipStream_t st, double *ws, const BallGeom &g) {
    const int64_t grid = ceil_div(g.nplanes(), kThreads / kWave);
    SA_REQUIRE(grid < (int64_t)1 << 31, "ball: too many planes for one launch");
    hipLaunchKernelGGL(ball_totals_kernel, dim3((unsigned)grid), dim3(kThreads), 0, st, (const double *)ws,
                       ws + g.partial_doubles(), g);
    SA_HIP(hipGetLastError());
}

template <typename T> int launch_ball_y0step(hipStream_t st, const BallArgs<T> &a, const BallGeom &g, double *partials) {
    ball_check(g);
    SA_REQUIRE(a.ax0nr && a.y0 && a.ws && partials, "ball_y0step: null argument");
    const int mode = ball_mode(a);
    const int grid = (int)std::min<int64_t>(g.ntiles(), kMaxPartialBlocks);
    const size_t lds = sizeof(double) * 5 * (kThreads / kWave);
    SA_BALL_DISPATCH(ball_y0step_kernel, dim3(grid), dim3(kThreads), lds, st, a, g, partials);
    SA_HIP(hipGetLastError());
    return grid;
}

#define SA_BALL_INST(T)                                                                              \
    template void launch_ball_norms<T>(hipStream_t, const BallArgs<T> &, const BallGeom &);         \
    template int launch_ball_y0step<T>(hipStream_t, const BallArgs<T> &, const BallGeom &, double *);
SA_BALL_INST(float)
SA_BALL_INST(double)

}  // namespace sporco_amd
