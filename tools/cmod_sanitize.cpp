// cmod_sanitize.cpp -- a stand-alone host program for AddressSanitizer / UndefinedBehaviorSanitizer runs of the
// CnstrMOD handle (sporco_amd/csrc/api_cmod.inc) and the kernels of csc_cmod.hip in their CPU fiber-simulator build
// (tests/hostsim).  CPU only; never loaded into Python, never run on a GPU.  At (N, M, K) = 8 x 16 x 5, 33 x 40 x 1,
// 5 x 176 x 49, 24 x 16 x 33, 64 x 132 x 97 (four slabs, two row and three column blocks of the output) and
// 512 x 512 x 3 (the largest tiles of cmod_iter), in float32 and float64: set_signal, set_coef from a host array,
// the downloads of G and S Z^T, set_solve, uploads of Y and U, an iteration with ZeroMean at Y and one without at X
// with a pending u_scale, a second set_coef on the same handle, the stand-alone dfid call, and the downloads.  Build
// and run from the repository root:
//
//   S=sporco_amd/csrc; F="-O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -mfma -ffp-contract=off \
//     -std=c++17 -Itests/hostsim -I$S -x c++ -Wno-unknown-pragmas -Wno-attributes"
//   for f in $S/csc_cmod.hip $S/ck_misc.hip tests/hostsim/hostsim_runtime.cpp tools/cmod_sanitize.cpp;
//     do g++ $F -c $f -o build/$(basename $f).o; done          (mkdir -p build first)
//   g++ -fsanitize=address,undefined build/*.o -o build/cmod_sanitize
//   ASAN_OPTIONS=detect_leaks=0 build/cmod_sanitize
//
// (detect_leaks=0 as for the `asan` target of tests/hostsim/Makefile: the simulator keeps its 256 fiber stacks,
// hostsim_runtime.cpp run_grid, until the process ends; they are the only thing the leak check reports.)
// The solve matrix comes from a Gauss-Jordan inverse in double here.  It prints the Gram matrices and the sums against
// a host evaluation, and exits non-zero when one is off.
#include "csc_impl.h"

#include <cstdio>
#include <vector>

namespace sporco_amd {
std::atomic<int64_t> g_xfer[4];
const char *kProfNames[PS_COUNT] = {};
#include "api_cmod.inc"
}  // namespace sporco_amd

using namespace sporco_amd;

// (G + rho I)^-1, row-major (M, M)
static std::vector<double> solve_matrix(const std::vector<double> &G, int M, double rho) {
    std::vector<double> A(G), P((size_t)M * M, 0.0);
    for (int i = 0; i < M; ++i) {
        A[(size_t)i * M + i] += rho;
        P[(size_t)i * M + i] = 1.0;
    }
    for (int k = 0; k < M; ++k) {      // (symmetric positive definite: no pivoting)
        const double d = 1.0 / A[(size_t)k * M + k];
        for (int j = 0; j < M; ++j) {
            A[(size_t)k * M + j] *= d;
            P[(size_t)k * M + j] *= d;
        }
        for (int i = 0; i < M; ++i) {
            if (i == k) continue;
            const double f = A[(size_t)i * M + k];
            if (f == 0.0) continue;
            for (int j = 0; j < M; ++j) {
                A[(size_t)i * M + j] -= f * A[(size_t)k * M + j];
                P[(size_t)i * M + j] -= f * P[(size_t)k * M + j];
            }
        }
    }
    return P;
}

template <typename T> static int run(int N, int M, int64_t K) {
    const size_t E = (size_t)N * M;
    std::vector<T> z((size_t)M * K), s((size_t)N * K), y(E), u(E), x(E), yo(E), uo(E), szt(E);
    std::vector<double> G((size_t)M * M), SZ(E);
    unsigned seed = 4321u + (unsigned)(N * 131 + M * 7 + K);
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return (double)(seed >> 8) / (double)(1u << 24) - 0.5;
    };
    for (auto &v : z) v = (T)rnd();
    for (auto &v : s) v = (T)rnd();
    for (size_t i = 0; i < E; ++i) {
        y[i] = (T)rnd();
        u[i] = (T)(0.05 * rnd());
    }
    const double rho = 0.8;
    const double rtol = sizeof(T) == 4 ? 1e-4 : 1e-10;
    auto off = [&](double a, double b) { return !(std::fabs(a - b) <= rtol * (1 + std::fabs(b))); };
    int bad = 0;
    std::unique_ptr<CmodBase> h(make_cmod(sizeof(T) == 4 ? SPORCO_AMD_F32 : SPORCO_AMD_F64, N, M, K, 0, nullptr));
    int64_t pl[8];
    h->plan(pl);
    h->set_signal(s.data(), false);
    auto set_coef = [&]() {
        h->set_coef(z.data(), false);
        h->download(SPORCO_AMD_CMOD_G, G.data());
        h->download(SPORCO_AMD_CMOD_SZTD, SZ.data());
        h->download(SPORCO_AMD_CMOD_SZT, szt.data());
        double err = 0, nrm = 0;
        for (int r = 0; r < M + N; ++r)
            for (int m = 0; m < M; ++m) {
                double a = 0;
                const T *row = r < M ? &z[(size_t)r * K] : &s[(size_t)(r - M) * K];
                for (int64_t k = 0; k < K; ++k) a += (double)row[k] * (double)z[(size_t)m * K + k];
                const double got = r < M ? G[(size_t)r * M + m] : SZ[(size_t)(r - M) * M + m];
                err += (a - got) * (a - got);
                nrm += a * a;
                if (r >= M && (T)got != szt[(size_t)(r - M) * M + m]) bad = 1;
            }
        const std::vector<double> Qd = solve_matrix(G, M, rho);
        std::vector<T> Q(Qd.size());
        for (size_t i = 0; i < Q.size(); ++i) Q[i] = (T)Qd[i];
        h->set_solve(Q.data());
        return std::sqrt(err / (nrm + 1e-300));
    };
    double gerr = set_coef();
    h->upload(SPORCO_AMD_CMOD_Y, y.data());
    h->upload(SPORCO_AMD_CMOD_U, u.data());
    sporco_amd_cmod_params p = {};
    p.rho = rho;
    p.rlx = 1.8;
    p.u_scale = 1.0;
    p.zero_mean = 1;
    p.geval_y = 1;
    p.want_dfid = 1;
    double out[SPORCO_AMD_OUT_COUNT], out2[SPORCO_AMD_OUT_COUNT];
    auto check = [&](const char *what) {
        h->download(SPORCO_AMD_CMOD_X, x.data());
        h->download(SPORCO_AMD_CMOD_Y, yo.data());
        h->download(SPORCO_AMD_CMOD_U, uo.data());
        double x2 = 0, y2 = 0, u2 = 0, r2 = 0, df = 0, cmax = 0;
        for (size_t i = 0; i < E; ++i) {
            x2 += (double)x[i] * (double)x[i];
            y2 += (double)yo[i] * (double)yo[i];
            u2 += (double)uo[i] * (double)uo[i];
            r2 += ((double)x[i] - (double)yo[i]) * ((double)x[i] - (double)yo[i]);
        }
        for (int m = 0; m < M; ++m) {      // every column of Y' has unit norm (no input column is zero here)
            double c2 = 0;
            for (int n = 0; n < N; ++n) c2 += (double)yo[(size_t)n * M + m] * (double)yo[(size_t)n * M + m];
            cmax = std::max(cmax, std::fabs(c2 - 1.0));
        }
        const std::vector<T> &f = p.feval_x ? x : yo;
        for (int n = 0; n < N; ++n)
            for (int64_t k = 0; k < K; ++k) {
                double a = 0;
                for (int m = 0; m < M; ++m) a += (double)f[(size_t)n * M + m] * (double)z[(size_t)m * K + k];
                a -= (double)s[(size_t)n * K + k];
                df += a * a;
            }
        h->dfid(p.feval_x ? SPORCO_AMD_CMOD_X : SPORCO_AMD_CMOD_Y, out2);
        const bool fail = !(gerr <= rtol) || off(out[SPORCO_AMD_OUT_AX2], x2) || off(out[SPORCO_AMD_OUT_Y2], y2) ||
                          off(out[SPORCO_AMD_OUT_U2], u2) || off(out[SPORCO_AMD_OUT_R2], r2) ||
                          off(out[SPORCO_AMD_OUT_DFID], df) || out2[SPORCO_AMD_OUT_DFID] != out[SPORCO_AMD_OUT_DFID] ||
                          !(cmax <= (sizeof(T) == 4 ? 1e-5 : 1e-13)) || !std::isfinite(out[SPORCO_AMD_OUT_CNSTR]);
        std::printf("(%d, %d, %ld) %s %-14s slab %ld slabs %ld blocks %ld x %ld: Gram err %.1e ||X||^2 %.6f DFid %.6f Cnstr %.2e%s\n",
                    N, M, (long)K, sizeof(T) == 4 ? "f32" : "f64", what, (long)pl[1], (long)pl[2], (long)pl[3], (long)pl[4], gerr,
                    x2, 0.5 * df, std::sqrt(out[SPORCO_AMD_OUT_CNSTR]), fail ? "  <-- off" : "");
        return fail ? 1 : 0;
    };
    h->iter(p, out);
    bad |= check("zero mean, Y");
    p.zero_mean = 0;
    p.geval_y = 0;
    p.feval_x = 1;
    p.u_scale = 0.5;
    h->iter(p, out);
    bad |= check("at X, u_scale");
    for (auto &v : z) v = (T)rnd();      // a second set_coef on the same handle
    gerr = set_coef();
    p.u_scale = 1.0;
    p.rlx = 1.0;
    h->iter(p, out);
    bad |= check("second setcoef");
    return bad;
}

int main() {
    int bad = 0;
    try {
        const int shapes[6][3] = {{8, 16, 5}, {33, 40, 1}, {5, 176, 49}, {24, 16, 33}, {64, 132, 97}, {512, 512, 3}};
        for (const auto &sh : shapes) {
            bad |= run<double>(sh[0], sh[1], sh[2]);
            bad |= run<float>(sh[0], sh[1], sh[2]);
        }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
