// bpdn_sanitize.cpp -- a stand-alone host program for AddressSanitizer / UndefinedBehaviorSanitizer runs of the
// BPDN / BPDNJoint / ElasticNet handle (sporco_amd/csrc/api_bpdn.inc) and the kernels of csc_bpdn.hip in their CPU
// fiber-simulator build (tests/hostsim).  CPU only; never loaded into Python, never run on a GPU.  At 8 x 16 x 5,
// 33 x 40 x 1, 5 x 176 x 49 (the 16-column block in float32, four blocks) and 24 x 16 x 33, in float32 and float64:
// set_dict, set_solve, an array L1Weight, two plain iterations with LinSolveCheck (the second with X not requested),
// a second set_dict / set_solve on the same handle, two joint iterations with gEvalY on and off (every lazily
// made array), and the downloads.  Build and run from the repository root:
//
//   S=sporco_amd/csrc; F="-O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -mfma -ffp-contract=off \
//     -std=c++17 -Itests/hostsim -I$S -x c++ -Wno-unknown-pragmas -Wno-attributes"
//   for f in $S/csc_bpdn.hip $S/ck_misc.hip tests/hostsim/hostsim_runtime.cpp tools/bpdn_sanitize.cpp;
//     do g++ $F -c $f -o build/$(basename $f).o; done          (mkdir -p build first)
//   g++ -fsanitize=address,undefined build/*.o -o build/bpdn_sanitize
//   ASAN_OPTIONS=detect_leaks=0 build/bpdn_sanitize
//
// (detect_leaks=0 as for the `asan` target of tests/hostsim/Makefile: the simulator keeps its 256 fiber stacks,
// hostsim_runtime.cpp run_grid, until the process ends; they are the only thing the leak check reports.)
// The solve matrix comes from a Gauss-Jordan inverse in double here.  It prints the relative residual of the x step
// and the sums against a host evaluation, and exits non-zero when one is off.
#include "csc_impl.h"

#include <cstdio>
#include <vector>

namespace sporco_amd {
std::atomic<int64_t> g_xfer[4];
const char *kProfNames[PS_COUNT] = {};
#include "api_bpdn.inc"
}  // namespace sporco_amd

using namespace sporco_amd;

// (D^T D + c I)^-1, row-major (M, M)
static std::vector<double> solve_matrix(const std::vector<double> &D, int N, int M, double c) {
    std::vector<double> A((size_t)M * M, 0.0), P((size_t)M * M, 0.0);
    for (int i = 0; i < M; ++i) {
        for (int j = 0; j < M; ++j) {
            double s = 0;
            for (int n = 0; n < N; ++n) s += D[(size_t)n * M + i] * D[(size_t)n * M + j];
            A[(size_t)i * M + j] = s + (i == j ? c : 0.0);
        }
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

template <typename T> static int run(int N, int M, int64_t K, double tol) {
    const int64_t E = (int64_t)M * K;
    std::vector<double> Dd((size_t)N * M);
    std::vector<T> D((size_t)N * M), s((size_t)N * K), w(E), y(E), u(E), x(E), yo(E), uo(E), dts(E);
    unsigned seed = 12345u + (unsigned)(N * 131 + M * 7 + K);
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return (double)(seed >> 8) / (double)(1u << 24) - 0.5;
    };
    for (auto &v : Dd) v = rnd();
    for (size_t i = 0; i < D.size(); ++i) D[i] = (T)Dd[i];
    for (auto &v : s) v = (T)rnd();
    for (int64_t i = 0; i < E; ++i) {
        w[i] = (T)(1.0 + (i % 3) * 0.25);
        y[i] = (T)(0.1 * rnd());
        u[i] = (T)(0.05 * rnd());
    }
    const double rho = 0.8, mu = 0.05;
    int bad = 0;
    std::unique_ptr<BpdnBase> h(make_bpdn(sizeof(T) == 4 ? SPORCO_AMD_F32 : SPORCO_AMD_F64, N, M, K, 0, nullptr));
    auto set_solve = [&](double c) {
        const std::vector<double> Pd = solve_matrix(Dd, N, M, c);
        std::vector<T> P(Pd.size());
        for (size_t i = 0; i < P.size(); ++i) P[i] = (T)Pd[i];
        h->set_solve(P.data());
    };
    h->upload(SPORCO_AMD_BPDN_S, s.data());
    h->set_dict(D.data());
    set_solve(rho);
    h->upload(SPORCO_AMD_BPDN_WL1, w.data());
    h->upload(SPORCO_AMD_BPDN_Y, y.data());
    h->upload(SPORCO_AMD_BPDN_U, u.data());
    int64_t pl[4];
    h->plan(pl);
    sporco_amd_bpdn_params p = {};
    p.rho = rho;
    p.lmbda = 0.2;
    p.mu = mu;
    p.rlx = 1.8;
    p.u_scale = 0.5;
    p.wl1 = 1.0;
    p.c = rho;
    p.nonneg = 1;
    p.geval_y = 1;
    p.want_x = 1;
    p.lin_solve_check = 1;
    double out[SPORCO_AMD_OUT_COUNT];
    auto check = [&](const char *what) {
        h->download(SPORCO_AMD_BPDN_X, x.data());
        h->download(SPORCO_AMD_BPDN_Y, yo.data());
        h->download(SPORCO_AMD_BPDN_U, uo.data());
        h->download(SPORCO_AMD_BPDN_DTS, dts.data());
        const double nrm = std::max(std::sqrt(out[SPORCO_AMD_OUT_XRRS_AX2]), std::sqrt(out[SPORCO_AMD_OUT_XRRS_B2]));
        const double xrrs = nrm > 0 ? std::sqrt(out[SPORCO_AMD_OUT_XRRS_D2]) / nrm : 0.0;
        double x2 = 0, y2 = 0, u2 = 0, r2 = 0, df = 0;
        for (int64_t i = 0; i < E; ++i) {
            x2 += (double)x[i] * (double)x[i];
            y2 += (double)yo[i] * (double)yo[i];
            u2 += (double)uo[i] * (double)uo[i];
            r2 += ((double)x[i] - (double)yo[i]) * ((double)x[i] - (double)yo[i]);
        }
        const std::vector<T> &g = p.feval_x ? x : yo;
        for (int n = 0; n < N; ++n)
            for (int64_t k = 0; k < K; ++k) {
                double a = 0;
                for (int m = 0; m < M; ++m) a += Dd[(size_t)n * M + m] * (double)g[(size_t)m * K + k];
                a -= (double)s[(size_t)n * K + k];
                df += a * a;
            }
        double dt_err = 0, dt_n = 0;
        for (int m = 0; m < M; ++m)
            for (int64_t k = 0; k < K; ++k) {
                double a = 0;
                for (int n = 0; n < N; ++n) a += Dd[(size_t)n * M + m] * (double)s[(size_t)n * K + k];
                dt_err += (a - (double)dts[(size_t)m * K + k]) * (a - (double)dts[(size_t)m * K + k]);
                dt_n += a * a;
            }
        const double rtol = sizeof(T) == 4 ? 1e-4 : 1e-10;
        auto off = [&](double a, double b) { return !(std::fabs(a - b) <= rtol * (1 + std::fabs(b))); };
        const bool fail = !(xrrs <= tol) || off(out[SPORCO_AMD_OUT_AX2], x2) || off(out[SPORCO_AMD_OUT_Y2], y2) ||
                          off(out[SPORCO_AMD_OUT_U2], u2) || off(out[SPORCO_AMD_OUT_R2], r2) ||
                          off(out[SPORCO_AMD_OUT_DFID], df) || !(std::sqrt(dt_err / (dt_n + 1e-300)) <= rtol);
        std::printf("(%d, %d, %ld) %s %-12s KB %ld blocks %ld: XSlvRelRes %.2e ||X||^2 %.6f DFid %.6f D^T S err %.1e%s\n", N,
                    M, (long)K, sizeof(T) == 4 ? "f32" : "f64", what, (long)pl[0], (long)pl[1], xrrs, x2, 0.5 * df,
                    std::sqrt(dt_err / (dt_n + 1e-300)), fail ? "  <-- off" : "");
        return fail ? 1 : 0;
    };
    h->iter(p, out);
    bad |= check("plain");
    p.want_x = 0;
    p.u_scale = 1.0;
    p.feval_x = 1;
    p.geval_y = 0;
    h->iter(p, out);           // (LinSolveCheck stores X all the same)
    bad |= check("plain, fEvalX");
    // the dictionary and the solve matrix set again on the same handle (ElasticNet's c), the weight back to a scalar
    for (auto &v : Dd) v = rnd();
    for (size_t i = 0; i < D.size(); ++i) D[i] = (T)Dd[i];
    h->set_dict(D.data());
    set_solve(rho + mu);
    p.c = rho + mu;
    h->upload(SPORCO_AMD_BPDN_WL1, nullptr);
    p.joint = 1;
    p.feval_x = 0;
    p.geval_y = 1;
    h->iter(p, out);
    bad |= check("joint");
    h->upload(SPORCO_AMD_BPDN_WL1, w.data());
    p.geval_y = 0;
    p.feval_x = 1;
    h->iter(p, out);
    bad |= check("joint, at X");
    if (!(out[SPORCO_AMD_OUT_L21] > 0.0) || !std::isfinite(out[SPORCO_AMD_OUT_L1])) bad = 1;
    return bad;
}

int main() {
    int bad = 0;
    try {
        const int shapes[4][3] = {{8, 16, 5}, {33, 40, 1}, {5, 176, 49}, {24, 16, 33}};
        for (const auto &sh : shapes) {
            bad |= run<double>(sh[0], sh[1], sh[2], 1e-12);
            bad |= run<float>(sh[0], sh[1], sh[2], 2e-5);
        }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
