// spline_sanitize.cpp -- a stand-alone host program for AddressSanitizer / UndefinedBehaviorSanitizer runs of the
// SplineL1 handle (sporco_amd/csrc/api_spline.inc) and the kernels of csc_spline.hip in their CPU fiber-simulator
// build (tests/hostsim).  CPU only; never loaded into Python, never run on a GPU.  One SplineL1 iteration with
// LinSolveCheck and an array DFidWeight, a download of X, and one dctii / idctii round trip, at (5, 4) and
// (7, 9, 3) in float32 and float64 (and a single row, H = 1).  Build and run from the repository root:
//
//   S=sporco_amd/csrc; F="-O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -mfma -ffp-contract=off \
//     -std=c++17 -Itests/hostsim -I$S -x c++ -Wno-unknown-pragmas -Wno-attributes"
//   for f in $S/csc_spline.hip $S/fft.hip $S/ck_misc.hip tests/hostsim/hostsim_runtime.cpp tools/spline_sanitize.cpp;
//     do g++ $F -c $f -o build/$(basename $f).o; done          (mkdir -p build first)
//   g++ -fsanitize=address,undefined build/*.o -o build/spline_sanitize
//   ASAN_OPTIONS=detect_leaks=0 build/spline_sanitize
//
// (detect_leaks=0 as for the `asan` target of tests/hostsim/Makefile: the simulator keeps its 256 fiber stacks,
// hostsim_runtime.cpp run_grid, until the process ends; they are the only thing the leak check reports.)
// It prints the round-trip errors and the relative residual of the x step, and exits non-zero when one is off.
#include "csc_impl.h"

#include <cstdio>
#include <vector>

namespace sporco_amd {
std::atomic<int64_t> g_xfer[4];
const char *kProfNames[PS_COUNT] = {};
#include "api_spline.inc"
}  // namespace sporco_amd

using namespace sporco_amd;

template <typename T> static int run(int H, int W, int64_t P, double tol) {
    const int64_t E = (int64_t)H * W * P;
    std::vector<T> s(E), w(E), x(E), c(E), back(E);
    unsigned seed = 12345u + (unsigned)(H * 131 + W * 7 + P);
    for (int64_t i = 0; i < E; ++i) {
        seed = seed * 1664525u + 1013904223u;
        s[i] = (T)((double)(seed >> 8) / (double)(1u << 24) - 0.5);
        w[i] = (i % 5 == 0) ? T(0) : T(1);
    }
    int bad = 0;
    {
        std::unique_ptr<SplBase> h(make_spl(sizeof(T) == 4 ? SPORCO_AMD_F32 : SPORCO_AMD_F64, H, W, P, 0, nullptr));
        h->upload(SPORCO_AMD_SPL_S, s.data(), false);
        h->upload(SPORCO_AMD_SPL_WDF, w.data(), false);
        h->upload(SPORCO_AMD_SPL_Y, s.data(), false);
        h->upload(SPORCO_AMD_SPL_U, w.data(), false);
        sporco_amd_spl_params p = {0.7, 1.0, 1.8, 0.5, 1.0, 0, 1, 1, 0};
        double out[SPORCO_AMD_OUT_COUNT];
        h->xstep(p);
        h->ystep(p, out);
        h->download(SPORCO_AMD_SPL_X, x.data(), false);
        h->download(SPORCO_AMD_SPL_Y, back.data(), false);
        int64_t pl[4];
        h->plan(pl);
        const double nrm = std::max(std::sqrt(out[SPORCO_AMD_OUT_XRRS_AX2]), std::sqrt(out[SPORCO_AMD_OUT_XRRS_B2]));
        const double xrrs = nrm > 0 ? std::sqrt(out[SPORCO_AMD_OUT_XRRS_D2]) / nrm : 0.0;
        std::printf("(%d, %d, %ld) %s: V %ld, XSlvRelRes %.2e, ||X||^2 %.6f, ||S||^2 %.6f\n", H, W, (long)P,
                    sizeof(T) == 4 ? "f32" : "f64", (long)pl[0], xrrs, out[SPORCO_AMD_OUT_AX2], out[SPORCO_AMD_OUT_C2]);
        double x2 = 0, s2 = 0;
        for (int64_t i = 0; i < E; ++i) {
            x2 += (double)x[i] * (double)x[i];
            s2 += (double)s[i] * (double)s[i];
        }
        if (!(xrrs <= tol) || !(std::fabs(x2 - out[SPORCO_AMD_OUT_AX2]) <= 1e-4 * (1 + x2)) ||
            !(std::fabs(s2 - out[SPORCO_AMD_OUT_C2]) <= 1e-4 * (1 + s2)))
            bad = 1;
    }
    const int dt = sizeof(T) == 4 ? SPORCO_AMD_F32 : SPORCO_AMD_F64;
    spl_dct_dispatch(dt, H, W, P, s.data(), c.data(), false, false);
    spl_dct_dispatch(dt, H, W, P, c.data(), back.data(), true, false);
    double d2 = 0, s2 = 0, c2 = 0;
    for (int64_t i = 0; i < E; ++i) {
        d2 += ((double)back[i] - (double)s[i]) * ((double)back[i] - (double)s[i]);
        s2 += (double)s[i] * (double)s[i];
        c2 += (double)c[i] * (double)c[i];
    }
    std::printf("    dctii / idctii round trip %.2e, Parseval %.2e\n", std::sqrt(d2 / s2), std::fabs(c2 - s2) / s2);
    if (!(std::sqrt(d2 / s2) <= tol) || !(std::fabs(c2 - s2) / s2 <= tol)) bad = 1;
    return bad;
}

int main() {
    int bad = 0;
    try {
        const int shapes[3][3] = {{5, 4, 1}, {7, 9, 3}, {1, 33, 2}};
        for (const auto &sh : shapes) {
            bad |= run<double>(sh[0], sh[1], sh[2], 1e-12);
            bad |= run<float>(sh[0], sh[1], sh[2], 1e-5);
        }
    } catch (const std::exception &e) {
        std::printf("error: %s\n", e.what());
        return 2;
    }
    std::printf(bad ? "FAILED\n" : "ok\n");
    return bad;
}
