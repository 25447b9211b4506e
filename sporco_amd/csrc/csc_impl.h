// csc_impl.h -- what the translation units behind the C ABI share: transfer counting, the
// per-kernel event profiler, the type-erased solver interface (CscBase) that the extern "C"
// glue (csc_abi.hip) talks to, the base of the side handles (SideBase) with their type-erased
// interfaces, and the error-to-return-code macros.  The solver itself
// (template Csc<T>, csc_api.hip + api_*.inc) is only visible through make_csc().
#pragma once
#include "../../include/sporco_amd.h"

#include <cmath>
#include <cstdlib>
#include <memory>
#include <string>
#include <utility>
#include <cstring>
#include <vector>

#include "common.h"
#include "csc_ball.h"
#include "csc_fused.h"
#include "csc_inhib.h"
#include "csc_kernels.h"
#include "csc_l1l1.h"
#include "csc_pd.h"
#include "csc_pdl1.h"
#include "csc_pgm.h"
#include "csc_projl1.h"
#include "csc_rows.h"
#include "csc_rtv.h"
#include "csc_tv.h"
#include "csc_tvd.h"
#include "csc_tvdc.h"
#include "csc_spline.h"
#include "csc_bpdn.h"
#include "csc_pgm_bpdn.h"
#include "csc_cmod.h"
#include "csc_pgm_cmod.h"
#include "csc_rpca.h"
#include "fft.h"

#include <atomic>

namespace sporco_amd {

constexpr long kAllocAlignMb = 64;    // alignment of the large device buffers, MiB (csc_api.hip big_alloc)

extern thread_local std::string g_last_error;

// Every host <-> device copy of this file is counted (sporco_amd_transfer_stats): the claim
// "the pipeline makes one upload and one download" is then something a test can check.
extern std::atomic<int64_t> g_xfer[4];
static inline void count_xfer(hipMemcpyKind k, size_t bytes) {
    if (k == hipMemcpyHostToDevice) {
        g_xfer[0] += (int64_t)bytes;
        g_xfer[1] += 1;
    } else if (k == hipMemcpyDeviceToHost) {
        g_xfer[2] += (int64_t)bytes;
        g_xfer[3] += 1;
    }
}
static inline hipError_t sa_memcpy(void *d, const void *s, size_t n, hipMemcpyKind k) {
    count_xfer(k, n);
    return hipMemcpy(d, s, n, k);
}
static inline hipError_t sa_memcpy_async(void *d, const void *s, size_t n, hipMemcpyKind k,
                                         hipStream_t st) {
    count_xfer(k, n);
    return hipMemcpyAsync(d, s, n, k, st);
}
static inline hipError_t sa_memcpy2d_async(void *d, size_t dp, const void *s, size_t sp, size_t w,
                                           size_t h, hipMemcpyKind k, hipStream_t st) {
    count_xfer(k, w * h);
    return hipMemcpy2DAsync(d, dp, s, sp, w, h, k, st);
}
#define hipMemcpy sa_memcpy
#define hipMemcpyAsync sa_memcpy_async
#define hipMemcpy2DAsync sa_memcpy2d_async

enum ProfSlot {
    PS_FFT_R2C = 0,
    PS_FFT_C2C_FWD,
    PS_SM_SOLVE,
    PS_FFT_C2C_INV,
    PS_FFT_C2R,
    PS_ADMM_POST,
    PS_FUSED_COLS,
    PS_ROWS_FWD,
    PS_ROWS_INV_POST,
    PS_ROWS_INV_POST_EMIT,
    PS_ROWS_FWD_V,              // the same three in the single-array state (csc_rows.h):
    PS_ROWS_INV_POST_V,         // V in and out (the (Y, U) -> V transition counts with the
    PS_ROWS_INV_POST_V_EMIT,    // (Y, U) slots: it reads both arrays)
    PS_PGM_GRAD_IFFT,
    PS_PGM_ROWS_PROX,
    PS_PGM_FFT_MOM,
    PS_FINALIZE,
    PS_PGM,
    PS_OTHER,
    PS_PERSIST,                 // a run of iterations in one launch (csc_rows.h admm_persist)
    PS_SETCOEF_ROWS,            // dictionary update: row / column transform of the coefficient maps
    PS_SETCOEF_COLS,            // into the tile-major spectrum Zf (ccmod_setcoef)
    PS_CCMOD_GRAD,              // ... and the gradient over tiles (ccmod_grad_tiled + group sum)
    PS_C2R_VPOST,               // generic chain: c2r row pass + epilogue of the single-array state in one
    PS_C2R_VPOST_EMIT,          // kernel (fft.h fft_c2r_vpost), ... + the next iteration's row spectrum
    PS_INHIB,                   // ConvBPDNInhib: the inhibition-weight update (csc_inhib.h)
    PS_TV_YSTEP,                // ConvBPDNScalarTV / VectorTV: relax + y step + u step + sums (csc_tv.h)
    PS_TV_ADJOINT,              // ... and P = A^T Y, Q = A^T U with the dual-residual sums
    PS_RTV_SOLVE,               // ConvBPDNRecTV: the rank-one / rank-two x step solve (csc_rtv.h)
    PS_RTV_YSTEP,               // ... relax + y step + u step + sums, coefficient and gradient block
    PS_RTV_DUAL,                // ... the adjoint maps and the frequency-domain residual norms
    PS_PD_SOLVE,                // ConvProdDictBPDN: the eigen-channel rank-one x step solve (csc_pd.h)
    PS_PD_RECON,                // ... the reconstruction spectrum through B (reconstruct, fidelity at Y)
    PS_L1L1_Y0STEP,             // ConvL1L1Grd: relax + soft threshold + u step of block 0 (csc_l1l1.h)
    PS_L1L1_DUAL,               // ... both dual-residual norms in one read pass
    PS_BALL_NORMS,              // ConvMinL1InL2Ball: the plane norms of block 0, tiles and totals (csc_ball.h)
    PS_BALL_Y0STEP,             // ... relax + projection onto the l2 balls + u step of block 0
    PS_PDL1_SOLVE,              // ConvProdDictL1L1Grd: the eigen-channel diagonal-plus-rank-one x step (csc_pdl1.h)
    PS_PDL1_DUAL,               // ... the norm of A^T u through B in one read pass
    PS_PROJL1_SEARCH,           // ConvBPDNProjL1: the threshold search passes of the l1-ball projection (csc_projl1.h)
    PS_PROJL1_APPLY,            // ... relax + shrink + u step
    PS_PROJL1_PASS0,            // ... the first search pass of the y step alone: every image, whole arrays
    PS_PROJL1_CNSTR,            // ... the constraint measure's read pass
    PS_TVD_SWEEP,               // TVL2Denoise: one Jacobi sweep of the x step (csc_tvd.h)
    PS_TVD_YSTEP,               // ... relax + y step + u step + the sums that need X
    PS_TVD_ADJOINT,             // ... A^T (Y - U), A^T U and the dual-residual sums
    PS_TVL1_YSTEP,              // TVL1Denoise: relax + y step + u step of the three blocks + the sums that need X
    PS_TVL1_ADJOINT,            // ... A^T (Y - U), A^T U with the identity block, || A^T U ||^2 and || U ||^2
    PS_TVDC_RFFT2,              // TVL2Deconv / TVL1Deconv: the forward transform pair of the right-hand side (csc_tvdc.h)
    PS_TVDC_SOLVE,              // ... the pointwise x step solve with its by-products
    PS_TVDC_IRFFT2,             // ... the inverse transform pair: X (l1: X and H X)
    PS_TVDC_YSTEP,              // ... periodic gradient + relax + y step + u step + sums
    PS_TVDC_ADJOINT,            // ... G^T Y, G^T U (l1: with the data blocks beside them) and the l2 dual-residual sums
    PS_TVDC_DUAL,               // ... l1: the transform of (G^T U_g, U_d) and the norm of A^T U over spectra
    PS_SPL_RFFT2,               // SplineL1: the forward transform pair of the permuted right-hand side (csc_spline.h)
    PS_SPL_SOLVE,               // ... post-twiddle, Gamma, pre-twiddle in place, Reg and the LinSolveCheck sums
    PS_SPL_IRFFT2,              // ... the inverse transform pair: X in permuted order
    PS_SPL_YSTEP,               // ... relax + y step + u step + sums + the permuted arrays of the next x step
    PS_BPDN_DTS,                // BPDN / BPDNJoint / ElasticNet: D^T S (csc_bpdn.h)
    PS_BPDN_ITER,               // ... the whole iteration of a column block (joint: up to the l1 shrinkage)
    PS_BPDN_JOINT_ROWS,         // ... joint: the fixed-order row reductions
    PS_BPDN_JOINT_APPLY,        // ... joint: row scaling, u step, sums
    PS_BPDN_LSC,                // ... the relative residual of the x step (LinSolveCheck)
    PS_BPDN_PGM_STEP,           // pgm.bpdn BPDN / WeightedBPDN: the phases of a proximal gradient step (csc_pgm_bpdn.h)
    PS_BPDN_PGM_YSTEP,          // ... the Y update as a launch of its own (Monotone)
    PS_CMOD_GRAM,               // CnstrMOD: the slab partials of [Z; S] Z^T (csc_cmod.h)
    PS_CMOD_GRAM_REDUCE,        // ... added in slab order
    PS_CMOD_RHS,                // ... the right-hand side of the x step
    PS_CMOD_ITER,               // ... the whole iteration of a block of 16 dictionary columns
    PS_CMOD_DFID,               // ... sum (F Z - S)^2
    PS_CMOD_PGM_GRAD,           // pgm.cmod CnstrMOD / WeightedCnstrMOD: the slab partials of (w (Y Z - S)) Z^T (csc_pgm_cmod.h)
    PS_CMOD_PGM_REDUCE,         // ... added in slab order, || G ||^2 and the Barzilai-Borwein sums
    PS_CMOD_PGM_PROX,           // ... X' = Pcn(Y - G / L), the next Y, the sums of a block of 16 dictionary columns
    PS_CMOD_PGM_DFID,           // ... sum w (X' Z - S)^2, || G Z ||^2 (cmod_dfid with the weight)
    PS_CMOD_PGM_YROBUST,        // ... the Y of the robust backtracking rule
    PS_RPCA_GRAM,               // RobustPCA / prox_nuclear: the slab partials of the Gram matrix of V (csc_rpca.h)
    PS_RPCA_GRAM_REDUCE,        // ... added in slab order
    PS_RPCA_ITER,               // ... X = V T, relax, y step, u step, sums (apply: X alone)
    PS_COUNT
};
extern const char *kProfNames[PS_COUNT];

struct Profiler {
    bool on = false;
    hipStream_t st = nullptr;
    struct Rec {
        int slot;
        hipEvent_t a, b;
    };
    std::vector<Rec> pending;
    std::vector<hipEvent_t> pool;
    double total_ms[PS_COUNT] = {0};
    int64_t count[PS_COUNT] = {0};

    hipEvent_t get() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e;
        SA_HIP(hipEventCreate(&e));
        return e;
    }
    void drain() {
        for (auto &r : pending) {
            SA_HIP(hipEventSynchronize(r.b));
            float ms = 0.f;
            SA_HIP(hipEventElapsedTime(&ms, r.a, r.b));
            total_ms[r.slot] += ms;
            count[r.slot] += 1;
            pool.push_back(r.a);
            pool.push_back(r.b);
        }
        pending.clear();
    }
    ~Profiler() {
        for (auto &r : pending) {
            (void)hipEventDestroy(r.a);
            (void)hipEventDestroy(r.b);
        }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
};

// RAII timing scope around one kernel (group) on the handle's stream.
struct ProfScope {
    Profiler &p;
    int slot;
    hipEvent_t a = nullptr;
    ProfScope(Profiler &p_, int slot_) : p(p_), slot(slot_) {
        if (p.on) {
            a = p.get();
            SA_HIP(hipEventRecord(a, p.st));
        }
    }
    ~ProfScope() {
        if (p.on && a) {
            hipEvent_t b = p.get();
            (void)hipEventRecord(b, p.st);
            p.pending.push_back({slot, a, b});
            if (p.pending.size() >= 200) p.drain();
        }
    }
};

struct CscBase {
    virtual ~CscBase() {}
    virtual void sync() = 0;
    virtual void *stream_handle() = 0;
    virtual int query(int what) = 0;
    virtual std::string placement() = 0;
    virtual void set_hint(int what, int value) = 0;
    virtual void set_signal(const void *S) = 0;
    virtual void set_signal_dev(const void *S_dev) = 0;
    virtual void reconstruct_dev(int var, void *dst_dev) = 0;
    virtual void set_dict(const void *D, int dH, int dW) = 0;
    virtual void set_dict_imag(const void *D, int dH, int dW) = 0;
    virtual void set_weight(int which, const void *w, const int64_t shape[5]) = 0;
    virtual void set_grad_weight(const void *w) = 0;
    virtual void set_filter_sizes(const int32_t *fh, const int32_t *fw) = 0;
    virtual void upload(int var, const void *src) = 0;
    virtual void download(int var, void *dst) = 0;
    virtual void *device_ptr(int var) = 0;
    virtual void admm_iter(const sporco_amd_admm_params &p, double *out_dev) = 0;
    virtual int admm_run(const sporco_amd_admm_params &p, const sporco_amd_admm_ctrl &c,
                         sporco_amd_admm_record *records, double *rho_out, double *u_scale_out,
                         sporco_amd_reduce_fn reduce, void *user) = 0;
    virtual void admm_xstep(const sporco_amd_admm_params &p, double *out_dev) = 0;
    virtual void admm_relax(double rlx) = 0;
    virtual void admm_ystep(const sporco_amd_admm_params &p) = 0;
    virtual void admm_ustep(const sporco_amd_admm_params &p) = 0;
    virtual void admm_stats(const sporco_amd_admm_params &p, double *out_dev) = 0;
    virtual void scale_u(double s) = 0;
    virtual void reconstruct(int var, void *dst) = 0;
    virtual void dhs_absmax(double *out_host) = 0;
    virtual void pgm_grad(int var, double *out_dev) = 0;
    virtual void pgm_eval(int var, double *out_dev) = 0;
    virtual void pgm_iter(const sporco_amd_pgm_params &p, double *out_dev) = 0;
    virtual void pgm_commit() = 0;
    virtual void pgm_prox_step(double L, double lmbda, uint32_t flags, int dH, int dW,
                               double *out_dev) = 0;
    virtual void lincomb(int dst, double a, int va, double b, int vb, double c, int vc) = 0;
    virtual void pair_stats(int va, int vb, int vg, double *out_dev) = 0;
    virtual void pgm_resid(int var, int slot) = 0;
    virtual void pgm_resid_stats(int a, int b, int c, int d, double *out_dev) = 0;
    virtual void copy(int dst, int src) = 0;
    virtual void ccmod_setcoef(int var) = 0;
    virtual void ccmod_grad(int var, bool write_grad, double *out_dev) = 0;
    virtual void ccmod_prox_step(double L, int dH, int dW, bool zm) = 0;
    virtual void ccmod_sgd_step(double eta, int dH, int dW, bool zm, double *out_dev) = 0;
    virtual void ccmod_cnstr(int dH, int dW, bool zm, double *out_dev) = 0;
    virtual void ccmod_getdict(int dH, int dW, void *dst) = 0;
    virtual void setdict_from_dstep(int dH, int dW) = 0;
    virtual void asum(int var, double *out_dev) = 0;
    virtual void masked_grad(int var, bool dstep, int mode, double *out_dev) = 0;
    virtual void cns_init(const void *Y0, double rho) = 0;
    virtual void cns_iter(const sporco_amd_cns_params &p, double *out_dev) = 0;
    virtual void cns_md_init(const void *S) = 0;
    virtual void *cns_mean_ptr(int64_t *count) = 0;
    virtual void mdcpl_init(const void *S) = 0;
    virtual void mdcpl_iter(const sporco_amd_admm_params &p, double *out_dev) = 0;
    virtual void l1l1_iter(const sporco_amd_admm_params &p, double *out_dev) = 0;
    virtual void ball_iter(const sporco_amd_admm_params &p, double *out_dev) = 0;
    virtual void projl1_iter(const sporco_amd_admm_params &p, double gamma, double *out_dev, double *out_host) = 0;
    virtual void dstep_init(const void *Y0) = 0;
    virtual void dstep_md_init(const void *Y0, const void *S) = 0;
    virtual void dstep_iter(const sporco_amd_dstep_params &p, double *out_dev) = 0;
    virtual void fft_var(int rvar, int cvar, bool inverse) = 0;
    virtual void inhib_setup(const double *Wg, int Ng, const double *taps_h, int nth, const double *taps_w,
                             int ntw, bool want_self, double lmbda) = 0;
    virtual void inhib_update(const sporco_amd_inhib_params &p, double *out_dev) = 0;
    virtual void tv_setup(const double *tvw, int n, bool vector_tv) = 0;
    virtual void tv_xstep(const sporco_amd_admm_params &p, double *out_dev) = 0;
    virtual void tv_ystep(const sporco_amd_admm_params &p, double *out_dev) = 0;
    virtual void tv_adjoint(double u_scale, double *out_dev) = 0;
    virtual void rtv_setup(const double *tvw, int n) = 0;
    virtual void rtv_xstep(const sporco_amd_admm_params &p, double *out_dev) = 0;
    virtual void rtv_ystep(const sporco_amd_admm_params &p, double *out_dev) = 0;
    virtual void rtv_dual(const sporco_amd_admm_params &p, double *out_dev) = 0;
    virtual void pd_setup(const double *B, const double *Q, const double *gamma, const void *S, int cs) = 0;
    virtual void pd_xstep(const sporco_amd_admm_params &p, double *out_dev) = 0;
    virtual void pd_dfid(int var, double *out_dev) = 0;
    virtual void pd_reconstruct(int var, void *dst) = 0;
    virtual void pdl1_setup(const double *B, const double *Q, const double *gamma, const void *S, int cs,
                            const void *mask) = 0;
    virtual void pdl1_block0(int which, bool to_device, void *host) = 0;
    virtual void pdl1_iter(const sporco_amd_admm_params &p, double *out_dev) = 0;
    virtual void read_out(const double *out_dev, double *out_host) = 0;
    double *out_dev_default = nullptr;
    Profiler prof;
    void *comm_user = nullptr;   // sporco_amd_csc_set_comm: admm_run sums its 16 doubles over the ranks
};
// (csc_comm.hip) all-reduce of the 16 per-iteration sums on `st`
void comm_reduce_sums(void *user, double *sums_dev, hipStream_t st);

static bool var_is_complex(int var) {
    switch (var) {
    case SPORCO_AMD_VAR_XF:
    case SPORCO_AMD_VAR_DF:
    case SPORCO_AMD_VAR_SF:
    case SPORCO_AMD_VAR_YF:
    case SPORCO_AMD_VAR_XFPRV:
    case SPORCO_AMD_VAR_YFPRV:
    case SPORCO_AMD_VAR_VF:
    case SPORCO_AMD_VAR_GF:
    case SPORCO_AMD_VAR_T0:
    case SPORCO_AMD_VAR_T1:
    case SPORCO_AMD_VAR_T2:
    case SPORCO_AMD_VAR_ZF:
    case SPORCO_AMD_VAR_DXF:
    case SPORCO_AMD_VAR_DYF:
    case SPORCO_AMD_VAR_DXFPRV:
    case SPORCO_AMD_VAR_DYFPRV:
    case SPORCO_AMD_VAR_DVF:
    case SPORCO_AMD_VAR_DGF:
    case SPORCO_AMD_VAR_DT0:
    case SPORCO_AMD_VAR_DT1:
    case SPORCO_AMD_VAR_DT2:
        return true;
    default:
        return false;
    }
}

static bool var_is_dict_sized(int var) {
    return var == SPORCO_AMD_VAR_DF || (var >= SPORCO_AMD_VAR_DX && var < SPORCO_AMD_VAR_COUNT);
}

static bool var_is_valid(int var) {
    return (var >= 0 && var <= SPORCO_AMD_VAR_RTVU1) ||
           (var >= SPORCO_AMD_VAR_DX && var < SPORCO_AMD_VAR_COUNT);
}

// What every side handle (TVL2Denoise ... RobustPCA: a problem of its own beside the convolutional solver) has: the
// device and stream, the profiler, the sums with their pinned read-back, and the list of the device buffers it keeps
// for its lifetime.  Base destructors run when a derived constructor throws, so a handle that allocates through
// dev_alloc leaves nothing behind whichever allocation fails.
struct SideBase {
    const int device;
    hipStream_t st = nullptr;
    bool own_stream = false;
    Profiler prof;
    double *out_dev = nullptr, *out_pinned = nullptr;
    FftPlan planH, planW;           // of the handles that transform (Tvdc, Spl); their tables go with the handle
    std::vector<void *> owned;

    SideBase(int device_, void *stream) : device(device_) {
        SA_HIP(hipSetDevice(device));
        if (stream) {
            st = (hipStream_t)stream;
        } else {
            SA_HIP(hipStreamCreate(&st));
            own_stream = true;
        }
        prof.st = st;
        try {
            out_dev = dev_alloc<double>(kOutSlots, true);
            SA_HIP(hipHostMalloc((void **)&out_pinned, sizeof(double) * kOutSlots, 0));
        } catch (...) {
            release();      // (the one constructor that has to: no base below it)
            throw;
        }
    }
    SideBase(const SideBase &) = delete;
    SideBase &operator=(const SideBase &) = delete;
    virtual ~SideBase() { release(); }

    // count elements of U for the handle's lifetime, zeroed on its stream if asked
    template <class U> U *dev_alloc(size_t count, bool zero) {
        owned.push_back(nullptr);      // (first: a pointer that hipMalloc has returned is on the list)
        SA_HIP(hipMalloc(&owned.back(), sizeof(U) * count));
        if (zero) SA_HIP(hipMemsetAsync(owned.back(), 0, sizeof(U) * count, st));
        return (U *)owned.back();
    }
    void sync() { SA_HIP(hipStreamSynchronize(st)); }
    void read_out(double *out_host) {
        SA_HIP(hipMemcpyAsync(out_pinned, out_dev, sizeof(double) * kOutSlots, hipMemcpyDeviceToHost, st));
        sync();
        std::memcpy(out_host, out_pinned, sizeof(double) * kOutSlots);
    }

private:
    void release() {
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(st);
        for (void *p : owned) (void)hipFree(p);
        if (out_pinned) (void)hipHostFree(out_pinned);
        planH.destroy();
        planW.destroy();
        if (own_stream) (void)hipStreamDestroy(st);
    }
};

// The handle of TVL2Denoise and, in its l1 mode, TVL1Denoise (api_tvd.inc): the arrays of one (H, W, P)
// problem and a stream.
struct TvdBase : SideBase {
    using SideBase::SideBase;
    virtual void plan(int64_t out[6]) = 0;
    virtual void upload(int var, const void *src, bool on_device) = 0;
    virtual void download(int var, void *dst, bool on_device) = 0;
    virtual void sweeps(const sporco_amd_tvd_params &p, int n) = 0;
    virtual void gsres(const sporco_amd_tvd_params &p, double *out_host) = 0;
    virtual void ystep(const sporco_amd_tvd_params &p, double *out_host) = 0;
    virtual void adjoint() = 0;
};
TvdBase *make_tvd(int dtype, int H, int W, int64_t P, int C, bool vector_tv, bool l1, int device, void *stream);

// The handle of TVL2Deconv and, in its l1 mode, TVL1Deconv (api_tvdc.inc): the arrays and spectra of one
// (H, W, P) problem, the transform plans of H and W and a stream.
struct TvdcBase : SideBase {
    using SideBase::SideBase;
    virtual void plan(int64_t out[8]) = 0;
    virtual void upload(int var, const void *src, bool on_device) = 0;
    virtual void download(int var, void *dst, bool on_device) = 0;
    virtual void set_kernel(const void *src, int ah, int aw, bool on_device) = 0;
    virtual void xstep(const sporco_amd_tvdc_params &p) = 0;
    virtual void ystep(const sporco_amd_tvdc_params &p, double *out_host) = 0;
    virtual void adjoint() = 0;
};
TvdcBase *make_tvdc(int dtype, int H, int W, int64_t P, int C, bool vector_tv, bool l1, int64_t PA, int device,
                    void *stream);

// The handle of SplineL1 (api_spline.inc): the arrays of one (H, W, P) problem, the work spectrum, the DCT's
// tables, the transform plans of H and W and a stream.
struct SplBase : SideBase {
    using SideBase::SideBase;
    virtual void plan(int64_t out[4]) = 0;
    virtual void upload(int var, const void *src, bool on_device) = 0;
    virtual void download(int var, void *dst, bool on_device) = 0;
    virtual void xstep(const sporco_amd_spl_params &p) = 0;
    virtual void ystep(const sporco_amd_spl_params &p, double *out_host) = 0;
};
SplBase *make_spl(int dtype, int H, int W, int64_t P, int device, void *stream);
// the stateless orthonormal DCT-II (inverse: its inverse) over axes (0, 1) of an (H, W, P) array
void spl_dct_dispatch(int dtype, int H, int W, int64_t P, const void *in, void *out, bool inverse, bool on_device);

// The handle of BPDN, BPDNJoint and ElasticNet (api_bpdn.inc): the arrays of one (N, M, K) problem, the dictionary and
// the solve matrix in the order the product routine reads them, and a stream.
struct BpdnBase : SideBase {
    using SideBase::SideBase;
    virtual void plan(int64_t out[4]) = 0;
    virtual void set_dict(const void *D) = 0;
    virtual void set_solve(const void *P) = 0;
    virtual void upload(int var, const void *src) = 0;
    virtual void download(int var, void *dst) = 0;
    virtual void iter(const sporco_amd_bpdn_params &p, double *out_host) = 0;
    virtual void *var_ptr(int var) = 0;      // the device buffer of a variable (nullptr: not allocated)
    // the proximal gradient steps of pgm.bpdn (api_pgm_bpdn.inc): served by a handle of sporco_amd_bpdn_pgm_create
    virtual void pgm_step(const sporco_amd_bpdn_pgm_params &, double *) { no_pgm(); }
    virtual void pgm_ystep(double, double, int, int, double *) { no_pgm(); }
    virtual void pgm_copy(int, int) { no_pgm(); }
    [[noreturn]] static void no_pgm() {
        throw Error(SPORCO_AMD_EINVAL, "bpdn: the handle was not made by sporco_amd_bpdn_pgm_create");
    }
};
BpdnBase *make_bpdn(int dtype, int N, int M, int64_t K, int device, void *stream);
BpdnBase *make_pgm_bpdn(int dtype, int N, int M, int64_t K, int device, void *stream);

// The handle of CnstrMOD (api_cmod.inc): the dictionary variables of one (N, M, K) problem in the order the product
// routine reads them, the Gram matrices of the coefficients, its own or a borrowed Z and S, and a stream.
struct CmodBase : SideBase {
    using SideBase::SideBase;
    virtual void plan(int64_t out[8]) = 0;
    virtual void set_signal(const void *S, bool on_device) = 0;
    virtual void set_coef(const void *Z, bool on_device) = 0;
    virtual void set_solve(const void *Q) = 0;
    virtual void upload(int var, const void *src) = 0;
    virtual void download(int var, void *dst) = 0;
    virtual void iter(const sporco_amd_cmod_params &p, double *out_host) = 0;
    virtual void dfid(int var, double *out_host) = 0;
    // the proximal gradient steps of pgm.cmod (api_pgm_cmod.inc): served by a handle of sporco_amd_cmod_pgm_create
    virtual void set_weight(const void *, bool) { no_pgm(); }
    virtual void pgm_step(const sporco_amd_cmod_pgm_params &, double *) { no_pgm(); }
    [[noreturn]] static void no_pgm() {
        throw Error(SPORCO_AMD_EINVAL, "cmod: the handle was not made by sporco_amd_cmod_pgm_create");
    }
};
CmodBase *make_cmod(int dtype, int N, int M, int64_t K, int device, void *stream);
CmodBase *make_pgm_cmod(int dtype, int N, int M, int64_t K, int device, void *stream);

// The handle of RobustPCA and of the stateless prox_nuclear / norm_nuclear (api_rpca.inc): X, Y, U of one (R, C)
// problem as NumPy has them, its own or a borrowed S, the Gram matrix and its slab partials, T, and a stream.
struct RpcaBase : SideBase {
    using SideBase::SideBase;
    virtual void plan(int64_t out[10]) = 0;
    virtual void set_signal(const void *S, bool on_device) = 0;
    virtual void upload(int var, const void *src) = 0;
    virtual void download(int var, void *dst) = 0;
    virtual void *var_ptr(int var) = 0;
    virtual void gram(int mode, double u_scale, double *G_host) = 0;
    virtual void iter(const sporco_amd_rpca_params &p, const double *T_host, double *out_host) = 0;
    virtual void apply(const double *T_host) = 0;
};
RpcaBase *make_rpca(int dtype, int R, int C, int device, void *stream);

// the one place that instantiates Csc<float> / Csc<double> (csc_api.hip)
CscBase *make_csc(const sporco_amd_dims &dims, int dict_channels, int device, void *stream,
                  int depth = 1);

}  // namespace sporco_amd


struct sporco_amd_csc {
    std::unique_ptr<sporco_amd::CscBase> impl;
    int device;
    int depth = 1;                // > 1: a volume handle (sporco_amd_csc_create_volume)
    double *stats_dev = nullptr;  // scratch for pgm_stats into a separate buffer
    ~sporco_amd_csc() {
        if (stats_dev) (void)hipFree(stats_dev);
    }
};

// the six side handles: the implementation and the device that the glue selects before it calls
template <class B> struct SideHandle {
    std::unique_ptr<B> impl;
    int device;
};
struct sporco_amd_tvd : SideHandle<sporco_amd::TvdBase> {};
struct sporco_amd_tvdc : SideHandle<sporco_amd::TvdcBase> {};
struct sporco_amd_spl : SideHandle<sporco_amd::SplBase> {};
struct sporco_amd_bpdn : SideHandle<sporco_amd::BpdnBase> {};
struct sporco_amd_cmod : SideHandle<sporco_amd::CmodBase> {};
struct sporco_amd_rpca : SideHandle<sporco_amd::RpcaBase> {};

#define SA_API_BEGIN try {
#define SA_API_END                                                                     \
    }                                                                                  \
    catch (const sporco_amd::Error &e) {                                               \
        g_last_error = e.what();                                                       \
        return e.code;                                                                 \
    }                                                                                  \
    catch (const std::bad_alloc &) {                                                   \
        g_last_error = "host allocation failed";                                       \
        return SPORCO_AMD_ENOMEM;                                                      \
    }                                                                                  \
    catch (const std::exception &e) {                                                  \
        g_last_error = e.what();                                                       \
        return SPORCO_AMD_EINVAL;                                                      \
    }                                                                                  \
    return SPORCO_AMD_OK;

#define SA_HANDLE_ANY(h)                                                               \
    SA_REQUIRE((h) != nullptr && (h)->impl, "null handle");                            \
    SA_HIP(hipSetDevice((h)->device));
// (every entry point that has not been taught the third transform axis refuses a volume handle)
#define SA_HANDLE(h)                                                                   \
    SA_HANDLE_ANY(h)                                                                   \
    SA_REQUIRE((h)->depth == 1,                                                        \
               "a volume handle (dimN = 3) serves the ADMM sparse coding calls only");
