/*
 * sporco_amd.h -- C ABI of libsporco_amd.so, the MI355X (gfx950) backend for
 * SPORCO's FFT-domain convolutional sparse coding path.
 *
 * The reference (bwohlberg/sporco) is pure Python and has no FFI of its own
 * (SURVEY.md section 8(b)); its "operator API" is the Python class API.  This
 * header is therefore the binding surface that a reference-side backend shim
 * would load with ctypes (INTEGRATION.md shows that shim).  Every entry point
 * cites the reference function(s) whose arithmetic it replaces, as
 * `sporco/<file>:<lines>` relative to the reference root.
 *
 * Conventions
 *   - plain C: opaque handle, pointers and sizes only, no C++/torch types;
 *   - every function returns 0 on success, a negative code on failure; the
 *     message is available from sporco_amd_last_error() (thread local);
 *   - pointers are HOST pointers unless the parameter name ends in `_dev`;
 *   - arrays use the reference's internal C-contiguous layout
 *     (H, W, C, N, K), filter index K fastest (sporco/cnvrep.py:86-111;
 *     BASELINE letters: N = images = SPORCO `K`, K = filters = SPORCO `M`);
 *     frequency-domain arrays are (H, W/2+1, C, N, K) interleaved complex;
 *   - `dtype` is SPORCO_AMD_F32 (float / complex64) or SPORCO_AMD_F64;
 *   - a handle owns one HIP stream (or borrows the one passed at creation);
 *     calls on one handle must not be issued concurrently from two threads.
 *
 * Environment switches of the library (15).  None is needed in normal use: they pin one code path
 * against another in the tests and in A/B measurements.  All are read ONCE, when a handle is made
 * (csc_api.hip struct Switches) -- except HOST_LOOP and RUN_LAG, which callers flip between runs of
 * one handle and sporco_amd_csc_admm_run reads at its entry -- and RCCL_LIB, read when RCCL is first
 * opened.  Launch forms, staggers and the variants of reverted experiments are constants of the
 * sources since round 5, not switches.
 *   SPORCO_AMD_UNFUSED=1        generic kernel chain (line FFTs + streaming kernels) for every shape
 *   SPORCO_AMD_OLD_ROWS=1       generic row passes around the register-resident column kernel
 *   SPORCO_AMD_NO_PAD=1         no zero filter appended to an odd filter count
 *   SPORCO_AMD_NO_VFORM=1       keep the ADMM iterate as (Y, U): no single-array state (csc_rows.h)
 *   SPORCO_AMD_NO_SPECULATION=1 the row epilogue never emits the next iteration's row spectra
 *   SPORCO_AMD_HOST_LOOP=1      one sporco_amd_csc_admm_iter per iteration, no sporco_amd_csc_admm_run
 *   SPORCO_AMD_RUN_LAG=n        (tests) admm_run pretends not to have seen its newest n records
 *   SPORCO_AMD_PERSIST=1|0      small problems: a run of iterations as ONE launch (off unless the
 *                               handle has SPORCO_AMD_HINT_ONE_LAUNCH; see there)
 *   SPORCO_AMD_NO_COLS_SM=1     generic chain: the column pass as three kernels, not one (fft.h)
 *   SPORCO_AMD_COLS_SM_FORCE_SLAB=k   (tests) ... in slabs of k filters even where the tile fits
 *   SPORCO_AMD_MD_GENERIC=1     ConvBPDNMaskDcpl on the generic chain
 *   SPORCO_AMD_CNS_GENERIC=1    consensus dictionary update on the generic chain
 *   SPORCO_AMD_PDL1_GENERIC=1   (tests) pdl1_solve in its one-thread-per-system form on every shape
 *   SPORCO_AMD_BPDN_PLAIN=1     (tests, measurements) the float32 products of the bpdn handle as fused
 *                               multiply-add chains instead of the matrix instruction; same bits
 *   SPORCO_AMD_CMOD_PLAIN=1     (tests, measurements) the same for the float32 products of the cmod handle
 *   SPORCO_AMD_RPCA_PLAIN=1     (tests, measurements) the float64 Gram products and the float32 product with T of
 *                               the rpca handle as fused multiply-add chains (the latter with the same bits)
 *   SPORCO_AMD_CG_HOST=1        CG dictionary update: the scalars read back every iteration
 *   SPORCO_AMD_PLACEMENT=0|force   no placement search for concurrently written arrays / the search
 *                               (and the striped column output) also for small arrays -- tests
 *                               (sporco_amd_csc_placement_report)
 *   SPORCO_AMD_RCCL_LIB=path    the RCCL library to open (default librccl.so.1, librccl.so)
 * Outside the library: SPORCO_AMD_LIBRARY=path and SPORCO_AMD_SHARE_TORCH_RUNTIME=0 (the Python
 * binding: which build to load / do not pre-load torch's HIP runtime), SPORCO_AMD_BENCH_* (bench.py).
 */
#ifndef SPORCO_AMD_H
#define SPORCO_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPORCO_AMD_F32 0
#define SPORCO_AMD_F64 1

/* error codes */
#define SPORCO_AMD_OK 0
#define SPORCO_AMD_EINVAL (-1)   /* bad argument / unsupported size        */
#define SPORCO_AMD_EHIP (-2)     /* HIP runtime error (message has detail) */
#define SPORCO_AMD_ENOMEM (-3)
#define SPORCO_AMD_ESTATE (-4)   /* call order violated (e.g. no dictionary set) */

/* ---- library-level ------------------------------------------------------ */

const char *sporco_amd_version(void);
const char *sporco_amd_last_error(void);
/* Number of visible HIP devices (0 when none: product code must then fail). */
int sporco_amd_device_count(int *count);
/* Device name and compute-unit count of `device`. */
int sporco_amd_device_info(int device, char *name, size_t name_len, int *cu_count,
                           size_t *hbm_bytes);

/* ---- solver handle ------------------------------------------------------ */

typedef struct sporco_amd_csc *sporco_amd_csc_t;

typedef struct {
    int32_t H, W;   /* spatial size Nv (sporco/cnvrep.py:186)                  */
    int32_t C;      /* channels of S and of X; dictionary is single channel   */
    int32_t N;      /* images,  SPORCO cri.K (cnvrep.py:176-180)              */
    int32_t K;      /* filters, SPORCO cri.M (cnvrep.py:183)                  */
    int32_t dtype;  /* SPORCO_AMD_F32 | SPORCO_AMD_F64                        */
} sporco_amd_dims;

/* State arrays addressable through upload/download. */
#define SPORCO_AMD_VAR_Y 0     /* real  (H,W,C,N,K)   ADMM auxiliary variable        */
#define SPORCO_AMD_VAR_U 1     /* real  (H,W,C,N,K)   ADMM scaled dual variable       */
#define SPORCO_AMD_VAR_X 2     /* real  (H,W,C,N,K)   primal variable                 */
#define SPORCO_AMD_VAR_XF 3    /* cplx  (H,Wf,C,N,K)  rfftn(X)                        */
#define SPORCO_AMD_VAR_DF 4    /* cplx  (H,Wf,1,1,K)  rfftn(D zero-padded)            */
#define SPORCO_AMD_VAR_SF 5    /* cplx  (H,Wf,C,N,1)  rfftn(S)                        */
#define SPORCO_AMD_VAR_YF 6    /* cplx  (H,Wf,C,N,K)  PGM auxiliary state Yf          */
#define SPORCO_AMD_VAR_XFPRV 7 /* cplx  PGM previous Xf                               */
#define SPORCO_AMD_VAR_YFPRV 8 /* cplx  PGM previous Yf                               */
#define SPORCO_AMD_VAR_VF 9    /* cplx  PGM gradient-step buffer Vf / generic scratch */
#define SPORCO_AMD_VAR_GF 10   /* cplx  PGM gradient buffer                           */
#define SPORCO_AMD_VAR_AX 11   /* real  relaxed AX of the staged ADMM path            */
#define SPORCO_AMD_VAR_YPREV 12 /* real Y of the previous iteration (staged ADMM path) */
#define SPORCO_AMD_VAR_T0 13   /* cplx  scratch state for host-composed policies        */
#define SPORCO_AMD_VAR_T1 14   /* cplx  (BB step size: previous x / gradient;           */
#define SPORCO_AMD_VAR_T2 15   /* cplx   robust backtracking: Z; monotone FISTA: ZZ)    */
#define SPORCO_AMD_VAR_ZF 16   /* cplx  (H,Wf,C,N,K) rfftn of the coefficient maps (D-step)   */
#define SPORCO_AMD_VAR_CX 17   /* real  (H,W,C,N,K) consensus D-step: dictionary copy per image */
#define SPORCO_AMD_VAR_CU 18   /* real  (H,W,C,N,K) consensus D-step: scaled dual per image     */
#define SPORCO_AMD_VAR_MY0 19  /* real  (H,W,C,N,1) ConvBPDNMaskDcpl: block 0 of Y (masked residual) */
#define SPORCO_AMD_VAR_MU0 20  /* real  (H,W,C,N,1) ConvBPDNMaskDcpl: block 0 of U                 */
#define SPORCO_AMD_VAR_DMY0 21 /* real  (H,W,C,N,1) mask-decoupling D-step: block 0 of Y           */
#define SPORCO_AMD_VAR_DMU0 22 /* real  (H,W,C,N,1) mask-decoupling D-step: block 0 of U           */
#define SPORCO_AMD_VAR_WML 23  /* real  (H,W,C,N,K) ConvBPDNInhib: lateral inhibition weights (inhib_update) */
#define SPORCO_AMD_VAR_WMS 24  /* real  (H,W,C,N,K) ConvBPDNInhib: self inhibition weights                  */
#define SPORCO_AMD_VAR_TVY 25  /* real  (3,H,W,C,N,K) ConvBPDNScalarTV / VectorTV: the blocks (y_0, y_1, y_L) of Y */
#define SPORCO_AMD_VAR_TVU 26  /* real  (3,H,W,C,N,K) ... and of U                                              */
#define SPORCO_AMD_VAR_RTVY1 27 /* real (H,W,C,N,2) ConvBPDNRecTV: the gradient block of Y (its coefficient block is VAR_Y) */
#define SPORCO_AMD_VAR_RTVU1 28 /* real (H,W,C,N,2) ... and of U (coefficient block: VAR_U)                               */
/* Dictionary-sized state of the D-step (pgm.ccmod.ConvCnstrMOD, admm.ccmod consensus Y =
 * DX): real (H,W,K) / complex (H,Wf,K).  Ids 29..31 are reserved. */
#define SPORCO_AMD_VAR_DX 32      /* real  dictionary iterate X (zero-padded filters)    */
#define SPORCO_AMD_VAR_DXF 33     /* cplx  rfftn(DX)                                     */
#define SPORCO_AMD_VAR_DYF 34     /* cplx  auxiliary (momentum) state                    */
#define SPORCO_AMD_VAR_DXFPRV 35  /* cplx  previous DXF                                  */
#define SPORCO_AMD_VAR_DYFPRV 36  /* cplx  previous DYF                                  */
#define SPORCO_AMD_VAR_DVF 37     /* cplx  gradient-step buffer                          */
#define SPORCO_AMD_VAR_DGF 38     /* cplx  gradient                                      */
#define SPORCO_AMD_VAR_DT0 39     /* cplx  scratch for host-composed policies            */
#define SPORCO_AMD_VAR_DT1 40
#define SPORCO_AMD_VAR_DT2 41
#define SPORCO_AMD_VAR_DSX 42     /* real  X of the single-copy ADMM D-step (dstep_iter)   */
#define SPORCO_AMD_VAR_DSU 43     /* real  its scaled dual variable U                      */
#define SPORCO_AMD_VAR_COUNT 44

/* Create a solver on HIP device `device`.  `stream` is a hipStream_t to borrow
 * (e.g. torch.cuda.current_stream().cuda_stream) or NULL to own a new one.
 * Replaces the allocation half of GenericConvBPDN.__init__
 * (sporco/admm/cbpdn.py:224-236) and PGM ConvBPDN.__init__
 * (sporco/pgm/cbpdn.py:216-233). */
int sporco_amd_csc_create(const sporco_amd_dims *dims, int device, void *stream,
                          sporco_amd_csc_t *out);
/* The same for a multi-channel dictionary (SPORCO cri.Cd > 1, sporco/cnvrep.py:186-194):
 * dict_channels == dims->C channels in D (host layout (dH,dW,Cd,K)) and in S; the coefficient
 * arrays then have a single channel, (H,W,1,N,K), Df is (H,Wf,Cd,1,K), and the X-step is the
 * iterated Sherman-Morrison solve linalg.solvemdbi_ism (sporco/linalg.py:370-444, call site
 * sporco/admm/cbpdn.py:277-279).  ADMM ConvBPDN only; dict_channels == 1 is
 * sporco_amd_csc_create. */
int sporco_amd_csc_create_mc(const sporco_amd_dims *dims, int32_t dict_channels, int device,
                             void *stream, sporco_amd_csc_t *out);
/* Volumes -- three spatial axes, dimN = 3 of sporco/cnvrep.py:33-198 (the constructor contract of
 * sporco/admm/cbpdn.py:175; the reference's examples/scripts/cdl/cbpdndl_video.py:74 is the use):
 * arrays (depth, height, W, C, N, K) are handed over as they lie in memory with dims->H =
 * depth * height, and `depth` tells the handle where the folded axis splits.  Everything per
 * pixel / frequency / row is unchanged on the folded array; the transform along the folded axis
 * runs as two passes.  Single-channel dictionary, given zero-padded to the full volume
 * (sporco_amd_csc_set_dict with dH = dims->H, dW = dims->W).  Such a handle serves the ADMM sparse
 * coding calls (set_signal, set_dict, set_l1_weight, upload / download, admm_iter / _run and the
 * staged steps, the staged PGM steps, reconstruct, dhs_absmax, asum) without NoBndryCross /
 * gradient term / AddMaskSim, and the PGM and consensus dictionary updates (ccmod_setcoef, _grad,
 * _eval, _prox_step, _cnstr, setdict_from_dstep, cns_init, cns_iter without mask decoupling;
 * SPORCO_AMD_VOLUME_FILTER_DEPTH below); every other
 * entry point returns SPORCO_AMD_EINVAL for it.  Generic transform chain. */
int sporco_amd_csc_create_volume(const sporco_amd_dims *dims, int32_t depth, int device, void *stream,
                                 sporco_amd_csc_t *out);
int sporco_amd_csc_destroy(sporco_amd_csc_t h);
int sporco_amd_csc_sync(sporco_amd_csc_t h);
/* The hipStream_t every launch of this handle goes to (the `stream` given at creation, or the
 * stream the handle created for itself): a caller that enqueues its own work between two
 * calls -- the all-reduce hook of sporco_amd_csc_admm_run under torch.distributed -- orders
 * it on this stream (no reference counterpart: the reference is synchronous NumPy). */
int sporco_amd_csc_stream(sporco_amd_csc_t h, void **stream);
/* Which kernels serve this handle's shape: *out = 1 when the fused path named by
 * `what` is active (float32, H and/or W in {128, 256, 512}, even K <= 64 -- or even
 * 64 < K <= 256, where the column pass runs as cooperating 64-filter slab workgroups; since
 * round 6 also H, W in 16 x {10, 12, 14, 15, 18, 20, 21, 24, 25, 27, 28, 30}, K <= 256, for the
 * ADMM ConvBPDN / Joint / GradReg / AddMaskSim / mask-decoupling calls, the fused PGM iteration and
 * the tile-major dictionary-update gradient with K <= 64: such a handle serves LinSolveCheck,
 * multi-channel dictionaries and the consensus update on its generic chain), else 0. */
#define SPORCO_AMD_QUERY_FUSED_COLS 0  /* register-resident column FFT + Sherman-Morrison */
#define SPORCO_AMD_QUERY_FUSED_ROWS 1  /* three-launch ADMM iteration                      */
#define SPORCO_AMD_QUERY_FUSED_PGM 2   /* fused PGM iteration / tile-major D-step               */
#define SPORCO_AMD_QUERY_DEVICE_FILTERS 3 /* filter count of the device-resident arrays: K, or
                                            K + 1 when an odd K was padded with one all-zero
                                            filter to reach the fused kernels (host arrays
                                            always have K; only sporco_amd_csc_device_ptr
                                            exposes the padded layout) */
#define SPORCO_AMD_QUERY_VFORM_LIVE 4   /* 1 while the ADMM iterate lives in the single-array
                                            form of the fused iteration (V = AX + U; Y and U
                                            are derived on the next access) -- diagnostics */
#define SPORCO_AMD_QUERY_PERSIST_RUNS 5  /* how many sporco_amd_csc_admm_run calls of this handle
                                            ran their iterations as one launch (small problems:
                                            see sporco_amd_csc_admm_run) -- diagnostics */
#define SPORCO_AMD_QUERY_CCMOD_GROUPS 6  /* image groups per row frequency of the tile-major
                                          * dictionary-update gradient (their partial gradients
                                          * are written and summed: bench.py's byte model) */
#define SPORCO_AMD_QUERY_PD_WAVE_LAUNCHES 7     /* how many pd_xstep calls of this handle ran the wave
                                                * form of pd_solve (the system in registers) ...        */
#define SPORCO_AMD_QUERY_PD_GENERIC_LAUNCHES 8  /* ... and how many the one-thread-per-system form --
                                                * diagnostics, so that a test can tell the two apart */
#define SPORCO_AMD_QUERY_COLS_SM_FORM 9  /* which form of the one-kernel column pass of the generic
                                          * X-step (forward transform along H, Sherman-Morrison solve,
                                          * inverse transform of a tile held in LDS) the handle's last
                                          * such launch took, or -1 when it has made none (the height
                                          * has a factor the pass does not serve, SPORCO_AMD_NO_COLS_SM,
                                          * a fused path).  Bits 0-11: threads per workgroup (256 or
                                          * 1024); bits 12-15: rows of solve operands a thread requests
                                          * together (float32 4, 8 or 12; float64 2, 4 or 6; 4 in the
                                          * slab form); bit 16: 1 for the instantiation that carries the
                                          * 6-, 10- and 12-point butterflies; bits 17 and up: filters
                                          * per slab, 0 when the whole tile fits LDS -- diagnostics, so
                                          * that a test can tell which instantiation it exercised */
#define SPORCO_AMD_QUERY_PDL1_WAVE_LAUNCHES 10     /* as PD_WAVE_LAUNCHES / PD_GENERIC_LAUNCHES, for the  */
#define SPORCO_AMD_QUERY_PDL1_GENERIC_LAUNCHES 11  /* pdl1_solve launches of sporco_amd_csc_pdl1_iter      */
int sporco_amd_csc_query(sporco_amd_csc_t h, int what, int *out);
/* Diagnostics, no reference counterpart: where the handle put the X-sized arrays that one kernel
 * writes at the same time (the spectrum buffer T and the iterate buffers of the fused ADMM
 * iteration).  Two arrays that take streaming stores concurrently share ~4.7 TB/s on the MI355X
 * when their physical memory lies in the same region of the device memory and get ~6.3 TB/s when
 * it does not (tools/ubench/place_probe.hip, profiles/r05_placement_notes.md), so the handle takes
 * such a buffer from a few candidate allocations, each timed against the arrays it must keep
 * clear of.  The report is a JSON list, one object per decision: role, bytes, candidates tried,
 * the same-region reference rate, probe rate / reference of the first and of the chosen candidate
 * (>= 1.09: clear).  Arrays below 256 MiB are placed as they come (empty list);
 * SPORCO_AMD_PLACEMENT=0 in the environment switches the search off. */
int sporco_amd_csc_placement_report(sporco_amd_csc_t h, char *buf, size_t cap);
/* Hints about how the handle will be used (never needed for correctness; no reference
 * counterpart).  KEEP_VFORM: the caller alternates short device-driven runs with
 * sporco_amd_csc_ccmod_setcoef(VAR_Y) and does not read Y or U in between -- the loop of
 * dictlrn.DictLearn.solve (sporco/dictlrn/dictlrn.py:319-375) -- so even a one-iteration
 * sporco_amd_csc_admm_run keeps the iterate in its single-array form and setcoef derives Y from
 * it on the way into its row transform. */
#define SPORCO_AMD_HINT_KEEP_VFORM 0
/* ONE_LAUNCH: this process has the device to itself and the caller accepts iterates that equal
 * the default loop's to float32 rounding (not bit for bit): sporco_amd_csc_admm_run then runs a
 * small problem (float32, square images of 128 or 256 pixels, K <= 64, at most 4 Mi coefficients,
 * plain ConvBPDN options: scalar weights, NonNegCoef) as ONE kernel launch whose workgroups wait
 * for each other between the passes of an iteration.  9-12 % faster at 256 x 256, K = 32, N = 1
 * (profiles/r03_persist.md).  A wait that cannot complete -- the device was shared after all --
 * ends the call with SPORCO_AMD_EHIP after a few seconds; the handle's iterate is then void.
 * The environment variable SPORCO_AMD_PERSIST=1 / 0 overrides the hint. */
#define SPORCO_AMD_HINT_ONE_LAUNCH 1
/* COMPLEX_PAIR -- not a hint: it changes what the dictionary-update calls compute.  The handle
 * (two-channel dictionary, Cd = 2; set before sporco_amd_csc_set_signal) serves complex-valued
 * signals, coefficient maps and dictionary, whose real and imaginary parts are its two channels:
 * sporco_amd_csc_dstep_iter / _cns_iter then solve the complex problem of
 * sporco/admm/ccmod.py:103-907 given complex input (its fftn / ifftn path, :219-231; the
 * reference's tests/admm/test_ccmod.py:49-140) with the coefficient maps staged per channel
 * (sporco_amd_csc_ccmod_setcoef(VAR_CX)).  Spectral arrays of such a handle hold A + iB and
 * A - iB (A, B the half spectra of the two parts) scaled as csrc/csc_kernels.h
 * launch_pm_butterfly describes; the real arrays (VAR_DX, VAR_DSX, VAR_DSU, VAR_CX, VAR_CU) are
 * (re, im) channel pairs.  Not with mask decoupling, image shards or the objective at X. */
#define SPORCO_AMD_MODE_COMPLEX_PAIR 2
/* VOLUME_FILTER_DEPTH -- a setting, for a volume handle (sporco_amd_csc_create_volume): how many
 * depth slabs the filter support spans.  The dictionary-update calls that take a support (dH, dW) --
 * sporco_amd_csc_ccmod_prox_step, _ccmod_cnstr, _cns_iter -- then crop to (value, dH, dW) (cnvrep.bcrop with
 * dimN = 3, sporco/cnvrep.py:553-606). */
#define SPORCO_AMD_VOLUME_FILTER_DEPTH 3
int sporco_amd_csc_set_hint(sporco_amd_csc_t h, int what, int value);

/* S: real (H,W,C,N) in the handle dtype.  Computes Sf = rfftn(S, axes=(0,1))
 * on device -- sporco/admm/cbpdn.py:228-231, sporco/fft.py:257-286. */
int sporco_amd_csc_set_signal(sporco_amd_csc_t h, const void *S);

/* D: real (dH,dW,K) filters.  Zero-pads to (H,W), Df = rfftn, and caches the
 * per-pixel Sherman-Morrison denominator sum_k |Df|^2 -- setdict,
 * sporco/admm/cbpdn.py:242-256 (DSf is never materialised), and
 * sporco/pgm/cbpdn.py:239-245. */
int sporco_amd_csc_set_dict(sporco_amd_csc_t h, const void *D, int32_t dH, int32_t dW);
/* Complex-valued signals and dictionaries (sporco/admm/cbpdn.py:209-217: real_dtype False, fftn /
 * ifftn in place of rfftn / irfftn; test tests/admm/test_cbpdn.py:179-201).  D_imag: the imaginary
 * part of the dictionary, (dH,dW,K) like D of set_dict, which then holds its real part.  The handle
 * is created with C = 2 Cc channels: the signal passed to set_signal is (Re S, Im S) along the
 * channel axis, and so is every coefficient array -- every transform stays a real one, and the
 * X step pairs the channel halves (A + iB at frequency f, A - iB = the conjugate at -f; two
 * Sherman-Morrison solves per stored frequency, linalg.solvedbi_sm).  The complex soft threshold
 * of the y step is the l2 shrinkage over the pair: callers run FLAG_JOINT with lmbda = 0 and
 * mu = lambda.  Generic kernel chain, single-channel dictionary, no FLAG_XRRS / FLAG_GRADREG.
 * D_imag == NULL returns the handle to a real dictionary. */
int sporco_amd_csc_set_dict_imag(sporco_amd_csc_t h, const void *D_imag, int32_t dH, int32_t dW);

/* l1 weight array (L1Weight option, sporco/admm/cbpdn.py:596-597 after
 * cnvrep.l1Wshape, sporco/cnvrep.py:492-550).  shape[d] is 1 (broadcast) or the
 * full extent of (H,W,C,N,K)[d]; w == NULL restores the scalar weight 1. */
int sporco_amd_csc_set_l1_weight(sporco_amd_csc_t h, const void *w, const int64_t shape[5]);
/* l2,1 weight (L21Weight, sporco/admm/cbpdn.py:781): broadcastable against
 * (H,W,1,N,K); shape[2] must be 1. */
int sporco_amd_csc_set_l21_weight(sporco_amd_csc_t h, const void *w, const int64_t shape[5]);
/* Per-filter weights of the gradient penalty (GradWeight option of ConvBPDNGradReg,
 * sporco/admm/cbpdn.py:1063-1071, :1134-1139): K values of the handle's dtype;
 * w == NULL restores the scalar weight 1. */
int sporco_amd_csc_set_grad_weight(sporco_amd_csc_t h, const void *w);
/* Multi-scale dictionary (a `dsz` made of size blocks, sporco/cnvrep.py:729-812: e.g.
 * ((8, 8, 32), (12, 12, 32), (16, 16, 32))): the support (rows fh[k], columns fw[k]) of each of
 * the K filters for every constraint projection this handle makes (cnvrep.Pcn: crop, zero mean
 * and norm over the filter's own support, cnvrep.py:634-662, :868-913).  The dH / dW arguments of
 * the dictionary-update calls then name the largest support (what bcrop returns).  NULL, NULL
 * returns to one support for all filters. */
int sporco_amd_csc_set_filter_sizes(sporco_amd_csc_t h, const int32_t *fh, const int32_t *fw);
/* Mask of the additive-mask-simulation wrapper (AddMaskSim, sporco/admm/cbpdn.py:2287-2485):
 * broadcastable against (H,W,C,N,1), shape[4] must be 1.  With SPORCO_AMD_FLAG_AMS the last
 * filter of the dictionary is taken to be the appended impulse (:2345-2353); its slice of Y
 * is AX + U zeroed where the mask is nonzero (:2378-2394) and is left out of the l1 / l2,1
 * sums (:2398-2412).  w == NULL removes the mask.
 * Handles made by sporco_amd_csc_create_mc (multi-channel dictionary, Cd channels): the last Cd
 * filters are the appended impulses, one per channel (:2339-2346), and the mask is
 * broadcastable against (H,W,1,N,Cd) -- shape[4] is 1 or Cd, the mask's channels on the filter
 * axis as the reference keeps them (:2358-2364). */
int sporco_amd_csc_set_ams_mask(sporco_amd_csc_t h, const void *w, const int64_t shape[5]);

/* Host <-> device transfer of one state array in the reference layout. */
int sporco_amd_csc_upload(sporco_amd_csc_t h, int var, const void *src);
int sporco_amd_csc_download(sporco_amd_csc_t h, int var, void *dst);
/* Raw device pointer of a state array (plumbing for torch.distributed / tests).
 * LIFETIME: the pointer is valid until the next call on this handle that iterates or changes state
 * (sporco_amd_csc_admm_iter / _admm_run / _pgm_iter / the dictionary-update steps, set_dict,
 * set_signal, upload): the iterates ping-pong between buffers, and the first fused iteration of a
 * handle may MOVE the variable -- the arrays a kernel writes at the same time are placed by
 * measurement then (sporco_amd_csc_placement_report) and the old buffer is freed.  Ask again after
 * such a call; do not cache the value across it. */
int sporco_amd_csc_device_ptr(sporco_amd_csc_t h, int var, void **ptr_dev);

/* ---- ADMM iteration (sporco/admm/admm.py:331-367 loop body) -------------- */

#define SPORCO_AMD_FLAG_NONNEG (1u << 0)     /* NonNegCoef    cbpdn.py:306-307 */
#define SPORCO_AMD_FLAG_NOBNDRY (1u << 1)    /* NoBndryCross  cbpdn.py:308-311 */
#define SPORCO_AMD_FLAG_JOINT (1u << 2)      /* ConvBPDNJoint ystep cbpdn.py:785-794 */
#define SPORCO_AMD_FLAG_RESID (1u << 3)      /* fill residual sums out[0..4]   */
#define SPORCO_AMD_FLAG_OBJ (1u << 4)        /* fill objective sums out[5..7]  */
#define SPORCO_AMD_FLAG_XRRS (1u << 5)       /* LinSolveCheck sums out[8..10]  */
#define SPORCO_AMD_FLAG_GEVAL_Y (1u << 6)    /* regularisers evaluated at Y (gEvalY) */
#define SPORCO_AMD_FLAG_FEVAL_Y (1u << 7)    /* data fidelity evaluated at Y (fEvalX False) */
#define SPORCO_AMD_FLAG_KEEP_X (1u << 8)     /* write X during the call (default: X, Xf are rebuilt
                                                on demand from the previous iterate, which
                                                the fused path keeps) */
#define SPORCO_AMD_FLAG_NO_X (1u << 9)       /* caller will not read X / Xf of this iteration:
                                                they are neither written nor recoverable, and
                                                reading them fails with SPORCO_AMD_ESTATE */
#define SPORCO_AMD_FLAG_GRADREG (1u << 10)   /* ConvBPDNGradReg xstep / objective
                                                (cbpdn.py:1163-1214): diagonal mu*GradWeight*GHGf
                                                + rho, params.mu = gradient weight mu; multi-channel
                                                dictionary: the iterated solve with that diagonal
                                                (:1181-1184) */
#define SPORCO_AMD_FLAG_AMS (1u << 11)       /* AddMaskSim y step / regulariser sums on the
                                                last filter slice (set_ams_mask) */
#define SPORCO_AMD_FLAG_DMASK (1u << 12)     /* pgm_iter: data fidelity (1/2)||W (D x - s)||^2 with
                                                the mask of set_data_mask (pgm.cbpdn.ConvBPDNMask,
                                                sporco/pgm/cbpdn.py:387-506): the residual goes
                                                through the spatial domain for W^2 between the
                                                inner product and the gradient; out[PGM_DFID] =
                                                sum (W R)^2 at the new Xf (want_stats; PGM_F and
                                                PGM_FY are not evaluated: masked_grad has them);
                                                K <= 64, no held trial */

typedef struct {
    double rho;      /* penalty parameter for this iteration                     */
    double lmbda;    /* l1 weight lambda                                          */
    double mu;       /* l2,1 weight (JOINT) / gradient penalty weight (GRADREG)   */
    double rlx;      /* RelaxParam alpha (sporco/admm/admm.py:877-885)            */
    double u_scale;  /* pending `U /= rsf` of update_rho (admm.py:573), applied
                        to U as it is read: U_true = u_scale * U_stored          */
    uint32_t flags;
    int32_t dH, dW;  /* filter support, for NOBNDRY                               */
} sporco_amd_admm_params;

/* Output slots of admm_iter (raw sums; the host forms r, s, eps exactly as
 * sporco/admm/admm.py:462-486 with ADMMEqual.rsdl_* :959-983). */
#define SPORCO_AMD_OUT_R2 0      /* sum (AXnr - Y)^2                               */
#define SPORCO_AMD_OUT_S2 1      /* sum (Y - Yprev)^2   (rho applied by host)      */
#define SPORCO_AMD_OUT_AX2 2     /* sum AXnr^2                                     */
#define SPORCO_AMD_OUT_Y2 3      /* sum Y^2                                        */
#define SPORCO_AMD_OUT_U2 4      /* sum U^2 (new U, before any rho rescale)        */
#define SPORCO_AMD_OUT_DFID 5    /* half-spectrum Parseval sum of |Df.Xf - Sf|^2 / (H W)
                                    (cbpdn.py:337-344, fft.py:449-484); host halves it */
#define SPORCO_AMD_OUT_L1 6      /* sum |wl1 * g-variable|   (cbpdn.py:624-630)    */
#define SPORCO_AMD_OUT_L21 7     /* sum wl21 * sqrt(sum_c g^2) (cbpdn.py:798-807)  */
#define SPORCO_AMD_OUT_XRRS_D2 8 /* sum |ax - b|^2 of the X-step system            */
#define SPORCO_AMD_OUT_XRRS_AX2 9
#define SPORCO_AMD_OUT_XRRS_B2 10
#define SPORCO_AMD_OUT_RGR 11    /* Parseval sum of GradWeight GHGf |Xf|^2 / (H W)  (twice RegGrad,
                                  * cbpdn.py:1204-1214; FLAG_GRADREG only)         */
#define SPORCO_AMD_OUT_CNSTR 12  /* sum (Pcn(Y) - Y)^2 of the consensus D-step (ccmod.py:888-894) */
#define SPORCO_AMD_OUT_CGIT 13   /* CG D-step: scipy's cg() status, 0 = converged, else MaxIter
                                    (what the reference records as XSlvCGIt, linalg.py:578) */
#define SPORCO_AMD_OUT_CGN 14    /* CG D-step: iterations actually run                     */
#define SPORCO_AMD_OUT_SN2 14    /* l1l1_iter: Parseval sum of |A^T u|^2 / (H W) (the slot of CGN, which
                                    no sparse coding call fills)                            */
#define SPORCO_AMD_OUT_R02 14    /* pdl1_iter: block 0's |AXnr - y0 - s|^2 (l1l1_iter keeps it in OUT_L21, which
                                    the joint class needs for its l2,1 sum)                 */
#define SPORCO_AMD_OUT_C2 12     /* tvl1 handles: ||c||^2 = ||S||^2 of the primal normaliser (the slot of CNSTR, which
                                    no TVL1Denoise call writes); formed once, when S is uploaded */
#define SPORCO_AMD_OUT_RGRX 15   /* l1l1_iter: what OUT_RGR is to ConvBPDNGradReg -- the two-block
                                    classes keep block 0's |AXnr|^2 in OUT_RGR                */
#define SPORCO_AMD_OUT_COUNT 16

/* One full ADMM iteration on device: xstep (cbpdn.py:267-281: rfftn(Y-U),
 * Sherman-Morrison solve linalg.py:232-297, irfftn), relax_AX, ystep
 * (prox_l1 prox/_lp.py:144-183 or prox_sl1l2 prox/_l21.py:51-88, NonNeg,
 * NoBndryCross), ustep (admm.py:434-437) and all reductions of
 * compute_residuals / eval_objfn.  Blocks until `out` is valid. */
int sporco_amd_csc_admm_iter(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                             double out[SPORCO_AMD_OUT_COUNT]);
/* Same, but leaves the sums in device memory at `out_dev` (double[16]) and does
 * not synchronise: used to all-reduce them over RCCL before reading. */
int sporco_amd_csc_admm_iter_dev(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                                 double *out_dev);

/* ---- Device-driven solve: the whole loop of ADMM.solve (sporco/admm/admm.py:331-377) ----
 * The residuals and tolerances (:462-486), the adaptive penalty parameter (:549-575) and the
 * stopping test (:375-377) are evaluated on the device at the end of every iteration, in the
 * precisions of the host code, and the next iteration's kernels read rho, lambda/rho and the
 * pending U scale from device memory: the host only enqueues launches (a few iterations
 * ahead) and reads the per-iteration records back when the run ends.  Iterates and statistics
 * are identical to those of the same number of sporco_amd_csc_admm_iter calls driven by the
 * host rule.  Available for the three-launch float32 path (query FUSED_ROWS; single-channel
 * dictionary; K <= 64, or 72 < K <= 256 on the slab column kernels -- not the 64 < K <= 72
 * tail form) without FLAG_XRRS / GRADREG / KEEP_X / FEVAL_Y; FLAG_JOINT is served when the
 * l2,1 row epilogue is (scalar weights, C <= 4, K a multiple of 32, no NoBndryCross /
 * AddMaskSim); otherwise the call returns SPORCO_AMD_EUNSUPPORTED and changes nothing.
 * With a `reduce` hook (image shards) the number of hook calls is a function of the
 * stopping iteration alone -- min(max_iter, stop + 1 + lookahead) -- so that every rank
 * issues the same number of collectives whatever its host's timing. */
#define SPORCO_AMD_EUNSUPPORTED (-5)
typedef struct {
    double abs_tol, rel_tol;        /* AbsStopTol, RelStopTol                                */
    double sqrt_nc, sqrt_nx;        /* sqrt of the constraint / primal sizes (admm.py:478-485) */
    double rho_tau, rho_mu, rho_xi; /* AutoRho Scaling, RsdlRatio, RsdlTarget (solver precision) */
    int32_t auto_rho, period, auto_scaling, std_residuals;
    int32_t need_residuals;         /* AutoRho enabled or not FastSolve                      */
    int32_t k0;                     /* iteration counter at entry (the solver's k)           */
    int32_t max_iter;               /* MaxMainIter                                            */
    int32_t lookahead;              /* iterations enqueued ahead of the last finished one; 0 = 3 */
} sporco_amd_admm_ctrl;
typedef struct {
    double sums[SPORCO_AMD_OUT_COUNT];
    double r, s, epri, edua;        /* residuals and tolerances of the iteration              */
    double rho, u_scale;            /* the values the iteration ran with                      */
    double seconds;                 /* device clock at the end of the iteration, from the start of the run */
    int32_t k, stop;
} sporco_amd_admm_record;
/* Optional hook between the local sums and the control update of every iteration: sum the 16
 * doubles at sums_dev over the ranks that hold the other images, in stream order (RCCL on the
 * handle's stream) or synchronously.  NULL for a single rank. */
typedef void (*sporco_amd_reduce_fn)(void *user, double *sums_dev);
int sporco_amd_csc_admm_run(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                            const sporco_amd_admm_ctrl *c, sporco_amd_admm_record *records,
                            int32_t *n_done, double *rho_out, double *u_scale_out,
                            sporco_amd_reduce_fn reduce, void *user);

/* Staged path, for callers that override individual ADMM steps
 * (SURVEY.md section 8(b) "monkey-patch hazard").  Each mirrors one method. */
int sporco_amd_csc_admm_xstep(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                              double out[SPORCO_AMD_OUT_COUNT]); /* GenericConvBPDN.xstep */
int sporco_amd_csc_admm_relax(sporco_amd_csc_t h, double rlx);   /* ADMMEqual.relax_AX    */
int sporco_amd_csc_admm_ystep(sporco_amd_csc_t h, const sporco_amd_admm_params *p);
int sporco_amd_csc_admm_ustep(sporco_amd_csc_t h, const sporco_amd_admm_params *p);
int sporco_amd_csc_admm_stats(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                              double out[SPORCO_AMD_OUT_COUNT]);
/* U *= s (the eager form of update_rho's `U /= rsf`, admm.py:573). */
int sporco_amd_csc_scale_u(sporco_amd_csc_t h, double s);

/* irfftn(sum_k Df * rfftn(V)) for V = state `var` (Y or X): reconstruct,
 * sporco/admm/cbpdn.py:373-380.  dst: real (H,W,C,N). */
int sporco_amd_csc_reconstruct(sporco_amd_csc_t h, int var, void *dst);
/* max |conj(Df) * Sf| for the default lambda rule, sporco/admm/cbpdn.py:573-578. */
int sporco_amd_csc_dhs_absmax(sporco_amd_csc_t h, double *out);

/* ---- PGM / FISTA steps (sporco/pgm/pgm.py:779-846, pgm/cbpdn.py:263-372) -- */

#define SPORCO_AMD_PGM_F 0       /* 0.5 * sum |Df.v - Sf|^2 in the unnormalised DFT domain
                                    (obfn_f, pgm/cbpdn.py:358-372)                       */
#define SPORCO_AMD_PGM_DFID 1    /* Parseval-weighted sum |Df.v - Sf|^2 / (H W), not halved
                                    (obfn_dfd, pgm/cbpdn.py:332-345)                     */
#define SPORCO_AMD_PGM_L1 2      /* sum |wl1 * X| of the last prox step (obfn_reg :347-356) */
#define SPORCO_AMD_PGM_HESS 3    /* sum |sum_k Df v|^2 = Re <v, hessian_f(v)> (:302-312)  */

#define SPORCO_AMD_PGM_RSDL 4    /* rfl2norm2(Xf - Yfprv) of pgm_iter (rsdl, pgm/cbpdn.py:314-320) */
#define SPORCO_AMD_PGM_FY 5      /* f at the Yf the step started from (pgm_iter)             */
#define SPORCO_AMD_PGM_LIN 6     /* sum Re(conj(Xf - Yf) grad f(Yf)) of a held pgm_iter
                                    (eval_linear_approx, pgm.py:886-894)                  */
#define SPORCO_AMD_PGM_DXY2 7    /* sum |Xf - Yf|^2, unweighted (backtrack.py:98-100)       */

/* One whole default-option FISTA iteration on device (float32, H and W in {128, 256, 512},
 * even K <= 64 or 72 < K <= 256; since round 6 also H, W in 16 x {10, 12, 14, 15, 18, 20, 21, 24, 25,
 * 27, 28, 30} with even K <= 64 -- SPORCO_AMD_QUERY_FUSED_PGM says which;
 * SPORCO_AMD_EINVAL otherwise -- compose the calls below instead):
 * on_iteration_start (Xfprv = Xf, Yfprv = Yf, by buffer rotation), PGMDFT.xstep
 * (grad_f at Yf, Vf = Yf - grad/L, X = prox_g(irfftn(Vf)), Xf = rfftn(X);
 * sporco/pgm/pgm.py:779-811) and PGMDFT.ystep with the caller's momentum factor
 * Yf = Xf + beta (Xf - Xfprv) (pgm.py:815-831).  out[PGM_F], out[PGM_DFID] (at the
 * new Xf; only with `want_stats`), out[PGM_L1], out[PGM_RSDL], out[PGM_FY].
 * The spectral iterates stay in an internal tile-major layout between such calls
 * and X is rebuilt on demand; any other entry point sees the reference layout. */
typedef struct {
    double L;        /* inverse step size                                   */
    double lmbda;    /* l1 weight (times a scalar L1Weight)                 */
    double beta;     /* momentum factor (t_prev - 1) / t                    */
    uint32_t flags;  /* SPORCO_AMD_FLAG_NONNEG | _NOBNDRY | _DMASK           */
    int32_t dH, dW;  /* filter support, for NOBNDRY                         */
    int32_t want_stats; /* evaluate the objective at the new Xf             */
    int32_t hold;    /* backtracking trial: also out[PGM_LIN], out[PGM_DXY2] (the terms of
                        Q_L, backtrack.py:95-100); the new iterates are kept aside and the
                        call may be repeated with another L from the same Yf until
                        sporco_amd_csc_pgm_commit adopts the last trial.  2: the same for a
                        rule that forms Yf itself (BacktrackRobust, backtrack.py:162-208: Yf
                        is set by sporco_amd_csc_lincomb before the call): no momentum
                        output is written, and after the commit VAR_YF holds the Yf of the
                        PREVIOUS iteration (what PGM.rsdl compares with, pgm.py:835-846,
                        pgm/cbpdn.py:314-320) and VAR_YFPRV the one this trial used        */
} sporco_amd_pgm_params;
int sporco_amd_csc_pgm_iter(sporco_amd_csc_t h, const sporco_amd_pgm_params *p,
                            double out[SPORCO_AMD_OUT_COUNT]);
/* Adopt the iterates of the last held pgm_iter (the buffer rotation of on_iteration_start,
 * pgm.py:835-846); SPORCO_AMD_EINVAL without one. */
int sporco_amd_csc_pgm_commit(sporco_amd_csc_t h);

/* GF = conj(Df) * (sum_k Df*v - Sf) for v = complex state `var` (grad_f,
 * pgm/cbpdn.py:263-279); out[PGM_F], out[PGM_DFID] receive f(v). */
int sporco_amd_csc_pgm_grad(sporco_amd_csc_t h, int var, double out[SPORCO_AMD_OUT_COUNT]);
/* f(v) only (no gradient written): out[PGM_F], out[PGM_DFID], out[PGM_HESS]. */
int sporco_amd_csc_pgm_eval(sporco_amd_csc_t h, int var, double out[SPORCO_AMD_OUT_COUNT]);
/* Proximal step of PGMDFT.xstep (pgm.py:800-803): Vf = Yf - GF/L;
 * X = prox_g(irfftn(Vf)) with prox_l1(., lmbda/L * wl1) + NonNeg/NoBndry
 * (pgm/cbpdn.py:288-300); Xf = rfftn(X); out[PGM_L1] = ||wl1 X||_1. */
int sporco_amd_csc_pgm_prox_step(sporco_amd_csc_t h, double L, double lmbda, uint32_t flags,
                                 int32_t dH, int32_t dW, double out[SPORCO_AMD_OUT_COUNT]);
/* dst = a*va + b*vb + c*vc over complex state arrays (vb, vc may be -1):
 * the momentum step Yf = Xf + beta (Xf - Xfprv) (PGMDFT.ystep, pgm.py:815-831),
 * robust-backtracking and monotone combinations (backtrack.py:181-200).  Between fused
 * iterations (pgm_iter) a combination of iterates / scratch spectra (VAR_T0..T2) into VAR_YF
 * or a scratch spectrum is formed in the internal tile-major layout, like pair_stats of such
 * operands: the iterates stay where the fused kernels want them. */
int sporco_amd_csc_lincomb(sporco_amd_csc_t h, int dst, double a, int va, double b, int vb,
                           double c, int vc);
/* Statistics of d = va - vb (vb may be -1) and g = vg (may be -1):
 *   out[0] = rfl2norm2(d) (half-spectrum Parseval, / (H W): rsdl, pgm/cbpdn.py:314-320)
 *   out[1] = sum Re(conj(d) g)   (eval_linear_approx, pgm.py:886-894)
 *   out[2] = sum |d|^2           out[3] = sum |g|^2 */
int sporco_amd_csc_pair_stats(sporco_amd_csc_t h, int va, int vb, int vg,
                              double out[SPORCO_AMD_OUT_COUNT]);
/* Residual spectra for the step-size policies (sporco/pgm/stepsize.py:67-145), so that they run
 * beside the fused iteration without an X-sized gradient array: the gradient at v is
 * g = conj(Df) e with e = sum_m Df v - Sf (grad_f, pgm/cbpdn.py:263-279), signal sized.
 * pgm_resid stores e of the X-sized spectrum `var` in slot 0..3 (one read pass; shapes the fused
 * kernels serve, single-channel dictionary).  pgm_resid_stats: with d1 = e[a] - e[b],
 * d2 = e[c] - e[d] (b, c, d may be -1; c = -1: d2 = d1) and G = sum_m |Df|^2,
 *   out[0] = sum G |d1|^2        = <g1, g1>                (StepSizePolicyCauchy den, BB num)
 *   out[1] = sum G^2 |d1|^2      = <g1, hessian_f(g1)>     (StepSizePolicyCauchy num, :84-87)
 *   out[2] = sum Re(conj(d2) d1) = <dx, dg> for iterates whose residuals differ by d2 and
 *            gradients by conj(Df) d1                      (StepSizePolicyBB den, :137-141)
 * summed over the rfftn arrays as they are (no Parseval weights), as the reference's np.sum does. */
int sporco_amd_csc_pgm_resid(sporco_amd_csc_t h, int var, int slot);
int sporco_amd_csc_pgm_resid_stats(sporco_amd_csc_t h, int a, int b, int c, int d,
                                   double out[SPORCO_AMD_OUT_COUNT]);
/* cplx_var = rfftn(real_var) / real_var = irfftn(cplx_var) between X-sized state
 * arrays (Xf = rfftn(X), pgm/cbpdn.py:231; Zf = rfftn(Z), pgm/ccmod.py:264-279). */
int sporco_amd_csc_fft_var(sporco_amd_csc_t h, int real_var, int cplx_var);
int sporco_amd_csc_ifft_var(sporco_amd_csc_t h, int cplx_var, int real_var);
/* dst = src (state copy of equal size: on_iteration_start, pgm.py:835-846). */
int sporco_amd_csc_copy(sporco_amd_csc_t h, int dst_var, int src_var);

/* ---- dictionary update (pgm.ccmod.ConvCnstrMOD, sporco/pgm/ccmod.py:139-404) --- */

/* ZF = rfftn(real state `var`): setcoef (pgm/ccmod.py:264-279).  With a handle
 * shared between the X-step and the D-step, var = VAR_Y keeps the coefficient
 * maps on the device (DictLearn.post_xstep, dictlrn/dictlrn.py:379-382).
 * Handles of sporco_amd_csc_create_mc: var = VAR_CX hands over coefficient maps that carry the
 * dictionary's channels, in the layout of that array (H, W, N, Cd, K) -- Cd single-channel
 * updates sharing the penalty / step size (the reference's broadcasting:
 * tests/admm/test_ccmod.py:278-295); VAR_CX is zeroed afterwards.  Served by
 * sporco_amd_csc_ccmod_grad, sporco_amd_csc_masked_grad (dstep) and sporco_amd_csc_cns_iter. */
int sporco_amd_csc_ccmod_setcoef(sporco_amd_csc_t h, int var);
/* DGF = sum_n conj(Zf) (sum_k Zf*v - Sf) for the D-sized complex state `var`
 * (grad_f, pgm/ccmod.py:295-309: inner over axisM then over axisK, channels of
 * a single-channel dictionary folded into the image axis); out[PGM_F],
 * out[PGM_DFID], out[PGM_HESS] as for pgm_grad. */
int sporco_amd_csc_ccmod_grad(sporco_amd_csc_t h, int var, double out[SPORCO_AMD_OUT_COUNT]);
/* Same sums without writing the gradient (obfn_f / obfn_dfd, ccmod.py:340-372). */
int sporco_amd_csc_ccmod_eval(sporco_amd_csc_t h, int var, double out[SPORCO_AMD_OUT_COUNT]);
/* DVF = DYF - DGF/L; DX = Pcn(irfftn(DVF)); DXF = rfftn(DX)  (PGMDFT.xstep with
 * prox_g = Pcn, pgm/ccmod.py:320-323; cnvrep.Pcn, sporco/cnvrep.py:868-913:
 * crop to (dH,dW), zero-pad, optional zero-mean, unit l2 norm per filter). */
int sporco_amd_csc_ccmod_prox_step(sporco_amd_csc_t h, double L, int32_t dH, int32_t dW,
                                   int32_t zero_mean);
/* out[0] = ||Pcn(DX) - DX||_2  (obfn_cns, pgm/ccmod.py:350-355). */
int sporco_amd_csc_ccmod_cnstr(sporco_amd_csc_t h, int32_t dH, int32_t dW, int32_t zero_mean,
                               double out[SPORCO_AMD_OUT_COUNT]);
/* dst(dH,dW,K) = DX[:dH,:dW,:]  (getdict(crop=True), pgm/ccmod.py:283-291). */
int sporco_amd_csc_ccmod_getdict(sporco_amd_csc_t h, int32_t dH, int32_t dW, void *dst);
/* Df = DXF and its Sherman-Morrison denominators, device to device: the
 * X-step's setdict(dstep.getdict()) of DictLearn.post_dstep without PCIe
 * (dictlrn/dictlrn.py:386-389, admm/cbpdn.py:242-256). */
int sporco_amd_csc_setdict_from_dstep(sporco_amd_csc_t h, int32_t dH, int32_t dW);
/* out[0] = sum |v| over the real state `var` (RegL1 of DictLearn.evaluate,
 * dictlrn/cbpdndl.py:519). */
/* ---- masked data fidelity (pgm.cbpdn.ConvBPDNMask, sporco/pgm/cbpdn.py:387-506; ----------
 * pgm.ccmod.ConvCnstrMODMask, sporco/pgm/ccmod.py:408-604) --------------------------------
 * W (cnvrep.mskWshape layout, broadcastable against (H,W,C,N,1)); NULL removes it. */
int sporco_amd_csc_set_data_mask(sporco_amd_csc_t h, const void *w, const int64_t shape[5]);
/* Gradient of (1/2)||W (sum_m d_m * x_m - s)||^2: residual -> irfftn -> W^2 -> rfftn -> adjoint.
 * dstep == 0: `var` is a coefficient spectrum, the gradient goes to SPORCO_AMD_VAR_GF
 * (conj(Df) .), pgm/cbpdn.py:454-477; dstep != 0: `var` is a dictionary spectrum, the gradient
 * goes to SPORCO_AMD_VAR_DGF (sum over images of conj(Zf) .), pgm/ccmod.py:552-575.
 * write_grad == 0: evaluation only -- out[SPORCO_AMD_PGM_DFID] = sum (W R)^2 (spatial domain,
 * twice the data fidelity term) and out[SPORCO_AMD_PGM_F] = (1/2) sum |rfftn(W R)|^2 over the
 * half spectrum (the value backtracking compares, :493-506).  With write_grad != 0 only
 * out[SPORCO_AMD_PGM_DFID] is filled.
 * write_grad == 2 (dstep only in practice): as 1 with the residual weighted by W once instead of
 * W^2 -- the gradient of OnlineConvBPDNMaskDictLearn.dstep (onlinecdl.py:574-590). */
int sporco_amd_csc_masked_grad(sporco_amd_csc_t h, int var, int32_t dstep, int32_t write_grad,
                               double out[SPORCO_AMD_OUT_COUNT]);

/* ---- ADMM consensus dictionary update (admm.ccmod.ConvCnstrMOD_Consensus, -----------
 * sporco/admm/ccmod.py:605-908 on admm.ADMMConsensus, sporco/admm/admm.py:1441-1707) ----
 * One dictionary copy X_n and dual U_n per image (VAR_CX, VAR_CU), consensus variable
 * Y = VAR_DX (its spectrum VAR_DXF is kept current, so sporco_amd_csc_ccmod_getdict and
 * sporco_amd_csc_setdict_from_dstep serve this D-step too).  Coefficient maps come from
 * sporco_amd_csc_ccmod_setcoef.  Handles of sporco_amd_csc_create_mc (a dictionary with Cd > 1
 * channels, ccmod.py:696-698): VAR_CX / VAR_CU are (H, W, N, Cd, K) -- one (Cd, K) block per
 * image --, VAR_DX is (H, W, Cd, K); both the plain and the mask-decoupled update serve them. */
/* Y = Y0 (real (H,W,K), zero-padded filters) or 0; U_n = Y0 / rho or 0 (uinit, ccmod.py:734-742). */
int sporco_amd_csc_cns_init(sporco_amd_csc_t h, const void *Y0, double rho);
typedef struct {
    double rho;      /* penalty parameter                                               */
    double rlx;      /* RelaxParam                                                      */
    double u_scale;  /* pending U /= rsf, as in sporco_amd_admm_params                  */
    uint32_t flags;  /* SPORCO_AMD_FLAG_RESID | SPORCO_AMD_FLAG_OBJ                     */
    int32_t dH, dW;  /* filter support of the constraint set                            */
    int32_t zero_mean;
    int32_t mask_dcpl;  /* 1: ConvCnstrMODMaskDcpl_Consensus (sporco/admm/ccmodmd.py:766-1083), the
                           consensus update with the masked data fidelity split off into a
                           signal-sized block (Y1, U1 = VAR_DMY0, VAR_DMU0; mask by
                           sporco_amd_csc_set_data_mask; state by sporco_amd_csc_cns_md_init).
                           out then holds: R2 = sum_n |X_n - Y|^2, AX2 = sum_n |X_n|^2, Y2 = |Y|^2,
                           U2 = sum_n |U_n|^2, S2 = Parseval sum of |rfftn(U_n) + conj(Zf_n)
                           rfftn(U1_n)|^2 / (H W) (the dual residual's A^T u, :993-996), and for
                           the signal-sized block XRRS_D2 = |AX1nr - Y1 - S|^2, XRRS_AX2 =
                           |AX1nr|^2, XRRS_B2 = |Y1|^2, CGIT = |U1|^2; DFID = |W irfftn(sum_m Zf Yf
                           - Sf)|^2 (:961-970), CNSTR as for the unmasked update.              */
    int32_t phase;      /* image shards over ranks (one process per GPU): 0 = the whole iteration;
                           1 = up to the local mean over this rank's images of alpha X_n +
                           (1 - alpha) Y + U_n, left in the buffer of sporco_amd_csc_cns_mean_ptr;
                           2 = the rest (constraint projection, dual update, sums), after the
                           caller has made that buffer the mean over ALL images -- the consensus
                           average is the one array all-reduce of this update (SURVEY.md 8(e);
                           reference: admm.py:1585-1591).  The X-sized sums of phase 2 are
                           rank-local and are added over the ranks by the caller; S2, Y2 and
                           CNSTR of the unmasked update are dictionary sized (identical on every
                           rank). */
} sporco_amd_cns_params;
/* The dictionary-sized real buffer (H, W, K) that holds the consensus mean between the two
 * phases, and its element count. */
int sporco_amd_csc_cns_mean_ptr(sporco_amd_csc_t h, void **ptr_dev, int64_t *count);
/* State of the masked consensus update: the real signal S (H,W,C,N) kept on the device, Y1 = U1 = 0
 * (ccmodmd.py:869-871).  Call after sporco_amd_csc_cns_init. */
int sporco_amd_csc_cns_md_init(sporco_amd_csc_t h, const void *S);
/* One iteration: xstep per image by Sherman-Morrison (ccmod.py:766-778), relax_AX
 * (admm.py:1608-1616), ystep Y = Pcn(mean_n(AX_n + U_n)) (admm.py:1585-1591, ccmod.py:832-835),
 * ustep.  out: R2 = sum_n |X_n - Y|^2, S2 = |Y - Yprev|^2, AX2 = sum_n |X_n|^2, Y2 = |Y|^2,
 * U2 = sum_n |U_n|^2 (the host applies the sqrt(Nb) and rho factors of admm.py:1673-1707),
 * DFID = Parseval sum of |sum_m Zf Yf - Sf|^2 / (H W) and CNSTR, both evaluated at Y
 * (fEvalX False, gEvalY True: the class defaults, ccmod.py:853-894). */
int sporco_amd_csc_cns_iter(sporco_amd_csc_t h, const sporco_amd_cns_params *p,
                            double out[SPORCO_AMD_OUT_COUNT]);

/* ---- ADMM with mask decoupling: sporco.admm.cbpdn.ConvBPDNMaskDcpl (cbpdn.py:2066-2283) on
 * ConvTwoBlockCnstrnt (:1401-1826) / ADMMTwoBlockCnstrnt (admm.py:989-1437) ------------------
 * Constraint [D; I] x - [y0; y1] = [s; 0].  Block 1 (coefficient sized) lives in the ADMM state
 * VAR_Y / VAR_U, block 0 (signal sized) in VAR_MY0 / VAR_MU0; X / Xf as for ConvBPDN.  The mask W
 * is the data mask of sporco_amd_csc_set_weights(which = 3); single-channel dictionaries. */
/* S: the real signal (H,W,C,N) (the handle otherwise keeps only its spectrum); zeroes Y, U. */
int sporco_amd_csc_mdcpl_init(sporco_amd_csc_t h, const void *S);
/* One iteration.  params: rho, lmbda, rlx, u_scale, flags (NONNEG | NOBNDRY | OBJ | XRRS |
 * GEVAL_Y = AuxVarObj), dH, dW.  xstep (:1610-1643, rho-free), relax_AX (:1664-1677), ystep
 * (:2236-2247, :1647-1660), ustep.  out, block 1 sums in the ADMM slots and block 0 sums beside
 * them (the host adds the pairs): R2 / L21 = |AXnr - y - c|^2, AX2 / RGR = |AXnr|^2, Y2 / CNSTR
 * = |y|^2, U2 / CGIT = |u|^2; S2 = |A^T u|^2 = |irfftn(conj(Df) rfftn(u0)) + u1|^2 (:1814-1818);
 * DFID = |W g0|^2 (twice the data fidelity, :2262-2268), L1 = |wl1 g1|_1; XRRS sums. */
int sporco_amd_csc_mdcpl_iter(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                              double out[SPORCO_AMD_OUT_COUNT]);

/* ---- l1 data fidelity with l1 and gradient regularisation: sporco.admm.cbpdn.ConvL1L1Grd
 * (cbpdn.py:2488-2774) on the state of the mask-decoupling calls above (sporco_amd_csc_mdcpl_init;
 * mask, L1Weight and GradWeight through set_data_mask / set_l1_weight / set_grad_weight).
 * One iteration.  params as for mdcpl_iter plus mu (SPORCO_AMD_FLAG_GRADREG is accepted and implied).
 * xstep (:2676-2699): (D^H D + (mu / rho) Wgrd GHG + I) x = D^H (y0 - u0 + s) + y1 - u1; ystep
 * (:2716-2726): y0 = soft(AX0 + u0 - s, W / rho), y1 as for mdcpl_iter; ustep.  out as for mdcpl_iter,
 * except: DFID = sum |W g0| (the data fidelity itself, :2744-2749); RGRX = Parseval sum of GradWeight
 * GHGf |Xf|^2 / (H W) (twice RegGrad); S2 = |A^T (Yprev - Y)|^2 and SN2 = |A^T u|^2, A^T v =
 * irfftn(conj(Df) rfftn(v0)) + v1 (:2753-2763), both with SPORCO_AMD_FLAG_RESID only.  Generic
 * transforms on every shape; single- and multi-channel dictionaries (at most 8 channels). */
int sporco_amd_csc_l1l1_iter(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                             double out[SPORCO_AMD_OUT_COUNT]);

/* ---- l1 objective inside l2 balls: sporco.admm.cbpdn.ConvMinL1InL2Ball (cbpdn.py:1830-2060),
 * minimise sum_m ||x_m||_1 such that ||sum_m d_m * x_m - s_k||_2 <= epsilon for every channel and image
 * k, on the state of the mask-decoupling calls above (sporco_amd_csc_mdcpl_init; L1Weight through
 * set_l1_weight; the data mask is not read).
 * One iteration.  params as for mdcpl_iter; EPSILON TRAVELS IN params.mu, which mdcpl_iter leaves unused
 * (SPORCO_AMD_FLAG_GRADREG is refused, as there); lmbda = 1 gives block 1 the reference's threshold
 * wl1 / rho.  xstep, relax_AX, block 1 and ustep as mdcpl_iter, on the same two paths (the
 * register-resident kernels where mdcpl_iter takes them, else the generic chain; SPORCO_AMD_MD_GENERIC
 * forces the latter); ystep of block 0 (:2024-2026): y0 = proj_l2(AX0 + u0 - s, epsilon), one ball per
 * channel and image with the norm over the image plane (csrc/csc_ball.h).  out as for mdcpl_iter, except:
 * DFID, which this class has no other use for, holds the constraint measure sum_p max(g_p - epsilon, 0)^2
 * over the planes p, g_p the plane norm of AXnr0 - s, or of the new y0 with GEVAL_Y -- the square of the
 * reference's ||proj_l2(g0) - g0|| (:2034-2040). */
int sporco_amd_csc_ball_iter(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                             double out[SPORCO_AMD_OUT_COUNT]);

/* ---- ConvBPDN inside l1 balls: sporco.admm.cbpdn.ConvBPDNProjL1 (cbpdn.py:1220-1395),
 * minimise (1/2) ||sum_m d_m * x_m - s||^2 such that sum_m ||x_m||_1 <= gamma for every image, on the
 * state of sporco_amd_csc_admm_iter (VAR_X, VAR_Y, VAR_U).
 * One iteration: the x step of admm_iter with lmbda = 0 (the same launches as sporco_amd_csc_admm_xstep),
 * the threshold search of the projection of AX + U onto one l1 ball per image (csrc/csc_projl1.h: a few
 * streaming reduction passes, no sort), and one pass that relaxes, shrinks by the image's threshold,
 * applies NonNegCoef / NoBndryCross and updates the dual variable.  params as for admm_iter (lmbda and mu
 * are not read).  out as for admm_iter, except:
 *   OUT_L1, which this class has no other use for, holds the squared constraint measure
 *     sum_n sum_i min(|g_i|, tau_n(g))^2 = ||proj_l1(g) - g||^2, g = X, or the new Y with GEVAL_Y
 *     (:1385-1395); it takes a threshold search of its own and is formed with FLAG_OBJ only;
 *   OUT_CGIT is the number of images whose search had not ended when the call returned (always 0: the
 *     call enqueues further passes until every search has ended and never applies another threshold);
 *   OUT_CNSTR is the same count for the constraint measure's search (always 0 on return, likewise);
 *   OUT_CGN / OUT_RGRX are the search passes the slowest image took (y step / constraint measure).
 * SPORCO_AMD_EUNSUPPORTED: a volume handle, a handle with a communicator, complex data. */
int sporco_amd_csc_projl1_iter(sporco_amd_csc_t h, const sporco_amd_admm_params *p, double gamma,
                               double out[SPORCO_AMD_OUT_COUNT]);

/* ---- ADMM with inhibition: sporco.admm.cbpdnin.ConvBPDNInhib (cbpdnin.py:28-352) -------------
 * The iteration is the ConvBPDN one (sporco_amd_csc_admm_iter, or the staged calls) with an array
 * l1 weight that sporco_amd_csc_inhib_update rewrites after every iteration: the thresholds
 * T = lmbda wl1 + mu wml + gamma wms live in the handle's L1-weight array, so the y step is called
 * with params.lmbda = 1 and needs X written (SPORCO_AMD_FLAG_KEEP_X, no FLAG_NO_X).
 *
 * The reference's window (cbpdnin.py:253-283) is separable: taps_rows act along H, taps_cols along
 * W, tap t at offset t - ntaps / 2, circularly (a convolution, not a correlation: the taps of
 * scipy's periodic windows are not symmetric).  1 <= ntaps_rows <= H, 1 <= ntaps_cols <= W; a
 * folded dimN = 1 problem (H = 1) passes taps_rows = {1}.  Taps and Wg are doubles whatever the
 * handle's dtype.
 *
 * setup: Wg (Ng, K) row-major grouping matrix, or NULL / Ng = 0: no lateral term.  want_self != 0:
 * the self-inhibition weights exist.  The L1-weight array set before (sporco_amd_csc_set_l1_weight;
 * none: 1) becomes wl1 of the formula above; the handle's L1-weight array is replaced by T,
 * initialised to lmbda wl1 (wml = wms = 0, cbpdnin.py:229); VAR_WML / VAR_WMS are zeroed (only the
 * live ones are allocated).  A later sporco_amd_csc_set_l1_weight ends the inhibition state.
 * Single-channel dictionaries, no volume handles. */
int sporco_amd_csc_inhib_setup(sporco_amd_csc_t h, const double *Wg, int32_t Ng,
                               const double *taps_rows, int32_t ntaps_rows, const double *taps_cols,
                               int32_t ntaps_cols, int32_t want_self, double lmbda);
typedef struct {
    double lmbda;    /* lmbda (times a scalar L1Weight)                                   */
    double mu;       /* lateral term; > 0 updates VAR_WML (needs Wg), else it is left out */
    double gamma;    /* self term; > 0 updates VAR_WMS (needs want_self), else left out   */
    double smooth;   /* SmoothWeight: w <- smooth w + (1 - smooth) w_new                  */
    uint32_t flags;  /* SPORCO_AMD_FLAG_GEVAL_Y: the sums are taken against Y, else X     */
} sporco_amd_inhib_params;
/* One launch (profile slot "inhib_update"): c = h (*) |X| per map (cbpdnin.py:310-317),
 * lat_m = sum_g Wg[g,m] (sum_n Wg[g,n] c_n) - (sum_g Wg[g,m]) c_m (:319-320),
 * self_m = c_m - h(0) |X_m| (:330-331), the smoothing of both (:322-323, :333-334), the new T, and
 * out[SPORCO_AMD_OUT_L1] = sum |wl1 G|, out[SPORCO_AMD_OUT_L21] = sum |wml G|,
 * out[SPORCO_AMD_OUT_RGR] = sum |wms G| with the updated weights (obfn_reg, :341-352); the other
 * slots of out are zero. */
int sporco_amd_csc_inhib_update(sporco_amd_csc_t h, const sporco_amd_inhib_params *p,
                                double out[SPORCO_AMD_OUT_COUNT]);

/* ---- ADMM with total-variation terms: sporco.admm.cbpdntv.ConvBPDNScalarTV (cbpdntv.py:31-571)
 * and ConvBPDNVectorTV (:577-727) ------------------------------------------------------------------
 * The constraint is (Gamma_0; Gamma_1; I) x = (y_0; y_1; y_L) (:56-65): Y and U have three blocks,
 * kept block after block in VAR_TVY / VAR_TVU.  The reference's gradient filters are the two-tap
 * [1, -1] (signal.gradient_filters), so G_i x = x - (its circular predecessor along axis i) and
 * G_i^T v = v - (its circular successor): the kernels below are stencils, not transforms.
 *
 * One iteration, driven by the caller:
 *   1. sporco_amd_csc_tv_xstep, which is sporco_amd_csc_admm_xstep with SPORCO_AMD_FLAG_GRADREG |
 *      SPORCO_AMD_FLAG_KEEP_X, params.mu = params.rho: the system (D^H D + rho Wtv^2 GHGf + rho) x = D^H s + rho A^T (Y - U) (:277-298)
 *      is ConvBPDNGradReg's with the grad-weight array Wtv^2 (tv_setup sets it), and the handle's own
 *      VAR_Y / VAR_U hold P = A^T Y and Q = A^T U (tv_adjoint writes them), so the x step's
 *      rfftn(Y - u_scale U) is the reference's right-hand side.  LinSolveCheck: its FLAG_XRRS sums.
 *   2. sporco_amd_csc_tv_ystep;  3. sporco_amd_csc_tv_adjoint.
 *
 * setup: tvw holds n = 1 (scalar TVWeight) or n = K weights (:213-218), doubles whatever the
 * handle's dtype; vector_tv != 0 selects ConvBPDNVectorTV's norm.  Replaces the handle's
 * grad-weight array.  VAR_TVY / VAR_TVU start at zero; after uploading a Y0 / U0 into them call
 * tv_adjoint once.  Single-channel dictionaries, no volume handles. */
int sporco_amd_csc_tv_setup(sporco_amd_csc_t h, const double *tvw, int32_t n, int32_t vector_tv);
/* The x step of the TV classes on VAR_Y = A^T Y, VAR_U = A^T U: sporco_amd_csc_admm_xstep with
 * FLAG_GRADREG | FLAG_KEEP_X and mu = rho (set here; params.mu is ignored) when every filter has the
 * same TVWeight.  With different weights per filter the reference hands its diagonal to
 * linalg.solvedbi_sm (cbpdntv.py:290-292), whose formula solves the system only for a diagonal that
 * is constant along the filter axis; the reference's arithmetic is reproduced then (generic chain,
 * profile slot "sm_solve"), and FLAG_XRRS reports the residual the reference's LinSolveCheck reports.
 * out[DFID] (FLAG_OBJ without FLAG_FEVAL_Y) and out[XRRS_*] as sporco_amd_csc_admm_xstep. */
int sporco_amd_csc_tv_xstep(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                            double out[SPORCO_AMD_OUT_COUNT]);
/* One launch (profile slot "tv_ystep") after the x step, reading X: relax_AX (:542-559) with
 * AXnr = (Wtv G_0 x, Wtv G_1 x, x); Y_{0,1} = prox_l2(AX_{0,1} + U_{0,1}, mu / rho) over the two
 * gradient components of a filter (:314-321) or, vector TV, over the components and all filters of a
 * pixel of one channel and signal (:707-715); Y_L = prox_l1(AX_L + U_L, (lmbda / rho) wl1);
 * U += AX - Y (admm.py:434-437).  Uses params.rho, lmbda, mu, rlx, u_scale (applied to VAR_TVU as it
 * is read) and the flags GEVAL_Y, OBJ, FEVAL_Y.  out[R2] = sum (AXnr - Y)^2, out[AX2] = sum AXnr^2,
 * out[Y2] = sum Y^2 over the three blocks (admm.py:722-775), out[L1] = sum |wl1 g_L|, out[L21] =
 * sum sqrt(sum g_{0,1}^2) (obfn_reg, :439-446 / :719-727; g is Y with FLAG_GEVAL_Y, else AXnr), and
 * with FLAG_OBJ | FLAG_FEVAL_Y out[DFID] at rfftn(y_L) (:325-331); the other slots are zero. */
int sporco_amd_csc_tv_ystep(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                            double out[SPORCO_AMD_OUT_COUNT]);
/* One launch (profile slot "tv_adjoint"): VAR_Y <- p = y_L + Wtv sum_i G_i^T y_i (cnst_AT, :470-520),
 * VAR_U <- q = u_scale (the same of U); out[S2] = sum (p - previous VAR_Y)^2 -- the dual residual
 * ||A^T (Y - Yprev)||^2 of admm.py:745-752 without its rho --, out[U2] = sum q^2 (:765-775). */
int sporco_amd_csc_tv_adjoint(sporco_amd_csc_t h, double u_scale, double out[SPORCO_AMD_OUT_COUNT]);

/* ---- ConvBPDNRecTV (sporco/admm/cbpdntv.py:733-1356): total variation of the reconstruction ----
 * The constraint is (I; Gamma_0; Gamma_1) x = (y0; y1), Gamma_i x = G_i sum_m w_m d_m * x_m.  The
 * coefficient blocks of Y and U are the handle's VAR_Y / VAR_U, the gradient blocks VAR_RTVY1 /
 * VAR_RTVU1, (H, W, C, N, 2) with the gradient component fastest.  The reference's rank-3 iterated
 * Sherman-Morrison has two collinear rows per frequency: the system is ConvBPDN's rank-one system
 * with the scale 1 + rho w^2 GHGf for equal TVWeights and a rank-two (2 x 2 Woodbury) system for
 * different ones; G_i and G_i^T are stencils on signal-shaped maps (csrc/csc_rtv.h).
 * An iteration is rtv_xstep, rtv_ystep, rtv_dual, driven from the host.  Single-channel real
 * dictionaries, H, W >= 2, no volume handles; every K-map transform is the generic chain's.
 * tvw: n = 1 (scalar) or n = K weights.  rtv_setup also computes the spectra of the blocks the
 * handle holds; after uploading a Y0 / U0 into the four block variables call rtv_dual once. */
int sporco_amd_csc_rtv_setup(sporco_amd_csc_t h, const double *tvw, int32_t n);
/* Profile slot "rtv_solve": Xf from rfftn(y0), rfftn(u0) and the adjoint-map spectra that the last
 * rtv_dual left (params.u_scale applied to the U side), X = irfftn(Xf), and the weighted
 * reconstruction irfftn(sum_m w_m Df_m Xf_m) for the y step.  out[DFID] with FLAG_OBJ (unless
 * FLAG_FEVAL_Y), out[XRRS_*] with FLAG_XRRS (the residual of the system actually solved). */
int sporco_amd_csc_rtv_xstep(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                             double out[SPORCO_AMD_OUT_COUNT]);
/* Profile slot "rtv_ystep" (two launches: coefficient block, gradient block): relax_AX (:1319-1339),
 * y0 = prox_l1(. , (lmbda / rho) L1Weight), y1 = prox_l2 over (channel, component) per pixel with
 * mu / rho (:1098-1106), U += AX - Y.  out[R2], out[AX2], out[Y2] over both blocks, out[L1] =
 * sum |L1Weight g0|, out[L21] = sum sqrt(sum_{c,i} g1^2), g at Y with FLAG_GEVAL_Y, else at AXnr. */
int sporco_amd_csc_rtv_ystep(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                             double out[SPORCO_AMD_OUT_COUNT]);
/* Profile slot "rtv_dual" (+ the transform slots): the spectra of the blocks as they stand, out[S2] =
 * ||A^T (Y - Yprev)||^2 (Yprev: the blocks at the previous call), out[U2] = ||A^T U||^2 (admm.py:722-775
 * without rho), and with FLAG_OBJ | FLAG_FEVAL_Y out[DFID] at rfftn(y0).  Uses params.flags only. */
int sporco_amd_csc_rtv_dual(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                            double out[SPORCO_AMD_OUT_COUNT]);

/* ---- ConvProdDictBPDN / ConvProdDictBPDNJoint (sporco/admm/pdcsc.py:28-287): product dictionary ----
 * minimise (1/2) || D X B^T - S ||^2 + lambda ||X||_1 (+ mu ||X||_2,1 over the channel axis), D a
 * single-channel convolutional dictionary, B (Cs x Cb) a standard dictionary over the channel axis.
 * The handle is created with C = Cb channels (those of the coefficient maps) and its signal slot is
 * given the mixed signal S (B Q), (H, W, Cb, N), through sporco_amd_csc_set_signal, B^T B = Q Gamma Q^T.
 * Y, U, X, the weights, admm_relax / admm_ystep (FLAG_JOINT for the joint class) / admm_ustep /
 * admm_stats are the handle's own; the x step, the data fidelity at Y and the reconstruction are the
 * calls below (csrc/csc_pd.h).  Single-channel real dictionaries, Cb <= 16, no volume handles; every
 * K-map transform is the generic chain's; the iteration is driven from the host.
 * pd_setup: B (cs x Cb) and Q (Cb x Cb) row-major, gamma (Cb) >= 0, S the cs-channel signal
 * (H, W, cs, N) in the handle's dtype.  A second call replaces the state of the first. */
int sporco_amd_csc_pd_setup(sporco_amd_csc_t h, const double *B, const double *Q, const double *gamma,
                            const void *S, int32_t cs);
/* Profile slot "pd_solve" (+ the transform slots): zf = rfftn(Y - u_scale U); per frequency and image
 * zh = Q^T z, xh_c' = (b - conj(d) gamma_c' (d.b) / (rho + gamma_c' |d|^2)) / rho with b = conj(d) sh_c' +
 * rho zh_c', x = Q xh; X = irfftn(Xf).  K even with K / 2 a power of two <= 64 and Cb <= 8: the system
 * in registers, sums by wave shuffles; otherwise one thread per system.  out[DFID] = ||B Df.Xf - Sf||^2
 * with FLAG_OBJ (unless FLAG_FEVAL_Y), out[XRRS_*] with FLAG_XRRS (in eigen-coordinates). */
int sporco_amd_csc_pd_xstep(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                            double out[SPORCO_AMD_OUT_COUNT]);
/* Profile slot "pd_recon": out[DFID] = ||B sum_m Df_m rfftn(var)_m - Sf||^2 (half-spectrum Parseval) of
 * a real K-map variable -- the data fidelity at Y when fEvalX is off. */
int sporco_amd_csc_pd_dfid(sporco_amd_csc_t h, int var, double out[SPORCO_AMD_OUT_COUNT]);
/* out (H, W, cs, N) = irfftn(B sum_m Df_m rfftn(var)_m), host memory. */
int sporco_amd_csc_pd_reconstruct(sporco_amd_csc_t h, int var, void *out);

/* ---- product dictionary with l1 data fidelity and gradient regularisation:
 * sporco.admm.pdcsc.ConvProdDictL1L1Grd / ConvProdDictL1L1GrdJoint (pdcsc.py:293-701) on a handle as for
 * the pd calls above (C = Cb channels, single-channel dictionary; L1Weight and GradWeight through
 * set_l1_weight / set_grad_weight).  The two-block constraint is y0 = D X B^T - S (cs channels), y1 = X:
 * block 1 lives in VAR_Y / VAR_U, block 0 in buffers of cs N planes that the handle owns.
 * sporco_amd_csc_pdl1_setup: what sporco_amd_csc_pd_setup does, plus the mask (NULL: none; else an array
 * (H, W, cs, N) of the handle's dtype) and block 0, which the first call creates at zero and a later
 * call keeps (a change of B or S between two solves).  sporco_amd_csc_pd_reconstruct serves these
 * classes too. */
int sporco_amd_csc_pdl1_setup(sporco_amd_csc_t h, const double *B, const double *Q, const double *gamma,
                              const void *S, int32_t cs, const void *mask);
/* Host copy of block 0: which = 0 (y0) or 1 (u0, without a pending u_scale), (H, W, cs, N); upload != 0
 * writes the device array from `buf`, else `buf` receives it. */
int sporco_amd_csc_pdl1_block0(sporco_amd_csc_t h, int32_t which, int32_t upload, void *buf);
/* One iteration.  params as for l1l1_iter; with SPORCO_AMD_FLAG_JOINT block 1 is the l2,1 shrinkage over
 * the channel axis with threshold lmbda / rho and no l1 term (prox_sl1l2(., 0, .), :681-692).
 * xstep (:509-540): per eigen-channel c' of B^T B = Q Gamma Q^T, (gamma_c' conj(d) d^T + diag(1 + (mu / rho)
 * Wgrd GHG)) xh_c' = conj(d) ((BQ)^T z0)_c' + (Q^T z1)_c', x = Q xh (profile slot "pdl1_solve"), which also
 * writes the block-0 constraint spectrum (BQ)(d . xh); then the block steps of l1l1_iter.  out as for
 * l1l1_iter, except: block 0's |AXnr - y0 - s|^2 is in R02; L21 = the l2,1 sum (FLAG_JOINT); S2 = the
 * Parseval sum of |B^T conj(Df) rfftn(u0) + rfftn(u1)|^2 / (H W) at the new u (this class's dual
 * residual, :568-571; profile slot "pdl1_dual"; FLAG_RESID only) and no SN2: sn = rho ||u|| is U2 + CGIT.
 * The XRRS sums are those of the reference's check (:530-538) in eigen-coordinates.  Generic transforms
 * on every shape. */
int sporco_amd_csc_pdl1_iter(sporco_amd_csc_t h, const sporco_amd_admm_params *p,
                             double out[SPORCO_AMD_OUT_COUNT]);

/* ---- online dictionary learning (sporco.dictlrn.onlinecdl.OnlineConvBPDNDictLearn.dstep,
 * onlinecdl.py:310-333) -------------------------------------------------------------------
 * After sporco_amd_csc_ccmod_setcoef and sporco_amd_csc_ccmod_grad(h, SPORCO_AMD_VAR_DF) (the
 * gradient at the current dictionary, left in VAR_DGF): G = irfftn(Df - eta * gradient),
 * D = Pcn(G) -> VAR_DX (and its spectrum VAR_DXF; read with sporco_amd_csc_ccmod_getdict).
 * out[SPORCO_AMD_OUT_CNSTR] = sum (Pcn(G) - G)^2, the square of the reference's Cnstr (:398). */
int sporco_amd_csc_ccmod_sgd_step(sporco_amd_csc_t h, double eta, int32_t dH, int32_t dW,
                                  int32_t zero_mean, double out[SPORCO_AMD_OUT_COUNT]);

/* ---- ADMM dictionary update with one dictionary copy ---------------------------------------
 * sporco.admm.ccmod.ConvCnstrMOD_IterSM / ConvCnstrMOD_CG (ccmod.py:433-601) on ConvCnstrMODBase
 * (:103-429) and ADMMEqual (admm.py:808-983).  X = VAR_DSX, Y = VAR_DX (spectrum VAR_DXF kept
 * current, as for the consensus update), U = VAR_DSU, all (H,W,K) real; Xf = VAR_DYF persists
 * between calls (the CG warm start, ccmod.py:583,594-597).  Coefficient maps come from
 * sporco_amd_csc_ccmod_setcoef.  Single-channel dictionaries. */
#define SPORCO_AMD_DSTEP_ISM 0   /* X-step by linalg.solvemdbi_ism over the images (<= 8 images
                                    times channels), ccmod.py:496-505                        */
#define SPORCO_AMD_DSTEP_CG 1    /* X-step by linalg.solvemdbi_cg (scipy cg semantics: stop at
                                    ||r|| < tol ||b|| at the top of an iteration), :587-601   */
/* Y = U = Y0 (uinit, ccmod.py:298-307) or 0; Xf = 0. */
int sporco_amd_csc_dstep_init(sporco_amd_csc_t h, const void *Y0);
typedef struct {
    double rho;      /* penalty parameter                                               */
    double rlx;      /* RelaxParam                                                      */
    double u_scale;  /* pending U /= rsf, as in sporco_amd_admm_params                  */
    double cg_tol;   /* CG StopTol                                                      */
    uint32_t flags;  /* SPORCO_AMD_FLAG_OBJ | _XRRS | _FEVAL_Y | _GEVAL_Y               */
    int32_t dH, dW;  /* filter support of the constraint set                            */
    int32_t zero_mean;
    int32_t method;  /* SPORCO_AMD_DSTEP_ISM / SPORCO_AMD_DSTEP_CG                      */
    int32_t cg_maxiter;
    int32_t mask_dcpl; /* != 0: ConvCnstrMODMaskDcpl_IterSM / _CG (sporco/admm/ccmodmd.py:27-762):
                        constraint [Z; I] d - [y0; y1] = [s; 0] with block 0 in VAR_DMY0 / _DMU0,
                        mask = the data mask (set_data_mask), X-step system Z^H Z + I (rho-free),
                        y0 = rho (AX0 + u0 - s) / (W^2 + rho).  out then carries the block-0 sums
                        beside the block-1 ones -- L1 / R2 = |AXnr - y - c|^2, L21 / AX2 = |AXnr|^2,
                        RGR / Y2 = |y|^2, slot 15 / U2 = |u|^2 --, S2 = |A^T u|^2 (:557-561),
                        DFID = |W g0|^2 with g0 = y0 (FLAG_GEVAL_Y) or Z d - s (:508-524).     */
} sporco_amd_dstep_params;
/* One iteration: xstep (b = sum_n conj(Zf_n) Sf_n + rho rfftn(Y - U); Xf = (Z^H Z + rho I)^-1 b),
 * relax_AX (admm.py:877-885), ystep Y = Pcn(AX + U) (ccmod.py:363-368), ustep.  out: R2 = |X - Y|^2,
 * S2 = |Y - Yprev|^2, AX2 = |X|^2, Y2, U2; with FLAG_OBJ: DFID (at Xf, or at rfftn(Y) with
 * FLAG_FEVAL_Y) and CNSTR (at X, or at Y with FLAG_GEVAL_Y), ccmod.py:372-410; with FLAG_XRRS the
 * sums of xstep_check (:343-357); CGIT / CGN for the CG method. */
/* State of the mask-decoupling variant: as sporco_amd_csc_dstep_init plus block 0 zeroed and the
 * real signal S (H,W,C,N) kept on the device (NULL: keep the one a previous
 * sporco_amd_csc_mdcpl_init / dstep_md_init call stored). */
int sporco_amd_csc_dstep_md_init(sporco_amd_csc_t h, const void *Y0, const void *S);
int sporco_amd_csc_dstep_iter(sporco_amd_csc_t h, const sporco_amd_dstep_params *p,
                              double out[SPORCO_AMD_OUT_COUNT]);

int sporco_amd_csc_asum(sporco_amd_csc_t h, int var, double out[SPORCO_AMD_OUT_COUNT]);

/* ---- per-kernel timing (HIP events on the handle's stream) ---------------- */

int sporco_amd_csc_profile(sporco_amd_csc_t h, int enable);
/* Reads and clears accumulated time of timing slot `slot`; returns its name. */
int sporco_amd_csc_profile_read(sporco_amd_csc_t h, int slot, const char **name,
                                double *total_ms, int64_t *launches);
int sporco_amd_profile_slots(void);

/* ---- stateless primitives on host arrays (parity entry points) ------------ */

/* rfftn over axes (0,1) of real (H,W,P) -> complex (H,W/2+1,P); sporco/fft.py:257-286. */
int sporco_amd_rfftn2(int dtype, int32_t H, int32_t W, int64_t P, const void *in, void *out);
/* irfftn with s=(H,W): complex (H,W/2+1,P) -> real (H,W,P); sporco/fft.py:288-314. */
int sporco_amd_irfftn2(int dtype, int32_t H, int32_t W, int64_t P, const void *in, void *out);
/* solvedbi_sm (sporco/linalg.py:232-297) with ah: complex (npix,1,K),
 * b, x: complex (npix,CN,K); solves (rho I + a a^H) x = b along K. */
int sporco_amd_solvedbi_sm(int dtype, int64_t npix, int64_t CN, int32_t K, const void *ah,
                           double rho, const void *b, void *x);
/* inner(x, y, axis=K) (sporco/linalg.py:41-88): x complex (npix,1,K) broadcast
 * over CN, y complex (npix,CN,K) -> out complex (npix,CN). */
int sporco_amd_inner(int dtype, int64_t npix, int64_t CN, int32_t K, const void *x,
                     const void *y, void *out);
/* ---- Device arrays and the pre / post-processing around the solvers -------------------------
 * The reference's example pipelines (examples/scripts/csc/cbpdn_gry.py:45-47, :66-77) highpass
 * the image with signal.tikhonov_filter, sparse-code the highpass part and add the lowpass part
 * back to the reconstruction.  With the entry points below the whole chain stays in HBM: one
 * upload of the image, one download of the result.  Buffers are plain device pointers. */
int sporco_amd_dev_malloc(size_t bytes, void **ptr_dev);
int sporco_amd_dev_free(void *ptr_dev);
int sporco_amd_dev_upload(void *dst_dev, const void *src_host, size_t bytes);
int sporco_amd_dev_download(void *dst_host, const void *src_dev, size_t bytes);
/* out = a x + b y on real device arrays of n elements (y may be NULL). */
int sporco_amd_dev_axpby(int dtype, int64_t n, double a, const void *x, double b, const void *y,
                         void *out);
/* signal.tikhonov_filter (sporco/signal.py:244-301) on a device array s (H, W, P), P = product of
 * the remaining axes: symmetric padding by npd, division by 1 + lmbda sum_i |G_i|^2 in the DFT
 * domain, crop; slp and shp = s - slp are device arrays of the shape of s. */
int sporco_amd_tikhonov_filter_dev(int dtype, int32_t H, int32_t W, int64_t P, const void *s_dev,
                                   double lmbda, int32_t npd, void *slp_dev, void *shp_dev);
/* fft.fftconv (sporco/fft.py:376-417) over axes (0, 1) of real device arrays a (ha, wa, ...) and
 * b (hb, wb, ...) whose remaining (up to three, after merging) axes have the extents da / db --
 * each 1 or the output extent d -- circular over (max(ha,hb), max(wa,wb)), result rolled by
 * -(origin_h, origin_w).  out: (H, W, d0, d1, d2). */
int sporco_amd_fftconv_dev(int dtype, int32_t ha, int32_t wa, const int64_t da[3], const void *a_dev,
                           int32_t hb, int32_t wb, const int64_t db[3], const void *b_dev,
                           int32_t origin_h, int32_t origin_w, void *out_dev);
/* set_signal from a device array (H, W, C, N) (no host copy). */
int sporco_amd_csc_set_signal_dev(sporco_amd_csc_t h, const void *S_dev);
/* reconstruct into a device array (H, W, C, N). */
int sporco_amd_csc_reconstruct_dev(sporco_amd_csc_t h, int var, void *dst_dev);
/* Bytes and calls of host <-> device copies made by this library since the last reset:
 * out = {h2d_bytes, h2d_calls, d2h_bytes, d2h_calls}. */
int sporco_amd_transfer_stats(int64_t out[4], int reset);

/* ---- image shards over the GPUs of a node: RCCL inside the library ---------------------------
 * (SURVEY.md 8(b) `allreduce_scalars`, 8(e); the reference's own multi-process split is
 * sporco/dictlrn/prlcnscdl.py:241,508 -- multiprocessing over shared memory, no counterpart of a
 * communicator.)  One communicator per process (one process per GPU): rank 0 obtains an id,
 * the host program hands its 128 bytes to the other ranks by whatever means it has (MPI,
 * torch.distributed's store, a file), every rank creates its communicator from it.  librccl is
 * opened at run time (dlopen: SPORCO_AMD_RCCL_LIB, then librccl.so.1 / librccl.so): the library
 * has no link-time dependency on it, and SPORCO_AMD_EUNSUPPORTED comes back when it is absent. */
typedef struct sporco_amd_comm *sporco_amd_comm_t;
#define SPORCO_AMD_COMM_ID_BYTES 128
#define SPORCO_AMD_COMM_SUM 0
#define SPORCO_AMD_COMM_MAX 2
int sporco_amd_comm_unique_id(void *id128);                      /* ncclGetUniqueId          */
int sporco_amd_comm_create(const void *id128, int32_t rank, int32_t world, int32_t device,
                           sporco_amd_comm_t *out);              /* ncclCommInitRank         */
int sporco_amd_comm_destroy(sporco_amd_comm_t c);
int sporco_amd_comm_info(sporco_amd_comm_t c, int32_t *rank, int32_t *world);
/* In-place all-reduce of `count` reals (SPORCO_AMD_F32 / _F64) of DEVICE memory, enqueued on
 * `stream` (a hipStream_t; NULL: the null stream) -- no host synchronisation. */
int sporco_amd_comm_allreduce(sporco_amd_comm_t c, void *buf_dev, int64_t count, int dtype, int op,
                              void *stream);
/* The same for a handful of HOST doubles (staged through a device buffer of the communicator;
 * returns when the result is in `vals`). */
int sporco_amd_comm_allreduce_host(sporco_amd_comm_t c, double *vals, int32_t n, int op);
/* Attach a communicator to a solver handle (NULL detaches): sporco_amd_csc_admm_run then sums the
 * 16 per-iteration doubles over the ranks itself, on the handle's stream, between the local sums
 * and the control update -- no callback into the host program per iteration (a `reduce` hook
 * given to admm_run takes precedence).  The communicator must outlive the handle's use of it. */
int sporco_amd_csc_set_comm(sporco_amd_csc_t h, sporco_amd_comm_t c);

/* prox_l1 (sporco/prox/_lp.py:144-183), real v of n elements, scalar alpha. */
int sporco_amd_prox_l1(int dtype, int64_t n, const void *v, double alpha, void *out);
/* The same with an array-valued threshold (sporco/prox/_lp.py:144-183 accepts one): v viewed as
 * a 5-D array of `shape`, alpha of `ashape` with extent 1 or the full extent on each axis. */
int sporco_amd_prox_l1w(int dtype, const int64_t shape[5], const void *v, const int64_t ashape[5],
                        const void *alpha, void *out);
/* prox_sl1l2 (sporco/prox/_l21.py:51-88) with the l2 norm over the middle axis
 * of real v shaped (outer, C, inner). */
int sporco_amd_prox_sl1l2(int dtype, int64_t outer, int32_t C, int64_t inner, const void *v,
                          double alpha, double beta, void *out);
/* proj_l2 (sporco/prox/_lp.py:334-340): projection onto the l2 ball of radius gamma, the norm over the
 * middle axis of real v shaped (outer, C, inner); a vector of norm 0 stays 0. */
int sporco_amd_proj_l2(int dtype, int64_t outer, int64_t C, int64_t inner, const void *v, double gamma,
                       void *out);
/* proj_l1 (sporco/prox/_l1proj.py:24-154): Euclidean projection onto the l1 ball of radius gamma of
 * each of the P interleaved sets of real v shaped (outer, P, inner) -- element i belongs to set
 * (i / inner) % P, and the norm of a set runs over its outer and inner indices; P = 1: the whole array.
 * A set with l1 norm <= gamma comes back bit for bit. */
int sporco_amd_proj_l1(int dtype, int64_t outer, int64_t P, int64_t inner, const void *v, double gamma,
                       void *out);
/* rfl2norm2 (sporco/fft.py:449-484) of complex xf (H,W/2+1,P) for spatial (H,W). */
int sporco_amd_rfl2norm2(int dtype, int32_t H, int32_t W, int64_t P, const void *xf,
                         double *out);
/* out = x * y, elementwise, on real device arrays of n elements (DeviceArray * DeviceArray). */
int sporco_amd_dev_mul(int dtype, int64_t n, const void *x, const void *y, void *out);

/* ---- l2-TV denoising: sporco.admm.tvl2.TVL2Denoise (sporco/admm/tvl2.py:27-372) ----------------
 * minimise (1/2) ||Wdf (x - s)||^2 + lmbda ||Wtv sqrt((G_0 x)^2 + (G_1 x)^2)||_1 by ADMM on
 * (G_0; G_1) x = (y_0; y_1), G_i the forward difference along axis i with a zero last row.  Every step
 * is a nearest-neighbour stencil (csrc/csc_tvd.h); the handle is a small one of its own: the arrays of
 * one (H, W, P) problem, P the product of the trailing axes, and a stream -- no dictionary, no
 * transforms.  vector_tv: the l2 norm of the y step also runs over the first of the trailing axes
 * (C channels, P = C N, C <= 8; the reference's caxis=2), else every plane is a problem of its own.
 * X starts at S (set by uploading S); Y, U start at zero. */
typedef struct sporco_amd_tvd *sporco_amd_tvd_t;
#define SPORCO_AMD_TVD_S 0    /* real (H,W,P)    the signal; uploading it also sets X = S          */
#define SPORCO_AMD_TVD_X 1    /* real (H,W,P)    the iterate of the x step                         */
#define SPORCO_AMD_TVD_Y 2    /* real (2,H,W,P)  the blocks (y_0, y_1) of Y                        */
#define SPORCO_AMD_TVD_U 3    /* real (2,H,W,P)  ... and of U (without a pending u_scale)          */
#define SPORCO_AMD_TVD_WDF 4  /* real (H,W,P)    DFidWeight array (upload NULL: the scalar wdf)    */
#define SPORCO_AMD_TVD_WTV 5  /* real (H,W,P)    TVWeight array (upload NULL: the scalar wtv;      */
                              /*                 not with vector_tv)                               */
typedef struct {
    double rho, lmbda, rlx;
    double u_scale;   /* pending U /= rsf (admm.py:573): the sweeps and the y step apply it          */
    double wdf, wtv;  /* scalar weights, read where no array is set                                   */
    int32_t geval_y;  /* RegTV at Y (else at A X)                                                     */
} sporco_amd_tvd_params;
int sporco_amd_tvd_create(int dtype, int32_t H, int32_t W, int64_t P, int32_t C, int32_t vector_tv,
                          int device, void *stream, sporco_amd_tvd_t *out);
/* l1-TV denoising, sporco.admm.tvl1.TVL1Denoise (sporco/admm/tvl1.py:27-399):
 *     minimise ||Wdf (x - s)||_1 + lmbda ||Wtv sqrt((G_0 x)^2 + (G_1 x)^2)||_1
 * by ADMM on (G_0; G_1; I) x - (y_0; y_1; y_d) = (0; 0; s).  The same arguments as sporco_amd_tvd_create; the
 * handle is a sporco_amd_tvd_t in l1 mode and every sporco_amd_tvd_* call serves it, with these differences:
 *   TVD_Y, TVD_U   are real (3,H,W,P): the two gradient blocks, then the data block;
 *   tvd_sweeps     tvl1.py:240-260: the sweep with rho = 1 and a unit DFidWeight on P = A^T (Y - u_scale U),
 *                  A^T including the identity block (p->rho and the DFidWeight do not enter);
 *   tvd_gsres      the norms of linalg.rrs(G^T G X + X, P + S);
 *   tvd_ystep      Y_g = prox_l2(AX_g + U_g, (lmbda / rho) Wtv), Y_d = prox_l1(AX_d + U_d - S, Wdf / rho) with
 *                  AX_d = rlx X + (1 - rlx) (Y_d + S), U += AX - Y - c.  out: OUT_R2 = ||(G X - Y_g; X - Y_d - S)||^2,
 *                  OUT_AX2 = ||(G X; X)||^2, OUT_Y2 = ||Y||^2, OUT_C2 = ||S||^2, OUT_S2 = ||A^T U||^2 and
 *                  OUT_U2 = ||U||^2 over the three blocks (tvl1.py:362-372; rho applied by the host),
 *                  OUT_DFID = sum |Wdf g_d| and OUT_L21 = sum Wtv sqrt(sum g_g^2), g = Y with geval_y, else
 *                  (G X; X - S); OUT_XRRS_* as for tvd_gsres.  There is no Y - Yprev in this problem.
 * The profiler names its two kernels tvl1_ystep and tvl1_adjoint. */
int sporco_amd_tvl1_create(int dtype, int32_t H, int32_t W, int64_t P, int32_t C, int32_t vector_tv,
                           int device, void *stream, sporco_amd_tvd_t *out);
int sporco_amd_tvd_destroy(sporco_amd_tvd_t h);
int sporco_amd_tvd_sync(sporco_amd_tvd_t h);
/* The launch plan: out = (V, items per row, strips, rows per segment, segments, columns a strip covers);
 * V is the elements of an item (the access width; the channel count with vector_tv). */
int sporco_amd_tvd_plan(sporco_amd_tvd_t h, int64_t out[6]);
/* Copy an array in or out; on_device: src / dst is a device pointer (no host traffic).  After Y, U or X
 * have been written, sporco_amd_tvd_adjoint must run before the next sweep. */
int sporco_amd_tvd_upload(sporco_amd_tvd_t h, int var, const void *src, int on_device);
int sporco_amd_tvd_download(sporco_amd_tvd_t h, int var, void *dst, int on_device);
/* n Jacobi sweeps of the x step (tvl2.py:362-371) on P = A^T (Y - u_scale U). */
int sporco_amd_tvd_sweeps(sporco_amd_tvd_t h, const sporco_amd_tvd_params *p, int32_t n);
/* The norms of linalg.rrs(rho A^T A X + Wdf^2 X, Wdf^2 S + rho P) at the current X (tvl2.py:248-251):
 * out[OUT_XRRS_D2], out[OUT_XRRS_AX2], out[OUT_XRRS_B2]; one launch and one host read (GSTol > 0). */
int sporco_amd_tvd_gsres(sporco_amd_tvd_t h, const sporco_amd_tvd_params *p,
                         double out[SPORCO_AMD_OUT_COUNT]);
/* relax_AX + ystep + ustep in one launch, then A^T of the new Y, U and of Y - Yprev in a second, and one
 * host read.  out: OUT_R2, OUT_AX2, OUT_Y2 as for admm_iter; OUT_S2 = ||A^T (Y - Yprev)||^2 and
 * OUT_U2 = ||A^T U||^2 (rho applied by the host); OUT_DFID = ||Wdf (X - S)||^2 (not halved);
 * OUT_L21 = sum Wtv sqrt(sum g^2), g = Y with geval_y, else A X; OUT_XRRS_* as for tvd_gsres.
 * U is stored with u_scale applied: the caller's pending factor is 1 afterwards. */
int sporco_amd_tvd_ystep(sporco_amd_tvd_t h, const sporco_amd_tvd_params *p,
                         double out[SPORCO_AMD_OUT_COUNT]);
/* A^T (Y - U) and A^T U of the current arrays (after an upload of Y, U). */
int sporco_amd_tvd_adjoint(sporco_amd_tvd_t h);
/* Per-kernel event timing of the handle's launches, as sporco_amd_csc_profile / _profile_read. */
int sporco_amd_tvd_profile(sporco_amd_tvd_t h, int enable);
int sporco_amd_tvd_profile_read(sporco_amd_tvd_t h, int slot, const char **name, double *total_ms,
                                int64_t *count);

/* ---- TV deconvolution: sporco.admm.tvl2.TVL2Deconv (sporco/admm/tvl2.py:377-702) and
 * sporco.admm.tvl1.TVL1Deconv (sporco/admm/tvl1.py:403-758) ------------------------------------------
 *     l2:  minimise (1/2) ||H x - s||^2 + lmbda ||Wtv sqrt((G_0 x)^2 + (G_1 x)^2)||_1   on (G_0; G_1) x = y
 *     l1:  minimise ||Wdf (H x - s)||_1 + lmbda ||Wtv sqrt((G_0 x)^2 + (G_1 x)^2)||_1   on (G_0; G_1; H) x - y = (0; 0; s)
 * H the circular convolution with the kernel A, G_i the CIRCULAR difference (G_i x)[j] = x[j] - x[j - 1]
 * (sporco/signal.py:204-240).  The x step is a pointwise solve between one forward and one inverse
 * transform (rfft2 / irfft2 on the generic chain); the gradients, their adjoints, the y and u steps are
 * periodic stencils (csrc/csc_tvdc.h).  The handle owns S, X, Y, U, the spectra of S and A, the work
 * spectrum and the transform plans of H and W; a transform length that does not fit is refused at creation
 * ("transform length too large").  vector_tv, C, P as for sporco_amd_tvd_create.  PA: the planes of the
 * kernel A, P (one kernel per plane) or 1 (one for all).  Y, U start at zero. */
typedef struct sporco_amd_tvdc *sporco_amd_tvdc_t;
#define SPORCO_AMD_TVDC_S 0    /* real (H,W,P)     the signal                                             */
#define SPORCO_AMD_TVDC_X 1    /* real (H,W,P)     the result of the x step (download only)               */
#define SPORCO_AMD_TVDC_Y 2    /* real (nb,H,W,P)  the blocks of Y: nb = 2, or 3 in l1 mode (data block last) */
#define SPORCO_AMD_TVDC_U 3    /* real (nb,H,W,P)  ... and of U (without a pending u_scale)               */
#define SPORCO_AMD_TVDC_WDF 4  /* real (H,W,P)     l1: DFidWeight array (upload NULL: the scalar wdf)     */
#define SPORCO_AMD_TVDC_WTV 5  /* real (H,W,P)     TVWeight array (upload NULL: the scalar wtv; not with vector_tv) */
#define SPORCO_AMD_TVDC_HX 6   /* real (H,W,P)     l1: H X of the last x step (download only)             */
typedef struct {
    double rho, lmbda, rlx;
    double u_scale;           /* pending U /= rsf (admm.py:573): the x and y steps apply it                 */
    double wdf, wtv;          /* scalar weights, read where no array is set                                 */
    int32_t geval_y;          /* RegTV (l1: and DFid) at Y, else at A X - c                                 */
    int32_t lin_solve_check;  /* the x step also forms OUT_XRRS_*                                           */
    int32_t want_rsdl;        /* the y step also forms the dual residual's sums (l2: and writes Y - Yprev)  */
    int32_t want_stats;       /* l2: the x step also forms OUT_DFID                                         */
} sporco_amd_tvdc_params;
int sporco_amd_tvdc_create(int dtype, int32_t H, int32_t W, int64_t P, int32_t C, int32_t vector_tv, int64_t PA,
                           int device, void *stream, sporco_amd_tvdc_t *out);
int sporco_amd_tvl1dc_create(int dtype, int32_t H, int32_t W, int64_t P, int32_t C, int32_t vector_tv, int64_t PA,
                             int device, void *stream, sporco_amd_tvdc_t *out);
int sporco_amd_tvdc_destroy(sporco_amd_tvdc_t h);
int sporco_amd_tvdc_sync(sporco_amd_tvdc_t h);
/* The launch plan: out[0..5] as sporco_amd_tvd_plan for tvdc_ystep / tvdc_adjoint; out[6] = planes per access
 * of tvdc_solve (2: 16 bytes in float32), out[7] = its workgroups. */
int sporco_amd_tvdc_plan(sporco_amd_tvdc_t h, int64_t out[8]);
/* Copy an array in or out; on_device: src / dst is a device pointer (no host traffic).  Uploading S also
 * forms its spectrum (and AHSf, ||S||^2).  After Y or U have been written, sporco_amd_tvdc_adjoint must run
 * before the next x step. */
int sporco_amd_tvdc_upload(sporco_amd_tvdc_t h, int var, const void *src, int on_device);
int sporco_amd_tvdc_download(sporco_amd_tvdc_t h, int var, void *dst, int on_device);
/* The kernel: a real C-ordered (ah, aw, PA) array, ah <= H, aw <= W; zero-padded and transformed on the
 * device (the phase of sporco.signal.fftconv), then |Af|^2 and AHSf = conj(Af) Sf. */
int sporco_amd_tvdc_set_kernel(sporco_amd_tvdc_t h, const void *A, int32_t ah, int32_t aw, int on_device);
/* The x step: Xf = (AHSf + rho F(G^T (Y - u_scale U))) / (|Af|^2 + rho GHGf), l1: Xf = (AHSf + F(G^T (Y_g -
 * u_scale U_g)) + conj(Af) F(Y_d - u_scale U_d)) / (|Af|^2 + GHGf); X (l1: and H X) by one inverse transform. */
int sporco_amd_tvdc_xstep(sporco_amd_tvdc_t h, const sporco_amd_tvdc_params *p);
/* relax_AX + ystep + ustep in one launch, the adjoint arrays of the next x step in a second, and one host
 * read.  out: OUT_R2 = ||A X - Y - c||^2, OUT_AX2, OUT_Y2, OUT_L21 = sum Wtv sqrt(sum g_g^2);
 *   l2: OUT_DFID = ||H X - S||^2 by Parseval (not halved; from the x step), OUT_S2 = ||G^T (Y - Yprev)||^2,
 *       OUT_U2 = ||G^T U||^2 (rho applied by the host);
 *   l1: OUT_DFID = sum |Wdf g_d|, OUT_S2 = ||A^T U||^2 (over spectra), OUT_U2 = ||U||^2, OUT_C2 = ||S||^2;
 *   OUT_XRRS_* with lin_solve_check.  U is stored with u_scale applied: the pending factor is 1 afterwards. */
int sporco_amd_tvdc_ystep(sporco_amd_tvdc_t h, const sporco_amd_tvdc_params *p, double out[SPORCO_AMD_OUT_COUNT]);
/* The adjoint arrays of the current Y, U (after an upload of either). */
int sporco_amd_tvdc_adjoint(sporco_amd_tvdc_t h);
/* Per-kernel event timing of the handle's launches, as sporco_amd_csc_profile / _profile_read. */
int sporco_amd_tvdc_profile(sporco_amd_tvdc_t h, int enable);
int sporco_amd_tvdc_profile_read(sporco_amd_tvdc_t h, int slot, const char **name, double *total_ms,
                                 int64_t *count);

/* ---- l1-spline fit: sporco.admm.spline.SplineL1 (sporco/admm/spline.py:24-291) and the orthonormal DCT-II
 * of sporco.fft.dctii / idctii (sporco/fft.py:318-372) --------------------------------------------------
 *     minimise ||Wdf (x - s)||_1 + (lmbda / 2) ||D x||^2      on  x - y = s,
 * D the second difference with reflecting ends, diagonal under the DCT-II with eigenvalues
 * alpha[k1, k2] = (-2 + 2 cos(pi k1 / H)) + (-2 + 2 cos(pi k2 / W)).  The x step is
 * X = idct(Gamma dct(Y + S - U)), Gamma = 1 / (1 + (lmbda / rho) alpha^2): the DCT is computed through ONE
 * real transform of the same size on a permuted array (rfft2 / irfft2 on the generic chain) with a
 * pointwise twiddle kernel between the two (csrc/csc_spline.h).  The handle owns S, X, Y, U, the permuted
 * right-hand side arrays, the work spectrum and the transform plans of H and W; a transform length that
 * does not fit is refused at creation ("transform length too large").  A 1-D signal of N samples is served
 * as H = 1, W = N.  Y, U start at zero. */
typedef struct sporco_amd_spl *sporco_amd_spl_t;
#define SPORCO_AMD_SPL_S 0    /* real (H,W,P)  the signal                                               */
#define SPORCO_AMD_SPL_X 1    /* real (H,W,P)  the result of the x step (download only)                 */
#define SPORCO_AMD_SPL_Y 2    /* real (H,W,P)                                                           */
#define SPORCO_AMD_SPL_U 3    /* real (H,W,P)  (without a pending u_scale)                              */
#define SPORCO_AMD_SPL_WDF 4  /* real (H,W,P)  DFidWeight array (upload NULL: the scalar wdf)           */
typedef struct {
    double rho, lmbda, rlx;
    double u_scale;           /* pending U /= rsf (admm.py:573): the x and y steps apply it                 */
    double wdf;               /* scalar DFidWeight, read where no array is set                              */
    int32_t geval_y;          /* DFid at Y, else at X - S                                                   */
    int32_t lin_solve_check;  /* the x step also forms OUT_XRRS_*                                           */
    int32_t want_stats;       /* the x step also forms OUT_RGR                                              */
    int32_t reserved;
} sporco_amd_spl_params;
int sporco_amd_spl_create(int dtype, int32_t H, int32_t W, int64_t P, int device, void *stream, sporco_amd_spl_t *out);
int sporco_amd_spl_destroy(sporco_amd_spl_t h);
int sporco_amd_spl_sync(sporco_amd_spl_t h);
/* The launch plan: out[0] = planes per access (2: 16 bytes of spectrum in float32), out[1] = row pairs
 * {k1, H - k1} of spl_solve, out[2] = its workgroups, out[3] = the workgroups of spl_ystep. */
int sporco_amd_spl_plan(sporco_amd_spl_t h, int64_t out[4]);
/* Copy an array in or out; on_device: src / dst is a device pointer (no host traffic).  Uploading S also
 * forms ||S||^2; uploading S, Y or U also forms the permuted arrays of the next x step. */
int sporco_amd_spl_upload(sporco_amd_spl_t h, int var, const void *src, int on_device);
int sporco_amd_spl_download(sporco_amd_spl_t h, int var, void *dst, int on_device);
/* The x step: X = idct(Gamma dct(Y + S - u_scale U)), kept in the transform's permuted order. */
int sporco_amd_spl_xstep(sporco_amd_spl_t h, const sporco_amd_spl_params *p);
/* relax_AX + ystep + ustep and the arrays of the next x step in one launch, one reduction, one host read.
 * out: OUT_R2 = ||X - Y - S||^2, OUT_AX2 = ||X||^2, OUT_Y2, OUT_S2 = ||Y - Yprev||^2 (rho applied by the
 * host), OUT_U2 = ||U||^2, OUT_DFID = sum |Wdf g|, OUT_C2 = ||S||^2; from the x step, with want_stats:
 * OUT_RGR = sum (alpha Xhat)^2 (twice Reg), with lin_solve_check: OUT_XRRS_*.  U is stored with u_scale
 * applied: the pending factor is 1 afterwards. */
int sporco_amd_spl_ystep(sporco_amd_spl_t h, const sporco_amd_spl_params *p, double out[SPORCO_AMD_OUT_COUNT]);
/* Per-kernel event timing of the handle's launches, as sporco_amd_csc_profile / _profile_read. */
int sporco_amd_spl_profile(sporco_amd_spl_t h, int enable);
int sporco_amd_spl_profile_read(sporco_amd_spl_t h, int slot, const char **name, double *total_ms,
                                int64_t *count);
/* out(H, W, P) = the orthonormal DCT-II (idctii: its inverse) of in(H, W, P) over axes (0, 1), H >= 1,
 * W >= 2; on_device: both pointers are device pointers.  in != out.  Stateless: each call allocates its work
 * arrays and transform plans on the current device, runs on the null stream and synchronises the device. */
int sporco_amd_dctii(int dtype, int32_t H, int32_t W, int64_t P, const void *in, void *out, int on_device);
int sporco_amd_idctii(int dtype, int32_t H, int32_t W, int64_t P, const void *in, void *out, int on_device);

/* ---- dense sparse coding: sporco.admm.bpdn BPDN / BPDNJoint / ElasticNet (sporco/admm/bpdn.py:24-748) ----
 *     minimise (1/2) ||D x - s||^2 + lmbda ||wl1 x||_1 [+ mu ||x||_{2,1}] [+ (mu / 2) ||x||^2]   on  x = y,
 * D (N, M), S (N, K), X / Y / U (M, K), every array row-major as NumPy has it.  The x step is X = P B with
 * B = D^T S + rho (Y - U) and the solve matrix P = (D^T D + c I)^-1, c = rho (ElasticNet: mu + rho), which the
 * caller forms and sets again whenever c or D changes.  One call does an iteration (csrc/csc_bpdn.h); the
 * products run on the float32 matrix instruction (float64, or SPORCO_AMD_BPDN_PLAIN: as fma chains with the
 * same bits).  Y and U start at zero. */
typedef struct sporco_amd_bpdn *sporco_amd_bpdn_t;
#define SPORCO_AMD_BPDN_MAX_DIM 512 /* the largest N and M */
#define SPORCO_AMD_BPDN_S 0    /* (N,K)  the signals; setting it (or the dictionary) forms D^T S on the device */
#define SPORCO_AMD_BPDN_X 1    /* (M,K)  the result of the x step (download only)                            */
#define SPORCO_AMD_BPDN_Y 2    /* (M,K)                                                                      */
#define SPORCO_AMD_BPDN_U 3    /* (M,K)  (without a pending u_scale)                                         */
#define SPORCO_AMD_BPDN_WL1 4  /* (M,K)  L1Weight array (upload NULL: the scalar wl1)                        */
#define SPORCO_AMD_BPDN_DTS 5  /* (M,K)  D^T S (download only)                                               */
typedef struct {
    double rho, lmbda, mu, rlx;
    double u_scale;           /* pending U /= rsf (admm.py:573): the iteration applies it                   */
    double wl1;               /* scalar L1Weight, read where no array is set                                */
    double c;                 /* the c of the solve matrix in use (LinSolveCheck)                           */
    int32_t nonneg;           /* NonNegCoef                                                                 */
    int32_t feval_x;          /* DFid at X, else at Y                                                       */
    int32_t geval_y;          /* the regularisation terms at Y, else at X                                   */
    int32_t want_x;           /* store X (always stored with joint or lin_solve_check)                      */
    int32_t joint;            /* BPDNJoint: the l2,1 term with weight mu                                    */
    int32_t lin_solve_check;  /* also form OUT_XRRS_*                                                       */
    int32_t proj_l1;          /* BPDNProjL1 (bpdn.py:750-914): the y step projects every column of AX + U onto
                                 the l1 ball of radius gamma, and `lmbda` carries gamma (>= 0); wl1, mu and a
                                 weight array are not read; not with joint                                  */
    int32_t reserved;
} sporco_amd_bpdn_params;
int sporco_amd_bpdn_create(int dtype, int32_t N, int32_t M, int64_t K, int device, void *stream, sporco_amd_bpdn_t *out);
int sporco_amd_bpdn_destroy(sporco_amd_bpdn_t h);
int sporco_amd_bpdn_sync(sporco_amd_bpdn_t h);
/* out[0] = columns of a workgroup's block, out[1] = workgroups, out[2] = 1 where the products use the matrix
 * instruction, out[3] = bytes of LDS of a workgroup. */
int sporco_amd_bpdn_plan(sporco_amd_bpdn_t h, int64_t out[4]);
/* D: host (N, M) in the handle's precision; P: host (M, M).  Y and U are kept. */
int sporco_amd_bpdn_set_dict(sporco_amd_bpdn_t h, const void *D);
int sporco_amd_bpdn_set_solve(sporco_amd_bpdn_t h, const void *P);
/* Copy a host array in or out.  X and D^T S are results: an upload of either only prefills the array (tests). */
int sporco_amd_bpdn_upload(sporco_amd_bpdn_t h, int var, const void *src);
int sporco_amd_bpdn_download(sporco_amd_bpdn_t h, int var, void *dst);
/* One iteration: x step, relax_AX, y step, u step, one reduction, one host read.  out: OUT_R2 = ||X - Y||^2,
 * OUT_AX2 = ||X||^2, OUT_Y2, OUT_S2 = ||Y - Yprev||^2 (rho applied by the host), OUT_U2, OUT_DFID =
 * ||D g - S||^2 (the host halves it), OUT_L1 = sum |wl1 g|, joint: OUT_L21 = sum_m ||g_m||, with
 * lin_solve_check: OUT_XRRS_*.  U is stored with u_scale applied: the pending factor is 1 afterwards.
 * proj_l1: Y' = proj_l1(AX + U, gamma) per column [max(., 0)], OUT_L1 is not formed, and
 * SPORCO_AMD_OUT_BPDN_CNSTR = sum (proj_l1(g, gamma) - g)^2 over the columns of g = Y' (geval_y off: X), the
 * square of the reference's Cnstr (bpdn.py:906-914). */
#define SPORCO_AMD_OUT_BPDN_CNSTR SPORCO_AMD_OUT_CNSTR
int sporco_amd_bpdn_iter(sporco_amd_bpdn_t h, const sporco_amd_bpdn_params *p, double out[SPORCO_AMD_OUT_COUNT]);
/* prox.proj_l1(v, gamma, axis=0) of a host (M, K) array, row-major, M <= 512, gamma >= 0: one l1 ball per column,
 * by the column search of the proj_l1 mode above behind a kernel that loads tiles and stores the result
 * (csrc/csc_bpdn.h).  The columns of a workgroup's block are those of sporco_amd_bpdn_plan for (N = 1, M).  Stateless
 * as the primitives above: current device, null stream, synchronises. */
int sporco_amd_proj_l1_cols(int dtype, int32_t M, int64_t K, const void *v, double gamma, void *out);
/* Per-kernel event timing of the handle's launches, as sporco_amd_csc_profile / _profile_read. */
int sporco_amd_bpdn_profile(sporco_amd_bpdn_t h, int enable);
int sporco_amd_bpdn_profile_read(sporco_amd_bpdn_t h, int slot, const char **name, double *total_ms,
                                 int64_t *count);
/* *out = the device buffer of variable `var`, valid while the handle lives (NULL: the weight is a scalar).  What
 * lets another handle read the coefficients in place (sporco_amd_cmod_set_coef with on_device). */
int sporco_amd_bpdn_devptr(sporco_amd_bpdn_t h, int var, void **out);

/* ---- dense sparse coding by proximal gradient steps: sporco.pgm.bpdn BPDN / WeightedBPDN
 * (sporco/pgm/bpdn.py:26-375) ----
 *     minimise (1/2) ||D x - s||^2_W + lmbda ||wl1 x||_1,   W = diag(w).
 * A handle of sporco_amd_bpdn_pgm_create is a bpdn handle (sync, plan, set_dict, upload, download, profile,
 * devptr and destroy are those above; D^T S is formed as there, there is no solve matrix and no sporco_amd_bpdn_iter)
 * with the arrays of the iteration: two X arrays (the iterate and the one before; `advance` swaps their roles),
 * two Y arrays (the second for the robust backtracking rule), G, Z, ZZ, all (M, K), and the weight w (N, K).
 * One call of sporco_amd_bpdn_pgm_step launches the phases it is asked for (csrc/csc_pgm_bpdn.h) and the
 * fixed-order reduction; both phases in one call are a whole step X' = prox(Y - G / L) with every scalar of
 * F, Q_L, Rsdl, DFid and RegL1.  All arrays start at zero. */
#define SPORCO_AMD_BPDN_XPRV 6  /* (M,K)  the iterate before X                                                 */
#define SPORCO_AMD_BPDN_YPRV 7  /* (M,K)  robust rule: the Y of the iteration before                           */
#define SPORCO_AMD_BPDN_G 8     /* (M,K)  the gradient D^T W (D Y - S) of the last gradient phase              */
#define SPORCO_AMD_BPDN_Z 9     /* (M,K)  robust rule: Z                                                       */
#define SPORCO_AMD_BPDN_ZZ 10   /* (M,K)  Monotone: the X' of the last step before a revert                    */
#define SPORCO_AMD_BPDN_W 11    /* (N,K)  weight array of the data fidelity term (upload NULL: the scalar w)   */
#define SPORCO_AMD_PGMB_PHASE_GRAD 1
#define SPORCO_AMD_PGMB_PHASE_PROX 2
#define SPORCO_AMD_PGMB_Y_LOAD 0      /* Y as it stands                                                        */
#define SPORCO_AMD_PGMB_Y_MOMENTUM 1  /* Y = Xprv + beta (Xprv - Xold), formed on the way in and stored        */
#define SPORCO_AMD_PGMB_Y_ROBUST 2    /* [Z += zc (Xprv - Yprv);] Y = (tk Xprv + t Z) / (tk + t), stored       */
/* out[] of sporco_amd_bpdn_pgm_step (the halves applied) */
#define SPORCO_AMD_PGMB_FY 0    /* f(Y) = (1/2) sum w (D Y - S)^2        (gradient phase)                      */
#define SPORCO_AMD_PGMB_FX 1    /* f(X')                                  (prox phase)                          */
#define SPORCO_AMD_PGMB_DXG 2   /* <X' - Y, G>                                                                 */
#define SPORCO_AMD_PGMB_DXY2 3  /* ||X' - Y||^2                                                                */
#define SPORCO_AMD_PGMB_L1 4    /* ||wl1 X'||_1                                                                */
#define SPORCO_AMD_PGMB_X2 5    /* ||X'||^2                                                                    */
#define SPORCO_AMD_PGMB_RS2 6   /* ||X' - Yprv||^2 (Yprv: Y where the Y arrays were not swapped);
                                   sporco_amd_bpdn_pgm_ystep: ||X - Y||^2                                      */
#define SPORCO_AMD_PGMB_G2 7    /* ||G||^2                                (gradient phase)                      */
#define SPORCO_AMD_PGMB_DG2 8   /* ||D G||^2                              (gradient phase alone, cauchy)        */
#define SPORCO_AMD_PGMB_BBXG 9  /* <Xprv - Xold, G - Gold>                (gradient phase, bb)                  */
#define SPORCO_AMD_PGMB_BBG2 10 /* ||G - Gold||^2                                                              */
typedef struct {
    double L, lmbda;
    double wl1, w;            /* the scalar weights, read where no array is set                              */
    double beta;              /* Y_MOMENTUM                                                                  */
    double tk, t, zc;         /* Y_ROBUST                                                                    */
    int32_t phase;            /* SPORCO_AMD_PGMB_PHASE_GRAD | _PROX                                          */
    int32_t ymode;            /* SPORCO_AMD_PGMB_Y_* (gradient phase)                                        */
    int32_t advance;          /* first: X becomes Xprv and the array of the iterate before it receives X'    */
    int32_t advance_y;        /* ... and Y becomes Yprv (the robust rule)                                    */
    int32_t nonneg;           /* NonNegCoef                                                                  */
    int32_t revert;           /* prox phase: X' = Xprv (Monotone's revert) with the sums of that X'          */
    int32_t z_update;         /* Y_ROBUST: apply zc first                                                    */
    int32_t cauchy;           /* gradient phase alone: form OUT DG2                                          */
    int32_t bb;               /* gradient phase: form BBXG, BBG2 against the G of the gradient phase before  */
    int32_t keep_zz;          /* prox phase: also store X' to ZZ                                             */
    int32_t reserved[2];
} sporco_amd_bpdn_pgm_params;
int sporco_amd_bpdn_pgm_create(int dtype, int32_t N, int32_t M, int64_t K, int device, void *stream,
                               sporco_amd_bpdn_t *out);
/* out == NULL: no reduction is read back (the launches are queued and the call returns). */
int sporco_amd_bpdn_pgm_step(sporco_amd_bpdn_t h, const sporco_amd_bpdn_pgm_params *p, double out[SPORCO_AMD_OUT_COUNT]);
/* Y = X + gamma (ZZ - X) + beta (X - Xprv) (use_zz == 0: without the ZZ term), written to the other Y array with
 * advance_y (Y becomes Yprv first); out[SPORCO_AMD_PGMB_RS2] = ||X - Y||^2, out == NULL as above. */
int sporco_amd_bpdn_pgm_ystep(sporco_amd_bpdn_t h, double beta, double gamma, int use_zz, int advance_y,
                              double out[SPORCO_AMD_OUT_COUNT]);
/* variable dst <- variable src on the device, both (M,K). */
int sporco_amd_bpdn_pgm_copy(sporco_amd_bpdn_t h, int dst, int src);

/* ---- dense dictionary update: sporco.admm.cmod CnstrMOD (sporco/admm/cmod.py:21-342) ----
 *     minimise ||D Z - S||^2  such that  ||d_m|| = 1 [, mean(d_m) = 0]   on  d = g,
 * Z (M, K), S (N, K), X / Y / U (N, M), every array row-major as NumPy has it.  set_coef forms Z Z^T and S Z^T on
 * the device, reduced over K (csrc/csc_cmod.h), and leaves them in double for the caller, who forms
 * Q = (Z Z^T + rho I)^-1 and sets it again whenever rho changes.  The x step is X = (S Z^T + rho (Y - U)) Q, the y
 * step the projection onto unit-norm (zero-mean) columns.  The products run on the float32 matrix instruction
 * (float64, or SPORCO_AMD_CMOD_PLAIN: as fma chains with the same bits).  Y and U start at zero. */
typedef struct sporco_amd_cmod *sporco_amd_cmod_t;
#define SPORCO_AMD_CMOD_MAX_DIM 512 /* the largest N and M */
#define SPORCO_AMD_CMOD_X 0      /* (N,M)  the result of the x step                                          */
#define SPORCO_AMD_CMOD_Y 1      /* (N,M)                                                                    */
#define SPORCO_AMD_CMOD_U 2      /* (N,M)  (without a pending u_scale)                                       */
#define SPORCO_AMD_CMOD_SZT 3    /* (N,M)  S Z^T in the handle's precision (an upload only prefills: tests)  */
#define SPORCO_AMD_CMOD_G 4      /* (M,M)  Z Z^T, doubles whatever the handle's dtype (likewise)             */
#define SPORCO_AMD_CMOD_SZTD 5   /* (N,M)  S Z^T, doubles (likewise)                                         */
typedef struct {
    double rho, rlx;
    double u_scale;           /* pending U /= rsf (admm.py:573): the iteration applies it                    */
    int32_t zero_mean;        /* ZeroMean: the projection subtracts the column means first                   */
    int32_t feval_x;          /* DFid at X, else at Y                                                        */
    int32_t geval_y;          /* Cnstr at Y, else at X                                                       */
    int32_t want_dfid;        /* form OUT_DFID (one more launch that reads Z and S)                          */
} sporco_amd_cmod_params;
int sporco_amd_cmod_create(int dtype, int32_t N, int32_t M, int64_t K, int device, void *stream, sporco_amd_cmod_t *out);
int sporco_amd_cmod_destroy(sporco_amd_cmod_t h);
int sporco_amd_cmod_sync(sporco_amd_cmod_t h);
/* out[0] = columns of K staged per step, out[1] = columns of a slab, out[2] = slabs, out[3], out[4] = row and
 * column blocks of the output, out[5] = 1 where the products use the matrix instruction, out[6], out[7] = bytes
 * of LDS of a workgroup of cmod_gram and of cmod_iter. */
int sporco_amd_cmod_plan(sporco_amd_cmod_t h, int64_t out[8]);
/* S (N, K) / Z (M, K) in the handle's precision.  on_device: a device pointer that is read in place, not copied;
 * it stays valid and unchanged until the next set_signal / set_coef or the handle's end (Z is read again by every
 * iteration that forms OUT_DFID).  set_coef needs S; it runs cmod_gram and cmod_gram_reduce. */
int sporco_amd_cmod_set_signal(sporco_amd_cmod_t h, const void *S, int on_device);
int sporco_amd_cmod_set_coef(sporco_amd_cmod_t h, const void *Z, int on_device);
/* Q: host (M, M) in the handle's precision. */
int sporco_amd_cmod_set_solve(sporco_amd_cmod_t h, const void *Q);
/* Copy a host array in or out. */
int sporco_amd_cmod_upload(sporco_amd_cmod_t h, int var, const void *src);
int sporco_amd_cmod_download(sporco_amd_cmod_t h, int var, void *dst);
/* One iteration: cmod_rhs, cmod_iter [, cmod_dfid], one reduction, one host read.  out: OUT_R2 = ||X - Y||^2,
 * OUT_AX2 = ||X||^2, OUT_Y2, OUT_S2 = ||Y - Yprev||^2 (rho applied by the host), OUT_U2, OUT_CNSTR =
 * ||Pcn(g) - g||^2, OUT_DFID = ||f Z - S||^2 (the host halves it).  U is stored with u_scale applied. */
int sporco_amd_cmod_iter(sporco_amd_cmod_t h, const sporco_amd_cmod_params *p, double out[SPORCO_AMD_OUT_COUNT]);
/* out[OUT_DFID] = ||V Z - S||^2 for V = variable `var` (X or Y) and the Z and S in use. */
int sporco_amd_cmod_dfid(sporco_amd_cmod_t h, int var, double out[SPORCO_AMD_OUT_COUNT]);
int sporco_amd_cmod_profile(sporco_amd_cmod_t h, int enable);
int sporco_amd_cmod_profile_read(sporco_amd_cmod_t h, int slot, const char **name, double *total_ms,
                                 int64_t *count);

/* ---- dense dictionary update by proximal gradient steps: sporco.pgm.cmod CnstrMOD / WeightedCnstrMOD
 * (sporco/pgm/cmod.py:24-407) ----
 *     minimise (1/2) ||D Z - S||^2_W  such that  ||d_m|| = 1 [, mean(d_m) = 0 | d_m >= 0],   W = diag(w).
 * A handle of sporco_amd_cmod_pgm_create is a cmod handle (sync, plan, set_signal, set_coef, upload, download, dfid,
 * profile and destroy are those above; set_coef forms no Gram matrix, there is no solve matrix and no
 * sporco_amd_cmod_iter; sporco_amd_cmod_dfid takes SPORCO_AMD_CMOD_X and applies the weight) with the arrays of the
 * iteration: two X arrays (the iterate and the one before; `advance` swaps their roles), two Y arrays (`advance_y`
 * swaps them), G, Z, ZZ, all (N, M).  sporco_amd_cmod_plan gives out[3] = blocks of 32 rows, out[4] = 16-column tiles
 * of G per wave, out[6], out[7] = bytes of LDS of a workgroup of cmod_pgm_grad and of cmod_pgm_prox.  One call of
 * sporco_amd_cmod_pgm_step launches the phases it is asked for in the order of the bits below (csrc/csc_pgm_cmod.h)
 * and, with `finalize`, the fixed-order reduction of every sum.  All arrays start at zero. */
#define SPORCO_AMD_CMOD_XPRV 6  /* (N,M)  the iterate before X                                                 */
#define SPORCO_AMD_CMOD_YALT 7  /* (N,M)  the other Y array: the next Y after a prox phase with write_y, the Y of
                                          the iteration before under the robust rule                           */
#define SPORCO_AMD_CMOD_PG 8    /* (N,M)  the gradient (w (Y Z - S)) Z^T of the last gradient phase             */
#define SPORCO_AMD_CMOD_PZ 9    /* (N,M)  robust rule: Z                                                       */
#define SPORCO_AMD_CMOD_ZZ 10   /* (N,M)  Monotone: the X' of the last step before a revert                    */
#define SPORCO_AMD_PGMC_PHASE_YROBUST 1 /* [Z += zc (Xprv - Yprv);] Y = (tk Xprv + t Z) / (tk + t)             */
#define SPORCO_AMD_PGMC_PHASE_GRAD 2    /* G from Y: cmod_pgm_grad, cmod_pgm_reduce (two launches, one pass over K) */
#define SPORCO_AMD_PGMC_PHASE_GZ2 4     /* ||G Z||^2: cmod_dfid on G (one pass over K)                         */
#define SPORCO_AMD_PGMC_PHASE_PROX 8    /* X' = Pcn(Y - G / L) and the next Y: cmod_pgm_prox                   */
#define SPORCO_AMD_PGMC_PHASE_DFID 16   /* F(X'): cmod_dfid with the weight (one pass over K)                  */
/* out[] of sporco_amd_cmod_pgm_step (the halves applied) */
#define SPORCO_AMD_PGMC_FY 0    /* f(Y) = (1/2) sum w (Y Z - S)^2        (gradient phase)                      */
#define SPORCO_AMD_PGMC_FX 1    /* f(X')                                  (dfid phase)                          */
#define SPORCO_AMD_PGMC_DXG 2   /* <X' - Y, G>                            (prox phase)                          */
#define SPORCO_AMD_PGMC_DXY2 3  /* ||X' - Y||^2                                                                */
#define SPORCO_AMD_PGMC_CNSTR 4 /* ||Pcn(X') - X'||^2                                                          */
#define SPORCO_AMD_PGMC_RS2 6   /* ||X' - Yprv||^2 (Yprv: Y unless yprv_alt)                                   */
#define SPORCO_AMD_PGMC_G2 7    /* ||G||^2                                (gradient phase)                      */
#define SPORCO_AMD_PGMC_GZ2 8   /* ||G Z||^2                              (gz2 phase)                           */
#define SPORCO_AMD_PGMC_BBXG 9  /* <Xprv - Xold, G - Gold>                (gradient phase, bb)                  */
#define SPORCO_AMD_PGMC_BBG2 10 /* ||G - Gold||^2                                                              */
typedef struct {
    double L;
    double w;                 /* the scalar weight, read where no array is set                               */
    double beta, gamma;       /* prox phase: Ynext = X' + gamma (ZZ - X') + beta (X' - Xprv); the gamma term
                                 under revert only (elsewhere ZZ = X')                                       */
    double tk, t, zc;         /* robust rule                                                                 */
    int32_t phase;            /* SPORCO_AMD_PGMC_PHASE_*                                                     */
    int32_t advance;          /* first: X becomes Xprv and the array of the iterate before it receives X'    */
    int32_t advance_y;        /* ... and the Y arrays change roles                                           */
    int32_t zero_mean, nonneg; /* the projection: ZeroMean, NonNegCoef (not both)                            */
    int32_t revert;           /* prox phase: X' = Xprv (Monotone's revert) with the sums of that X'          */
    int32_t z_update;         /* robust rule: apply zc first                                                 */
    int32_t bb;               /* gradient phase: form BBXG, BBG2 against the G of the gradient phase before  */
    int32_t keep_zz;          /* prox phase: also store X' to ZZ                                             */
    int32_t write_y;          /* prox phase: store Ynext in the other Y array                                */
    int32_t yprv_alt;         /* prox phase: Yprv of RS2 is the other Y array (robust rule)                  */
    int32_t finalize;         /* reduce the sums; out == NULL: without reading them back                     */
    int32_t rs_ynext;         /* prox phase: RS2 = ||X' - Ynext||^2 (the residual under Monotone)              */
} sporco_amd_cmod_pgm_params;
int sporco_amd_cmod_pgm_create(int dtype, int32_t N, int32_t M, int64_t K, int device, void *stream,
                               sporco_amd_cmod_t *out);
/* W (N, K) in the handle's precision, host or (on_device) read in place as S and Z are; NULL: the scalar w. */
int sporco_amd_cmod_pgm_set_weight(sporco_amd_cmod_t h, const void *W, int on_device);
int sporco_amd_cmod_pgm_step(sporco_amd_cmod_t h, const sporco_amd_cmod_pgm_params *p, double out[SPORCO_AMD_OUT_COUNT]);

/* ---- robust PCA: sporco.admm.rpca RobustPCA (sporco/admm/rpca.py:23-262) and sporco.prox prox_nuclear ----
 *     minimise ||X||_* + lambda ||Y||_1  such that  X + Y = S,
 * S, X, Y, U (R, C) row-major as NumPy has them, n = min(R, C) <= SPORCO_AMD_RPCA_MAX_DIM, R C < 2^31.  The x step
 * needs no SVD on the device: sporco_amd_rpca_gram leaves the n x n Gram matrix G of V = S - Y - U (V^T V for
 * R >= C, else V V^T; csrc/csc_rpca.h) in double, the caller takes eigh(G) = W diag(sigma^2) W^T and hands
 * T = W diag(max(0, 1 - (1 / rho) / sigma)) W^T to sporco_amd_rpca_iter, which forms X = V T (T V), relaxes, shrinks
 * Y, updates U and sums in one launch.  Gram products run on the float64 matrix instruction for both dtypes, the
 * product with T on the float32 one (float64: fma chains); SPORCO_AMD_RPCA_PLAIN=1 makes fma chains of both.
 * X, Y, U start at zero. */
typedef struct sporco_amd_rpca *sporco_amd_rpca_t;
#define SPORCO_AMD_RPCA_MAX_DIM 512 /* the largest min(R, C) */
#define SPORCO_AMD_RPCA_X 0      /* (R,C)  the result of the x step (of sporco_amd_rpca_apply)                */
#define SPORCO_AMD_RPCA_Y 1      /* (R,C)                                                                    */
#define SPORCO_AMD_RPCA_U 2      /* (R,C)  (without a pending u_scale)                                       */
#define SPORCO_AMD_RPCA_V_SYU 0  /* sporco_amd_rpca_gram of S - Y - u_scale U: the x step                     */
#define SPORCO_AMD_RPCA_V_SY 1   /* ... of S - Y: the nuclear norm term evaluated at Y (fEvalX off)          */
#define SPORCO_AMD_RPCA_V_S 2    /* ... of S alone: the stateless prox_nuclear / norm_nuclear                */
typedef struct {
    double rho, lmbda, rlx;
    double u_scale;           /* pending U /= rsf (admm.py:573): gram and iter apply it, iter stores U with it */
} sporco_amd_rpca_params;
int sporco_amd_rpca_create(int dtype, int32_t R, int32_t C, int device, void *stream, sporco_amd_rpca_t *out);
int sporco_amd_rpca_destroy(sporco_amd_rpca_t h);
int sporco_amd_rpca_sync(sporco_amd_rpca_t h);
/* out[0] = positions of the long axis staged per step of rpca_gram, out[1] = positions of a slab, out[2] = slabs,
 * out[3] = 64 x 64 blocks a side of G, out[4] = positions of a block of rpca_iter, out[5] = its workgroups,
 * out[6], out[7] = 1 where rpca_gram / rpca_iter use a matrix instruction, out[8], out[9] = bytes of LDS of a
 * workgroup of rpca_gram and of rpca_iter. */
int sporco_amd_rpca_plan(sporco_amd_rpca_t h, int64_t out[10]);
/* S (R, C) in the handle's precision.  on_device: a device pointer that is read in place, not copied; it stays
 * valid and unchanged until the next set_signal or the handle's end.  Forms ||S||^2 (OUT_C2 of every later out). */
int sporco_amd_rpca_set_signal(sporco_amd_rpca_t h, const void *S, int on_device);
/* Copy a host (R, C) array in or out. */
int sporco_amd_rpca_upload(sporco_amd_rpca_t h, int var, const void *src);
int sporco_amd_rpca_download(sporco_amd_rpca_t h, int var, void *dst);
/* *out = the device buffer of X, Y or U, valid while the handle lives. */
int sporco_amd_rpca_devptr(sporco_amd_rpca_t h, int var, void **out);
/* G (host, n x n doubles) <- the Gram matrix of V by `mode`: rpca_gram, rpca_gram_reduce, one download. */
int sporco_amd_rpca_gram(sporco_amd_rpca_t h, int mode, double u_scale, double *G);
/* One iteration after the host step.  T: host (n, n) doubles, symmetric.  out: OUT_R2 = ||X + Y - S||^2,
 * OUT_S2 = ||Y - Yprev||^2 (rho applied by the host), OUT_AX2 = ||X||^2, OUT_Y2, OUT_U2, OUT_L1 = sum |Y|,
 * OUT_L21 = sum |S - X| (NrmL1 with gEvalY off), OUT_C2 = ||S||^2.  U is stored with u_scale applied. */
int sporco_amd_rpca_iter(sporco_amd_rpca_t h, const sporco_amd_rpca_params *p, const double *T,
                         double out[SPORCO_AMD_OUT_COUNT]);
/* X <- S T (R >= C) or T S: singular value thresholding of the signal itself.  Y and U are not touched. */
int sporco_amd_rpca_apply(sporco_amd_rpca_t h, const double *T);
int sporco_amd_rpca_profile(sporco_amd_rpca_t h, int enable);
int sporco_amd_rpca_profile_read(sporco_amd_rpca_t h, int slot, const char **name, double *total_ms,
                                 int64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* SPORCO_AMD_H */
