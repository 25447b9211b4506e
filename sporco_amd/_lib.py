"""ctypes binding of libsporco_amd.so (the C ABI declared in include/sporco_amd.h).

There is exactly one compute path: the HIP library built for gfx950.  If the
shared object is missing, or no AMD GPU is visible, the functions here raise
:class:`BackendError`; nothing falls back to NumPy.
"""

import ctypes
import os

import numpy as np

F32, F64 = 0, 1

VAR_Y, VAR_U, VAR_X, VAR_XF, VAR_DF, VAR_SF = 0, 1, 2, 3, 4, 5
VAR_YF, VAR_XFPRV, VAR_YFPRV, VAR_VF, VAR_GF, VAR_AX, VAR_YPREV = 6, 7, 8, 9, 10, 11, 12
VAR_T0, VAR_T1, VAR_T2, VAR_ZF = 13, 14, 15, 16
VAR_CX, VAR_CU = 17, 18
VAR_MY0, VAR_MU0 = 19, 20
VAR_DMY0, VAR_DMU0 = 21, 22
VAR_WML, VAR_WMS = 23, 24
VAR_TVY, VAR_TVU = 25, 26
VAR_RTVY1, VAR_RTVU1 = 27, 28
VAR_DX, VAR_DXF, VAR_DYF, VAR_DXFPRV, VAR_DYFPRV = 32, 33, 34, 35, 36
VAR_DVF, VAR_DGF, VAR_DT0, VAR_DT1, VAR_DT2 = 37, 38, 39, 40, 41
VAR_DSX, VAR_DSU = 42, 43
DSTEP_ISM, DSTEP_CG = 0, 1

FLAG_NONNEG = 1 << 0
FLAG_NOBNDRY = 1 << 1
FLAG_JOINT = 1 << 2
FLAG_RESID = 1 << 3
FLAG_OBJ = 1 << 4
FLAG_XRRS = 1 << 5
FLAG_GEVAL_Y = 1 << 6
FLAG_FEVAL_Y = 1 << 7
FLAG_KEEP_X = 1 << 8
FLAG_NO_X = 1 << 9
FLAG_GRADREG = 1 << 10
FLAG_AMS = 1 << 11
FLAG_DMASK = 1 << 12
QUERY_FUSED_COLS, QUERY_FUSED_ROWS, QUERY_FUSED_PGM, QUERY_DEVICE_FILTERS, QUERY_VFORM_LIVE = 0, 1, 2, 3, 4
QUERY_PERSIST_RUNS = 5
QUERY_CCMOD_GROUPS = 6
QUERY_PD_WAVE_LAUNCHES, QUERY_PD_GENERIC_LAUNCHES = 7, 8
QUERY_PDL1_WAVE_LAUNCHES, QUERY_PDL1_GENERIC_LAUNCHES = 10, 11
QUERY_COLS_SM_FORM = 9
HINT_KEEP_VFORM = 0
HINT_ONE_LAUNCH = 1
MODE_COMPLEX_PAIR = 2
VOLUME_FILTER_DEPTH = 3

OUT_R2, OUT_S2, OUT_AX2, OUT_Y2, OUT_U2 = 0, 1, 2, 3, 4
OUT_DFID, OUT_L1, OUT_L21 = 5, 6, 7
OUT_XRRS_D2, OUT_XRRS_AX2, OUT_XRRS_B2 = 8, 9, 10
OUT_RGR = 11
OUT_CNSTR = 12
OUT_CGIT, OUT_CGN = 13, 14
OUT_C2 = 12                    # tvl1 handles: ||S||^2 of the primal normaliser
OUT_R02 = 14                 # pdl1_iter: block 0's |AXnr - y0 - s|^2
OUT_SN2, OUT_RGRX = 14, 15      # l1l1_iter: |A^T u|^2, and RegGrad's sum beside block 0's use of OUT_RGR
OUT_COUNT = 16

PGM_F, PGM_DFID, PGM_L1, PGM_HESS, PGM_RSDL, PGM_FY, PGM_LIN, PGM_DXY2 = range(8)

EXPORTS = (
    'sporco_amd_version', 'sporco_amd_last_error', 'sporco_amd_device_count',
    'sporco_amd_device_info', 'sporco_amd_csc_create', 'sporco_amd_csc_create_mc', 'sporco_amd_csc_create_volume',
    'sporco_amd_csc_destroy',
    'sporco_amd_csc_sync', 'sporco_amd_csc_stream', 'sporco_amd_csc_query', 'sporco_amd_csc_placement_report', 'sporco_amd_csc_set_hint', 'sporco_amd_csc_set_signal', 'sporco_amd_csc_set_dict', 'sporco_amd_csc_set_dict_imag',
    'sporco_amd_csc_set_l1_weight', 'sporco_amd_csc_set_l21_weight',
    'sporco_amd_csc_set_grad_weight', 'sporco_amd_csc_set_ams_mask',
    'sporco_amd_csc_upload', 'sporco_amd_csc_download', 'sporco_amd_csc_device_ptr',
    'sporco_amd_csc_admm_iter', 'sporco_amd_csc_admm_iter_dev', 'sporco_amd_csc_admm_run',
    'sporco_amd_csc_admm_xstep', 'sporco_amd_csc_admm_relax',
    'sporco_amd_csc_admm_ystep', 'sporco_amd_csc_admm_ustep',
    'sporco_amd_csc_admm_stats', 'sporco_amd_csc_scale_u',
    'sporco_amd_csc_reconstruct', 'sporco_amd_csc_dhs_absmax',
    'sporco_amd_csc_pgm_grad', 'sporco_amd_csc_pgm_eval', 'sporco_amd_csc_pgm_prox_step',
    'sporco_amd_csc_pgm_iter', 'sporco_amd_csc_pgm_commit',
    'sporco_amd_csc_lincomb', 'sporco_amd_csc_pair_stats', 'sporco_amd_csc_copy',
    'sporco_amd_csc_pgm_resid', 'sporco_amd_csc_pgm_resid_stats',
    'sporco_amd_csc_fft_var', 'sporco_amd_csc_ifft_var',
    'sporco_amd_csc_ccmod_setcoef', 'sporco_amd_csc_ccmod_grad', 'sporco_amd_csc_ccmod_eval',
    'sporco_amd_csc_ccmod_prox_step', 'sporco_amd_csc_ccmod_cnstr',
    'sporco_amd_csc_ccmod_getdict', 'sporco_amd_csc_setdict_from_dstep', 'sporco_amd_csc_asum',
    'sporco_amd_csc_set_filter_sizes', 'sporco_amd_csc_cns_init', 'sporco_amd_csc_cns_iter', 'sporco_amd_csc_cns_md_init', 'sporco_amd_csc_cns_mean_ptr',
    'sporco_amd_csc_dstep_init', 'sporco_amd_csc_dstep_iter', 'sporco_amd_csc_ccmod_sgd_step',
    'sporco_amd_csc_mdcpl_init', 'sporco_amd_csc_mdcpl_iter', 'sporco_amd_csc_l1l1_iter', 'sporco_amd_csc_ball_iter', 'sporco_amd_csc_projl1_iter', 'sporco_amd_csc_dstep_md_init',
    'sporco_amd_csc_set_data_mask', 'sporco_amd_csc_masked_grad',
    'sporco_amd_csc_inhib_setup', 'sporco_amd_csc_inhib_update',
    'sporco_amd_csc_tv_setup', 'sporco_amd_csc_tv_xstep', 'sporco_amd_csc_tv_ystep', 'sporco_amd_csc_tv_adjoint',
    'sporco_amd_csc_rtv_setup', 'sporco_amd_csc_rtv_xstep', 'sporco_amd_csc_rtv_ystep', 'sporco_amd_csc_rtv_dual',
    'sporco_amd_csc_pd_setup', 'sporco_amd_csc_pd_xstep', 'sporco_amd_csc_pd_dfid', 'sporco_amd_csc_pd_reconstruct',
    'sporco_amd_csc_pdl1_setup', 'sporco_amd_csc_pdl1_block0', 'sporco_amd_csc_pdl1_iter',
    'sporco_amd_csc_profile', 'sporco_amd_csc_profile_read', 'sporco_amd_profile_slots',
    'sporco_amd_dev_malloc', 'sporco_amd_dev_free', 'sporco_amd_dev_upload',
    'sporco_amd_dev_download', 'sporco_amd_dev_axpby', 'sporco_amd_tikhonov_filter_dev',
    'sporco_amd_fftconv_dev', 'sporco_amd_csc_set_signal_dev', 'sporco_amd_csc_reconstruct_dev',
    'sporco_amd_transfer_stats',
    'sporco_amd_comm_unique_id', 'sporco_amd_comm_create', 'sporco_amd_comm_destroy',
    'sporco_amd_comm_info', 'sporco_amd_comm_allreduce', 'sporco_amd_comm_allreduce_host',
    'sporco_amd_csc_set_comm',
    'sporco_amd_rfftn2', 'sporco_amd_irfftn2', 'sporco_amd_solvedbi_sm',
    'sporco_amd_inner', 'sporco_amd_prox_l1', 'sporco_amd_prox_l1w', 'sporco_amd_prox_sl1l2',
    'sporco_amd_proj_l2', 'sporco_amd_proj_l1', 'sporco_amd_proj_l1_cols', 'sporco_amd_rfl2norm2',
    'sporco_amd_dev_mul',
    'sporco_amd_tvd_create', 'sporco_amd_tvl1_create', 'sporco_amd_tvd_destroy', 'sporco_amd_tvd_sync', 'sporco_amd_tvd_plan',
    'sporco_amd_tvd_upload', 'sporco_amd_tvd_download', 'sporco_amd_tvd_sweeps', 'sporco_amd_tvd_gsres',
    'sporco_amd_tvd_ystep', 'sporco_amd_tvd_adjoint', 'sporco_amd_tvd_profile', 'sporco_amd_tvd_profile_read',
    'sporco_amd_tvdc_create', 'sporco_amd_tvl1dc_create', 'sporco_amd_tvdc_destroy', 'sporco_amd_tvdc_sync',
    'sporco_amd_tvdc_plan', 'sporco_amd_tvdc_upload', 'sporco_amd_tvdc_download', 'sporco_amd_tvdc_set_kernel',
    'sporco_amd_tvdc_xstep', 'sporco_amd_tvdc_ystep', 'sporco_amd_tvdc_adjoint', 'sporco_amd_tvdc_profile',
    'sporco_amd_tvdc_profile_read',
    'sporco_amd_spl_create', 'sporco_amd_spl_destroy', 'sporco_amd_spl_sync', 'sporco_amd_spl_plan',
    'sporco_amd_spl_upload', 'sporco_amd_spl_download', 'sporco_amd_spl_xstep', 'sporco_amd_spl_ystep',
    'sporco_amd_spl_profile', 'sporco_amd_spl_profile_read', 'sporco_amd_dctii', 'sporco_amd_idctii',
    'sporco_amd_bpdn_create', 'sporco_amd_bpdn_destroy', 'sporco_amd_bpdn_sync', 'sporco_amd_bpdn_plan',
    'sporco_amd_bpdn_set_dict', 'sporco_amd_bpdn_set_solve', 'sporco_amd_bpdn_upload', 'sporco_amd_bpdn_download',
    'sporco_amd_bpdn_iter', 'sporco_amd_bpdn_profile', 'sporco_amd_bpdn_profile_read', 'sporco_amd_bpdn_devptr',
    'sporco_amd_bpdn_pgm_create', 'sporco_amd_bpdn_pgm_step', 'sporco_amd_bpdn_pgm_ystep', 'sporco_amd_bpdn_pgm_copy',
    'sporco_amd_cmod_create', 'sporco_amd_cmod_destroy', 'sporco_amd_cmod_sync', 'sporco_amd_cmod_plan',
    'sporco_amd_cmod_set_signal', 'sporco_amd_cmod_set_coef', 'sporco_amd_cmod_set_solve', 'sporco_amd_cmod_upload',
    'sporco_amd_cmod_download', 'sporco_amd_cmod_iter', 'sporco_amd_cmod_dfid', 'sporco_amd_cmod_profile',
    'sporco_amd_cmod_profile_read',
    'sporco_amd_cmod_pgm_create', 'sporco_amd_cmod_pgm_set_weight', 'sporco_amd_cmod_pgm_step',
    'sporco_amd_rpca_create', 'sporco_amd_rpca_destroy', 'sporco_amd_rpca_sync', 'sporco_amd_rpca_plan',
    'sporco_amd_rpca_set_signal', 'sporco_amd_rpca_upload', 'sporco_amd_rpca_download', 'sporco_amd_rpca_devptr',
    'sporco_amd_rpca_gram', 'sporco_amd_rpca_iter', 'sporco_amd_rpca_apply', 'sporco_amd_rpca_profile',
    'sporco_amd_rpca_profile_read',
)


class BackendError(RuntimeError):
    """The HIP backend is missing, failed to load, or reported an error."""


class Dims(ctypes.Structure):
    _fields_ = [('H', ctypes.c_int32), ('W', ctypes.c_int32), ('C', ctypes.c_int32),
                ('N', ctypes.c_int32), ('K', ctypes.c_int32), ('dtype', ctypes.c_int32)]


class PgmParams(ctypes.Structure):
    _fields_ = [('L', ctypes.c_double), ('lmbda', ctypes.c_double), ('beta', ctypes.c_double),
                ('flags', ctypes.c_uint32), ('dH', ctypes.c_int32), ('dW', ctypes.c_int32),
                ('want_stats', ctypes.c_int32), ('hold', ctypes.c_int32)]


class CnsParams(ctypes.Structure):
    _fields_ = [('rho', ctypes.c_double), ('rlx', ctypes.c_double), ('u_scale', ctypes.c_double),
                ('flags', ctypes.c_uint32), ('dH', ctypes.c_int32), ('dW', ctypes.c_int32),
                ('zero_mean', ctypes.c_int32), ('mask_dcpl', ctypes.c_int32),
                ('phase', ctypes.c_int32)]


class DstepParams(ctypes.Structure):
    _fields_ = [('rho', ctypes.c_double), ('rlx', ctypes.c_double), ('u_scale', ctypes.c_double),
                ('cg_tol', ctypes.c_double), ('flags', ctypes.c_uint32), ('dH', ctypes.c_int32),
                ('dW', ctypes.c_int32), ('zero_mean', ctypes.c_int32), ('method', ctypes.c_int32),
                ('cg_maxiter', ctypes.c_int32), ('mask_dcpl', ctypes.c_int32)]


class AdmmCtrl(ctypes.Structure):
    """sporco_amd_admm_ctrl (include/sporco_amd.h): constants of a device-driven solve."""
    _fields_ = [('abs_tol', ctypes.c_double), ('rel_tol', ctypes.c_double),
                ('sqrt_nc', ctypes.c_double), ('sqrt_nx', ctypes.c_double),
                ('rho_tau', ctypes.c_double), ('rho_mu', ctypes.c_double),
                ('rho_xi', ctypes.c_double),
                ('auto_rho', ctypes.c_int32), ('period', ctypes.c_int32),
                ('auto_scaling', ctypes.c_int32), ('std_residuals', ctypes.c_int32),
                ('need_residuals', ctypes.c_int32), ('k0', ctypes.c_int32),
                ('max_iter', ctypes.c_int32), ('lookahead', ctypes.c_int32)]


class AdmmRecord(ctypes.Structure):
    """sporco_amd_admm_record: what one iteration of a device-driven solve leaves behind."""
    _fields_ = [('sums', ctypes.c_double * 16), ('r', ctypes.c_double), ('s', ctypes.c_double),
                ('epri', ctypes.c_double), ('edua', ctypes.c_double), ('rho', ctypes.c_double),
                ('u_scale', ctypes.c_double), ('seconds', ctypes.c_double),
                ('k', ctypes.c_int32), ('stop', ctypes.c_int32)]


class InhibParams(ctypes.Structure):
    """sporco_amd_inhib_params: scalars of one inhibition-weight update."""
    _fields_ = [('lmbda', ctypes.c_double), ('mu', ctypes.c_double), ('gamma', ctypes.c_double),
                ('smooth', ctypes.c_double), ('flags', ctypes.c_uint32)]


class TvdParams(ctypes.Structure):
    """sporco_amd_tvd_params: scalars of one TVL2Denoise launch group."""
    _fields_ = [('rho', ctypes.c_double), ('lmbda', ctypes.c_double), ('rlx', ctypes.c_double),
                ('u_scale', ctypes.c_double), ('wdf', ctypes.c_double), ('wtv', ctypes.c_double),
                ('geval_y', ctypes.c_int32)]


TVD_S, TVD_X, TVD_Y, TVD_U, TVD_WDF, TVD_WTV = range(6)


class TvdcParams(ctypes.Structure):
    """sporco_amd_tvdc_params: scalars of one TVL2Deconv / TVL1Deconv step."""
    _fields_ = [('rho', ctypes.c_double), ('lmbda', ctypes.c_double), ('rlx', ctypes.c_double),
                ('u_scale', ctypes.c_double), ('wdf', ctypes.c_double), ('wtv', ctypes.c_double),
                ('geval_y', ctypes.c_int32), ('lin_solve_check', ctypes.c_int32), ('want_rsdl', ctypes.c_int32),
                ('want_stats', ctypes.c_int32)]


TVDC_S, TVDC_X, TVDC_Y, TVDC_U, TVDC_WDF, TVDC_WTV, TVDC_HX = range(7)


class SplParams(ctypes.Structure):
    """sporco_amd_spl_params: scalars of one SplineL1 step."""
    _fields_ = [('rho', ctypes.c_double), ('lmbda', ctypes.c_double), ('rlx', ctypes.c_double),
                ('u_scale', ctypes.c_double), ('wdf', ctypes.c_double),
                ('geval_y', ctypes.c_int32), ('lin_solve_check', ctypes.c_int32), ('want_stats', ctypes.c_int32),
                ('reserved', ctypes.c_int32)]


SPL_S, SPL_X, SPL_Y, SPL_U, SPL_WDF = range(5)


class BpdnParams(ctypes.Structure):
    """sporco_amd_bpdn_params: scalars of one BPDN / BPDNJoint / ElasticNet / BPDNProjL1 iteration.  ``proj_l1``: the
    y step projects every column onto the l1 ball, ``lmbda`` carries its radius gamma and the sums come back with
    ``OUT_BPDN_CNSTR``."""
    _fields_ = [('rho', ctypes.c_double), ('lmbda', ctypes.c_double), ('mu', ctypes.c_double),
                ('rlx', ctypes.c_double), ('u_scale', ctypes.c_double), ('wl1', ctypes.c_double),
                ('c', ctypes.c_double),
                ('nonneg', ctypes.c_int32), ('feval_x', ctypes.c_int32), ('geval_y', ctypes.c_int32),
                ('want_x', ctypes.c_int32), ('joint', ctypes.c_int32), ('lin_solve_check', ctypes.c_int32),
                ('proj_l1', ctypes.c_int32), ('reserved', ctypes.c_int32)]


OUT_BPDN_CNSTR = OUT_CNSTR     # bpdn_iter with proj_l1: sum (proj_l1(g, gamma) - g)^2
BPDN_S, BPDN_X, BPDN_Y, BPDN_U, BPDN_WL1, BPDN_DTS = range(6)
BPDN_MAX_DIM = 512


class BpdnPgmParams(ctypes.Structure):
    """sporco_amd_bpdn_pgm_params: scalars and phases of one proximal gradient step of pgm.bpdn."""
    _fields_ = [('L', ctypes.c_double), ('lmbda', ctypes.c_double), ('wl1', ctypes.c_double), ('w', ctypes.c_double),
                ('beta', ctypes.c_double), ('tk', ctypes.c_double), ('t', ctypes.c_double), ('zc', ctypes.c_double),
                ('phase', ctypes.c_int32), ('ymode', ctypes.c_int32), ('advance', ctypes.c_int32),
                ('advance_y', ctypes.c_int32), ('nonneg', ctypes.c_int32), ('revert', ctypes.c_int32),
                ('z_update', ctypes.c_int32), ('cauchy', ctypes.c_int32), ('bb', ctypes.c_int32),
                ('keep_zz', ctypes.c_int32), ('reserved', ctypes.c_int32 * 2)]


# the arrays a handle of sporco_amd_bpdn_pgm_create adds, its phases, Y modes and out[] slots (SPORCO_AMD_PGMB_*)
BPDN_XPRV, BPDN_YPRV, BPDN_G, BPDN_Z, BPDN_ZZ, BPDN_W = range(6, 12)
PGMB_PHASE_GRAD, PGMB_PHASE_PROX = 1, 2
PGMB_Y_LOAD, PGMB_Y_MOMENTUM, PGMB_Y_ROBUST = range(3)
(PGMB_FY, PGMB_FX, PGMB_DXG, PGMB_DXY2, PGMB_L1, PGMB_X2, PGMB_RS2, PGMB_G2, PGMB_DG2, PGMB_BBXG,
 PGMB_BBG2) = range(11)


class CmodParams(ctypes.Structure):
    """sporco_amd_cmod_params: scalars of one CnstrMOD iteration."""
    _fields_ = [('rho', ctypes.c_double), ('rlx', ctypes.c_double), ('u_scale', ctypes.c_double),
                ('zero_mean', ctypes.c_int32), ('feval_x', ctypes.c_int32), ('geval_y', ctypes.c_int32),
                ('want_dfid', ctypes.c_int32)]


CMOD_X, CMOD_Y, CMOD_U, CMOD_SZT, CMOD_G, CMOD_SZTD = range(6)
CMOD_MAX_DIM = 512             # SPORCO_AMD_CMOD_MAX_DIM


class CmodPgmParams(ctypes.Structure):
    """sporco_amd_cmod_pgm_params: scalars and phases of one proximal gradient step of pgm.cmod."""
    _fields_ = [('L', ctypes.c_double), ('w', ctypes.c_double), ('beta', ctypes.c_double), ('gamma', ctypes.c_double),
                ('tk', ctypes.c_double), ('t', ctypes.c_double), ('zc', ctypes.c_double),
                ('phase', ctypes.c_int32), ('advance', ctypes.c_int32), ('advance_y', ctypes.c_int32),
                ('zero_mean', ctypes.c_int32), ('nonneg', ctypes.c_int32), ('revert', ctypes.c_int32),
                ('z_update', ctypes.c_int32), ('bb', ctypes.c_int32), ('keep_zz', ctypes.c_int32),
                ('write_y', ctypes.c_int32), ('yprv_alt', ctypes.c_int32), ('finalize', ctypes.c_int32),
                ('rs_ynext', ctypes.c_int32)]


# the arrays a handle of sporco_amd_cmod_pgm_create adds, its phases and out[] slots (SPORCO_AMD_PGMC_*)
CMOD_XPRV, CMOD_YALT, CMOD_PG, CMOD_PZ, CMOD_ZZ = range(6, 11)
PGMC_PHASE_YROBUST, PGMC_PHASE_GRAD, PGMC_PHASE_GZ2, PGMC_PHASE_PROX, PGMC_PHASE_DFID = 1, 2, 4, 8, 16
PGMC_FY, PGMC_FX, PGMC_DXG, PGMC_DXY2, PGMC_CNSTR = range(5)
PGMC_RS2, PGMC_G2, PGMC_GZ2, PGMC_BBXG, PGMC_BBG2 = range(6, 11)


class RpcaParams(ctypes.Structure):
    """sporco_amd_rpca_params: scalars of one RobustPCA iteration."""
    _fields_ = [('rho', ctypes.c_double), ('lmbda', ctypes.c_double), ('rlx', ctypes.c_double),
                ('u_scale', ctypes.c_double)]


RPCA_X, RPCA_Y, RPCA_U = range(3)
RPCA_V_SYU, RPCA_V_SY, RPCA_V_S = range(3)
RPCA_MAX_DIM = 512             # SPORCO_AMD_RPCA_MAX_DIM

REDUCE_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p)
EUNSUPPORTED = -5


class AdmmParams(ctypes.Structure):
    _fields_ = [('rho', ctypes.c_double), ('lmbda', ctypes.c_double),
                ('mu', ctypes.c_double), ('rlx', ctypes.c_double),
                ('u_scale', ctypes.c_double), ('flags', ctypes.c_uint32),
                ('dH', ctypes.c_int32), ('dW', ctypes.c_int32)]


_DEFAULT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                             'libsporco_amd.so')
_lib = None
_lib_path = None


def default_library_path():
    return _DEFAULT_PATH


def _share_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME libamdhip64.so.7) and
    link it by file name, so a process that loads this library (which needs the SONAME
    from /opt/rocm) *and* torch ends up with two HIP runtimes, and the second one to
    initialise finds no GPU.  torch.distributed is how the multi-GPU path talks to
    RCCL, so when torch is installed its copy is loaded first: the dynamic linker then
    resolves our dependency to it by SONAME and a later ``import torch`` reuses the
    same object.  SPORCO_AMD_SHARE_TORCH_RUNTIME=0 disables this."""
    if os.environ.get('SPORCO_AMD_SHARE_TORCH_RUNTIME', '1') == '0':
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec('torch')
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], 'lib', 'libamdhip64.so')
        if os.path.exists(cand):
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except Exception:
        pass     # fall back to the system runtime


def load(path=None):
    """Load the backend shared library (default: the in-tree hipcc build).

    ``path`` exists so that the test-suite can point the binding at the CPU
    fiber simulator build of the same sources (tests/hostsim); product code
    never passes it.
    """
    global _lib, _lib_path
    # (SPORCO_AMD_LIBRARY: an alternative hipcc build of the same sources, for A/B timing)
    path = os.path.abspath(path or os.environ.get('SPORCO_AMD_LIBRARY') or _DEFAULT_PATH)
    if not os.path.exists(path):
        raise BackendError(
            "sporco_amd: HIP library %s not found. Build it with "
            "`make -C sporco_amd/csrc` (or `python -c 'import __graft_entry__ as g; "
            "g.build()'`). There is no CPU fallback." % path)
    _share_torch_hip_runtime()
    try:
        lib = ctypes.CDLL(path)
    except OSError as e:
        raise BackendError("sporco_amd: cannot load %s: %s" % (path, e))
    missing = [s for s in EXPORTS if not hasattr(lib, s)]
    if missing:
        raise BackendError("sporco_amd: %s lacks symbols %s" % (path, missing))
    lib.sporco_amd_version.restype = ctypes.c_char_p
    lib.sporco_amd_last_error.restype = ctypes.c_char_p
    for name in EXPORTS:
        if name not in ('sporco_amd_version', 'sporco_amd_last_error'):
            getattr(lib, name).restype = ctypes.c_int
    lib.sporco_amd_csc_create.argtypes = [ctypes.POINTER(Dims), ctypes.c_int,
                                          ctypes.c_void_p,
                                          ctypes.POINTER(ctypes.c_void_p)]
    lib.sporco_amd_csc_create_mc.argtypes = [ctypes.POINTER(Dims), ctypes.c_int32, ctypes.c_int,
                                             ctypes.c_void_p,
                                             ctypes.POINTER(ctypes.c_void_p)]
    lib.sporco_amd_csc_create_volume.argtypes = lib.sporco_amd_csc_create_mc.argtypes
    vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    dptr = ctypes.POINTER(ctypes.c_double)
    pptr = ctypes.POINTER(AdmmParams)
    sig = {
        'sporco_amd_device_count': [ctypes.POINTER(ctypes.c_int)],
        'sporco_amd_device_info': [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t,
                                   ctypes.POINTER(ctypes.c_int),
                                   ctypes.POINTER(ctypes.c_size_t)],
        'sporco_amd_csc_destroy': [vp], 'sporco_amd_csc_sync': [vp],
        'sporco_amd_csc_stream': [vp, ctypes.POINTER(ctypes.c_void_p)],
        'sporco_amd_csc_query': [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)],
        'sporco_amd_csc_placement_report': [vp, ctypes.c_char_p, ctypes.c_size_t],
        'sporco_amd_csc_set_hint': [vp, ctypes.c_int, ctypes.c_int],
        'sporco_amd_csc_set_signal': [vp, vp],
        'sporco_amd_csc_set_dict': [vp, vp, i32, i32],
        'sporco_amd_csc_set_dict_imag': [vp, vp, i32, i32],
        'sporco_amd_csc_set_l1_weight': [vp, vp, ctypes.POINTER(i64)],
        'sporco_amd_csc_set_l21_weight': [vp, vp, ctypes.POINTER(i64)],
        'sporco_amd_csc_set_grad_weight': [vp, vp],
        'sporco_amd_csc_set_filter_sizes': [vp, ctypes.POINTER(ctypes.c_int32),
                                            ctypes.POINTER(ctypes.c_int32)],
        'sporco_amd_csc_set_ams_mask': [vp, vp, ctypes.POINTER(i64)],
        'sporco_amd_csc_upload': [vp, ctypes.c_int, vp],
        'sporco_amd_csc_download': [vp, ctypes.c_int, vp],
        'sporco_amd_csc_device_ptr': [vp, ctypes.c_int, ctypes.POINTER(vp)],
        'sporco_amd_csc_admm_iter': [vp, pptr, dptr],
        'sporco_amd_csc_admm_iter_dev': [vp, pptr, vp],
        'sporco_amd_csc_admm_run': [vp, pptr, ctypes.POINTER(AdmmCtrl), ctypes.POINTER(AdmmRecord),
                                    ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(dbl),
                                    ctypes.POINTER(dbl), REDUCE_FN, vp],
        'sporco_amd_csc_admm_xstep': [vp, pptr, dptr],
        'sporco_amd_csc_admm_relax': [vp, dbl],
        'sporco_amd_csc_admm_ystep': [vp, pptr],
        'sporco_amd_csc_admm_ustep': [vp, pptr],
        'sporco_amd_csc_admm_stats': [vp, pptr, dptr],
        'sporco_amd_csc_scale_u': [vp, dbl],
        'sporco_amd_csc_reconstruct': [vp, ctypes.c_int, vp],
        'sporco_amd_csc_dhs_absmax': [vp, dptr],
        'sporco_amd_csc_pgm_grad': [vp, ctypes.c_int, dptr],
        'sporco_amd_csc_pgm_eval': [vp, ctypes.c_int, dptr],
        'sporco_amd_csc_pgm_iter': [vp, ctypes.POINTER(PgmParams), dptr],
        'sporco_amd_csc_pgm_commit': [vp],
        'sporco_amd_csc_pgm_prox_step': [vp, dbl, dbl, ctypes.c_uint32, i32, i32, dptr],
        'sporco_amd_csc_lincomb': [vp, ctypes.c_int, dbl, ctypes.c_int, dbl, ctypes.c_int, dbl,
                                   ctypes.c_int],
        'sporco_amd_csc_pair_stats': [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, dptr],
        'sporco_amd_csc_pgm_resid': [vp, ctypes.c_int, ctypes.c_int],
        'sporco_amd_csc_pgm_resid_stats': [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, dptr],
        'sporco_amd_csc_copy': [vp, ctypes.c_int, ctypes.c_int],
        'sporco_amd_csc_fft_var': [vp, ctypes.c_int, ctypes.c_int],
        'sporco_amd_csc_ifft_var': [vp, ctypes.c_int, ctypes.c_int],
        'sporco_amd_csc_ccmod_setcoef': [vp, ctypes.c_int],
        'sporco_amd_csc_ccmod_grad': [vp, ctypes.c_int, dptr],
        'sporco_amd_csc_ccmod_eval': [vp, ctypes.c_int, dptr],
        'sporco_amd_csc_ccmod_prox_step': [vp, dbl, i32, i32, i32],
        'sporco_amd_csc_ccmod_cnstr': [vp, i32, i32, i32, dptr],
        'sporco_amd_csc_ccmod_getdict': [vp, i32, i32, vp],
        'sporco_amd_csc_cns_init': [vp, vp, dbl],
        'sporco_amd_csc_cns_md_init': [vp, vp],
        'sporco_amd_csc_cns_mean_ptr': [vp, ctypes.POINTER(vp), ctypes.POINTER(i64)],
        'sporco_amd_csc_set_data_mask': [vp, vp, ctypes.POINTER(i64)],
        'sporco_amd_csc_masked_grad': [vp, ctypes.c_int, i32, i32, dptr],
        'sporco_amd_csc_cns_iter': [vp, ctypes.POINTER(CnsParams), dptr],
        'sporco_amd_csc_ccmod_sgd_step': [vp, dbl, i32, i32, i32, dptr],
        'sporco_amd_csc_mdcpl_init': [vp, vp],
        'sporco_amd_csc_inhib_setup': [vp, dptr, i32, dptr, i32, dptr, i32, i32, dbl],
        'sporco_amd_csc_inhib_update': [vp, ctypes.POINTER(InhibParams), dptr],
        'sporco_amd_csc_tv_setup': [vp, dptr, i32, i32],
        'sporco_amd_csc_tv_xstep': [vp, ctypes.POINTER(AdmmParams), dptr],
        'sporco_amd_csc_tv_ystep': [vp, ctypes.POINTER(AdmmParams), dptr],
        'sporco_amd_csc_tv_adjoint': [vp, dbl, dptr],
        'sporco_amd_csc_rtv_setup': [vp, dptr, i32],
        'sporco_amd_csc_rtv_xstep': [vp, ctypes.POINTER(AdmmParams), dptr],
        'sporco_amd_csc_rtv_ystep': [vp, ctypes.POINTER(AdmmParams), dptr],
        'sporco_amd_csc_rtv_dual': [vp, ctypes.POINTER(AdmmParams), dptr],
        'sporco_amd_csc_pd_setup': [vp, dptr, dptr, dptr, vp, i32],
        'sporco_amd_csc_pd_xstep': [vp, ctypes.POINTER(AdmmParams), dptr],
        'sporco_amd_csc_pd_dfid': [vp, i32, dptr],
        'sporco_amd_csc_pd_reconstruct': [vp, i32, vp],
        'sporco_amd_csc_pdl1_setup': [vp, dptr, dptr, dptr, vp, i32, vp],
        'sporco_amd_csc_pdl1_block0': [vp, i32, i32, vp],
        'sporco_amd_csc_pdl1_iter': [vp, ctypes.POINTER(AdmmParams), dptr],
        'sporco_amd_csc_mdcpl_iter': [vp, ctypes.POINTER(AdmmParams), dptr],
        'sporco_amd_csc_l1l1_iter': [vp, ctypes.POINTER(AdmmParams), dptr],
        'sporco_amd_csc_ball_iter': [vp, ctypes.POINTER(AdmmParams), dptr],
        'sporco_amd_csc_projl1_iter': [vp, ctypes.POINTER(AdmmParams), dbl, dptr],
        'sporco_amd_csc_dstep_init': [vp, vp],
        'sporco_amd_csc_dstep_md_init': [vp, vp, vp],
        'sporco_amd_csc_dstep_iter': [vp, ctypes.POINTER(DstepParams), dptr],
        'sporco_amd_csc_setdict_from_dstep': [vp, i32, i32],
        'sporco_amd_csc_asum': [vp, ctypes.c_int, dptr],
        'sporco_amd_csc_profile': [vp, ctypes.c_int],
        'sporco_amd_csc_profile_read': [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p),
                                        dptr, ctypes.POINTER(i64)],
        'sporco_amd_profile_slots': [],
        'sporco_amd_rfftn2': [ctypes.c_int, i32, i32, i64, vp, vp],
        'sporco_amd_irfftn2': [ctypes.c_int, i32, i32, i64, vp, vp],
        'sporco_amd_solvedbi_sm': [ctypes.c_int, i64, i64, i32, vp, dbl, vp, vp],
        'sporco_amd_inner': [ctypes.c_int, i64, i64, i32, vp, vp, vp],
        'sporco_amd_dev_malloc': [ctypes.c_size_t, ctypes.POINTER(vp)],
        'sporco_amd_dev_free': [vp],
        'sporco_amd_dev_upload': [vp, vp, ctypes.c_size_t],
        'sporco_amd_dev_download': [vp, vp, ctypes.c_size_t],
        'sporco_amd_dev_axpby': [ctypes.c_int, i64, dbl, vp, dbl, vp, vp],
        'sporco_amd_tikhonov_filter_dev': [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, i64, vp, dbl,
                                           ctypes.c_int32, vp, vp],
        'sporco_amd_fftconv_dev': [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(i64),
                                   vp, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(i64), vp,
                                   ctypes.c_int32, ctypes.c_int32, vp],
        'sporco_amd_csc_set_signal_dev': [vp, vp],
        'sporco_amd_csc_reconstruct_dev': [vp, ctypes.c_int, vp],
        'sporco_amd_transfer_stats': [ctypes.POINTER(i64), ctypes.c_int],
        'sporco_amd_comm_unique_id': [vp],
        'sporco_amd_comm_create': [vp, i32, i32, i32, ctypes.POINTER(vp)],
        'sporco_amd_comm_destroy': [vp],
        'sporco_amd_comm_info': [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)],
        'sporco_amd_comm_allreduce': [vp, vp, i64, ctypes.c_int, ctypes.c_int, vp],
        'sporco_amd_comm_allreduce_host': [vp, dptr, i32, ctypes.c_int],
        'sporco_amd_csc_set_comm': [vp, vp],
        'sporco_amd_prox_l1': [ctypes.c_int, i64, vp, dbl, vp],
        'sporco_amd_prox_l1w': [ctypes.c_int, ctypes.POINTER(i64), vp, ctypes.POINTER(i64), vp, vp],
        'sporco_amd_prox_sl1l2': [ctypes.c_int, i64, i32, i64, vp, dbl, dbl, vp],
        'sporco_amd_proj_l2': [ctypes.c_int, i64, i64, i64, vp, dbl, vp],
        'sporco_amd_proj_l1': [ctypes.c_int, i64, i64, i64, vp, dbl, vp],
        'sporco_amd_proj_l1_cols': [ctypes.c_int, i32, i64, vp, dbl, vp],
        'sporco_amd_rfl2norm2': [ctypes.c_int, i32, i32, i64, vp, dptr],
        'sporco_amd_dev_mul': [ctypes.c_int, i64, vp, vp, vp],
        'sporco_amd_tvd_create': [ctypes.c_int, i32, i32, i64, i32, i32, ctypes.c_int, vp, ctypes.POINTER(vp)],
        'sporco_amd_tvl1_create': [ctypes.c_int, i32, i32, i64, i32, i32, ctypes.c_int, vp, ctypes.POINTER(vp)],
        'sporco_amd_tvd_destroy': [vp], 'sporco_amd_tvd_sync': [vp],
        'sporco_amd_tvd_plan': [vp, ctypes.POINTER(i64)],
        'sporco_amd_tvd_upload': [vp, ctypes.c_int, vp, ctypes.c_int],
        'sporco_amd_tvd_download': [vp, ctypes.c_int, vp, ctypes.c_int],
        'sporco_amd_tvd_sweeps': [vp, ctypes.POINTER(TvdParams), i32],
        'sporco_amd_tvd_gsres': [vp, ctypes.POINTER(TvdParams), dptr],
        'sporco_amd_tvd_ystep': [vp, ctypes.POINTER(TvdParams), dptr],
        'sporco_amd_tvd_adjoint': [vp],
        'sporco_amd_tvd_profile': [vp, ctypes.c_int],
        'sporco_amd_tvdc_create': [ctypes.c_int, i32, i32, i64, i32, i32, i64, ctypes.c_int, vp, ctypes.POINTER(vp)],
        'sporco_amd_tvl1dc_create': [ctypes.c_int, i32, i32, i64, i32, i32, i64, ctypes.c_int, vp, ctypes.POINTER(vp)],
        'sporco_amd_tvdc_destroy': [vp], 'sporco_amd_tvdc_sync': [vp],
        'sporco_amd_tvdc_plan': [vp, ctypes.POINTER(i64)],
        'sporco_amd_tvdc_upload': [vp, ctypes.c_int, vp, ctypes.c_int],
        'sporco_amd_tvdc_download': [vp, ctypes.c_int, vp, ctypes.c_int],
        'sporco_amd_tvdc_set_kernel': [vp, vp, i32, i32, ctypes.c_int],
        'sporco_amd_tvdc_xstep': [vp, ctypes.POINTER(TvdcParams)],
        'sporco_amd_tvdc_ystep': [vp, ctypes.POINTER(TvdcParams), dptr],
        'sporco_amd_tvdc_adjoint': [vp],
        'sporco_amd_tvdc_profile': [vp, ctypes.c_int],
        'sporco_amd_tvdc_profile_read': [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), dptr,
                                         ctypes.POINTER(ctypes.c_int64)],
        'sporco_amd_tvd_profile_read': [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), dptr,
                                        ctypes.POINTER(i64)],
        'sporco_amd_spl_create': [ctypes.c_int, i32, i32, i64, ctypes.c_int, vp, ctypes.POINTER(vp)],
        'sporco_amd_spl_destroy': [vp], 'sporco_amd_spl_sync': [vp],
        'sporco_amd_spl_plan': [vp, ctypes.POINTER(i64)],
        'sporco_amd_spl_upload': [vp, ctypes.c_int, vp, ctypes.c_int],
        'sporco_amd_spl_download': [vp, ctypes.c_int, vp, ctypes.c_int],
        'sporco_amd_spl_xstep': [vp, ctypes.POINTER(SplParams)],
        'sporco_amd_spl_ystep': [vp, ctypes.POINTER(SplParams), dptr],
        'sporco_amd_spl_profile': [vp, ctypes.c_int],
        'sporco_amd_bpdn_create': [ctypes.c_int, i32, i32, i64, ctypes.c_int, vp, ctypes.POINTER(vp)],
        'sporco_amd_bpdn_destroy': [vp], 'sporco_amd_bpdn_sync': [vp],
        'sporco_amd_bpdn_plan': [vp, ctypes.POINTER(i64)],
        'sporco_amd_bpdn_set_dict': [vp, vp], 'sporco_amd_bpdn_set_solve': [vp, vp],
        'sporco_amd_bpdn_upload': [vp, ctypes.c_int, vp],
        'sporco_amd_bpdn_download': [vp, ctypes.c_int, vp],
        'sporco_amd_bpdn_iter': [vp, ctypes.POINTER(BpdnParams), dptr],
        'sporco_amd_bpdn_profile': [vp, ctypes.c_int],
        'sporco_amd_bpdn_profile_read': [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), dptr,
                                         ctypes.POINTER(i64)],
        'sporco_amd_bpdn_devptr': [vp, ctypes.c_int, ctypes.POINTER(vp)],
        'sporco_amd_bpdn_pgm_create': [ctypes.c_int, i32, i32, i64, ctypes.c_int, vp, ctypes.POINTER(vp)],
        'sporco_amd_bpdn_pgm_step': [vp, ctypes.POINTER(BpdnPgmParams), dptr],
        'sporco_amd_bpdn_pgm_ystep': [vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, dptr],
        'sporco_amd_bpdn_pgm_copy': [vp, ctypes.c_int, ctypes.c_int],
        'sporco_amd_cmod_create': [ctypes.c_int, i32, i32, i64, ctypes.c_int, vp, ctypes.POINTER(vp)],
        'sporco_amd_cmod_destroy': [vp], 'sporco_amd_cmod_sync': [vp],
        'sporco_amd_cmod_plan': [vp, ctypes.POINTER(i64)],
        'sporco_amd_cmod_set_signal': [vp, vp, ctypes.c_int], 'sporco_amd_cmod_set_coef': [vp, vp, ctypes.c_int],
        'sporco_amd_cmod_set_solve': [vp, vp],
        'sporco_amd_cmod_upload': [vp, ctypes.c_int, vp],
        'sporco_amd_cmod_download': [vp, ctypes.c_int, vp],
        'sporco_amd_cmod_iter': [vp, ctypes.POINTER(CmodParams), dptr],
        'sporco_amd_cmod_dfid': [vp, ctypes.c_int, dptr],
        'sporco_amd_cmod_pgm_create': [ctypes.c_int, i32, i32, i64, ctypes.c_int, vp, ctypes.POINTER(vp)],
        'sporco_amd_cmod_pgm_set_weight': [vp, vp, ctypes.c_int],
        'sporco_amd_cmod_pgm_step': [vp, ctypes.POINTER(CmodPgmParams), dptr],
        'sporco_amd_cmod_profile': [vp, ctypes.c_int],
        'sporco_amd_cmod_profile_read': [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), dptr,
                                         ctypes.POINTER(i64)],
        'sporco_amd_rpca_create': [ctypes.c_int, i32, i32, ctypes.c_int, vp, ctypes.POINTER(vp)],
        'sporco_amd_rpca_destroy': [vp], 'sporco_amd_rpca_sync': [vp],
        'sporco_amd_rpca_plan': [vp, ctypes.POINTER(i64)],
        'sporco_amd_rpca_set_signal': [vp, vp, ctypes.c_int],
        'sporco_amd_rpca_upload': [vp, ctypes.c_int, vp],
        'sporco_amd_rpca_download': [vp, ctypes.c_int, vp],
        'sporco_amd_rpca_devptr': [vp, ctypes.c_int, ctypes.POINTER(vp)],
        'sporco_amd_rpca_gram': [vp, ctypes.c_int, dbl, vp],
        'sporco_amd_rpca_iter': [vp, ctypes.POINTER(RpcaParams), vp, dptr],
        'sporco_amd_rpca_apply': [vp, vp],
        'sporco_amd_rpca_profile': [vp, ctypes.c_int],
        'sporco_amd_rpca_profile_read': [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), dptr,
                                         ctypes.POINTER(i64)],
        'sporco_amd_spl_profile_read': [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), dptr,
                                        ctypes.POINTER(i64)],
        'sporco_amd_dctii': [ctypes.c_int, i32, i32, i64, vp, vp, ctypes.c_int],
        'sporco_amd_idctii': [ctypes.c_int, i32, i32, i64, vp, vp, ctypes.c_int],
    }
    for name, argtypes in sig.items():
        getattr(lib, name).argtypes = argtypes
    _lib, _lib_path = lib, path
    return lib


def lib():
    """Return the loaded library, loading the default one on first use."""
    if _lib is None:
        load()
    return _lib


def library_path():
    return _lib_path


def transfer_stats(reset=False):
    """Host <-> device traffic of the library since the last reset:
    ``{'h2d_bytes', 'h2d_calls', 'd2h_bytes', 'd2h_calls'}``."""
    out = (ctypes.c_int64 * 4)()
    check(lib().sporco_amd_transfer_stats(out, 1 if reset else 0))
    return dict(h2d_bytes=out[0], h2d_calls=out[1], d2h_bytes=out[2], d2h_calls=out[3])


def check(rc):
    if rc != 0:
        msg = lib().sporco_amd_last_error()
        raise BackendError("sporco_amd backend error %d: %s" %
                           (rc, msg.decode('utf-8', 'replace') if msg else '?'))


def device_count():
    n = ctypes.c_int(0)
    check(lib().sporco_amd_device_count(ctypes.byref(n)))
    return n.value


def device_info(device=0):
    name = ctypes.create_string_buffer(256)
    cu = ctypes.c_int(0)
    mem = ctypes.c_size_t(0)
    check(lib().sporco_amd_device_info(device, name, 256, ctypes.byref(cu),
                                       ctypes.byref(mem)))
    return name.value.decode(), cu.value, mem.value


def dtype_code(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return F32
    if dtype == np.float64:
        return F64
    raise TypeError("sporco_amd supports float32 and float64 data, not %s" % dtype)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _carr(a, dtype):
    a = np.asarray(a)
    if np.iscomplexobj(a) and not np.issubdtype(np.dtype(dtype), np.complexfloating):
        # (the reference solves complex-valued problems with complex FFTs,
        # sporco/admm/cbpdn.py:213-217; this backend's transforms are real-to-complex)
        raise NotImplementedError("complex-valued signals, dictionaries and weights are not "
                                  "supported by the sporco_amd backend")
    return np.ascontiguousarray(a, dtype=dtype)


class _Handle(object):
    """What the owners of an opaque C handle share.  ``_prefix`` names the family's entry points
    (``<_prefix>_destroy``, ``_sync``, ``_profile``, ``_profile_read``, ...)."""

    _prefix = None
    _all_slots = False      # profile_read returns every slot, not only those that ran

    def _open(self, create, *args):
        """``create(*args, &handle)``: the family's arguments, the device and the stream."""
        h = ctypes.c_void_p()
        check(create(*args, ctypes.byref(h)))
        self._h = h
        self._lib = lib()

    def _fn(self, name):
        return getattr(self._lib, self._prefix + '_' + name)

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self._fn('destroy')(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self._fn('sync')(self._h))

    def _sums(self, fn, *args):
        """``fn(handle, *args, out)``: the ``OUT_COUNT`` sums of a call as a list."""
        out = (ctypes.c_double * OUT_COUNT)()
        check(fn(self._h, *args, out))
        return list(out)

    def profile(self, enable):
        check(self._fn('profile')(self._h, 1 if enable else 0))

    def profile_read(self):
        """``{kernel: (total ms, launches)}`` since the last read, for the slots that ran (a
        :class:`Solver`: for every slot), and reset the counters."""
        res = {}
        read = self._fn('profile_read')
        for slot in range(self._lib.sporco_amd_profile_slots()):
            name, ms, cnt = ctypes.c_char_p(), ctypes.c_double(0.0), ctypes.c_int64(0)
            check(read(self._h, slot, ctypes.byref(name), ctypes.byref(ms), ctypes.byref(cnt)))
            if cnt.value or self._all_slots:
                res[name.value.decode()] = (ms.value, cnt.value)
        return res


class _PlaneArrays(object):
    """``upload`` / ``download`` of the handles whose variables are (H, W, P) arrays, host or device side; the class
    has ``var_shape(var)``."""

    def upload(self, var, a):
        """``a``: a host array, a device pointer (int) of an array of the variable's size, or None
        (a weight goes back to its scalar)."""
        up = self._fn('upload')
        if a is None:
            check(up(self._h, int(var), None, 0))
        elif isinstance(a, int):
            check(up(self._h, int(var), ctypes.c_void_p(a), 1))
        else:
            a = _carr(a, self.dtype)
            if a.size != int(np.prod(self.var_shape(var))):
                raise ValueError("array of %d elements for a variable of shape %s" % (a.size, self.var_shape(var)))
            check(up(self._h, int(var), _ptr(a), 0))

    def download(self, var, dst_ptr=None):
        """To a new host array, or (``dst_ptr``: device pointer) device to device."""
        if dst_ptr is not None:
            check(self._fn('download')(self._h, int(var), ctypes.c_void_p(dst_ptr), 1))
            return None
        out = np.empty(self.var_shape(var), dtype=self.dtype)
        check(self._fn('download')(self._h, int(var), _ptr(out), 0))
        return out


class Solver(_Handle):
    """Owner of one device-side ConvBPDN problem (opaque C handle)."""

    _prefix = 'sporco_amd_csc'
    _all_slots = True       # (the callers of profile_read filter)

    def __init__(self, H, W, C, N, K, dtype, device=0, stream=None, Cd=1, depth=1):
        """``C``: channels of the signal.  ``Cd`` > 1 (== C): multi-channel dictionary, the
        coefficient arrays then have a single channel (cnvrep.py:186-194).  ``depth`` > 1: a
        volume handle (dimN = 3), ``H`` = depth * height (include/sporco_amd.h
        sporco_amd_csc_create_volume)."""
        self.Cd = int(Cd)
        self.depth = int(depth)
        self.Cs = int(C)
        self.dims = (int(H), int(W), 1 if self.Cd > 1 else int(C), int(N), int(K))
        self.dtype = np.dtype(dtype)
        self.cdtype = np.dtype(np.complex64 if self.dtype == np.float32
                               else np.complex128)
        d = Dims(int(H), int(W), int(C), int(N), int(K), dtype_code(dtype))
        if self.depth > 1:
            self._open(lib().sporco_amd_csc_create_volume, ctypes.byref(d), self.depth, int(device),
                       ctypes.c_void_p(stream or 0))
        else:
            self._open(lib().sporco_amd_csc_create_mc, ctypes.byref(d), self.Cd, int(device),
                       ctypes.c_void_p(stream or 0))

    # -- shapes -----------------------------------------------------------
    @property
    def shape_x(self):
        return self.dims

    @property
    def shape_xf(self):
        H, W, C, N, K = self.dims
        return (H, W // 2 + 1, C, N, K)

    def var_shape_dtype(self, var):
        H, W, C, N, K = self.dims
        Wf = W // 2 + 1
        if var == VAR_DF:
            return (H, Wf, self.Cd, 1, K), self.cdtype
        if var == VAR_SF:
            return (H, Wf, self.Cs, N, 1), self.cdtype
        if var in (VAR_MY0, VAR_MU0, VAR_DMY0, VAR_DMU0):
            return (H, W, self.Cs, N, 1), self.dtype
        if var in (VAR_XF, VAR_YF, VAR_XFPRV, VAR_YFPRV, VAR_VF, VAR_GF, VAR_T0, VAR_T1, VAR_T2,
                   VAR_ZF):
            return (H, Wf, C, N, K), self.cdtype
        if var in (VAR_DX, VAR_DSX, VAR_DSU):
            return (H, W, self.Cd, 1, K), self.dtype
        if VAR_DXF <= var <= VAR_DT2:
            return (H, Wf, self.Cd, 1, K), self.cdtype
        if var in (VAR_CX, VAR_CU) and self.Cd > 1:
            # consensus copies of a multi-channel dictionary: one (Cd, K) block per image
            return (H, W, N, self.Cd, K), self.dtype
        if var in (VAR_TVY, VAR_TVU):
            return (3, H, W, C, N, K), self.dtype
        if var in (VAR_RTVY1, VAR_RTVU1):
            return (H, W, C, N, 2), self.dtype
        return (H, W, C, N, K), self.dtype

    # -- set-up -----------------------------------------------------------
    def stream_handle(self):
        """hipStream_t (as an int) of every launch this handle makes."""
        out = ctypes.c_void_p(0)
        check(self._lib.sporco_amd_csc_stream(self._h, ctypes.byref(out)))
        return int(out.value or 0)

    def set_hint(self, what, value):
        check(self._lib.sporco_amd_csc_set_hint(self._h, int(what), int(value)))

    def set_comm(self, comm_handle):
        """Attach a native RCCL communicator (sporco_amd_csc_set_comm; None detaches): the
        device-driven solve then all-reduces its per-iteration sums itself."""
        check(self._lib.sporco_amd_csc_set_comm(self._h, ctypes.c_void_p(comm_handle or 0)))

    def query(self, what):
        out = ctypes.c_int(0)
        check(self._lib.sporco_amd_csc_query(self._h, int(what), ctypes.byref(out)))
        return out.value

    def placement_report(self):
        """Where the handle put the arrays one kernel writes at the same time
        (sporco_amd_csc_placement_report): a list of dicts, one per decision."""
        import json
        buf = ctypes.create_string_buffer(8192)
        check(self._lib.sporco_amd_csc_placement_report(self._h, buf, len(buf)))
        return json.loads(buf.value.decode() or '[]')

    def _query(self, what):
        return bool(self.query(what))

    def uses_fused_cols(self):
        """True when the register-resident column kernel serves this shape."""
        return self._query(0)

    def uses_fused_rows(self):
        """True when an ADMM iteration runs as the three fused launches."""
        return self._query(1)

    def uses_fused_pgm(self):
        """True when pgm_iter / the tile-major D-step serve this shape."""
        return self._query(2)

    def set_signal(self, S):
        H, W, C, N, K = self.dims
        S = _carr(S, self.dtype).reshape(H, W, self.Cs, N)
        check(self._lib.sporco_amd_csc_set_signal(self._h, _ptr(S)))

    def set_dict(self, D):
        K = self.dims[4]
        D = _carr(D, self.dtype)
        dH, dW = D.shape[0], D.shape[1]
        D = D.reshape(dH, dW, self.Cd * K)      # (dH, dW, Cd, 1, K) is contiguous as (.., Cd K)
        check(self._lib.sporco_amd_csc_set_dict(self._h, _ptr(D), dH, dW))

    def set_dict_imag(self, D_imag):
        """The imaginary part of a complex dictionary (complex mode, sporco_amd_csc_set_dict_imag);
        None: back to a real dictionary."""
        if D_imag is None:
            check(self._lib.sporco_amd_csc_set_dict_imag(self._h, None, 1, 1))
            return
        K = self.dims[4]
        D = _carr(D_imag, self.dtype)
        dH, dW = D.shape[0], D.shape[1]
        check(self._lib.sporco_amd_csc_set_dict_imag(self._h, _ptr(D.reshape(dH, dW, K)), dH, dW))

    def _set_weight(self, fn, w):
        if w is None:
            check(fn(self._h, None, None))
            return
        w = _carr(w, self.dtype)
        shape = (ctypes.c_int64 * 5)(*w.shape)
        check(fn(self._h, _ptr(w), shape))

    def set_l1_weight(self, w):
        self._set_weight(self._lib.sporco_amd_csc_set_l1_weight, w)

    def set_l21_weight(self, w):
        self._set_weight(self._lib.sporco_amd_csc_set_l21_weight, w)

    def set_filter_sizes(self, sizes):
        """Per-filter supports [(rows, cols)] * K of a multi-scale dictionary, or None.
        (The call synchronises the stream and re-allocates two small device arrays: unchanged
        sizes -- an online learner sets them every step -- return at once.)"""
        key = None if sizes is None else tuple((int(s[0]), int(s[1])) for s in sizes)
        if getattr(self, '_filter_sizes_set', False) and getattr(self, '_filter_sizes', None) == key:
            return
        self._filter_sizes, self._filter_sizes_set = key, True
        if sizes is None:
            check(self._lib.sporco_amd_csc_set_filter_sizes(self._h, None, None))
            return
        H, W, C, N, K = self.dims
        if len(sizes) != K:
            self._filter_sizes_set = False
            raise ValueError("one (rows, cols) pair per filter")
        fh = (ctypes.c_int32 * K)(*[int(s[0]) for s in sizes])
        fw = (ctypes.c_int32 * K)(*[int(s[1]) for s in sizes])
        check(self._lib.sporco_amd_csc_set_filter_sizes(self._h, fh, fw))

    def set_ams_mask(self, w):
        """AddMaskSim mask, 5-D with every axis 1 or full and a singleton filter axis."""
        self._set_weight(self._lib.sporco_amd_csc_set_ams_mask, w)

    def set_data_mask(self, w):
        """Data-fidelity mask of the *Mask PGM classes, 5-D, singleton filter axis."""
        self._set_weight(self._lib.sporco_amd_csc_set_data_mask, w)

    def masked_grad(self, var, dstep, write_grad):
        """Masked data-fidelity gradient / evaluation (sporco_amd_csc_masked_grad)."""
        out = self._out()
        check(self._lib.sporco_amd_csc_masked_grad(self._h, int(var), 1 if dstep else 0,
                                                   int(write_grad), out))
        return list(out)

    def set_grad_weight(self, w):
        """K per-filter weights of the gradient penalty, or None for 1."""
        if w is None:
            check(self._lib.sporco_amd_csc_set_grad_weight(self._h, None))
            return
        w = _carr(w, self.dtype).ravel()
        if w.size != self.dims[4]:
            raise ValueError("GradWeight must hold one value per filter")
        check(self._lib.sporco_amd_csc_set_grad_weight(self._h, _ptr(w)))

    # -- transfers --------------------------------------------------------
    def upload(self, var, a):
        shape, dt = self.var_shape_dtype(var)
        a = _carr(a, dt)
        if a.size != int(np.prod(shape)):
            raise ValueError("array of shape %s cannot fill state of shape %s" %
                             (a.shape, shape))
        check(self._lib.sporco_amd_csc_upload(self._h, var, _ptr(a)))

    def download(self, var):
        shape, dt = self.var_shape_dtype(var)
        out = np.empty(shape, dtype=dt)
        check(self._lib.sporco_amd_csc_download(self._h, var, _ptr(out)))
        return out

    def device_reals(self, var):
        """(number of real scalars, torch dtype) of the device array behind ``var`` -- the
        device layout, i.e. with the padding filter of an odd dictionary."""
        import torch
        shape, dt = self.var_shape_dtype(var)
        kdev = self.query(QUERY_DEVICE_FILTERS)
        n = int(np.prod(shape[:-1])) * (kdev if shape[-1] == self.dims[4] else shape[-1])
        if np.dtype(dt).kind == 'c':
            n *= 2
        return n, (torch.float32 if self.dtype == np.float32 else torch.float64)

    def device_ptr(self, var):
        p = ctypes.c_void_p()
        check(self._lib.sporco_amd_csc_device_ptr(self._h, var, ctypes.byref(p)))
        return p.value

    # -- ADMM ---------------------------------------------------------------
    @staticmethod
    def _out():
        return (ctypes.c_double * OUT_COUNT)()

    def admm_iter(self, params):
        out = self._out()
        check(self._lib.sporco_amd_csc_admm_iter(self._h, ctypes.byref(params), out))
        return list(out)

    def admm_run(self, params, ctrl, reduce=None):
        """Device-driven solve (sporco_amd_csc_admm_run): up to ``ctrl.max_iter`` iterations,
        stopping on the tolerance test evaluated on the device.  ``reduce(sums_dev_ptr)``, when
        given, sums the 16 doubles at that device address over the ranks.  Returns ``(records,
        rho, u_scale)``, or None when this configuration has to be driven from the host."""
        n = ctypes.c_int32(0)
        rho, usc = ctypes.c_double(0.0), ctypes.c_double(0.0)
        recs = (AdmmRecord * max(int(ctrl.max_iter), 1))()
        cb = REDUCE_FN(lambda user, ptr: reduce(ptr)) if reduce is not None else \
            ctypes.cast(None, REDUCE_FN)
        rc = self._lib.sporco_amd_csc_admm_run(self._h, ctypes.byref(params), ctypes.byref(ctrl),
                                               recs, ctypes.byref(n), ctypes.byref(rho),
                                               ctypes.byref(usc), cb, None)
        if rc == EUNSUPPORTED:
            return None
        check(rc)
        return [recs[i] for i in range(n.value)], rho.value, usc.value

    def mdcpl_init(self, S):
        """ConvBPDNMaskDcpl state: keeps the real signal on the device, zeroes Y and U."""
        H, W, C, N, K = self.dims
        S = _carr(S, self.dtype)
        if S.size != H * W * self.Cs * N:
            raise ValueError("signal of shape %s does not match the solver" % (S.shape,))
        check(self._lib.sporco_amd_csc_mdcpl_init(self._h, _ptr(S)))

    def mdcpl_iter(self, params):
        out = self._out()
        check(self._lib.sporco_amd_csc_mdcpl_iter(self._h, ctypes.byref(params), out))
        return list(out)

    def l1l1_iter(self, params):
        """One iteration of ConvL1L1Grd on the mask-decoupling state (sporco_amd_csc_l1l1_iter);
        ``params.mu`` carries mu.  Returns the sums."""
        out = self._out()
        check(self._lib.sporco_amd_csc_l1l1_iter(self._h, ctypes.byref(params), out))
        return list(out)

    def ball_iter(self, params):
        """One iteration of ConvMinL1InL2Ball on the mask-decoupling state (sporco_amd_csc_ball_iter);
        ``params.mu`` carries epsilon.  Returns the sums (``OUT_DFID``: the squared constraint measure)."""
        out = self._out()
        check(self._lib.sporco_amd_csc_ball_iter(self._h, ctypes.byref(params), out))
        return list(out)

    def projl1_iter(self, params, gamma):
        """One iteration of ConvBPDNProjL1 (sporco_amd_csc_projl1_iter).  Returns the sums (``OUT_L1``:
        the squared constraint measure; ``OUT_CGN`` / ``OUT_RGRX``: the search passes taken)."""
        out = self._out()
        check(self._lib.sporco_amd_csc_projl1_iter(self._h, ctypes.byref(params), float(gamma), out))
        return list(out)

    def inhib_setup(self, Wg, taps_rows, taps_cols, want_self, lmbda):
        """ConvBPDNInhib state (sporco_amd_csc_inhib_setup): ``Wg`` (Ng, K) or None, the window
        taps along H and W; the handle's L1-weight array becomes the thresholds."""
        K = self.dims[4]
        tr = np.ascontiguousarray(taps_rows, dtype=np.float64).ravel()
        tc = np.ascontiguousarray(taps_cols, dtype=np.float64).ravel()
        dp = ctypes.POINTER(ctypes.c_double)
        if Wg is None:
            wg, ng = None, 0
        else:
            wg = np.ascontiguousarray(Wg, dtype=np.float64)
            if wg.ndim != 2 or wg.shape[1] != K:
                raise ValueError("Wg must be (groups, filters) = (Ng, %d), not %s" % (K, wg.shape))
            ng = wg.shape[0]
        check(self._lib.sporco_amd_csc_inhib_setup(
            self._h, None if wg is None else wg.ctypes.data_as(dp), ng, tr.ctypes.data_as(dp),
            tr.size, tc.ctypes.data_as(dp), tc.size, 1 if want_self else 0, float(lmbda)))

    def inhib_update(self, lmbda, mu, gamma, smooth, flags):
        """One inhibition-weight update (sporco_amd_csc_inhib_update); returns the sums."""
        p = InhibParams(float(lmbda), float(mu), float(gamma), float(smooth), int(flags))
        out = self._out()
        check(self._lib.sporco_amd_csc_inhib_update(self._h, ctypes.byref(p), out))
        return list(out)

    def tv_setup(self, tvw, vector_tv):
        """ConvBPDNScalarTV / ConvBPDNVectorTV state (sporco_amd_csc_tv_setup): ``tvw`` a scalar or
        one weight per filter."""
        w = np.ascontiguousarray(tvw, dtype=np.float64).ravel()
        if w.size not in (1, self.dims[4]):
            raise ValueError("TVWeight must be a scalar or hold one value per filter")
        check(self._lib.sporco_amd_csc_tv_setup(
            self._h, w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), w.size, 1 if vector_tv else 0))

    def tv_xstep(self, params):
        """The x step of the TV classes (sporco_amd_csc_tv_xstep); returns the sums."""
        out = self._out()
        check(self._lib.sporco_amd_csc_tv_xstep(self._h, ctypes.byref(params), out))
        return list(out)

    def tv_ystep(self, params):
        """relax + y step + u step of the TV classes (sporco_amd_csc_tv_ystep); returns the sums."""
        out = self._out()
        check(self._lib.sporco_amd_csc_tv_ystep(self._h, ctypes.byref(params), out))
        return list(out)

    def tv_adjoint(self, u_scale=1.0):
        """P = A^T Y, Q = u_scale A^T U into VAR_Y / VAR_U (sporco_amd_csc_tv_adjoint); returns the
        sums."""
        out = self._out()
        check(self._lib.sporco_amd_csc_tv_adjoint(self._h, float(u_scale), out))
        return list(out)

    def rtv_setup(self, tvw):
        """ConvBPDNRecTV state (sporco_amd_csc_rtv_setup): ``tvw`` a scalar or one weight per filter."""
        w = np.ascontiguousarray(tvw, dtype=np.float64).ravel()
        if w.size not in (1, self.dims[4]):
            raise ValueError("TVWeight must be a scalar or hold one value per filter")
        check(self._lib.sporco_amd_csc_rtv_setup(
            self._h, w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), w.size))

    def rtv_xstep(self, params):
        """The x step of ConvBPDNRecTV (sporco_amd_csc_rtv_xstep); returns the sums."""
        out = self._out()
        check(self._lib.sporco_amd_csc_rtv_xstep(self._h, ctypes.byref(params), out))
        return list(out)

    def rtv_ystep(self, params):
        """relax + y step + u step of ConvBPDNRecTV (sporco_amd_csc_rtv_ystep); returns the sums."""
        out = self._out()
        check(self._lib.sporco_amd_csc_rtv_ystep(self._h, ctypes.byref(params), out))
        return list(out)

    def rtv_dual(self, params):
        """The spectra of the blocks and the dual residual norms (sporco_amd_csc_rtv_dual); returns
        the sums."""
        out = self._out()
        check(self._lib.sporco_amd_csc_rtv_dual(self._h, ctypes.byref(params), out))
        return list(out)

    def pd_setup(self, B, Q, gamma, S):
        """Product-dictionary state (sporco_amd_csc_pd_setup): ``B`` (Cs, Cb), ``Q`` (Cb, Cb), ``gamma``
        (Cb) and the Cs-channel signal ``S`` (H, W, Cs, N).  The handle's own signal is S (B Q)."""
        H, W, Cb, N, K = self.dims
        B = np.ascontiguousarray(B, dtype=np.float64)
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        gamma = np.ascontiguousarray(gamma, dtype=np.float64).ravel()
        if B.ndim != 2 or B.shape[1] != Cb or Q.shape != (Cb, Cb) or gamma.size != Cb:
            raise ValueError("B must be (Cs, %d), Q (%d, %d) and gamma hold %d values" % (Cb, Cb, Cb, Cb))
        self.pd_Cs = int(B.shape[0])
        S = _carr(S, self.dtype).reshape(H, W, self.pd_Cs, N)
        dp = ctypes.POINTER(ctypes.c_double)
        check(self._lib.sporco_amd_csc_pd_setup(self._h, B.ctypes.data_as(dp), Q.ctypes.data_as(dp),
                                                gamma.ctypes.data_as(dp), _ptr(S), self.pd_Cs))

    def pd_xstep(self, params):
        """The x step of ConvProdDictBPDN (sporco_amd_csc_pd_xstep); returns the sums."""
        out = self._out()
        check(self._lib.sporco_amd_csc_pd_xstep(self._h, ctypes.byref(params), out))
        return list(out)

    def pd_dfid(self, var):
        """||B sum_m Df_m rfftn(var)_m - Sf||^2 (sporco_amd_csc_pd_dfid)."""
        out = self._out()
        check(self._lib.sporco_amd_csc_pd_dfid(self._h, int(var), out))
        return out[OUT_DFID]

    def pd_reconstruct(self, var):
        """irfftn(B sum_m Df_m rfftn(var)_m), (H, W, Cs, N) (sporco_amd_csc_pd_reconstruct)."""
        H, W, Cb, N, K = self.dims
        out = np.empty((H, W, self.pd_Cs, N), dtype=self.dtype)
        check(self._lib.sporco_amd_csc_pd_reconstruct(self._h, int(var), _ptr(out)))
        return out

    def pdl1_setup(self, B, Q, gamma, S, mask=None):
        """State of ConvProdDictL1L1Grd (sporco_amd_csc_pdl1_setup): the arguments of :meth:`pd_setup` and
        the mask, ``None`` or an array that broadcasts against ``S`` (H, W, Cs, N).  Block 0 of Y and U is
        created at zero by the first call and kept by later ones."""
        H, W, Cb, N, K = self.dims
        B = np.ascontiguousarray(B, dtype=np.float64)
        Q = np.ascontiguousarray(Q, dtype=np.float64)
        gamma = np.ascontiguousarray(gamma, dtype=np.float64).ravel()
        if B.ndim != 2 or B.shape[1] != Cb or Q.shape != (Cb, Cb) or gamma.size != Cb:
            raise ValueError("B must be (Cs, %d), Q (%d, %d) and gamma hold %d values" % (Cb, Cb, Cb, Cb))
        self.pd_Cs = int(B.shape[0])
        shp = (H, W, self.pd_Cs, N)
        S = _carr(S, self.dtype).reshape(shp)
        if mask is not None:
            mask = _carr(np.broadcast_to(np.asarray(mask, dtype=self.dtype), shp), self.dtype)
        dp = ctypes.POINTER(ctypes.c_double)
        check(self._lib.sporco_amd_csc_pdl1_setup(self._h, B.ctypes.data_as(dp), Q.ctypes.data_as(dp),
                                                  gamma.ctypes.data_as(dp), _ptr(S), self.pd_Cs,
                                                  None if mask is None else _ptr(mask)))

    def pdl1_block0(self, which, value=None):
        """Block 0 of Y (``which`` 0) or U (1), (H, W, Cs, N, 1): returned, or with ``value`` uploaded
        (sporco_amd_csc_pdl1_block0)."""
        H, W, Cb, N, K = self.dims
        shp = (H, W, self.pd_Cs, N, 1)
        if value is None:
            out = np.empty(shp, dtype=self.dtype)
            check(self._lib.sporco_amd_csc_pdl1_block0(self._h, int(which), 0, _ptr(out)))
            return out
        value = _carr(value, self.dtype).reshape(shp)
        check(self._lib.sporco_amd_csc_pdl1_block0(self._h, int(which), 1, _ptr(value)))

    def pdl1_iter(self, params):
        """One iteration of ConvProdDictL1L1Grd / ConvProdDictL1L1GrdJoint (sporco_amd_csc_pdl1_iter);
        returns the sums."""
        out = self._out()
        check(self._lib.sporco_amd_csc_pdl1_iter(self._h, ctypes.byref(params), out))
        return list(out)

    def admm_iter_dev(self, params, out_dev_ptr):
        check(self._lib.sporco_amd_csc_admm_iter_dev(self._h, ctypes.byref(params),
                                                     ctypes.c_void_p(out_dev_ptr)))

    def admm_xstep(self, params):
        out = self._out()
        check(self._lib.sporco_amd_csc_admm_xstep(self._h, ctypes.byref(params), out))
        return list(out)

    def admm_relax(self, rlx):
        check(self._lib.sporco_amd_csc_admm_relax(self._h, float(rlx)))

    def admm_ystep(self, params):
        check(self._lib.sporco_amd_csc_admm_ystep(self._h, ctypes.byref(params)))

    def admm_ustep(self, params):
        check(self._lib.sporco_amd_csc_admm_ustep(self._h, ctypes.byref(params)))

    def admm_stats(self, params):
        out = self._out()
        check(self._lib.sporco_amd_csc_admm_stats(self._h, ctypes.byref(params), out))
        return list(out)

    def scale_u(self, s):
        check(self._lib.sporco_amd_csc_scale_u(self._h, float(s)))

    def reconstruct(self, var):
        H, W, C, N, K = self.dims
        out = np.empty((H, W, self.Cs, N, 1), dtype=self.dtype)
        check(self._lib.sporco_amd_csc_reconstruct(self._h, var, _ptr(out)))
        return out

    def reconstruct_dev(self, var, dst_ptr):
        """The same into a device array (H, W, Cs, N) at ``dst_ptr``."""
        check(self._lib.sporco_amd_csc_reconstruct_dev(self._h, var, ctypes.c_void_p(dst_ptr)))

    def set_signal_dev(self, ptr):
        """set_signal from a device array (H, W, Cs, N): no host copy."""
        check(self._lib.sporco_amd_csc_set_signal_dev(self._h, ctypes.c_void_p(ptr)))

    def dhs_absmax(self):
        v = ctypes.c_double(0.0)
        check(self._lib.sporco_amd_csc_dhs_absmax(self._h, ctypes.byref(v)))
        return v.value

    # -- PGM ----------------------------------------------------------------
    def pgm_grad(self, var):
        out = self._out()
        check(self._lib.sporco_amd_csc_pgm_grad(self._h, var, out))
        return list(out)

    def pgm_iter(self, L, lmbda, beta, flags, dH, dW, want_stats, hold=False):
        """One fused default-option FISTA iteration (sporco_amd_csc_pgm_iter).  hold: a
        backtracking trial -- out[PGM_LIN], out[PGM_DXY2] too, and the new iterates wait for
        pgm_commit (the call may be repeated with another L)."""
        # (hold = 2: a trial of a rule that forms Yf itself -- no momentum output; after the
        # commit VAR_YF is the previous iteration's Yf and VAR_YFPRV the one this trial used)
        p = PgmParams(float(L), float(lmbda), float(beta), int(flags), int(dH), int(dW),
                      1 if want_stats else 0, int(hold))
        out = self._out()
        check(self._lib.sporco_amd_csc_pgm_iter(self._h, ctypes.byref(p), out))
        return list(out)

    def pgm_commit(self):
        check(self._lib.sporco_amd_csc_pgm_commit(self._h))

    def cns_init(self, Y0, rho):
        """Consensus D-step state: Y = Y0 (H, W, 1, 1, K) or zero, U_n = Y0 / rho or zero."""
        if Y0 is None:
            check(self._lib.sporco_amd_csc_cns_init(self._h, None, float(rho)))
            return
        H, W, C, N, K = self.dims
        Y0 = _carr(Y0, self.dtype).reshape(H, W, self.Cd, K)
        check(self._lib.sporco_amd_csc_cns_init(self._h, _ptr(Y0), float(rho)))

    def cns_md_init(self, S):
        """State of the masked consensus D-step: the real signal on the device, Y1 = U1 = 0."""
        H, W, C, N, K = self.dims
        S = _carr(S, self.dtype)
        if S.size != H * W * self.Cs * N:
            raise ValueError("signal of shape %s does not match the solver" % (S.shape,))
        check(self._lib.sporco_amd_csc_cns_md_init(self._h, _ptr(S)))

    def cns_mean_ptr(self):
        """(device address, element count) of the consensus-mean buffer (phase 1 -> phase 2)."""
        p, n = ctypes.c_void_p(), ctypes.c_int64(0)
        check(self._lib.sporco_amd_csc_cns_mean_ptr(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def cns_iter(self, rho, rlx, u_scale, flags, dH, dW, zero_mean, mask_dcpl=False, phase=0):
        """One consensus D-step iteration (sporco_amd_csc_cns_iter), or one of its two phases
        when the images are sharded over ranks."""
        p = CnsParams(float(rho), float(rlx), float(u_scale), int(flags), int(dH), int(dW),
                      1 if zero_mean else 0, 1 if mask_dcpl else 0, int(phase))
        out = self._out()
        check(self._lib.sporco_amd_csc_cns_iter(self._h, ctypes.byref(p), out))
        return list(out)

    def ccmod_sgd_step(self, eta, dH, dW, zero_mean):
        """Projected SGD step on the X-step dictionary (sporco_amd_csc_ccmod_sgd_step)."""
        out = self._out()
        check(self._lib.sporco_amd_csc_ccmod_sgd_step(self._h, float(eta), int(dH), int(dW),
                                                      1 if zero_mean else 0, out))
        return list(out)

    def dstep_init(self, Y0):
        """Single-copy ADMM D-step state: Y = U = Y0 (H, W, Cd, 1, K) or zero, Xf = 0."""
        if Y0 is None:
            check(self._lib.sporco_amd_csc_dstep_init(self._h, None))
            return
        H, W, C, N, K = self.dims
        Y0 = _carr(Y0, self.dtype).reshape(H, W, self.Cd, K)
        check(self._lib.sporco_amd_csc_dstep_init(self._h, _ptr(Y0)))

    def dstep_md_init(self, Y0, S):
        """Mask-decoupling D-step state: dstep_init(Y0), block 0 zeroed, real signal kept."""
        H, W, C, N, K = self.dims
        y0 = None if Y0 is None else _carr(Y0, self.dtype).reshape(H, W, self.Cd, K)
        s = None if S is None else _carr(S, self.dtype)
        check(self._lib.sporco_amd_csc_dstep_md_init(self._h, None if y0 is None else _ptr(y0),
                                                     None if s is None else _ptr(s)))

    def dstep_iter(self, method, rho, rlx, u_scale, flags, dH, dW, zero_mean, cg_tol=1e-3,
                   cg_maxiter=1000, mask_dcpl=False):
        """One IterSM / CG D-step iteration (sporco_amd_csc_dstep_iter)."""
        p = DstepParams(float(rho), float(rlx), float(u_scale), float(cg_tol), int(flags), int(dH),
                        int(dW), 1 if zero_mean else 0, int(method), int(cg_maxiter),
                        1 if mask_dcpl else 0)
        out = self._out()
        check(self._lib.sporco_amd_csc_dstep_iter(self._h, ctypes.byref(p), out))
        return list(out)

    def pgm_eval(self, var):
        out = self._out()
        check(self._lib.sporco_amd_csc_pgm_eval(self._h, var, out))
        return list(out)

    def pgm_prox_step(self, L, lmbda, flags, dH, dW):
        out = self._out()
        check(self._lib.sporco_amd_csc_pgm_prox_step(self._h, float(L), float(lmbda),
                                                     int(flags), int(dH), int(dW), out))
        return list(out)

    def lincomb(self, dst, a, va, b=0.0, vb=-1, c=0.0, vc=-1):
        check(self._lib.sporco_amd_csc_lincomb(self._h, dst, float(a), va, float(b), vb,
                                               float(c), vc))

    def pair_stats(self, va, vb=-1, vg=-1):
        out = self._out()
        check(self._lib.sporco_amd_csc_pair_stats(self._h, va, vb, vg, out))
        return list(out)[:4]

    def pgm_resid(self, var, slot):
        """e = sum_m Df var - Sf into residual slot 0..3 (sporco_amd_csc_pgm_resid)."""
        check(self._lib.sporco_amd_csc_pgm_resid(self._h, var, slot))

    def pgm_resid_stats(self, a, b=-1, c=-1, d=-1):
        """(<g1, g1>, <g1, H g1>, <dx, dg>) from residual slots (sporco_amd_csc_pgm_resid_stats)."""
        out = self._out()
        check(self._lib.sporco_amd_csc_pgm_resid_stats(self._h, a, b, c, d, out))
        return list(out)[:3]

    def copy(self, dst, src):
        check(self._lib.sporco_amd_csc_copy(self._h, dst, src))

    # -- dictionary update ---------------------------------------------------
    def ccmod_setcoef(self, var):
        check(self._lib.sporco_amd_csc_ccmod_setcoef(self._h, var))

    def ccmod_grad(self, var):
        out = self._out()
        check(self._lib.sporco_amd_csc_ccmod_grad(self._h, var, out))
        return list(out)

    def ccmod_eval(self, var):
        out = self._out()
        check(self._lib.sporco_amd_csc_ccmod_eval(self._h, var, out))
        return list(out)

    def ccmod_prox_step(self, L, dH, dW, zero_mean):
        check(self._lib.sporco_amd_csc_ccmod_prox_step(self._h, float(L), int(dH), int(dW),
                                                       1 if zero_mean else 0))

    def ccmod_cnstr(self, dH, dW, zero_mean):
        out = self._out()
        check(self._lib.sporco_amd_csc_ccmod_cnstr(self._h, int(dH), int(dW),
                                                   1 if zero_mean else 0, out))
        return out[0]

    def ccmod_getdict(self, dH, dW):
        K = self.dims[4]
        out = np.empty((dH, dW, self.Cd, 1, K), dtype=self.dtype)
        check(self._lib.sporco_amd_csc_ccmod_getdict(self._h, int(dH), int(dW), _ptr(out)))
        return out

    def setdict_from_dstep(self, dH, dW):
        check(self._lib.sporco_amd_csc_setdict_from_dstep(self._h, int(dH), int(dW)))

    def asum(self, var):
        out = self._out()
        check(self._lib.sporco_amd_csc_asum(self._h, var, out))
        return out[0]

    def fft_var(self, real_var, cplx_var):
        check(self._lib.sporco_amd_csc_fft_var(self._h, real_var, cplx_var))

    def ifft_var(self, cplx_var, real_var):
        check(self._lib.sporco_amd_csc_ifft_var(self._h, cplx_var, real_var))


class TvdHandle(_PlaneArrays, _Handle):
    """Owner of one device-side TVL2Denoise problem (sporco_amd_tvd_*): arrays of shape
    (H, W, P); ``vector_tv``: the l2 norm of the y step also runs over the first of the trailing axes
    (``C`` channels).  ``l1``: a TVL1Denoise problem (sporco_amd_tvl1_create) -- Y and U have three
    blocks, the last the data block."""

    _prefix = 'sporco_amd_tvd'

    def __init__(self, H, W, P, dtype, C=1, vector_tv=False, device=0, stream=None, l1=False):
        self.dims = (int(H), int(W), int(P))
        self.dtype = np.dtype(dtype)
        self.blocks = 3 if l1 else 2
        self._open(lib().sporco_amd_tvl1_create if l1 else lib().sporco_amd_tvd_create, dtype_code(dtype), int(H),
                   int(W), int(P), int(C), 1 if vector_tv else 0, int(device), ctypes.c_void_p(stream or 0))

    def plan(self):
        """``dict(V, items, strips, R, nseg, TW)``: elements per item, items per row, strips per row,
        rows per segment, segments, columns a strip covers."""
        out = (ctypes.c_int64 * 6)()
        check(self._lib.sporco_amd_tvd_plan(self._h, out))
        return dict(zip(('V', 'items', 'strips', 'R', 'nseg', 'TW'), (int(v) for v in out)))

    def var_shape(self, var):
        return ((self.blocks,) if var in (TVD_Y, TVD_U) else ()) + self.dims

    def sweeps(self, params, n):
        check(self._lib.sporco_amd_tvd_sweeps(self._h, ctypes.byref(params), int(n)))

    def gsres(self, params):
        return self._sums(self._lib.sporco_amd_tvd_gsres, ctypes.byref(params))

    def ystep(self, params):
        return self._sums(self._lib.sporco_amd_tvd_ystep, ctypes.byref(params))

    def adjoint(self):
        check(self._lib.sporco_amd_tvd_adjoint(self._h))


class TvdcHandle(_PlaneArrays, _Handle):
    """Owner of one device-side TVL2Deconv problem (sporco_amd_tvdc_*), or with ``l1`` of a TVL1Deconv
    problem (sporco_amd_tvl1dc_create: Y and U have three blocks, the last the data block).  Arrays of
    shape (H, W, P); ``PA``: the planes of the kernel A, ``P`` or 1."""

    _prefix = 'sporco_amd_tvdc'

    def __init__(self, H, W, P, dtype, C=1, vector_tv=False, PA=1, device=0, stream=None, l1=False):
        self.dims = (int(H), int(W), int(P))
        self.PA = int(PA)
        self.dtype = np.dtype(dtype)
        self.blocks = 3 if l1 else 2
        self._open(lib().sporco_amd_tvl1dc_create if l1 else lib().sporco_amd_tvdc_create, dtype_code(dtype), int(H),
                   int(W), int(P), int(C), 1 if vector_tv else 0, int(PA), int(device), ctypes.c_void_p(stream or 0))

    def plan(self):
        """``dict(V, items, strips, R, nseg, TW, SV, sblocks)``: elements per item, items per row, strips per
        row, rows per segment, segments, columns a strip covers (the stencil kernels); planes per access and
        workgroups of ``tvdc_solve``."""
        out = (ctypes.c_int64 * 8)()
        check(self._lib.sporco_amd_tvdc_plan(self._h, out))
        return dict(zip(('V', 'items', 'strips', 'R', 'nseg', 'TW', 'SV', 'sblocks'), (int(v) for v in out)))

    def var_shape(self, var):
        return ((self.blocks,) if var in (TVDC_Y, TVDC_U) else ()) + self.dims

    def set_kernel(self, a, ah=None, aw=None):
        """``a``: a host array of shape (ah, aw, PA), or a device pointer (int) with ``ah``, ``aw`` given."""
        if isinstance(a, int):
            check(self._lib.sporco_amd_tvdc_set_kernel(self._h, ctypes.c_void_p(a), int(ah), int(aw), 1))
        else:
            a = _carr(a, self.dtype)
            if a.ndim != 3 or a.shape[2] != self.PA:
                raise ValueError("the kernel has shape (ah, aw, %d)" % self.PA)
            check(self._lib.sporco_amd_tvdc_set_kernel(self._h, _ptr(a), a.shape[0], a.shape[1], 0))

    def xstep(self, params):
        check(self._lib.sporco_amd_tvdc_xstep(self._h, ctypes.byref(params)))

    def ystep(self, params):
        return self._sums(self._lib.sporco_amd_tvdc_ystep, ctypes.byref(params))

    def adjoint(self):
        check(self._lib.sporco_amd_tvdc_adjoint(self._h))


class SplHandle(_PlaneArrays, _Handle):
    """Owner of one device-side SplineL1 problem (sporco_amd_spl_*).  Arrays of shape (H, W, P); a 1-D
    signal of N samples is H = 1, W = N."""

    _prefix = 'sporco_amd_spl'

    def __init__(self, H, W, P, dtype, device=0, stream=None):
        self.dims = (int(H), int(W), int(P))
        self.dtype = np.dtype(dtype)
        self._open(lib().sporco_amd_spl_create, dtype_code(dtype), int(H), int(W), int(P), int(device),
                   ctypes.c_void_p(stream or 0))

    def plan(self):
        """``dict(V, pairs, sblocks, yblocks)``: planes per access, the row pairs {k1, H - k1} of ``spl_solve``,
        its workgroups and those of ``spl_ystep``."""
        out = (ctypes.c_int64 * 4)()
        check(self._lib.sporco_amd_spl_plan(self._h, out))
        return dict(zip(('V', 'pairs', 'sblocks', 'yblocks'), (int(v) for v in out)))

    def var_shape(self, var):
        return self.dims

    def xstep(self, params):
        check(self._lib.sporco_amd_spl_xstep(self._h, ctypes.byref(params)))

    def ystep(self, params):
        return self._sums(self._lib.sporco_amd_spl_ystep, ctypes.byref(params))


class BpdnHandle(_Handle):
    """Owner of one device-side BPDN / BPDNJoint / ElasticNet problem (sporco_amd_bpdn_*): D (N, M), S (N, K),
    X / Y / U (M, K), host arrays in and out."""

    _prefix = 'sporco_amd_bpdn'
    _create = 'sporco_amd_bpdn_create'

    def __init__(self, N, M, K, dtype, device=0, stream=None):
        self.dims = (int(N), int(M), int(K))
        self.dtype = np.dtype(dtype)
        self._open(getattr(lib(), self._create), dtype_code(dtype), int(N), int(M), int(K), int(device),
                   ctypes.c_void_p(stream or 0))

    def plan(self):
        """``dict(KB, blocks, mfma, lds)``: the columns of a workgroup's block, the workgroups, whether the
        products use the matrix instruction, the bytes of LDS of a workgroup."""
        out = (ctypes.c_int64 * 4)()
        check(self._lib.sporco_amd_bpdn_plan(self._h, out))
        return dict(zip(('KB', 'blocks', 'mfma', 'lds'), (int(v) for v in out)))

    def _shape(self, var):
        N, M, K = self.dims
        return (N, K) if var in (BPDN_S, BPDN_W) else (M, K)

    def set_dict(self, D):
        D = _carr(D, self.dtype)
        if D.shape != self.dims[:2]:
            raise ValueError("dictionary of shape %s where %s is expected" % (D.shape, self.dims[:2]))
        check(self._lib.sporco_amd_bpdn_set_dict(self._h, _ptr(D)))

    def set_solve(self, P):
        P = _carr(P, self.dtype)
        if P.shape != (self.dims[1], self.dims[1]):
            raise ValueError("solve matrix of shape %s where %s is expected" % (P.shape, (self.dims[1],) * 2))
        check(self._lib.sporco_amd_bpdn_set_solve(self._h, _ptr(P)))

    def upload(self, var, a):
        """``a``: a host array of the variable's shape, or None (the weight goes back to its scalar)."""
        if a is None:
            check(self._lib.sporco_amd_bpdn_upload(self._h, int(var), None))
            return
        a = _carr(a, self.dtype)
        if a.shape != self._shape(var):
            raise ValueError("array of shape %s where %s is expected" % (a.shape, self._shape(var)))
        check(self._lib.sporco_amd_bpdn_upload(self._h, int(var), _ptr(a)))

    def download(self, var, out=None):
        """To a new host array, or into ``out`` (C-ordered, the variable's shape and the handle's dtype)."""
        if out is None:
            out = np.empty(self._shape(var), dtype=self.dtype)
        elif out.shape != self._shape(var) or out.dtype != self.dtype or not out.flags['C_CONTIGUOUS']:
            raise ValueError("out does not have the variable's shape and dtype")
        check(self._lib.sporco_amd_bpdn_download(self._h, int(var), _ptr(out)))
        return out

    def iter(self, params):
        return self._sums(self._lib.sporco_amd_bpdn_iter, ctypes.byref(params))

    def device_view(self, var):
        """A :class:`sporco_amd.device.DeviceArray` over the buffer of variable ``var``: no copy, and the view
        keeps this handle alive.  It shows whatever the handle's calls leave in the buffer."""
        from .device import DeviceArray
        p = ctypes.c_void_p()
        check(self._lib.sporco_amd_bpdn_devptr(self._h, int(var), ctypes.byref(p)))
        if not p.value:
            raise ValueError("the variable has no device array")
        return DeviceArray(self._shape(var), self.dtype, ptr=p.value, base=self)


class PgmBpdnHandle(BpdnHandle):
    """Owner of one device-side pgm.bpdn BPDN / WeightedBPDN problem (sporco_amd_bpdn_pgm_*): a
    :class:`BpdnHandle` with the arrays of the proximal gradient iteration (``BPDN_XPRV`` ... ``BPDN_W``)."""

    _create = 'sporco_amd_bpdn_pgm_create'

    def step(self, params, read=True):
        """The phases ``params`` asks for and the reduction; the ``PGMB_*`` sums, or None without ``read``."""
        if read:
            return self._sums(self._lib.sporco_amd_bpdn_pgm_step, ctypes.byref(params))
        check(self._lib.sporco_amd_bpdn_pgm_step(self._h, ctypes.byref(params), None))
        return None

    def ystep(self, beta, gamma=0.0, use_zz=False, advance_y=False, read=True):
        """``Y = X + gamma (ZZ - X) + beta (X - Xprv)`` as a launch of its own, into the other Y array with
        ``advance_y``; ``out[PGMB_RS2] = ||X - Y||^2``, or None without ``read``."""
        args = (float(beta), float(gamma), int(bool(use_zz)), int(bool(advance_y)))
        if read:
            return self._sums(self._lib.sporco_amd_bpdn_pgm_ystep, *args)
        check(self._lib.sporco_amd_bpdn_pgm_ystep(self._h, *args, None))
        return None

    def copy(self, dst, src):
        check(self._lib.sporco_amd_bpdn_pgm_copy(self._h, int(dst), int(src)))


class CmodHandle(_Handle):
    """Owner of one device-side CnstrMOD problem (sporco_amd_cmod_*): Z (M, K) and S (N, K), host arrays that are
    copied or :class:`sporco_amd.device.DeviceArray` that are read in place (the handle keeps them alive);
    X / Y / U (N, M), host arrays in and out."""

    _prefix = 'sporco_amd_cmod'
    _create = 'sporco_amd_cmod_create'

    def __init__(self, N, M, K, dtype, device=0, stream=None):
        self.dims = (int(N), int(M), int(K))
        self.dtype = np.dtype(dtype)
        self._open(getattr(lib(), self._create), dtype_code(dtype), int(N), int(M), int(K), int(device),
                   ctypes.c_void_p(stream or 0))
        self._keep = {}

    def close(self):
        _Handle.close(self)
        self._keep = {}

    def plan(self):
        """``dict(KS, slab, slabs, row_blocks, col_blocks, mfma, lds_gram, lds_iter)``: the columns of K staged per
        step, the columns of a slab, the slabs, the 64 x 64 blocks of the output of cmod_gram, whether the products
        use the matrix instruction, the bytes of LDS of a workgroup of cmod_gram and cmod_iter."""
        out = (ctypes.c_int64 * 8)()
        check(self._lib.sporco_amd_cmod_plan(self._h, out))
        return dict(zip(('KS', 'slab', 'slabs', 'row_blocks', 'col_blocks', 'mfma', 'lds_gram', 'lds_iter'),
                        (int(v) for v in out)))

    def _shape(self, var):
        N, M, K = self.dims
        return (M, M) if var == CMOD_G else (N, M)

    def _dtype(self, var):
        return np.dtype(np.float64) if var in (CMOD_G, CMOD_SZTD) else self.dtype

    def _set_big(self, fn, key, a, rows):
        shape = (rows, self.dims[2])
        if isinstance(a, np.ndarray):
            a = _carr(a, self.dtype)
            if a.shape != shape:
                raise ValueError("array of shape %s where %s is expected" % (a.shape, shape))
            check(fn(self._h, _ptr(a), 0))
            self._keep.pop(key, None)
            return
        if tuple(a.shape) != shape or a.dtype != self.dtype:
            raise ValueError("device array of shape %s and dtype %s where %s, %s is expected"
                             % (tuple(a.shape), a.dtype, shape, self.dtype))
        check(fn(self._h, ctypes.c_void_p(a.ptr), 1))
        self._keep[key] = a

    def set_signal(self, S):
        self._set_big(self._lib.sporco_amd_cmod_set_signal, 'S', S, self.dims[0])

    def set_coef(self, Z):
        """Take Z and form Z Z^T and S Z^T on the device."""
        self._set_big(self._lib.sporco_amd_cmod_set_coef, 'Z', Z, self.dims[1])

    def set_solve(self, Q):
        Q = _carr(Q, self.dtype)
        if Q.shape != (self.dims[1], self.dims[1]):
            raise ValueError("solve matrix of shape %s where %s is expected" % (Q.shape, (self.dims[1],) * 2))
        check(self._lib.sporco_amd_cmod_set_solve(self._h, _ptr(Q)))

    def upload(self, var, a):
        a = _carr(a, self._dtype(var))
        if a.shape != self._shape(var):
            raise ValueError("array of shape %s where %s is expected" % (a.shape, self._shape(var)))
        check(self._lib.sporco_amd_cmod_upload(self._h, int(var), _ptr(a)))

    def download(self, var):
        out = np.empty(self._shape(var), dtype=self._dtype(var))
        check(self._lib.sporco_amd_cmod_download(self._h, int(var), _ptr(out)))
        return out

    def iter(self, params):
        return self._sums(self._lib.sporco_amd_cmod_iter, ctypes.byref(params))

    def dfid(self, var):
        """``||V Z - S||^2`` for V = X or Y."""
        return self._sums(self._lib.sporco_amd_cmod_dfid, int(var))[OUT_DFID]


class PgmCmodHandle(CmodHandle):
    """Owner of one device-side pgm.cmod CnstrMOD / WeightedCnstrMOD problem (sporco_amd_cmod_pgm_*): a
    :class:`CmodHandle` without Gram and solve matrices, with the arrays of the proximal gradient iteration
    (``CMOD_XPRV`` ... ``CMOD_ZZ``) and the weight W (N, K), a host array that is copied or a
    :class:`sporco_amd.device.DeviceArray` that is read in place."""

    _create = 'sporco_amd_cmod_pgm_create'

    def plan(self):
        """``dict(KS, slab, slabs, row_blocks, tiles_per_wave, mfma, lds_grad, lds_prox)``: the columns of K staged
        per step, the columns of a slab, the slabs, the blocks of 32 rows of cmod_pgm_grad, the 16-column tiles of G
        a wave accumulates, whether the products use the matrix instruction, the bytes of LDS of a workgroup of
        cmod_pgm_grad and cmod_pgm_prox."""
        out = (ctypes.c_int64 * 8)()
        check(self._lib.sporco_amd_cmod_plan(self._h, out))
        return dict(zip(('KS', 'slab', 'slabs', 'row_blocks', 'tiles_per_wave', 'mfma', 'lds_grad', 'lds_prox'),
                        (int(v) for v in out)))

    def set_weight(self, W):
        """W (N, K), or None: the scalar weight of the step's parameters."""
        if W is None:
            check(self._lib.sporco_amd_cmod_pgm_set_weight(self._h, None, 0))
            self._keep.pop('W', None)
            return
        self._set_big(self._lib.sporco_amd_cmod_pgm_set_weight, 'W', W, self.dims[0])

    def step(self, params, read=True):
        """The phases ``params`` asks for and, with ``params.finalize``, the reduction; the ``PGMC_*`` sums, or None
        without ``read``."""
        if read:
            return self._sums(self._lib.sporco_amd_cmod_pgm_step, ctypes.byref(params))
        check(self._lib.sporco_amd_cmod_pgm_step(self._h, ctypes.byref(params), None))
        return None

    def dfid(self):
        """``sum W (X Z - S)^2`` of the iterate."""
        return CmodHandle.dfid(self, CMOD_X)


class RpcaHandle(_Handle):
    """Owner of one device-side RobustPCA problem (sporco_amd_rpca_*), also the short-lived engine of
    ``prox.prox_nuclear`` / ``prox.norm_nuclear``: S (R, C), a host array that is copied or a
    :class:`sporco_amd.device.DeviceArray` that is read in place (the handle keeps it alive); X / Y / U (R, C), host
    arrays in and out, or views of the handle's buffers (:meth:`device_view`)."""

    _prefix = 'sporco_amd_rpca'

    def __init__(self, R, C, dtype, device=0, stream=None):
        self.dims = (int(R), int(C))
        self.n = min(self.dims)
        self.dtype = np.dtype(dtype)
        self._open(lib().sporco_amd_rpca_create, dtype_code(dtype), int(R), int(C), int(device),
                   ctypes.c_void_p(stream or 0))
        self._keep = None

    def close(self):
        _Handle.close(self)
        self._keep = None

    def plan(self):
        """``dict(KS, slab, slabs, blocks, KB, workgroups, mfma_gram, mfma_iter, lds_gram, lds_iter)``: the positions
        of the long axis staged per step of rpca_gram, those of a slab, the slabs, the 64 x 64 blocks a side of the
        Gram matrix, the positions of a block of rpca_iter and its workgroups, whether the two kernels use a matrix
        instruction, the bytes of LDS of a workgroup of each."""
        out = (ctypes.c_int64 * 10)()
        check(self._lib.sporco_amd_rpca_plan(self._h, out))
        return dict(zip(('KS', 'slab', 'slabs', 'blocks', 'KB', 'workgroups', 'mfma_gram', 'mfma_iter', 'lds_gram',
                         'lds_iter'), (int(v) for v in out)))

    def set_signal(self, S):
        if isinstance(S, np.ndarray):
            S = _carr(S, self.dtype)
            if S.shape != self.dims:
                raise ValueError("array of shape %s where %s is expected" % (S.shape, self.dims))
            check(self._lib.sporco_amd_rpca_set_signal(self._h, _ptr(S), 0))
            self._keep = None
            return
        if tuple(S.shape) != self.dims or S.dtype != self.dtype:
            raise ValueError("device array of shape %s and dtype %s where %s, %s is expected"
                             % (tuple(S.shape), S.dtype, self.dims, self.dtype))
        check(self._lib.sporco_amd_rpca_set_signal(self._h, ctypes.c_void_p(S.ptr), 1))
        self._keep = S

    def upload(self, var, a):
        a = _carr(a, self.dtype)
        if a.shape != self.dims:
            raise ValueError("array of shape %s where %s is expected" % (a.shape, self.dims))
        check(self._lib.sporco_amd_rpca_upload(self._h, int(var), _ptr(a)))

    def download(self, var):
        out = np.empty(self.dims, dtype=self.dtype)
        check(self._lib.sporco_amd_rpca_download(self._h, int(var), _ptr(out)))
        return out

    def device_view(self, var):
        """A :class:`sporco_amd.device.DeviceArray` over the buffer of X, Y or U: no copy, and the view keeps this
        handle alive.  It shows whatever the handle's calls leave in the buffer."""
        from .device import DeviceArray
        p = ctypes.c_void_p()
        check(self._lib.sporco_amd_rpca_devptr(self._h, int(var), ctypes.byref(p)))
        return DeviceArray(self.dims, self.dtype, ptr=p.value, base=self)

    def gram(self, mode, u_scale=1.0):
        """The (n, n) float64 Gram matrix of V by ``mode`` (RPCA_V_*), n = min(R, C)."""
        G = np.empty((self.n, self.n), dtype=np.float64)
        check(self._lib.sporco_amd_rpca_gram(self._h, int(mode), float(u_scale), _ptr(G)))
        return G

    def _t(self, T):
        T = _carr(T, np.float64)
        if T.shape != (self.n, self.n):
            raise ValueError("T of shape %s where %s is expected" % (T.shape, (self.n, self.n)))
        return T

    def iter(self, params, T):
        return self._sums(self._lib.sporco_amd_rpca_iter, ctypes.byref(params), _ptr(self._t(T)))

    def apply(self, T):
        """X <- S T (R >= C) or T S."""
        T = self._t(T)
        check(self._lib.sporco_amd_rpca_apply(self._h, _ptr(T)))


def dct2(a, out=None, inverse=False):
    """The orthonormal DCT-II (``inverse``: its inverse) over axes (0, 1) of a C-ordered (H, W, ...) array,
    H >= 1, W >= 2: a host array to a new host array, or a :class:`sporco_amd.device.DeviceArray` to ``out``
    (a DeviceArray of the same shape and dtype, every element of which is written exactly once)."""
    fn = lib().sporco_amd_idctii if inverse else lib().sporco_amd_dctii
    H, W = int(a.shape[0]), int(a.shape[1])
    P = int(np.prod(a.shape[2:])) if len(a.shape) > 2 else 1
    if isinstance(a, np.ndarray):
        a = _carr(a, a.dtype)
        res = np.empty(a.shape, dtype=a.dtype)
        check(fn(dtype_code(a.dtype), H, W, P, _ptr(a), _ptr(res), 0))
        return res
    if out is None or tuple(out.shape) != tuple(a.shape) or out.dtype != a.dtype or out.ptr == a.ptr:
        raise ValueError("a device array is transformed into another of the same shape and dtype")
    check(fn(dtype_code(a.dtype), H, W, P, ctypes.c_void_p(a.ptr), ctypes.c_void_p(out.ptr), 1))
    return out


def proj_l1_cols(v, gamma):
    """``proj_l1(v, gamma, axis=0)`` of a host ``(M, K)`` array, ``M <= 512``: one l1 ball per column, by the column
    search of the bpdn handle's projection mode (sporco_amd_proj_l1_cols).  What the tests reach that routine with."""
    v = np.asarray(v)
    if v.ndim != 2 or v.dtype not in (np.float32, np.float64):
        raise ValueError("proj_l1_cols takes a float32 or float64 array of shape (M, K)")
    v = _carr(v, v.dtype)
    out = np.full(v.shape, np.nan, dtype=v.dtype)
    check(lib().sporco_amd_proj_l1_cols(dtype_code(v.dtype), int(v.shape[0]), int(v.shape[1]), _ptr(v), float(gamma),
                                        _ptr(out)))
    return out
