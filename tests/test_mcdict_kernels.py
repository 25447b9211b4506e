"""Every dispatch branch of the multi-channel dictionary kernels (sporco_amd/csrc/ck_ism.hip) against the
float64 NumPy statements of tests/_mcdict_numpy.py: dense solves per frequency, written from the
definitions and pinned to the reference's recorded results in section 0.  Nothing is read back from the
library to build a reference.  The handle is driven directly (_lib.Solver), as in test_ism_tables.py.

What the launchers decide (restated here from their source), and the test that covers it:

* ism_dispatch_kr: a lane holds KR filters k = lane + 64 j, every access guarded by k < K; KR = 1 for
  K <= 64, 2 for K <= 128, 4 for K <= 256, K > 256 refused -- kr_of(); K = 3, 64 / 65, 128 / 129, 256
  in test_xstep_plain, K = 3, 65, 129 in test_xstep_gradient and test_gradient_eval_absmax, K = 3, 65
  in test_dstep_ism, K = 257 in test_more_than_256_filters_refused.
* launch_ism_solve, channel count: compile-time for 2, 3, 4; the run-time-count instantiation (eight
  register slots) for 1 and 5..8 and, with the gradient term, for every count <= 8; the LDS `_big`
  kernels above 8 (plain solve only) -- form_of(); every (KR, form) pair of the x step is in XSTEP_CASES
  (asserted at import); count 1, 2, 8 / 9, 12 terms in test_dstep_ism, whose terms are the images.
* ism_waves_per_pixel: N = 1 four frequencies a workgroup, N = 2 two waves a frequency, N >= 3 four
  waves on one frequency, N > 4 a wave takes images n, n + 4 -- N = 1, 2, 3, 5 in test_xstep_plain; the
  dictionary update always has one right-hand side (four (frequency, channel) systems a workgroup).
* launch_ism_setup: ism_setup_kernel up to 8 terms (with or without the gradient diagonal),
  ism_setup_big_kernel above -- reached by the same tests, the tables are built on the first call.
* grid caps: the solve has min(ceil(npix / ppb), 4096) workgroups, ppb = 4, 2, 1 as above; grid_for
  caps the setup and the one-wave-per-system kernels (mc_pgm_grad, the _big solve) at 4096 workgroups
  of four waves -- test_xstep_above_cap, test_gradient_above_cap (device only).
* launch_mc_inner: sixteen lanes an output for K >= 16 (strided tail at K = 20), else one thread --
  test_gradient_eval_absmax through pgm_eval's sums and reconstruct's array.
* mc_conj_outer: reached through masked_grad without a mask, which leaves conj(Df) applied to the
  residual (taken through the spatial domain and back) in VAR_GF -- test_gradient_eval_absmax; its
  `add` form is only used inside mdcpl_iter, whose X is downstream of a solve, and stays with the
  solver-level tests (test_maskdcpl.py).
* mc_dhs_absmax against Solver.dhs_absmax() -- test_gradient_eval_absmax.
* cns_xrrs_rhs_kernel / cns_xrrs_fin_kernel (the consensus update's LinSolveCheck) are left to the
  solver-level tests (test_ccmod_cns.py): no call leaves their arrays downloadable, and their sums are
  there compared with the reference's XSlvRelRes.

Images 12 x 10 (even W: a Nyquist column of Parseval weight 1) and 9 x 7 (odd, odd); dictionary support
3 x 3, every filter of unit norm over (rows, columns, channels); rho = 1.5.  X (and GF) are filled with
NaN before each call and every output is asserted finite.

Device only (marked gpu): the above-cap cases.  On the simulator everything else runs as it stands; no
smaller siblings were needed (the largest case, K = 256 with 8 channels at 12 x 10, takes it a few
seconds).

Tolerances.  float64: relative l2 error under 1e-10 for arrays; sums are compared as norms (square
roots), 1e-10, and the LinSolveCheck residual as sqrt(D2) <= 1e-10 sqrt(B2) -- it is zero in exact
arithmetic.  The dense solve and the recursion differ by conditioning x 1e-16: the largest condition
number over a case's frequencies is asserted under 1e3.  float32: the same expressions are evaluated
in NumPy float32 (transforms included; linalg.solvemdbi_ism's recursion for the solves; every sum
sequential) on the test's own seeded inputs and compared with the float64 reference; a bound is 4 x
the largest relative l2 error over the test's cases, rounded up to one significant digit.  A sum takes
the bound of the array it is a norm of.  No bound comes from a kernel's output;
test_f32_bounds_are_the_measured_ones repeats the measurement.

    test / array                          cases                      measured   bound
    test_xstep_plain, _only_the_sums / X  all XSTEP_CASES, FLAG_CASE 2.9e-07    2e-06
    test_xstep_gradient, _mu_zero / X     all GRAD_CASES, MU0_CASE   2.3e-07    1e-06
    test_xstep_above_cap / X              both CAP_CASES             1.7e-07    7e-07
    test_gradient_eval_absmax / gf        all GEA_CASES              1.4e-07    6e-07
      residual (PGM_F, PGM_DFID)          all GEA_CASES              1.3e-07    6e-07
      sum_k Df v (PGM_HESS)               all GEA_CASES              2.2e-07    9e-07
      reconstruct                         all GEA_CASES              2.3e-07    1e-06
      masked_grad / gf                    all GEA_CASES              1.7e-07    7e-07
      dhs_absmax                          all GEA_CASES              8.7e-08    4e-07
    test_gradient_above_cap / gf          192 x 176                  7.0e-08    3e-07
      residual (PGM_F, PGM_DFID)          192 x 176                  4.4e-08    2e-07
    test_dstep_ism / X                    all DSTEP_CASES            1.5e-06    6e-06

(The project's one other figure for this recursion in float32, 2-4e-5 in test_ccmod_ism_cg.py, is the
state after a whole ADMM run with a moving rho; a single well-conditioned solve sits two decades lower.)
"""

import functools
import math

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _mcdict_numpy as mn
from sporco_amd import _lib

RHO = 1.5
DH = DW = 3
F64_TOL = 1e-10
COND_MAX = 1e3
MAX_BLOCKS, WAVES_PER_BLOCK = 4096, 4      # kMaxPartialBlocks, kThreads / kWave

RDTS = [pytest.param(np.float64, id='f64'), pytest.param(np.float32, id='f32')]


def bound_of(measured):
    """4 x measured, rounded up to one significant digit."""
    x = 4.0 * measured
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


# Largest relative l2 error of the float32 NumPy evaluation against the float64 reference over each
# test's cases (test_f32_bounds_are_the_measured_ones repeats it).
F32_MEASURED = {
    'xstep_plain': 2.9e-07,
    'xstep_grad': 2.3e-07,
    'xstep_above_cap': 1.7e-07,
    'grad_gf': 1.4e-07,
    'grad_r': 1.3e-07,
    'grad_av': 2.2e-07,
    'recon': 2.3e-07,
    'masked_gf': 1.7e-07,
    'absmax': 8.7e-08,
    'grad_above_cap_gf': 7.0e-08,
    'grad_above_cap_r': 4.4e-08,
    'dstep': 1.5e-06,
}
F32_BOUND = {k: bound_of(v) for k, v in F32_MEASURED.items()}


def is_f32(dt):
    return np.dtype(dt) == np.float32


def tol_of(dt, key):
    return F32_BOUND[key] if is_f32(dt) else F64_TOL


def kr_of(K):
    """ism_dispatch_kr."""
    assert K <= 256
    return 1 if K <= 64 else (2 if K <= 128 else 4)


def form_of(terms, grad=False):
    """launch_ism_solve / launch_ism_setup."""
    if terms > 8:
        assert not grad
        return 'big'
    if grad or terms not in (2, 3, 4):
        return 'runtime'
    return 'cc%d' % terms


def waves_per_pixel(nrhs):
    """ism_waves_per_pixel with four waves a workgroup."""
    return 4 if nrhs >= 3 else (2 if nrhs == 2 else 1)


def norm_err(got2, want2):
    """Relative error of a norm given its square (the sums are squared norms)."""
    assert got2 >= 0.0 and want2 > 0.0
    return abs(math.sqrt(got2) - math.sqrt(want2)) / math.sqrt(want2)


# ---- problems ---------------------------------------------------------------------------------------------
def unit_dict(rng, Cd, K):
    D = rng.randn(DH, DW, Cd, 1, K)
    return D / np.sqrt(np.sum(D ** 2, axis=(0, 1, 2), keepdims=True))


@functools.lru_cache(maxsize=None)
def xproblem(H, W, K, Cd, N, dtname):
    rng = np.random.RandomState([101, H, W, K, Cd, N])
    g = {'D': unit_dict(rng, Cd, K), 'S': rng.randn(H, W, Cd, N), 'Y': rng.randn(H, W, 1, N, K),
         'U': 0.3 * rng.randn(H, W, 1, N, K), 'wg': 0.5 + rng.rand(K),
         'vf': rng.randn(H, W // 2 + 1, 1, N, K) + 1j * rng.randn(H, W // 2 + 1, 1, N, K)}
    dt = np.dtype(dtname)
    cdt = np.complex64 if dt == np.float32 else np.complex128
    out = {k: np.ascontiguousarray(v, dtype=cdt if np.iscomplexobj(v) else dt) for k, v in g.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def xref(H, W, K, Cd, N, dtname, u_scale, mu, weighted):
    g = xproblem(H, W, K, Cd, N, dtname)
    return mn.xstep(g['D'], g['S'], g['Y'], g['U'], RHO, u_scale, mu, g['wg'] if weighted else None)


def xhandle(g, dt, nan_x=True):
    H, W, Cd, N = g['S'].shape
    K = g['Y'].shape[4]
    s = _lib.Solver(H, W, Cd, N, K, dt, Cd=Cd)
    assert not s.uses_fused_cols() and not s.uses_fused_rows()
    s.set_dict(g['D'])
    s.set_signal(g['S'])
    s.upload(_lib.VAR_Y, g['Y'])
    s.upload(_lib.VAR_U, g['U'])
    if nan_x:
        s.upload(_lib.VAR_X, np.full(g['Y'].shape, np.nan, dtype=dt))
    return s


def xparams(flags, u_scale=1.0, mu=None):
    p = _lib.AdmmParams()
    p.rho, p.lmbda, p.mu = RHO, 0.05, 0.0 if mu is None else float(mu)
    p.rlx, p.u_scale = 1.8, float(u_scale)
    p.flags = flags | (0 if mu is None else _lib.FLAG_GRADREG)
    p.dH, p.dW = DH, DW
    return p


XSUM_SLOTS = (_lib.OUT_DFID, _lib.OUT_XRRS_D2, _lib.OUT_XRRS_AX2, _lib.OUT_XRRS_B2, _lib.OUT_RGR)


def check_xstep(case, dt, key, flags=_lib.FLAG_OBJ | _lib.FLAG_XRRS, mu=None, weighted=False, ref_mu='same',
                last=None):
    """One x step from NaN-filled X; X and the sums asked for against the dense solve, the other slots
    exactly zero."""
    H, W, K, Cd, N, u_scale = case
    dtname = np.dtype(dt).name
    g = xproblem(H, W, K, Cd, N, dtname)
    ref = xref(H, W, K, Cd, N, dtname, u_scale, mu if ref_mu == 'same' else ref_mu, weighted)
    assert ref['cond'] < COND_MAX, ref['cond']
    tol = tol_of(dt, key)
    s = xhandle(g, dt)
    if weighted:
        s.set_grad_weight(g['wg'])
    sums = s.admm_xstep(xparams(flags, u_scale, mu))
    X = s.download(_lib.VAR_X)
    assert X.dtype == dt and X.shape == (H, W, 1, N, K)
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(sums))
    err = rel_l2(X, ref['X'])
    print('x step %s %s: cond %.1f, X rel l2 %.3e (bound %.1e)' % (case, dtname, ref['cond'], err, tol))
    assert err < tol
    if last:
        # the frequencies a wrong stride or bound of the grid-stride loop drops: the tail of the spectrum
        Xf, want = mn.rfft2(mn.wide(X)).reshape(-1, N * K), ref['xf'].reshape(-1, N * K)
        assert rel_l2(Xf[-last:], want[-last:]) < tol
    asked = set()
    if flags & _lib.FLAG_OBJ:
        asked.add(_lib.OUT_DFID)
        e = norm_err(sums[_lib.OUT_DFID], ref['dfid'])
        print('  DFID %.3e' % e)
        assert e < tol
        if mu is not None:
            asked.add(_lib.OUT_RGR)
            e = norm_err(sums[_lib.OUT_RGR], ref['rgr'])
            print('  RGR %.3e' % e)
            assert e < tol
    if flags & _lib.FLAG_XRRS:
        asked.update((_lib.OUT_XRRS_D2, _lib.OUT_XRRS_AX2, _lib.OUT_XRRS_B2))
        ea, eb = norm_err(sums[_lib.OUT_XRRS_AX2], ref['xrrs_ax2']), norm_err(sums[_lib.OUT_XRRS_B2], ref['xrrs_b2'])
        res = math.sqrt(sums[_lib.OUT_XRRS_D2] / ref['xrrs_b2'])
        print('  XRRS: AX2 %.3e, B2 %.3e, residual %.3e' % (ea, eb, res))
        assert ea < tol and eb < tol
        # (ax - b is zero in exact arithmetic, for the kernel as for the dense solve)
        assert res < tol and math.sqrt(ref['xrrs_d2'] / ref['xrrs_b2']) < F64_TOL
    for i, v in enumerate(sums):
        if i not in asked:
            assert v == 0.0, (i, v)
    return X


# ---- 0. the NumPy statements against the reference's recorded results -------------------------------------
def test_numpy_statements_pinned_to_the_recorded_results():
    """The dense solve reproduces linalg.solvemdbi_ism's recorded solution (solvemdbi_ism.npz: which
    operand is conjugated, which axis is summed), and the first iteration of the reference's
    ConvBPDN / ConvBPDNGradReg runs with a multi-channel dictionary (Y = U = 0, rho = it_Rho[0]): its
    data fidelity and gradient term fix the layout of D, S and X, the Parseval weights, the gradient
    spectrum and the scale of the sums.  (The fixtures hold the final iterates only: X of the first
    iteration is pinned through DFid[0] and RegGrad[0], functions of it, and the transform convention
    through the recorded final X and Xf.)"""
    g = load_golden('solvemdbi_ism')
    A, b, rho = g['ah'][:, :, :, 0, :], g['b'][:, :, 0], float(g['rho'])
    M = np.einsum('hwck,hwcm->hwkm', np.conj(A), A) + rho * np.eye(A.shape[-1])
    x = np.swapaxes(np.linalg.solve(M, np.swapaxes(b, 2, 3)), 2, 3)[:, :, None]
    assert rel_l2(x, g['x']) < 1e-12
    # ... and the single-precision recursion is the same function
    x32 = mn.solvemdbi_ism_f32(A, np.full(A.shape[:2] + A.shape[3:], rho), b)[:, :, None]
    assert rel_l2(x32, g['x']) < 1e-5
    for name in ('admm_mcdict_f64', 'admm_gradreg_mcdict_f64'):
        g = load_golden(name)
        D, S = g['D'][:, :, :, None, :], g['S']
        H, W = S.shape[:2]
        Z = np.zeros(g['X'].shape)
        mu = float(g['mu'])
        kw = {'mu': mu, 'wg': g['optarr_GradWeight']} if mu > 0 else {}
        r = mn.xstep(D, S, Z, Z, float(g['it_Rho'][0]), **kw)
        assert abs(0.5 * r['dfid'] - g['it_DFid'][0]) < 1e-12 * g['it_DFid'][0]
        assert math.sqrt(r['xrrs_d2']) / max(math.sqrt(r['xrrs_ax2']), math.sqrt(r['xrrs_b2'])) < 1e-12
        assert g['it_XSlvRelRes'][0] < 1e-12
        assert rel_l2(mn.rfft2(g['X']), g['Xf']) < 1e-12
        if mu > 0:
            assert abs(0.5 * r['rgr'] - g['it_RegGrad'][0]) < 1e-12 * g['it_RegGrad'][0]
            ghg = mn.ghg(H, W)[:, :, None, None, None] * g['optarr_GradWeight']
            assert np.max(np.abs(ghg - g['GHGf'])) < 1e-12 * np.max(g['GHGf'])


# ---- 1. the x step ----------------------------------------------------------------------------------------
# (H, W, K, Cd, N, u_scale)
XSTEP_CASES = [
    (12, 10, 3, 2, 1, 1.0), (9, 7, 64, 3, 2, 1.0), (9, 7, 3, 4, 3, 1.0), (12, 10, 64, 5, 5, 1.0),
    (9, 7, 65, 2, 2, 1.0), (12, 10, 128, 3, 3, 1.0), (12, 10, 65, 4, 5, 1.0), (9, 7, 128, 8, 1, 1.0),
    (9, 7, 129, 2, 5, 1.0), (9, 7, 256, 3, 1, 1.0), (12, 10, 129, 4, 2, 1.0), (12, 10, 256, 8, 3, 1.0),
    (12, 10, 129, 5, 3, 0.75),
]
assert {(kr_of(c[2]), form_of(c[3])) for c in XSTEP_CASES} == \
    {(kr, f) for kr in (1, 2, 4) for f in ('cc2', 'cc3', 'cc4', 'runtime')}
assert {c[2] for c in XSTEP_CASES} == {3, 64, 65, 128, 129, 256} and {c[3] for c in XSTEP_CASES} == {2, 3, 4, 5, 8}
assert {c[4] for c in XSTEP_CASES} == {1, 2, 3, 5} and {waves_per_pixel(c[4]) for c in XSTEP_CASES} == {1, 2, 4}


def case_id(c):
    return '%dx%d-K%d-Cd%d-N%d' % c[:5] + ('' if len(c) < 6 or c[5] == 1.0 else '-uscale%g' % c[5])


@pytest.mark.parametrize('dt', RDTS)
@pytest.mark.parametrize('case', XSTEP_CASES, ids=case_id)
def test_xstep_plain(backend, case, dt):
    check_xstep(case, dt, 'xstep_plain')


FLAG_CASE = (9, 7, 65, 3, 2, 1.0)
FLAG_SETS = [pytest.param(_lib.FLAG_OBJ, id='obj'), pytest.param(_lib.FLAG_XRRS, id='xrrs'), pytest.param(0, id='none')]


@pytest.mark.parametrize('dt', RDTS)
@pytest.mark.parametrize('flags', FLAG_SETS)
def test_xstep_only_the_sums_asked_for(backend, flags, dt):
    """FLAG_OBJ alone, FLAG_XRRS alone, neither: X is the same, the slots not asked for are exactly zero."""
    check_xstep(FLAG_CASE, dt, 'xstep_plain', flags=flags)


# (H, W, K, Cd, N, u_scale): the gradient term, per-filter weights
GRAD_CASES = [(12, 10, 3, 2, 1, 1.0), (9, 7, 65, 8, 3, 1.0), (9, 7, 129, 2, 3, 1.0), (12, 10, 129, 8, 1, 1.0),
              (9, 7, 3, 8, 3, 1.0), (12, 10, 65, 2, 1, 0.75)]
MU = 0.3
MU0_CASE = (9, 7, 65, 2, 3, 1.0)
assert {(kr_of(c[2]), c[3]) for c in GRAD_CASES} == {(kr, cd) for kr in (1, 2, 4) for cd in (2, 8)}
assert {c[4] for c in GRAD_CASES} == {1, 3}


@pytest.mark.parametrize('dt', RDTS)
@pytest.mark.parametrize('case', GRAD_CASES, ids=case_id)
def test_xstep_gradient(backend, case, dt):
    assert form_of(case[3], grad=True) == 'runtime'
    check_xstep(case, dt, 'xstep_grad', mu=MU, weighted=True)


@pytest.mark.parametrize('dt', RDTS)
def test_xstep_gradient_with_mu_zero_is_the_plain_solve(backend, dt):
    """mu = 0: the GRAD instantiation (division by the diagonal, a run-time channel count) against the
    plain system's dense solve, within the same bound; OUT_RGR is still the weighted gradient norm."""
    Xg = check_xstep(MU0_CASE, dt, 'xstep_grad', mu=0.0, weighted=True)
    plain = xref(*MU0_CASE[:5], np.dtype(dt).name, MU0_CASE[5], None, False)
    assert rel_l2(Xg, plain['X']) < tol_of(dt, 'xstep_grad')


# ---- 2. gradient, evaluation, absmax ----------------------------------------------------------------------
# (H, W, K, Cd, N)
GEA_CASES = [(12, 10, 3, 2, 1), (9, 7, 15, 5, 3), (12, 10, 16, 2, 3), (9, 7, 20, 5, 1), (9, 7, 65, 2, 3),
             (12, 10, 129, 5, 1)]
assert {c[2] for c in GEA_CASES} == {3, 15, 16, 20, 65, 129} and {c[3] for c in GEA_CASES} == {2, 5}
assert {c[4] for c in GEA_CASES} == {1, 3}


@functools.lru_cache(maxsize=None)
def gref(H, W, K, Cd, N, dtname):
    g = xproblem(H, W, K, Cd, N, dtname)
    r = mn.pgm_grad(g['D'], g['S'], g['vf'])
    r['recon'] = mn.reconstruct(g['D'], g['Y'])
    r['masked_gf'] = mn.conj_outer_of_residual(g['D'], g['S'], g['vf'])
    r['absmax'] = mn.dhs_absmax(g['D'], g['S'])
    return r


def check_pgm_grad(s, g, ref, dt, keys, last=None):
    nan_gf = np.full(g['vf'].shape, np.nan, dtype=g['vf'].dtype)
    s.upload(_lib.VAR_VF, g['vf'])
    s.upload(_lib.VAR_GF, nan_gf)
    sums = s.pgm_grad(_lib.VAR_VF)
    gf = s.download(_lib.VAR_GF)
    assert gf.shape == g['vf'].shape and np.all(np.isfinite(gf)) and np.all(np.isfinite(sums))
    e = rel_l2(gf, ref['gf'])
    ef, ed = norm_err(sums[_lib.PGM_F], ref['f']), norm_err(sums[_lib.PGM_DFID], ref['dfid'])
    print('mc_pgm_grad: gf %.3e (bound %.1e), PGM_F %.3e, PGM_DFID %.3e (bound %.1e)'
          % (e, tol_of(dt, keys[0]), ef, ed, tol_of(dt, keys[1])))
    assert e < tol_of(dt, keys[0])
    assert ef < tol_of(dt, keys[1]) and ed < tol_of(dt, keys[1])
    if last:
        NK = gf.shape[3] * gf.shape[4]
        assert rel_l2(gf.reshape(-1, NK)[-last:], ref['gf'].reshape(-1, NK)[-last:]) < tol_of(dt, keys[0])
    return nan_gf


@pytest.mark.parametrize('dt', RDTS)
@pytest.mark.parametrize('case', GEA_CASES, ids=case_id)
def test_gradient_eval_absmax(backend, case, dt):
    H, W, K, Cd, N = case
    dtname = np.dtype(dt).name
    g, ref = xproblem(H, W, K, Cd, N, dtname), gref(H, W, K, Cd, N, dtname)
    s = xhandle(g, dt, nan_x=False)
    # mc_pgm_grad
    nan_gf = check_pgm_grad(s, g, ref, dt, ('grad_gf', 'grad_r'))
    # mc_inner through pgm_eval's sums ...
    sums = s.pgm_eval(_lib.VAR_VF)
    assert np.all(np.isfinite(sums))
    ef, ed = norm_err(sums[_lib.PGM_F], ref['f']), norm_err(sums[_lib.PGM_DFID], ref['dfid'])
    eh = norm_err(sums[_lib.PGM_HESS], ref['hess'])
    print('pgm_eval: PGM_F %.3e, PGM_DFID %.3e, PGM_HESS %.3e' % (ef, ed, eh))
    assert ef < tol_of(dt, 'grad_r') and ed < tol_of(dt, 'grad_r') and eh < tol_of(dt, 'grad_av')
    # ... and through reconstruct's array
    rec = s.reconstruct(_lib.VAR_Y)
    assert rec.shape == (H, W, Cd, N, 1) and np.all(np.isfinite(rec))
    e = rel_l2(rec, ref['recon'])
    print('reconstruct: %.3e (bound %.1e)' % (e, tol_of(dt, 'recon')))
    assert e < tol_of(dt, 'recon')
    # mc_inner and mc_conj_outer through masked_grad without a mask
    s.upload(_lib.VAR_GF, nan_gf)
    s.masked_grad(_lib.VAR_VF, False, 1)
    gf = s.download(_lib.VAR_GF)
    assert np.all(np.isfinite(gf))
    e = rel_l2(gf, ref['masked_gf'])
    print('masked_grad: gf %.3e (bound %.1e)' % (e, tol_of(dt, 'masked_gf')))
    assert e < tol_of(dt, 'masked_gf')
    # mc_dhs_absmax
    m = s.dhs_absmax()
    e = abs(m - ref['absmax']) / ref['absmax']
    print('dhs_absmax: %.3e (bound %.1e)' % (e, tol_of(dt, 'absmax')))
    assert e < tol_of(dt, 'absmax')


# ---- 3. the dictionary update, method ISM -----------------------------------------------------------------
# (H, W, K, Cd, N): N rank-one terms.  Cases that differ in N only share their inputs up to the extra
# images (every problem is cut from one of twelve images).
DSTEP_NMAX = 12
DSTEP_CASES = [(12, 10, 3, 1, 1), (9, 7, 65, 1, 2), (9, 7, 3, 1, 8), (9, 7, 3, 1, 9), (9, 7, 65, 1, 8),
               (9, 7, 65, 1, 9), (12, 10, 65, 1, 12), (12, 10, 3, 1, 12), (9, 7, 3, 3, 3)]
assert {c[4] for c in DSTEP_CASES} >= {1, 2, 8, 9, 12} and {c[2] for c in DSTEP_CASES} == {3, 65}
assert {(c[2], form_of(c[4])) for c in DSTEP_CASES} >= {(k, f) for k in (3, 65) for f in ('runtime', 'big')}


@functools.lru_cache(maxsize=None)
def dproblem(H, W, K, Cd, N, dtname):
    rng = np.random.RandomState([103, H, W, K, Cd])
    # sparse-ish coefficient maps, scaled so that Z^H Z is of the order of rho
    Z = rng.randn(H, W, 1, DSTEP_NMAX, K) * (rng.rand(H, W, 1, DSTEP_NMAX, K) < 0.3) / math.sqrt(K)
    g = {'Z': Z[:, :, :, :N], 'S': rng.randn(H, W, Cd, DSTEP_NMAX)[..., :N], 'Y0': rng.randn(H, W, Cd, 1, K),
         'U': 0.3 * rng.randn(H, W, Cd, 1, K)}
    out = {k: np.ascontiguousarray(v, dtype=np.dtype(dtname)) for k, v in g.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def dref(H, W, K, Cd, N, dtname):
    g = dproblem(H, W, K, Cd, N, dtname)
    return mn.dstep(g['Z'], g['S'], g['Y0'], g['U'], RHO)


@pytest.mark.parametrize('dt', RDTS)
@pytest.mark.parametrize('case', DSTEP_CASES, ids=case_id)
def test_dstep_ism(backend, case, dt):
    """X of one dstep_iter from a dstep_init(Y0) state (with a U of its own, so that Y - U is not zero)
    and its LinSolveCheck sums; the projection and the dual step that follow are not asserted here."""
    H, W, K, Cd, N = case
    dtname = np.dtype(dt).name
    g, ref = dproblem(H, W, K, Cd, N, dtname), dref(H, W, K, Cd, N, dtname)
    assert ref['cond'] < COND_MAX, ref['cond']
    tol = tol_of(dt, 'dstep')
    s = _lib.Solver(H, W, Cd, N, K, dt, Cd=Cd)
    s.set_signal(g['S'])
    s.upload(_lib.VAR_AX, g['Z'])
    s.ccmod_setcoef(_lib.VAR_AX)
    s.dstep_init(g['Y0'])
    s.upload(_lib.VAR_DSU, g['U'])
    s.upload(_lib.VAR_DSX, np.full(g['Y0'].shape, np.nan, dtype=dt))
    sums = s.dstep_iter(_lib.DSTEP_ISM, RHO, 1.8, 1.0, _lib.FLAG_XRRS, DH, DW, False)
    X = s.download(_lib.VAR_DSX)
    assert X.shape == (H, W, Cd, 1, K) and np.all(np.isfinite(X)) and np.all(np.isfinite(sums))
    err = rel_l2(X, ref['X'])
    ea, eb = norm_err(sums[_lib.OUT_XRRS_AX2], ref['xrrs_ax2']), norm_err(sums[_lib.OUT_XRRS_B2], ref['xrrs_b2'])
    res = math.sqrt(sums[_lib.OUT_XRRS_D2] / ref['xrrs_b2'])
    print('dstep %s %s (%s): cond %.1f, X %.3e, AX2 %.3e, B2 %.3e, residual %.3e (bound %.1e)'
          % (case, dtname, form_of(N), ref['cond'], err, ea, eb, res, tol))
    assert err < tol and ea < tol and eb < tol and res < tol
    assert math.sqrt(ref['xrrs_d2'] / ref['xrrs_b2']) < F64_TOL


def test_dstep_eight_and_nine_terms_share_their_inputs():
    """The 8 / 9 pair: identical inputs apart from the ninth image."""
    for K in (3, 65):
        a, b = dproblem(9, 7, K, 1, 8, 'float64'), dproblem(9, 7, K, 1, 9, 'float64')
        assert np.array_equal(a['Z'], b['Z'][:, :, :, :8]) and np.array_equal(a['S'], b['S'][..., :8])
        assert np.array_equal(a['Y0'], b['Y0']) and np.array_equal(a['U'], b['U'])
        assert form_of(8) == 'runtime' and form_of(9) == 'big'


# ---- 4. refusals ------------------------------------------------------------------------------------------
def test_more_than_256_filters_refused(backend):
    """K = 257: ism_dispatch_kr throws on the host before its caller reaches hipLaunchKernelGGL, in
    launch_ism_setup (the x step builds the tables first) as in launch_mc_pgm_grad; the handle goes on
    working for calls that need no such kernel."""
    H, W, K, Cd, N = 9, 7, 257, 2, 1
    g = xproblem(H, W, K, Cd, N, 'float64')
    s = xhandle(g, np.float64)
    with pytest.raises(_lib.BackendError, match='multi-channel dictionaries are handled for K <= 256 filters'):
        s.admm_xstep(xparams(0))
    s.upload(_lib.VAR_VF, g['vf'])
    with pytest.raises(_lib.BackendError, match='multi-channel dictionaries are handled for K <= 256 filters'):
        s.pgm_grad(_lib.VAR_VF)
    assert abs(s.dhs_absmax() - mn.dhs_absmax(g['D'], g['S'])) < F64_TOL * mn.dhs_absmax(g['D'], g['S'])


# ---- 5. above the grid caps (device only) -----------------------------------------------------------------
# (H, W, K, Cd, N, u_scale); neither height is one the fused multi-channel kernel takes
CAP_CASES = [(96, 88, 2, 2, 3, 1.0), (192, 176, 2, 2, 1, 1.0)]
assert 96 * 45 > MAX_BLOCKS * (WAVES_PER_BLOCK // waves_per_pixel(3))            # the solve, one frequency a workgroup
assert 192 * 89 > MAX_BLOCKS * (WAVES_PER_BLOCK // waves_per_pixel(1))           # the solve, four a workgroup
assert 192 * 89 > MAX_BLOCKS * WAVES_PER_BLOCK                                   # the setup, mc_pgm_grad


@pytest.mark.gpu
@pytest.mark.parametrize('dt', RDTS)
@pytest.mark.parametrize('case', CAP_CASES, ids=case_id)
def test_xstep_above_cap(backend, case, dt):
    """More frequencies than the capped grids cover in one pass: the solve (and, at 192 x 176, the setup)
    walk their loops a second time.  The float64 twin is the one that checks the indexing."""
    check_xstep(case, dt, 'xstep_above_cap', last=300)


@pytest.mark.gpu
@pytest.mark.parametrize('dt', RDTS)
def test_gradient_above_cap(backend, dt):
    H, W, K, Cd, N = CAP_CASES[1][:5]
    dtname = np.dtype(dt).name
    g = xproblem(H, W, K, Cd, N, dtname)
    ref = mn.pgm_grad(g['D'], g['S'], g['vf'])
    check_pgm_grad(xhandle(g, dt, nan_x=False), g, ref, dt, ('grad_above_cap_gf', 'grad_above_cap_r'), last=300)


# ---- the float32 bounds -----------------------------------------------------------------------------------
def measure_f32():
    """The float32 NumPy evaluation against the float64 reference on the very inputs of the tests above:
    the largest relative l2 error per key."""
    f32 = 'float32'
    m = {}

    def xs(case, mu=None, weighted=False):
        H, W, K, Cd, N, us = case
        g = xproblem(H, W, K, Cd, N, f32)
        got = mn.xstep_f32(g['D'], g['S'], g['Y'], g['U'], RHO, us, mu, g['wg'] if weighted else None)
        return rel_l2(got['X'], xref(H, W, K, Cd, N, f32, us, mu, weighted)['X'])

    m['xstep_plain'] = max(xs(c) for c in XSTEP_CASES + [FLAG_CASE])
    m['xstep_grad'] = max([xs(c, MU, True) for c in GRAD_CASES] + [xs(MU0_CASE, 0.0, True)])
    m['xstep_above_cap'] = max(xs(c) for c in CAP_CASES)
    e = {k: 0.0 for k in ('grad_gf', 'grad_r', 'grad_av', 'recon', 'masked_gf', 'absmax')}
    for H, W, K, Cd, N in GEA_CASES:
        g, ref = xproblem(H, W, K, Cd, N, f32), gref(H, W, K, Cd, N, f32)
        got = mn.pgm_grad_f32(g['D'], g['S'], g['vf'])
        e['grad_gf'] = max(e['grad_gf'], rel_l2(got['gf'], ref['gf']))
        e['grad_r'] = max(e['grad_r'], rel_l2(got['r'], ref['r']))
        e['grad_av'] = max(e['grad_av'], rel_l2(got['av'], ref['av']))
        e['recon'] = max(e['recon'], rel_l2(mn.reconstruct_f32(g['D'], g['Y']), ref['recon']))
        e['masked_gf'] = max(e['masked_gf'], rel_l2(mn.conj_outer_of_residual_f32(g['D'], g['S'], g['vf']),
                                                    ref['masked_gf']))
        e['absmax'] = max(e['absmax'], abs(mn.dhs_absmax_f32(g['D'], g['S']) - ref['absmax']) / ref['absmax'])
    m.update(e)
    H, W, K, Cd, N = CAP_CASES[1][:5]
    g = xproblem(H, W, K, Cd, N, f32)
    got, ref = mn.pgm_grad_f32(g['D'], g['S'], g['vf']), mn.pgm_grad(g['D'], g['S'], g['vf'])
    m['grad_above_cap_gf'] = rel_l2(got['gf'], ref['gf'])
    m['grad_above_cap_r'] = rel_l2(got['r'], ref['r'])
    m['dstep'] = 0.0
    for H, W, K, Cd, N in DSTEP_CASES:
        g = dproblem(H, W, K, Cd, N, f32)
        got = mn.dstep_f32(g['Z'], g['S'], g['Y0'], g['U'], RHO)
        m['dstep'] = max(m['dstep'], rel_l2(got['X'], dref(H, W, K, Cd, N, f32)['X']))
    return m


def test_f32_bounds_are_the_measured_ones():
    """F32_MEASURED is what NumPy gives in float32 (to the two digits recorded); every bound is four
    times that, rounded up to one significant digit (F32_BOUND is computed from it by bound_of)."""
    m = measure_f32()
    for k in sorted(m):
        print('%-20s measured %.3e   recorded %.1e   bound %.0e' % (k, m[k], F32_MEASURED[k], F32_BOUND[k]))
    assert set(m) == set(F32_MEASURED)
    for k, e in m.items():
        assert 0.5 * F32_MEASURED[k] < e < 1.5 * F32_MEASURED[k], k      # (the window of test_primitives_edges.py)
