"""sporco_amd.prox.proj_l1 and sporco_amd.admm.cbpdn.ConvBPDNProjL1 against the NumPy statements of
tests/_projl1_numpy.py: a sort-based projection onto the l1 ball, and the class's ADMM iteration built on
it.

Tolerances.  proj_l1: four times the floor that two NumPy evaluations of the threshold with different
summation orders show on the same input (measured in the helper for every case), never below 1e-12 in
float64 and 1e-6 in float32.  The class: the project's 1e-9 (float64) and 1e-4 on iterates / 1e-3 on
traces (float32 input against the float64 statement); Cnstr is a small difference late in a run and is
compared absolutely, |delta| <= tol * gamma.
"""

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _projl1_numpy as pn

from sporco_amd import prox
from sporco_amd.admm import cbpdn


def tol_for(dtype, floor):
    return max(4.0 * floor, 1e-12 if dtype == np.float64 else 1e-6)


# ---- prox.proj_l1 -----------------------------------------------------------------------------------------
PROJ_CASES = [((7, 9, 5), None), ((3, 10, 4), 1), ((3, 10, 5), -2), ((4, 3, 8), (1,)), ((6, 5, 3, 4), (0, 1, 3)),
              ((5, 7, 2, 6), (0, 1, 3))]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shape,axis', PROJ_CASES)
def test_proj_l1_against_sort(backend, shape, axis, dtype):
    rng = np.random.RandomState(11)
    v = rng.randn(*shape).astype(dtype)
    gamma = 2.5
    ref = pn.proj_l1(v, gamma, axis)
    assert np.any(ref != v)                       # (a set lies outside its ball)
    out = prox.proj_l1(v, gamma, axis=axis)
    assert out.dtype == v.dtype and out.shape == v.shape
    floor = pn.tau_floor(v, gamma, axis)
    err = rel_l2(out, ref)
    print('proj_l1 %s axis %s %s: err %.3e (floor %.3e)' % (shape, axis, np.dtype(dtype).name, err, floor))
    assert err <= tol_for(dtype, floor)
    # every set inside its ball
    axes = tuple(range(v.ndim)) if axis is None else ((axis,) if isinstance(axis, int) else axis)
    nrm = np.sum(np.abs(out.astype(np.float64)), axis=axes)
    nset = int(np.prod([shape[a] for a in axes]))
    assert np.all(nrm <= gamma * (1 + 4 * np.finfo(dtype).eps * nset))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_proj_l1_inside_ball_is_bitwise(backend, dtype):
    rng = np.random.RandomState(3)
    v = rng.randn(40, 2, 6).astype(dtype)
    v[:, 0] *= 1e-3                                # set 0 inside, set 1 outside
    gamma = 1.0
    assert np.abs(v[:, 0]).sum() < gamma < np.abs(v[:, 1]).sum()
    out = prox.proj_l1(v, gamma, axis=(0, 2))
    assert np.array_equal(out[:, 0], v[:, 0])
    ref = pn.proj_l1(v, gamma, (0, 2))
    assert rel_l2(out, ref) <= tol_for(dtype, pn.tau_floor(v, gamma, (0, 2)))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('case', ['zeros', 'gamma0', 'ties', 'single', 'pow2', 'long'])
def test_proj_l1_edges(backend, case, dtype):
    rng = np.random.RandomState(5)
    gamma = 1.5
    if case == 'zeros':
        v = np.zeros((9, 7), dtype)
    elif case == 'gamma0':
        v, gamma = rng.randn(33, 5).astype(dtype), 0.0
    elif case == 'ties':
        v = (0.75 * np.sign(rng.randn(101))).astype(dtype)
    elif case == 'single':
        v = np.zeros(77, dtype)
        v[13] = -4.0
    elif case == 'pow2':
        v = (2.0 ** -np.arange(60) * np.where(np.arange(60) % 2, -1, 1)).astype(dtype)
        gamma = 0.3
    else:
        v = rng.laplace(size=70001).astype(dtype)
        gamma = 50.0
    out = prox.proj_l1(v, gamma)
    ref = pn.proj_l1(v, gamma)
    if case in ('zeros', 'gamma0'):
        assert np.array_equal(out, np.zeros_like(v))
        return
    assert np.abs(out.astype(np.float64)).sum() <= gamma * (1 + 4 * np.finfo(dtype).eps * v.size)
    assert rel_l2(out, ref) <= tol_for(dtype, pn.tau_floor(v, gamma))


def test_proj_l1_arguments(backend):
    v = np.ones((3, 4))
    with pytest.raises(NotImplementedError):
        prox.proj_l1(v, np.ones(3))
    with pytest.raises(NotImplementedError):
        prox.proj_l1(v + 1j, 1.0)
    e = np.zeros((0, 4))
    assert prox.proj_l1(e, 1.0).shape == (0, 4)
    a = prox.proj_l1(v, 2.0)
    b = prox.proj_l1(v, 2.0)
    assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(256 * 256, 3, 6), (256 * 256, 1, 5)])
def test_proj_l1_gpu_sizes(gpu_backend, shape):
    rng = np.random.RandomState(17)
    v = rng.laplace(size=shape).astype(np.float32)
    gamma = 1000.0
    out = prox.proj_l1(v, gamma, axis=(0, 2))
    ref = pn.proj_l1(v, gamma, (0, 2))
    assert rel_l2(out, ref) <= tol_for(np.float32, pn.tau_floor(v, gamma, (0, 2)))
    nrm = np.sum(np.abs(out.astype(np.float64)), axis=(0, 2))
    assert np.all(nrm <= gamma * (1 + 4 * np.finfo(np.float32).eps * shape[0] * shape[2]))


# ---- the class: fixtures of the unmodified reference -------------------------------------------------------
CASES = ['default', 'fixed', 'autorho', 'auxvar', 'nonneg_nobndry', 'mcd', 'mcs', 'y0warm']
TRACES = ('ObjFun', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho')       # (Cnstr: absolutely)

# Measured, not taken from the library: the NumPy restatement run in float32 against each float64 fixture
# (test_f32_measured_figures repeats the measurement).  Worst case over the fixtures:
#   iterates and reconstruct(), relative l2: 3.0e-5 (U of mcd; the others 8.6e-8 ... 3.7e-6)
#   traces and the final rho:                3.0e-5 (the final rho of mcd, relative; its Rho trace 1.1e-5 in
#                                            relative l2, every other trace <= 1.4e-6)
#   Cnstr, worst |delta| / gamma:            8.4e-8
# Four times each of them lies below the project's figures, so those apply unchanged.
F32_ITER_MEASURED = 3.0e-5
F32_TRACE_MEASURED = 3.0e-5
F32_CNSTR_MEASURED = 8.4e-8
F32_ITER_TOL = max(4.0 * F32_ITER_MEASURED, 1e-4)
F32_TRACE_TOL = max(4.0 * F32_TRACE_MEASURED, 1e-3)
F32_CNSTR_TOL = max(4.0 * F32_CNSTR_MEASURED, 1e-3)

# Recovery (the analogue of the reference's test_22 for the l2 ball), measured between the two REFERENCE
# classes on the CPU: 16 x 17 image, 5 x 5 x 6 dictionary, seed 7, lambda = 0.2, 200 iterations each with
# default options; gamma = || Y ||_1 of the ConvBPDN solution.  Relative l2 difference of the two Y: 3.729e-3
# (of the reconstructions: 5.8e-4).  Allowed: twice that.
RECOVERY_MEASURED = 3.729e-3


def autorho_of(g):
    if not bool(g['opt_AutoRho']):
        return None
    return {'Period': int(g['opt_AutoRho_Period']), 'Scaling': float(g['opt_AutoRho_Scaling']),
            'RsdlRatio': float(g['opt_AutoRho_RsdlRatio']), 'AutoScaling': bool(g['opt_AutoRho_AutoScaling']),
            'RsdlTarget': float(g['opt_AutoRho_RsdlTarget'])}


def options_of(g, dtype, extra=None):
    o = {'Verbose': False, 'MaxMainIter': int(g['MaxMainIter']), 'RelStopTol': 0.0, 'rho': float(g['opt_rho']),
         'RelaxParam': float(g['opt_RelaxParam'])}
    for key in ('AuxVarObj', 'NonNegCoef', 'NoBndryCross'):
        if bool(g['opt_' + key]):
            o[key] = True
    ar = autorho_of(g)
    o['AutoRho'] = dict(ar, Enabled=True) if ar else {'Enabled': False}
    if 'optarr_Y0' in g:
        o['Y0'] = g['optarr_Y0'].astype(dtype)
    o.update(extra or {})
    return cbpdn.ConvBPDNProjL1.Options(o)


def five_d(g):
    """The fixture's D and S in the restatement's five-dimensional shapes."""
    D, S = g['D'], g['S']
    if S.ndim == 2:
        S5 = S.reshape(S.shape + (1, 1, 1))
    elif S.ndim == 3:
        S5 = S.reshape(S.shape[:2] + (1, S.shape[2], 1))
    else:
        S5 = S.reshape(S.shape + (1,))
    if D.ndim == 4:
        D5 = D.reshape(D.shape[:2] + (D.shape[2], 1, D.shape[3]))
    else:
        D5 = D.reshape(D.shape[:2] + (1, 1, D.shape[2]))
    return D5, S5


def restate(g, dtype=np.float64, iters=None, **kw):
    D5, S5 = five_d(g)
    return pn.admm_projl1(D5, S5, float(g['gamma']), int(g['MaxMainIter']) if iters is None else iters,
                          rho=float(g['opt_rho']), rlx=float(g['opt_RelaxParam']), auxvar=bool(g['opt_AuxVarObj']),
                          ar=autorho_of(g), nonneg=bool(g['opt_NonNegCoef']), nobndry=bool(g['opt_NoBndryCross']),
                          Y0=g['optarr_Y0'] if 'optarr_Y0' in g else None, dtype=dtype, **kw)


_GOLD, _F32 = {}, {}


def gold(case):
    if case not in _GOLD:
        _GOLD[case] = load_golden('projl1_%s_f64' % case)
    return _GOLD[case]


def errors(res, g):
    """res: X, Y, U, recon, rho and the traces (a restatement result, or collected from a solver)."""
    gamma = float(g['gamma'])
    e = {k: rel_l2(np.ravel(res[k]), np.ravel(g[k])) for k in ('X', 'Y', 'U', 'recon')}
    for k in TRACES:
        ref = g['it_' + k]
        e[k] = float(np.max(np.abs(res[k]))) if not np.any(ref) else rel_l2(np.asarray(res[k]), ref)
    e['rho_final'] = abs(float(res['rho']) - float(g['rho_final'])) / float(g['rho_final'])
    e['Cnstr'] = float(np.max(np.abs(np.asarray(res['Cnstr']) - g['it_Cnstr']))) / gamma
    return e


def check(e, ti, tt, tc):
    print({k: '%.2e' % v for k, v in e.items()})
    for k in ('X', 'Y', 'U', 'recon'):
        assert e[k] <= ti, (k, e[k])
    for k in TRACES + ('rho_final',):
        assert e[k] <= tt, (k, e[k])
    assert e['Cnstr'] <= tc, e['Cnstr']


def solved(g, dtype, extra=None, cls=None):
    cls = cls or cbpdn.ConvBPDNProjL1
    b = cls(g['D'].astype(dtype), g['S'].astype(dtype), float(g['gamma']), options_of(g, dtype, extra),
            dimK=int(g['dimK']))
    b.solve()
    its = b.getitstat()
    res = {k: np.array(getattr(its, k)) for k in TRACES + ('Cnstr',)}
    res.update(X=b.X, Y=b.Y, U=b.U, recon=b.reconstruct(), rho=float(b.rho))
    return b, res


@pytest.mark.parametrize('case', CASES)
def test_restatement_reproduces_fixture(case):
    g = gold(case)
    r = restate(g)
    check(errors(r, g), 1e-9, 1e-9, 1e-9)
    assert np.array_equal(np.mean(r['active'], axis=0), g['active_share'])


def test_restatement_one_step_from_39():
    g = load_golden('projl1_step_f64')
    f = gold('fixed')
    shp = g['Y_before'].shape
    st = dict(Y=g['Y_before'].copy(), U=g['U_before'].copy(), rho=np.float64(g['rho_before']))
    r = restate(f, iters=1, state=st, k0=int(g['k']))
    for k in ('X', 'Y', 'U'):
        assert rel_l2(r[k].reshape(shp), g[k]) <= 1e-9
    for k in ('ObjFun', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert abs(r[k][-1] - float(g['last_' + k])) <= 1e-9 * abs(float(g['last_' + k]))
    assert abs(r['Cnstr'][-1] - float(g['last_Cnstr'])) <= 1e-9 * float(g['gamma'])


def test_fixtures_take_both_branches():
    """From the recorded shares: in every two-image case one image projects in (nearly) every iteration and
    the other in some iterations and not in others."""
    for case in CASES:
        share = gold(case)['active_share']
        if case == 'y0warm':
            assert share.shape == (1,)
            continue
        assert np.any(share >= 0.9) and np.any((share >= 0.02) & (share <= 0.5)), (case, share)


@pytest.mark.parametrize('case', CASES)
def test_fixture_f64(backend, case):
    g = gold(case)
    b, res = solved(g, np.float64)
    check(errors(res, g), 1e-9, 1e-9, 1e-9)


def f32_restatement(case):
    if case not in _F32:
        _F32[case] = errors(restate(gold(case), dtype=np.float32), gold(case))
    return _F32[case]


def test_f32_measured_figures():
    """The float32 run of the restatement against the float64 fixtures gives the figures written above."""
    worst = {'iter': 0.0, 'trace': 0.0, 'cnstr': 0.0}
    for case in CASES:
        e = f32_restatement(case)
        worst['iter'] = max([worst['iter']] + [e[k] for k in ('X', 'Y', 'U', 'recon')])
        worst['trace'] = max([worst['trace']] + [e[k] for k in TRACES + ('rho_final',)])
        worst['cnstr'] = max(worst['cnstr'], e['Cnstr'])
    print(worst)
    assert 0.5 * F32_ITER_MEASURED <= worst['iter'] <= 1.05 * F32_ITER_MEASURED
    assert 0.5 * F32_TRACE_MEASURED <= worst['trace'] <= 1.05 * F32_TRACE_MEASURED
    assert 0.5 * F32_CNSTR_MEASURED <= worst['cnstr'] <= 1.05 * F32_CNSTR_MEASURED


@pytest.mark.parametrize('case', CASES)
def test_fixture_f32(backend, case):
    g = gold(case)
    b, res = solved(g, np.float32)
    check(errors(res, g), F32_ITER_TOL, F32_TRACE_TOL, F32_CNSTR_TOL)


def test_recovery_of_convbpdn_solution(backend):
    rng = np.random.RandomState(7)
    D = rng.randn(5, 5, 6)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(16, 17)
    o = {'Verbose': False, 'MaxMainIter': 200, 'RelStopTol': 0.0}
    a = cbpdn.ConvBPDN(D, S, 0.2, cbpdn.ConvBPDN.Options(o))
    Ya = a.solve()
    gamma = float(np.sum(np.abs(Ya)))
    b = cbpdn.ConvBPDNProjL1(D, S, gamma, cbpdn.ConvBPDNProjL1.Options(o))
    Yb = b.solve()
    err = rel_l2(Yb, Ya)
    print('recovery: gamma %.4f, rel l2 %.3e (reference classes: %.3e)' % (gamma, err, RECOVERY_MEASURED))
    assert err <= 2.0 * RECOVERY_MEASURED


# ---- the class: behaviour ----------------------------------------------------------------------------------
def problem(H, W, M, N, dtype, seed=7, dsz=5):
    rng = np.random.RandomState(seed)
    D = rng.randn(dsz, dsz, M)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(H, W, N) * np.array([0.02] + [1.0] * (N - 1))
    return D.astype(dtype), S.astype(dtype)


def fixed_opts(iters, **kw):
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0, 'rho': 2.0, 'RelaxParam': 1.8,
         'AutoRho': {'Enabled': False}}
    o.update(kw)
    return cbpdn.ConvBPDNProjL1.Options(o)


def numpy_run(D, S, gamma, iters, dtype=np.float64, ar=None, **kw):
    """The restatement on (H, W, N) signals and (dH, dW, M) dictionaries."""
    return pn.admm_projl1(D.astype(np.float64).reshape(D.shape[:2] + (1, 1, D.shape[2])),
                          S.astype(np.float64).reshape(S.shape[:2] + (1, S.shape[2], 1)), gamma, iters, rho=2.0,
                          rlx=1.8, ar=ar, dtype=dtype, **kw)


def compare(b, ref, dtype, gamma):
    ti, tt = (1e-9, 1e-9) if dtype == np.float64 else (F32_ITER_TOL, F32_TRACE_TOL)
    its = b.getitstat()
    errs = {'X': rel_l2(b.X, ref['X']), 'Y': rel_l2(b.Y, ref['Y']), 'U': rel_l2(b.U, ref['U']),
            'recon': rel_l2(b.reconstruct(), ref['recon']),
            'ObjFun': rel_l2(np.array(its.ObjFun), ref['ObjFun']),
            'PrimalRsdl': rel_l2(np.array(its.PrimalRsdl), ref['PrimalRsdl']),
            'DualRsdl': rel_l2(np.array(its.DualRsdl), ref['DualRsdl']),
            'Cnstr': np.max(np.abs(np.array(its.Cnstr) - ref['Cnstr'])) / gamma}
    print(errs)
    for k in ('X', 'Y', 'U', 'recon'):
        assert errs[k] <= ti, (k, errs[k])
    for k in ('ObjFun', 'PrimalRsdl', 'DualRsdl', 'Cnstr'):
        assert errs[k] <= tt, (k, errs[k])


def test_class_interface(backend):
    D, S = problem(16, 17, 6, 2, np.float64)
    opt = cbpdn.ConvBPDNProjL1.Options()
    assert opt['AutoRho', 'RsdlTarget'] == 1.0 and opt['AutoRho', 'Enabled']
    b = cbpdn.ConvBPDNProjL1(D, S, 4.0, cbpdn.ConvBPDNProjL1.Options({'MaxMainIter': 3, 'Verbose': False}))
    b.solve()
    assert b.getitstat()._fields == ('Iter', 'ObjFun', 'Cnstr', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual',
                                     'Rho', 'XSlvRelRes', 'Time')
    assert cbpdn.ConvBPDNProjL1.hdrtxt_objfn == ('Fnc', 'Cnstr')
    with pytest.raises(NotImplementedError):
        cbpdn.ConvBPDNProjL1(D[0], S[0], 4.0, dimN=1)
    with pytest.raises(NotImplementedError):
        cbpdn.ConvBPDNProjL1(D + 0j, S, 4.0)
    with pytest.raises(NotImplementedError):
        cbpdn.ConvBPDNProjL1(D, S, 4.0, reducer=object())
    with pytest.raises(NotImplementedError):
        cbpdn.ConvBPDNProjL1(D, S, 4.0, resident=True)
    from sporco_amd.device import DeviceArray
    with pytest.raises(NotImplementedError):
        cbpdn.ConvBPDNProjL1(D, DeviceArray.from_host(S), 4.0)
    with pytest.raises(NotImplementedError):
        cbpdn.ConvBPDNProjL1(DeviceArray.from_host(D), S, 4.0)
    with pytest.raises(NotImplementedError):
        cbpdn.AddMaskSim(cbpdn.ConvBPDNProjL1, D, S, np.ones(S.shape), 4.0)
    Y0 = np.random.RandomState(1).randn(16, 17, 1, 2, 6)
    b0 = cbpdn.ConvBPDNProjL1(D, S, 4.0, cbpdn.ConvBPDNProjL1.Options({'Y0': Y0, 'Verbose': False}))
    assert np.array_equal(b0.U, np.zeros_like(Y0)) and np.array_equal(b0.Y, Y0)


def test_class_two_runs_bitwise_linsolve_setdict(backend):
    D, S = problem(16, 17, 6, 2, np.float32)
    runs = []
    for _ in range(2):
        b = cbpdn.ConvBPDNProjL1(D, S, 4.0, cbpdn.ConvBPDNProjL1.Options(
            {'MaxMainIter': 8, 'Verbose': False, 'RelStopTol': 0.0, 'LinSolveCheck': True}))
        b.solve()
        runs.append((b.X.copy(), b.Y.copy(), b.U.copy(), np.array(b.getitstat().Cnstr)))
        assert b.getitstat().XSlvRelRes[-1] < 1e-4
    for a, c in zip(*runs):
        assert np.array_equal(a, c)


def test_class_setdict_mid_run(backend):
    """Four iterations, a new dictionary, four more: the restatement continued from its state with the new
    dictionary (the iteration count runs on, as ADMM.solve's does)."""
    D, S = problem(16, 17, 6, 2, np.float64)
    D2, _ = problem(16, 17, 6, 2, np.float64, seed=8)
    b = cbpdn.ConvBPDNProjL1(D, S, 4.0, fixed_opts(4))
    b.solve()
    b.setdict(D2.reshape(b.D.shape))
    b.solve()
    r1 = numpy_run(D, S, 4.0, 4)
    r2 = numpy_run(D2, S, 4.0, 4, state=r1['state'], k0=4)
    for k in ('X', 'Y', 'U'):
        assert rel_l2(getattr(b, k), r2[k]) <= 1e-9, k
    its = b.getitstat()
    assert rel_l2(np.array(its.ObjFun), np.concatenate((r1['ObjFun'], r2['ObjFun']))) <= 1e-9


@pytest.mark.parametrize('opts', [{}, {'NonNegCoef': True, 'NoBndryCross': True}, {'AuxVarObj': True}],
                         ids=['plain', 'nonneg_nobndry', 'auxvar'])
def test_class_staged_equals_one_call(backend, opts):
    D, S = problem(16, 17, 6, 2, np.float64)

    class Hooked(cbpdn.ConvBPDNProjL1):
        calls = 0

        def ystep(self):
            Hooked.calls += 1
            super(Hooked, self).ystep()

    o = fixed_opts(6, **opts)
    a = cbpdn.ConvBPDNProjL1(D, S, 4.0, o)
    a.solve()
    h = Hooked(D, S, 4.0, o)
    h.solve()
    assert Hooked.calls == 6
    Hooked.calls = 0
    assert rel_l2(h.Y, a.Y) <= 1e-9 and rel_l2(h.U, a.U) <= 1e-9 and rel_l2(h.X, a.X) <= 1e-9
    assert np.max(np.abs(np.array(h.getitstat().Cnstr) - np.array(a.getitstat().Cnstr))) <= 1e-9 * 4.0


def test_class_fastsolve_skips_second_search(backend):
    D, S = problem(16, 17, 6, 2, np.float32)
    counts = {}
    for fast in (False, True):
        b = cbpdn.ConvBPDNProjL1(D, S, 4.0, fixed_opts(4, FastSolve=fast))
        b.profile(True)
        b.solve()
        prof = b.profile_read()
        counts[fast] = prof['projl1_search']['count'] if isinstance(prof['projl1_search'], dict) else prof['projl1_search'][1]
        assert (b.search_passes[1] == 0) == fast
    assert counts[True] < counts[False]


GPU_SHAPES = [(128, 8, 3, np.float32), (128, 8, 3, np.float64), (256, 64, 2, np.float32)]


@pytest.mark.gpu
@pytest.mark.parametrize('HW,M,N,dtype', GPU_SHAPES)
def test_class_gpu_sizes(gpu_backend, HW, M, N, dtype):
    D, S = problem(HW, HW, M, N, dtype, dsz=8)
    gamma, iters = 50.0, 5
    b = cbpdn.ConvBPDNProjL1(D, S, gamma, fixed_opts(iters))
    b.solve()
    ref = numpy_run(D, S, gamma, iters)
    compare(b, ref, dtype, gamma)
    # one iteration from a random state
    rng = np.random.RandomState(23)
    Y0, U0 = (0.05 * rng.randn(*b.Y.shape)).astype(dtype), (0.05 * rng.randn(*b.Y.shape)).astype(dtype)
    b1 = cbpdn.ConvBPDNProjL1(D, S, gamma, fixed_opts(1, Y0=Y0, U0=U0))
    b1.solve()
    ref1 = numpy_run(D, S, gamma, 1, state=dict(Y=Y0.astype(np.float64), U=U0.astype(np.float64), rho=np.float64(2.0)))
    compare(b1, ref1, dtype, gamma)
    print('search passes (y step, constraint):', b.search_passes)


@pytest.mark.parametrize('dtype', [np.float32])
def test_class_hostsim_128(backend, dtype):
    D, S = problem(128, 128, 8, 3, dtype, dsz=8)
    gamma = 50.0
    b = cbpdn.ConvBPDNProjL1(D, S, gamma, fixed_opts(2))
    b.solve()
    ref = numpy_run(D, S, gamma, 2)
    compare(b, ref, dtype, gamma)
