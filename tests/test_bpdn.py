"""sporco_amd.admm.bpdn BPDN / BPDNJoint / ElasticNet against fixtures of the unmodified reference
(tests/golden/bpdn_*_f64.npz, tools/make_golden_bpdn.py) and against the NumPy statement of tests/_bpdn_numpy.py.

Tolerances.  float64: the project's 1e-9 relative l2 on iterates, traces and the final rho.  XSlvRelRes sits at
rounding level: the float64 statement differs from the fixtures by at most XRRS_STATEMENT_F64 (absolute), the
bound is four times that; in float32 four times what the float32 statement shows, XRRS_STATEMENT_F32.  float32
input against the float64 fixture: 1e-4 on iterates and 1e-3 on traces, or four times what the NumPy statement run
in float32 shows against the same fixture, whichever is larger, per case: F32_MEASURED below
(test_f32_measured_figures repeats the measurement on the CPU).  The margin of four covers the summation order
and the rounding of the solve matrix, which the device multiplies by where the statement solves with a Cholesky
factor.  In float64 the statement reproduces every fixture to 2.9e-11 (test_statement_reproduces_fixtures bounds it by
1e-10), `setdict` in its two stages included; the widest float32 figure is 2.8e-4 (`elnet`), so no float32 bound
is wider than 1.2e-3 on iterates.

The residuals follow the reference: admm.py:462-486 takes them on the unrelaxed X (`AXnr`), and so do the
fixtures.

Every fixture case was checked on the CPU to follow the reference's rho path in float32: the float32 statement's
final rho is within F32_MEASURED's trace figure of the fixture's, no case changes rho at another iteration
(test_f32_measured_figures asserts the same set of change points).
"""

import os
import pickle

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _bpdn_numpy as bn

from sporco_amd import _lib
from sporco_amd.admm import bpdn
from sporco_amd.device import DeviceArray

CASES = ['default', 'lmbda_none', 'auxvar_off', 'fixedrho', 'stdres', 'lsc', 'nonneg', 'w_atom', 'w_signal',
         'w_full', 'y0', 'y0u0', 'returnx', 'square', 'tall', 'k1', 'joint', 'joint_zero', 'joint_small',
         'joint_nonneg', 'elnet', 'elnet_lsc', 'elnet_auxvar_off', 'elnet_mu0']
ALG = ('PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho')
F64_TOL = 1e-9
# the NumPy statement against the fixtures: XSlvRelRes, absolute, worst case over the cases that record it
XRRS_STATEMENT_F64 = 3e-15
XRRS_STATEMENT_F32 = 5e-6
# case: (iterates, traces and final rho) of the float32 statement against the float64 fixture
F32_MEASURED = {'default': (3.0e-5, 2.5e-5), 'lmbda_none': (7.0e-5, 6.9e-5), 'auxvar_off': (3.0e-5, 2.5e-5),
                'fixedrho': (2.5e-6, 8.7e-7), 'stdres': (1.2e-5, 9.7e-6), 'lsc': (3.0e-5, 2.5e-5),
                'nonneg': (1.1e-5, 1.2e-5), 'w_atom': (6.2e-5, 6.1e-5), 'w_signal': (3.9e-5, 3.9e-5),
                'w_full': (4.4e-5, 4.4e-5), 'y0': (1.3e-5, 5.8e-6), 'y0u0': (3.2e-5, 3.1e-5),
                'returnx': (3.0e-5, 2.5e-5), 'square': (8.0e-6, 8.0e-6), 'tall': (1.4e-6, 1.3e-6),
                'k1': (1.6e-5, 1.1e-5), 'joint': (8.5e-5, 8.6e-5), 'joint_zero': (1.2e-5, 1.2e-5),
                'joint_small': (1.4e-6, 5.2e-7), 'joint_nonneg': (5.8e-6, 4.6e-6), 'elnet': (2.8e-4, 2.8e-4),
                'elnet_lsc': (2.8e-4, 2.8e-4), 'elnet_auxvar_off': (2.8e-4, 2.8e-4), 'elnet_mu0': (3.0e-5, 2.5e-5)}
# one step from the state of bpdn_step_f64.npz: the float32 statement against the recorded float64 values
F32_STEP_MEASURED = {'ObjFun': 1.3e-7, 'DFid': 1.4e-5, 'RegL1': 9.1e-7, 'PrimalRsdl': 6.3e-5, 'DualRsdl': 4.2e-5}

_GOLD = {}


def gold(case):
    if case not in _GOLD:
        _GOLD[case] = load_golden('bpdn_%s_f64' % case)
    return _GOLD[case]


def flat_opts(g, dtype):
    """The options a fixture records, as the flat dict of tests/_bpdn_numpy.py."""
    o = {}
    for k in g:
        if k.startswith('opt_'):
            v = float(g[k])
            name = k[4:]
            if name in ('MaxMainIter', 'AutoRho.Period'):
                v = int(v)
            elif name in ('AuxVarObj', 'LinSolveCheck', 'NonNegCoef', 'ReturnX', 'AutoRho.Enabled',
                          'AutoRho.StdResiduals'):
                v = bool(v)
            o[name] = v
        elif k.startswith('optarr_') and k != 'optarr_D2':
            o[k[7:]] = g[k].astype(dtype)
    return o


def options_of(cls, g, dtype, extra=None):
    o = {'Verbose': False}
    for k, v in flat_opts(g, dtype).items():
        if '.' in k:
            a, b = k.split('.')
            o.setdefault(a, {})[b] = v
        else:
            o[k] = v
    for k, v in (extra or {}).items():
        if isinstance(v, dict):
            o.setdefault(k, {}).update(v)
        else:
            o[k] = v
    return cls.Options(o)


def build(g, dtype, extra=None):
    cname = str(g['cls'])
    cls = getattr(bpdn, cname)
    lm = None if float(g['lmbda_given']) == 0.0 else float(g['lmbda_given'])
    args = (g['D'].astype(dtype), g['S'].astype(dtype), lm)
    if cname != 'BPDN':
        args += (float(g['mu']),)
    return cls(*args, opt=options_of(cls, g, dtype, extra))


def statement(g, dtype, **kw):
    cname = str(g['cls'])
    o = flat_opts(g, dtype)
    o.pop('ReturnX', None)
    lm = None if float(g['lmbda_given']) == 0.0 else float(g['lmbda_given'])
    return bn.run(cname, g['D'], g['S'], lm, float(g['mu']), o, dtype=dtype, **kw)


def trace_fields(g):
    return bn.FIELDS[str(g['cls'])] + ALG


def compare(res, g, traces_of):
    """(worst iterate error, worst trace error with the final rho, XSlvRelRes absolute error or None)."""
    ei = max(rel_l2(res['X'], g['X']), rel_l2(res['Y'], g['Y']), rel_l2(res['U'], g['U']))
    et = max(rel_l2(traces_of(f), g['it_' + f]) for f in trace_fields(g))
    et = max(et, abs(float(res['rho']) - float(g['rho_final'])) / float(g['rho_final']))
    ex = None
    if 'it_XSlvRelRes' in g:
        ex = float(np.max(np.abs(np.asarray(traces_of('XSlvRelRes'), dtype=np.float64) - g['it_XSlvRelRes'])))
    return ei, et, ex


def setdict_statement(g, dtype):
    """The two stages of the `setdict` fixture: a solve with D, then one with D2 from the state the first left."""
    o = flat_opts(g, dtype)
    r1 = bn.run('BPDN', g['D'], g['S'], float(g['lmbda']), 0.0, o, dtype=dtype)
    r = bn.run('BPDN', g['optarr_D2'], g['S'], float(g['lmbda']), 0.0, o, dtype=dtype, Y=r1['Y'], U=r1['U'],
               rho=r1['rho'], k0=int(g['opt_MaxMainIter']))
    r['Y_first'] = r1['Y']
    return r


def f32_tols(case):
    mi, mt = F32_MEASURED[case]
    return max(4.0 * mi, 1e-4), max(4.0 * mt, 1e-3)


def rho_changes(rho):
    rho = np.asarray(rho, dtype=np.float64)
    return tuple(np.nonzero(rho[1:] != rho[:-1])[0])


# ---- the statement and the fixtures (CPU only) ---------------------------------------------------------------
def test_statement_reproduces_fixtures():
    worst, worst_x = 0.0, 0.0
    for case in CASES + ['setdict']:
        g = gold(case)
        if case == 'setdict':
            r = setdict_statement(g, np.float64)
            assert rel_l2(r['Y_first'], g['Y_first']) <= 1e-10
        else:
            r = statement(g, np.float64)
        ei, et, ex = compare(r, g, lambda f: r[f])
        worst = max(worst, ei, et)
        if ex is not None:
            worst_x = max(worst_x, ex)
    print('statement in float64 against the fixtures: %.2e; XSlvRelRes %.2e' % (worst, worst_x))
    assert worst <= 1e-10
    assert worst_x <= XRRS_STATEMENT_F64


def test_f32_measured_figures():
    """The figures of F32_MEASURED, measured again; every case follows the fixture's rho path in float32."""
    worst_x = 0.0
    for case in CASES:
        g = gold(case)
        r = statement(g, np.float32)
        ei, et, ex = compare(r, g, lambda f: r[f])
        print("'%s': (%.1e, %.1e)," % (case, ei, et))
        assert rho_changes(r['Rho']) == rho_changes(g['it_Rho']), case
        assert ei <= F32_MEASURED[case][0] and et <= F32_MEASURED[case][1], (case, ei, et)
        if ex is not None:
            worst_x = max(worst_x, ex)
    print('XSlvRelRes %.2e' % worst_x)
    assert worst_x <= XRRS_STATEMENT_F32


def test_fixtures_hold_their_conditions():
    for case in CASES:
        g = gold(case)
        for f in trace_fields(g):
            assert np.all(np.isfinite(g['it_' + f])) and len(g['it_' + f]) == int(g['opt_MaxMainIter']), (case, f)
        if bool(g.get('opt_AutoRho.Enabled', 1.0)):
            assert len(rho_changes(g['it_Rho'])) >= 1, case
        else:
            assert len(rho_changes(g['it_Rho'])) == 0
    assert 'it_XSlvRelRes' in gold('lsc') and 'it_XSlvRelRes' in gold('elnet_lsc')
    assert 'it_XSlvRelRes' not in gold('default')
    for case in ('nonneg', 'joint_nonneg'):
        assert int(gold(case)['negative_unclipped']) > 0 and not np.any(gold(case)['Y'] < 0)
    rows = np.sqrt(np.sum(gold('joint_zero')['Y'] ** 2, axis=1))
    assert np.any(rows == 0) and np.any(rows > 0)
    assert np.all(np.sum(gold('joint_small')['Y'] ** 2, axis=1) > 0)
    assert gold('w_atom')['optarr_L1Weight'].shape == (16, 1)
    assert gold('w_signal')['optarr_L1Weight'].shape == (1, 5)
    assert gold('w_full')['optarr_L1Weight'].shape == (16, 5)
    assert gold('square')['D'].shape == (8, 8) and gold('tall')['D'].shape == (24, 16) and gold('k1')['S'].shape == (8, 1)
    assert float(gold('lmbda_none')['lmbda_given']) == 0.0
    assert abs(float(gold('lmbda_none')['lmbda']) - bn.default_lmbda(gold('lmbda_none')['D'], gold('lmbda_none')['S'])) < 1e-15
    assert 'optarr_Y0' in gold('y0') and 'optarr_U0' not in gold('y0') and 'optarr_U0' in gold('y0u0')
    for f in ('X', 'Y', 'U', 'it_ObjFun', 'it_Rho'):
        assert np.array_equal(gold('default')[f], gold('elnet_mu0')[f]), f
    assert not np.array_equal(gold('returnx')['X'], gold('returnx')['Y'])
    s = gold('setdict')
    assert not np.array_equal(s['D'], s['optarr_D2']) and not np.array_equal(s['Y_first'], s['Y'])
    r = load_golden('bpdn_recover_f64')
    assert np.linalg.norm(r['Y'] - r['x0']) < 1e-3 and np.count_nonzero(r['x0']) == 4


# ---- the classes against the fixtures of the unmodified reference --------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('case', CASES)
def test_against_reference_fixture(backend, case, dtype):
    g = gold(case)
    b = build(g, dtype)
    out = b.solve()
    its = b.getitstat()
    res = {'X': b.X, 'Y': b.Y, 'U': b.U, 'rho': b.rho}
    ei, et, ex = compare(res, g, lambda f: getattr(its, f))
    print('%s %s: iterates %.2e traces %.2e xrrs %s' % (case, np.dtype(dtype).name, ei, et, ex))
    tol_i, tol_t = (F64_TOL, F64_TOL) if dtype == np.float64 else f32_tols(case)
    assert out.dtype == dtype and out.shape == g['Y'].shape and b.X.dtype == dtype and b.U.dtype == dtype
    assert np.array_equal(out, b.X if case == 'returnx' else b.Y)
    assert np.array_equal(b.getcoef(), b.Y)
    assert its._fields == ('Iter',) + trace_fields(g) + ('XSlvRelRes', 'Time')
    assert np.array_equal(its.Iter, np.arange(len(g['it_ObjFun'])))
    if ex is None:
        assert all(v is None for v in its.XSlvRelRes)
    else:
        assert ex <= 4.0 * (XRRS_STATEMENT_F64 if dtype == np.float64 else XRRS_STATEMENT_F32)
    assert ei <= tol_i and et <= tol_t, (ei, et)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_setdict_between_solves(backend, dtype):
    g = gold('setdict')
    b = build(g, dtype)
    b.solve()
    first = b.Y.copy()
    b.itstat = []
    b.setdict(g['optarr_D2'].astype(dtype))
    assert np.array_equal(b.Y, first)                      # Y and U are kept
    assert rel_l2(b.DTS, g['optarr_D2'].T.dot(g['S'])) <= (1e-13 if dtype == np.float64 else 1e-6)
    b.solve()
    its = b.getitstat()
    res = {'X': b.X, 'Y': b.Y, 'U': b.U, 'rho': b.rho}
    ei, et, _ = compare(res, g, lambda f: getattr(its, f))
    r32 = None
    if dtype == np.float32:
        r32 = setdict_statement(g, np.float32)
        si, st, _ = compare(r32, g, lambda f: r32[f])
        print('float32 statement: %.2e %.2e' % (si, st))
        tol_i, tol_t = max(4.0 * si, 1e-4), max(4.0 * st, 1e-3)
    else:
        tol_i = tol_t = F64_TOL
    print('setdict %s: %.2e %.2e' % (np.dtype(dtype).name, ei, et))
    assert rel_l2(first, g['Y_first']) <= tol_i
    assert ei <= tol_i and et <= tol_t


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_one_step_from_recorded_state(backend, dtype):
    g = load_golden('bpdn_step_f64')
    o = {'Verbose': False, 'MaxMainIter': 1, 'RelStopTol': 0.0, 'rho': float(g['rho_before']),
         'AutoRho': {'Period': int(g['opt_AutoRho.Period'])}, 'Y0': g['Y_before'].astype(dtype),
         'U0': g['U_before'].astype(dtype)}
    b = bpdn.BPDN(g['D'].astype(dtype), g['S'].astype(dtype), float(g['lmbda']), bpdn.BPDN.Options(o))
    b.k = int(g['k'])
    b.solve()
    it = b.itstat[-1]
    fields = ('ObjFun', 'DFid', 'RegL1', 'PrimalRsdl', 'DualRsdl')
    terr = {f: abs(float(getattr(it, f)) - float(g['last_' + f])) / abs(float(g['last_' + f])) for f in fields}
    ei = max(rel_l2(b.X, g['X']), rel_l2(b.Y, g['Y']), rel_l2(b.U, g['U']))
    print('step %s: iterates %.2e %s' % (np.dtype(dtype).name, ei, {k: '%.1e' % v for k, v in terr.items()}))
    if dtype == np.float64:
        assert ei <= F64_TOL and max(terr.values()) <= F64_TOL
        assert abs(float(b.rho) - float(g['rho_final'])) <= F64_TOL * float(g['rho_final'])
    else:
        fo = {'AutoRho.Period': int(g['opt_AutoRho.Period'])}
        r = bn.run('BPDN', g['D'], g['S'], float(g['lmbda']), 0.0, fo, dtype=np.float32, iters=1, Y=g['Y_before'],
                   U=g['U_before'], rho=float(g['rho_before']), k0=int(g['k']))
        for f in fields:
            m = abs(float(r[f][-1]) - float(g['last_' + f])) / abs(float(g['last_' + f]))
            assert m <= F32_STEP_MEASURED[f], (f, m)
            assert terr[f] <= max(4.0 * F32_STEP_MEASURED[f], 1e-3), (f, terr[f])
        assert ei <= 1e-4


def test_sparse_recovery(backend):
    """The problem of the reference's tests/admm/test_bpdn.py::TestSet01::test_08 and what it asserts."""
    r = load_golden('bpdn_recover_f64')
    opt = bpdn.BPDN.Options({'Verbose': False, 'MaxMainIter': int(r['MaxMainIter']), 'RelStopTol': float(r['RelStopTol'])})
    b = bpdn.BPDN(r['D'], r['S'], float(r['lmbda']), opt)
    b.solve()
    x1 = b.Y
    assert np.abs(b.itstat[-1].ObjFun - 0.012009) < 1e-5
    assert np.abs(b.itstat[-1].DFid - 1.9636082e-06) < 1e-5
    assert np.abs(b.itstat[-1].RegL1 - 2.401446) < 1e-5
    assert np.linalg.norm(x1 - r['x0']) < 1e-3
    assert len(b.itstat) == int(r['iterations'])
    assert set(np.nonzero(np.abs(x1[:, 0]) > 1e-3)[0]) == set(np.nonzero(r['x0'][:, 0])[0])
    assert b.X is not None and rel_l2(b.X, b.Y) < 1e-2      # stopped by tolerance: X was stored


# ---- kernel edges against the NumPy statement ------------------------------------------------------------
def edge_problem(N, M, K, seed=5):
    rng = np.random.RandomState(seed + 7 * N + 13 * M + K)
    D = rng.randn(N, M)
    D /= np.sqrt(np.sum(D ** 2, axis=0, keepdims=True))
    S = rng.randn(N, K)
    return D, S, 0.1 * rng.randn(M, K), 0.05 * rng.randn(M, K)


def edge_check(cname, N, M, K, dtype, mu=0.0, nonneg=False, auxvar=True, lsc=False, iters=2):
    D, S, Y0, U0 = edge_problem(N, M, K)
    cls = getattr(bpdn, cname)
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0, 'Y0': Y0.astype(dtype), 'U0': U0.astype(dtype),
         'NonNegCoef': nonneg, 'AuxVarObj': auxvar, 'LinSolveCheck': lsc, 'AutoRho': {'Period': 2}, 'ReturnX': True}
    args = (D.astype(dtype), S.astype(dtype), 0.2) + (() if cname == 'BPDN' else (mu,))
    b = cls(*args, opt=cls.Options(o))
    # the results prefilled with NaN: an element the kernels do not write shows
    nan = np.full((M, K), np.nan, dtype=dtype)
    b._dev.upload(_lib.BPDN_X, nan)
    b._dev.upload(_lib.BPDN_DTS, nan)
    b.setdict(D.astype(dtype))
    X = b.solve()
    fo = {'MaxMainIter': iters, 'RelStopTol': 0.0, 'Y0': Y0, 'U0': U0, 'NonNegCoef': nonneg, 'AuxVarObj': auxvar,
          'LinSolveCheck': lsc, 'AutoRho.Period': 2}
    r = bn.run(cname, D, S, 0.2, mu, fo, dtype=np.float64)
    its = b.getitstat()
    tol = 1e-10 if dtype == np.float64 else 2e-4
    errs = {'X': rel_l2(X, r['X']), 'Y': rel_l2(b.Y, r['Y']), 'U': rel_l2(b.U, r['U']),
            'DTS': rel_l2(b.DTS, D.T.dot(S))}
    for f in bn.FIELDS[cname] + ALG:
        errs[f] = rel_l2(getattr(its, f), r[f])
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(b.Y)) and np.all(np.isfinite(b.U))
    assert max(errs.values()) <= tol, errs
    if lsc:
        assert max(its.XSlvRelRes) <= (1e-13 if dtype == np.float64 else 1e-5)
    return b


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('M', [1, 16, 31, 32, 33, 40, 132])
def test_edges_m(backend, M, dtype):
    edge_check('BPDN', 8, M, 5, dtype, lsc=True)
    edge_check('BPDNJoint', 8, M, 5, dtype, mu=0.05, auxvar=False)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('N', [1, 8, 33, 64])
def test_edges_n(backend, N, dtype):
    edge_check('ElasticNet', N, 16, 5, dtype, mu=0.3, lsc=True, auxvar=False)
    edge_check('BPDNJoint', N, 40, 5, dtype, mu=0.05, nonneg=True)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_edges_narrow_block(backend, dtype):
    """max(M, N) above 170: the 16-column block in float32 too, three blocks + 1."""
    assert bpdn.plan(8, 176, 5, dtype)['KB'] == 16 and bpdn.plan(172, 16, 5, dtype)['KB'] == 16
    assert bpdn.plan(8, 168, 5, np.float32)['KB'] == 32
    edge_check('BPDN', 8, 176, 3 * 16 + 1, dtype, lsc=True, nonneg=True)
    edge_check('BPDNJoint', 172, 16, 17, dtype, mu=0.05, auxvar=False, iters=1)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('kk', ['1', '5', 'KB-1', 'KB', 'KB+1', '3KB+1'])
def test_edges_k(backend, kk, dtype):
    KB = bpdn.plan(8, 16, 5, dtype)['KB']
    assert KB in (16, 32)
    K = {'1': 1, '5': 5, 'KB-1': KB - 1, 'KB': KB, 'KB+1': KB + 1, '3KB+1': 3 * KB + 1}[kk]
    edge_check('BPDN', 8, 16, K, dtype, nonneg=True)
    edge_check('BPDNJoint', 8, 16, K, dtype, mu=0.05, lsc=True)


def handle_iter(dtype, N, M, K, want_x, joint=False, lsc=False, seed=3):
    """One iteration through the handle, every output array prefilled with NaN where the handle lets it be set."""
    D, S, Y0, U0 = edge_problem(N, M, K, seed)
    h = _lib.BpdnHandle(N, M, K, dtype)
    try:
        nan = np.full((M, K), np.nan, dtype=dtype)
        h.upload(_lib.BPDN_S, S.astype(dtype))
        h.upload(_lib.BPDN_X, nan)
        h.upload(_lib.BPDN_DTS, nan)
        h.set_dict(D.astype(dtype))
        h.set_solve(bpdn.solve_matrix(D.astype(dtype), 0.8).astype(dtype))
        h.upload(_lib.BPDN_Y, Y0.astype(dtype))
        h.upload(_lib.BPDN_U, U0.astype(dtype))
        p = _lib.BpdnParams()
        p.rho, p.lmbda, p.mu, p.rlx, p.u_scale, p.wl1, p.c = 0.8, 0.2, 0.05, 1.8, 1.0, 1.0, 0.8
        p.geval_y, p.want_x, p.joint, p.lin_solve_check = 1, int(want_x), int(joint), int(lsc)
        sums = h.iter(p)
        return h.download(_lib.BPDN_Y), h.download(_lib.BPDN_U), h.download(_lib.BPDN_X), sums, h.download(_lib.BPDN_DTS)
    finally:
        h.close()


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_x_unrequested_same_bits_and_repeatable(backend, dtype):
    N, M = 8, 40
    K = 3 * bpdn.plan(N, M, 5, dtype)['KB'] + 1
    y1, u1, x1, s1, d1 = handle_iter(dtype, N, M, K, True)
    y0, u0, x0, s0, d0 = handle_iter(dtype, N, M, K, False)
    y2, u2, x2, s2, d2 = handle_iter(dtype, N, M, K, True)
    assert np.array_equal(y1, y0) and np.array_equal(u1, u0) and s1 == s0
    assert np.all(np.isnan(x0))                              # not requested: X is not written
    assert np.array_equal(y1, y2) and np.array_equal(u1, u2) and np.array_equal(x1, x2) and s1 == s2
    assert np.array_equal(d1, d2)
    assert np.all(np.isfinite(y1)) and np.all(np.isfinite(u1)) and np.all(np.isfinite(x1))
    j1 = handle_iter(dtype, N, M, K, True, joint=True, lsc=True)
    j2 = handle_iter(dtype, N, M, K, True, joint=True, lsc=True)
    for a, b in zip(j1, j2):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


@pytest.mark.gpu
def test_above_the_grid_cap(gpu_backend):
    """More column blocks than workgroups: a workgroup loops.  M = 16, 16 MB an array."""
    N, M = 8, 16
    pl = bpdn.plan(N, M, 5, np.float32)
    K = 262144
    assert (K + pl['KB'] - 1) // pl['KB'] > bpdn.plan(N, M, K, np.float32)['blocks']
    D, S, _, _ = edge_problem(N, M, K)
    o = {'Verbose': False, 'MaxMainIter': 2, 'RelStopTol': 0.0, 'ReturnX': True}
    b = bpdn.BPDN(D.astype(np.float32), S.astype(np.float32), 0.2, bpdn.BPDN.Options(o))
    X = b.solve()
    r = bn.run('BPDN', D, S, 0.2, 0.0, {'MaxMainIter': 2, 'RelStopTol': 0.0}, dtype=np.float64)
    assert rel_l2(X, r['X']) <= 2e-4 and rel_l2(b.Y, r['Y']) <= 2e-4 and rel_l2(b.U, r['U']) <= 2e-4
    assert rel_l2(b.getitstat().ObjFun, r['ObjFun']) <= 2e-4


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_largest_served(gpu_backend, dtype):
    edge_check('BPDN', 512, 512, 33, dtype, lsc=True)
    edge_check('BPDNJoint', 512, 512, 33, dtype, mu=0.05)


# ---- the matrix-instruction form against the plain form (GPU only) --------------------------------------------
_FORM_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(tests)r)
from sporco_amd.admm import bpdn
import test_bpdn as t
out = {}
KB = bpdn.plan(8, 16, 5, np.float32)['KB']
out['mfma'] = np.int64(bpdn.plan(8, 16, 5, np.float32)['mfma'])
for cname, mu in (('BPDN', 0.0), ('BPDNJoint', 0.05), ('ElasticNet', 0.3)):
    for M in (16, 40, 132, 176):
        for N in (8, 64):
            K = 3 * bpdn.plan(N, M, 5, np.float32)['KB'] + 1
            D, S, Y0, U0 = t.edge_problem(N, M, K)
            cls = getattr(bpdn, cname)
            o = {'Verbose': False, 'MaxMainIter': 5, 'RelStopTol': 0.0, 'ReturnX': True, 'AutoRho': {'Period': 2}}
            args = (D.astype(np.float32), S.astype(np.float32), 0.2) + (() if cname == 'BPDN' else (mu,))
            b = cls(*args, opt=cls.Options(o))
            b.solve()
            for v in 'XYU':
                out['%%s_%%d_%%d_%%s' %% (cname, M, N, v)] = getattr(b, v)
            out['%%s_%%d_%%d_obj' %% (cname, M, N)] = np.array(b.getitstat().ObjFun)
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_mfma_form_equals_plain_form(gpu_backend, tmp_path):
    """float32 with SPORCO_AMD_BPDN_PLAIN set and unset (the switch is read when a handle is made; one process
    each): X, Y and U after five iterations agree bit for bit, for the three classes; M = 176 is the 16-column block."""
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / 'forms.py'
    script.write_text(_FORM_SCRIPT % {'repo': repo, 'tests': os.path.join(repo, 'tests')})
    res = {}
    for tag in ('mfma', 'plain'):
        env = dict(os.environ)
        env.pop('SPORCO_AMD_BPDN_PLAIN', None)
        if tag == 'plain':
            env['SPORCO_AMD_BPDN_PLAIN'] = '1'
        path = str(tmp_path / (tag + '.npz'))
        subprocess.check_call([sys.executable, str(script), path], env=env, timeout=300)
        with np.load(path) as z:
            res[tag] = {k: z[k] for k in z.files}
    assert int(res['mfma']['mfma']) == 1 and int(res['plain']['mfma']) == 0
    keys = [k for k in res['mfma'] if k != 'mfma']
    assert len(keys) == 3 * 4 * 2 * 4
    diff = [k for k in keys if not np.array_equal(res['mfma'][k], res['plain'][k])]
    assert not diff, diff


# ---- contract and refusals ---------------------------------------------------------------------------------
def test_option_defaults_equal_the_reference():
    d = load_golden('bpdn_defaults')
    for cname in ('BPDN', 'BPDNJoint', 'ElasticNet'):
        cls = getattr(bpdn, cname)
        mine = {}
        for k, v in cls.Options.defaults.items():
            if isinstance(v, dict):
                for kk, vv in v.items():
                    mine['%s.%s' % (k, kk)] = repr(vv)
            else:
                mine[k] = repr(v)
        ref = dict(zip((str(k) for k in d[cname + '_keys']), (str(v) for v in d[cname + '_values'])))
        assert mine == ref, cname
        assert cls.IterationStats._fields == tuple(str(f) for f in d[cname + '_fields'])
    o = bpdn.BPDN.Options({'AuxVarObj': False})
    assert o['fEvalX'] is True and o['gEvalY'] is False
    o['AuxVarObj'] = True
    assert o['fEvalX'] is False and o['gEvalY'] is True


def test_iteration_stats_fields():
    alg = ('PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho', 'XSlvRelRes', 'Time')
    assert bpdn.BPDN.IterationStats._fields == ('Iter', 'ObjFun', 'DFid', 'RegL1') + alg
    assert bpdn.BPDNJoint.IterationStats._fields == ('Iter', 'ObjFun', 'DFid', 'RegL1', 'RegL21') + alg
    assert bpdn.ElasticNet.IterationStats._fields == ('Iter', 'ObjFun', 'DFid', 'RegL1', 'RegL2') + alg
    assert bpdn.BPDN.hdrtxt() == ('Itn', 'Fnc', 'DFid', u'Regℓ1', 'r', 's', u'ρ')
    assert bpdn.ElasticNet.hdrtxt() == ('Itn', 'Fnc', 'DFid', u'Regℓ1', u'Regℓ2', 'r', 's', u'ρ')
    assert bpdn.BPDNJoint.hdrtxt() == ('Itn', 'Fnc', 'DFid', u'Regℓ1', u'Regℓ2,1', 'r', 's', u'ρ')


def test_rules_and_attributes(backend):
    g = gold('default')
    D, S = g['D'].astype(np.float32), g['S'].astype(np.float32)
    Dc, Sc = D.copy(), S.copy()
    y0 = (0.1 * np.random.RandomState(1).randn(16, 5)).astype(np.float32)
    od = {'Verbose': False, 'MaxMainIter': 3, 'Y0': y0}
    odc = {'Verbose': False, 'MaxMainIter': 3, 'Y0': y0.copy()}
    opt = bpdn.BPDN.Options(od)
    b = bpdn.BPDN(D, S, opt=opt)
    lm = np.float32(0.1 * abs(D.T.dot(S)).max())
    assert b.lmbda == lm and b.lmbda.dtype == np.float32
    assert b.rho == np.float32(50.0 * lm + 1.0)
    assert abs(float(b.rho_xi) - (1.0 + 18.3 ** (np.log10(lm) + 1.0))) < 1e-6
    assert np.array_equal(b.U, ((lm / b.rho) * np.sign(y0)).astype(np.float32))     # uinit from a Y0 alone
    assert b.X is None
    out = b.solve()
    assert out.dtype == np.float32 and out.shape == (16, 5) and np.array_equal(out, b.Y)
    assert b.X.shape == (16, 5) and b.DTS.shape == (16, 5) and b.D.shape == (8, 16) and b.S.shape == (8, 5)
    assert rel_l2(b.DTS, D.T.dot(S)) < 1e-6
    assert b.wl1.shape == () and not hasattr(b, 'lu') and not hasattr(b, 'piv')
    assert b.timer.elapsed('solve') > 0.0 and len(b.getitstat().ObjFun) == 3
    assert bpdn.BPDN(D, S, 0.0).rho_xi == 1.0                      # the reference's lmbda == 0 branch
    # nothing the caller handed in was written to
    assert np.array_equal(D, Dc) and np.array_equal(S, Sc) and np.array_equal(y0, odc['Y0'])
    assert opt['MaxMainIter'] == 3 and opt['Y0'] is y0
    e = bpdn.ElasticNet(D.astype(np.float64), S, 0.1, 0.5, opt=bpdn.BPDN.Options({'DataType': np.float64}))
    assert e.dtype == np.float64 and e.mu == 0.5 and e.mu.dtype == np.float64
    # FastSolve: no statistics, the same iterates
    f = bpdn.BPDN(D, S, 0.1, bpdn.BPDN.Options({'Verbose': False, 'MaxMainIter': 4, 'FastSolve': True,
                                                'AutoRho': {'Enabled': False}}))
    n = bpdn.BPDN(D, S, 0.1, bpdn.BPDN.Options({'Verbose': False, 'MaxMainIter': 4, 'RelStopTol': 0.0,
                                                'AutoRho': {'Enabled': False}}))
    assert np.array_equal(f.solve(), n.solve()) and f.itstat == [] and np.array_equal(f.X, n.X)


def test_refusals(backend):
    D = np.random.RandomState(0).randn(8, 16)
    S = np.random.RandomState(1).randn(8, 5)
    with pytest.raises(TypeError):
        bpdn.BPDN(D.astype(np.complex128), S, 0.1)
    with pytest.raises(TypeError):
        bpdn.BPDN(D, S.astype(np.complex64), 0.1)
    with pytest.raises(TypeError):
        bpdn.BPDN(D.astype(np.float16), S.astype(np.float16), 0.1)
    with pytest.raises(TypeError):
        bpdn.ElasticNet(D, S.astype(np.int32), 0.1, 0.1)
    with pytest.raises(TypeError):
        bpdn.BPDN(D, S, 0.1, bpdn.BPDN.Options({'DataType': np.float16}))
    dS = DeviceArray.from_host(S)
    with pytest.raises(TypeError):
        bpdn.BPDN(D, dS, 0.1)
    with pytest.raises(TypeError):
        bpdn.BPDNJoint(dS, S, 0.1, 0.1)
    with pytest.raises(ValueError, match='512'):
        bpdn.BPDN(np.zeros((8, 513)), S, 0.1)
    with pytest.raises(ValueError, match='512'):
        bpdn.BPDN(np.zeros((513, 16)), np.zeros((513, 2)), 0.1)
    with pytest.raises(ValueError):
        bpdn.BPDN(D, S[:, 0], 0.1)
    with pytest.raises(ValueError):
        bpdn.BPDN(D, S.reshape(8, 5, 1), 0.1)
    with pytest.raises(ValueError):
        bpdn.BPDN(D, S[:7], 0.1)
    with pytest.raises(NotImplementedError):
        bpdn.BPDN(D, S, 0.1, reducer=object())
    b = bpdn.BPDN(D, S, 0.1)
    with pytest.raises(NotImplementedError):
        pickle.dumps(b)
    with pytest.raises(ValueError):
        b.setdict(D[:, :8])
    with pytest.raises(ValueError):
        bpdn.BPDN(D, S, 0.1, bpdn.BPDN.Options({'L1Weight': np.ones((3, 5))}))
    with pytest.raises(_lib.BackendError, match='512'):
        _lib.BpdnHandle(8, 513, 5, np.float32)
