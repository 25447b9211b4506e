"""sporco_amd.admm.bpdn.BPDNProjL1 against fixtures of the unmodified reference (tests/golden/bpdnprojl1_*_f64.npz,
tools/make_golden_bpdnprojl1.py) and against the NumPy statement of tests/_bpdnprojl1_numpy.py.

Tolerances, as in tests/test_bpdn.py.  float64: 1e-9 relative l2 on iterates, traces and the final rho.  float32 input
against the float64 fixture: 1e-4 on iterates and 1e-3 on traces, or four times what the NumPy statement run in
float32 shows against the same fixture, whichever is larger, per case: F32_MEASURED (test_f32_measured_figures repeats
the measurement on the CPU and asserts that the float32 statement changes rho at the fixture's iterations).  The margin
of four covers the summation order and the rounding of the solve matrix.

`Cnstr` under gEvalY is the distance of an already projected Y from its ball: rounding noise around zero in the
reference, so it is compared absolutely, within four times what the statement in the same precision shows against the
fixture (CNSTR_STATEMENT), and in float32 it stays below 1e-6 gamma.  Under `auxvar_off` it is the distance of X and
is compared like any other trace.  XSlvRelRes sits at rounding level and is bounded as in tests/test_bpdn.py.

`k1` has the shape of the reference's tests/admm/test_bpdn.py::TestSet01::test_14 but gamma = 2.5: with gamma = 1 the
single column settles on one non-zero entry after three iterations, the dual residual is exactly zero from then on,
AutoRho multiplies rho by 1000 every other iteration and the traces follow rounding noise, in float64 already.
"""

import os
import pickle

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _bpdnprojl1_numpy as pn

from sporco_amd import _lib
from sporco_amd.admm import bpdn
from sporco_amd.device import DeviceArray

CASES = ['default', 'auxvar_off', 'fixedrho', 'stdres', 'lsc', 'nonneg', 'inside', 'mixed', 'y0', 'y0u0', 'returnx',
         'square', 'tall', 'k1']
ALG = ('PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho')
F64_TOL = 1e-9
XRRS_STATEMENT_F64 = 1e-16
XRRS_STATEMENT_F32 = 2.8e-7
# Cnstr under gEvalY, absolute, the statement against the fixtures, worst case over the cases
CNSTR_STATEMENT_F64 = 9e-16
CNSTR_STATEMENT_F32 = 4.8e-7
# case: (iterates, traces and final rho) of the float32 statement against the float64 fixture
F32_MEASURED = {'default': (6.0e-5, 6.0e-5), 'auxvar_off': (6.0e-5, 6.0e-5), 'fixedrho': (2.9e-7, 1.9e-7),
                'stdres': (2.8e-4, 2.8e-4), 'lsc': (6.0e-5, 6.0e-5), 'nonneg': (7.1e-6, 7.2e-6),
                'inside': (1.8e-5, 3.3e-6), 'mixed': (4.9e-4, 4.9e-4), 'y0': (1.5e-5, 2.0e-5), 'y0u0': (4.7e-5, 4.8e-5),
                'returnx': (6.0e-5, 6.0e-5), 'square': (9.8e-6, 9.8e-6), 'tall': (8.4e-5, 8.5e-5),
                'k1': (5.3e-5, 3.8e-5), 'setdict': (7.0e-5, 7.0e-5)}

_GOLD = {}


def gold(case):
    if case not in _GOLD:
        _GOLD[case] = load_golden('bpdnprojl1_%s_f64' % case)
    return _GOLD[case]


def flat_opts(g, dtype):
    """The options a fixture records, as the flat dict of tests/_bpdnprojl1_numpy.py."""
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


def nested(flat, extra=None):
    o = {'Verbose': False}
    for k, v in flat.items():
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
    return o


def build(g, dtype, extra=None):
    opt = bpdn.BPDNProjL1.Options(nested(flat_opts(g, dtype), extra))
    return bpdn.BPDNProjL1(g['D'].astype(dtype), g['S'].astype(dtype), float(g['gamma']), opt)


def statement(g, dtype, **kw):
    o = flat_opts(g, dtype)
    o.pop('ReturnX', None)
    return pn.run(g['D'], g['S'], float(g['gamma']), o, dtype=dtype, **kw)


def cnstr_at_y(g):
    return bool(g.get('opt_AuxVarObj', 1.0))


def trace_fields(g):
    return ('ObjFun',) + (() if cnstr_at_y(g) else ('Cnstr',)) + ALG


def compare(res, g, traces_of):
    """(worst iterate error, worst trace error with the final rho, XSlvRelRes absolute error or None, Cnstr absolute
    error under gEvalY or None)."""
    ei = max(rel_l2(res['X'], g['X']), rel_l2(res['Y'], g['Y']), rel_l2(res['U'], g['U']))
    et = max(rel_l2(traces_of(f), g['it_' + f]) for f in trace_fields(g))
    et = max(et, abs(float(res['rho']) - float(g['rho_final'])) / float(g['rho_final']))
    ex = ec = None
    if 'it_XSlvRelRes' in g:
        ex = float(np.max(np.abs(np.asarray(traces_of('XSlvRelRes'), dtype=np.float64) - g['it_XSlvRelRes'])))
    if cnstr_at_y(g):
        ec = float(np.max(np.abs(np.asarray(traces_of('Cnstr'), dtype=np.float64) - g['it_Cnstr'])))
    return ei, et, ex, ec


def setdict_statement(g, dtype):
    """The two stages of the `setdict` fixture: a solve with D, then one with D2 from the state the first left."""
    o = flat_opts(g, dtype)
    r1 = pn.run(g['D'], g['S'], float(g['gamma']), o, dtype=dtype)
    r = pn.run(g['optarr_D2'], g['S'], float(g['gamma']), o, dtype=dtype, Y=r1['Y'], U=r1['U'], rho=r1['rho'],
               k0=int(g['opt_MaxMainIter']))
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
    worst, worst_x, worst_c = 0.0, 0.0, 0.0
    for case in CASES + ['setdict']:
        g = gold(case)
        if case == 'setdict':
            r = setdict_statement(g, np.float64)
            assert rel_l2(r['Y_first'], g['Y_first']) <= 1e-10
        else:
            r = statement(g, np.float64)
        ei, et, ex, ec = compare(r, g, lambda f: r[f])
        worst = max(worst, ei, et)
        worst_x = max(worst_x, ex or 0.0)
        worst_c = max(worst_c, ec or 0.0)
    print('statement in float64 against the fixtures: %.2e; XSlvRelRes %.2e; Cnstr at Y %.2e' % (worst, worst_x, worst_c))
    assert worst <= 1e-10
    assert worst_x <= XRRS_STATEMENT_F64 and worst_c <= CNSTR_STATEMENT_F64


def test_f32_measured_figures():
    """The figures of F32_MEASURED, measured again; every case follows the fixture's rho path in float32."""
    worst_x, worst_c = 0.0, 0.0
    for case in CASES + ['setdict']:
        g = gold(case)
        r = setdict_statement(g, np.float32) if case == 'setdict' else statement(g, np.float32)
        ei, et, ex, ec = compare(r, g, lambda f: r[f])
        print("'%s': (%.1e, %.1e)," % (case, ei, et))
        assert rho_changes(r['Rho']) == rho_changes(g['it_Rho']), case
        assert ei <= F32_MEASURED[case][0] and et <= F32_MEASURED[case][1], (case, ei, et)
        worst_x = max(worst_x, ex or 0.0)
        worst_c = max(worst_c, ec or 0.0)
    print('XSlvRelRes %.2e; Cnstr at Y %.2e' % (worst_x, worst_c))
    assert worst_x <= XRRS_STATEMENT_F32 and worst_c <= CNSTR_STATEMENT_F32


def test_fixtures_hold_their_conditions():
    for case in CASES + ['setdict']:
        g = gold(case)
        for f in ('ObjFun', 'Cnstr') + ALG:
            assert np.all(np.isfinite(g['it_' + f])) and len(g['it_' + f]) == int(g['opt_MaxMainIter']), (case, f)
        if bool(g.get('opt_AutoRho.Enabled', 1.0)):
            assert len(rho_changes(g['it_Rho'])) >= 1, case
        else:
            assert len(rho_changes(g['it_Rho'])) == 0
        assert np.all(np.sum(np.abs(g['Y']), axis=0) <= float(g['gamma']) * (1 + 1e-12)), case
    assert 'it_XSlvRelRes' in gold('lsc') and 'it_XSlvRelRes' not in gold('default')
    assert int(gold('nonneg')['negative_unclipped']) > 0 and not np.any(gold('nonneg')['Y'] < 0)
    g = gold('inside')
    assert np.all(g['it_Cnstr'] == 0.0) and np.all(np.sum(np.abs(g['Y']), axis=0) < 0.5 * float(g['gamma']))
    g = gold('mixed')
    gm, l1x, l1y = float(g['gamma']), np.sum(np.abs(g['X']), axis=0), np.sum(np.abs(g['Y']), axis=0)
    outside = l1x > gm * (1 + 1e-6)
    assert np.any(outside) and np.any(l1x < 0.99 * gm)
    assert np.all(np.abs(l1y[outside] - gm) <= 1e-12 * gm) and np.all(l1y[~outside] < gm)
    assert np.max(gold('auxvar_off')['it_Cnstr']) > 1e-3          # Cnstr at X: a trace like any other
    assert gold('square')['D'].shape == (8, 8) and gold('tall')['D'].shape == (24, 16) and gold('k1')['S'].shape == (8, 1)
    assert 'optarr_Y0' in gold('y0') and 'optarr_U0' not in gold('y0') and 'optarr_U0' in gold('y0u0')
    assert not np.array_equal(gold('returnx')['X'], gold('returnx')['Y'])
    s = gold('setdict')
    assert not np.array_equal(s['D'], s['optarr_D2']) and not np.array_equal(s['Y_first'], s['Y'])


# ---- the class against the fixtures of the unmodified reference ----------------------------------------------
FIELDS = ('Iter', 'ObjFun', 'Cnstr', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho', 'XSlvRelRes', 'Time')


def check_cnstr(ec, g, its, dtype):
    if ec is not None:
        assert ec <= 4.0 * (CNSTR_STATEMENT_F64 if dtype == np.float64 else CNSTR_STATEMENT_F32), ec
        if dtype == np.float32:
            assert max(its.Cnstr) <= 1e-6 * float(g['gamma'])


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('case', CASES)
def test_against_reference_fixture(backend, case, dtype):
    g = gold(case)
    b = build(g, dtype)
    out = b.solve()
    its = b.getitstat()
    res = {'X': b.X, 'Y': b.Y, 'U': b.U, 'rho': b.rho}
    ei, et, ex, ec = compare(res, g, lambda f: getattr(its, f))
    print('%s %s: iterates %.2e traces %.2e xrrs %s cnstr %s' % (case, np.dtype(dtype).name, ei, et, ex, ec))
    tol_i, tol_t = (F64_TOL, F64_TOL) if dtype == np.float64 else f32_tols(case)
    assert out.dtype == dtype and out.shape == g['Y'].shape and b.X.dtype == dtype and b.U.dtype == dtype
    assert np.array_equal(out, b.X if case == 'returnx' else b.Y)
    assert np.array_equal(b.getcoef(), b.Y)
    assert its._fields == FIELDS
    assert np.array_equal(its.Iter, np.arange(len(g['it_ObjFun'])))
    if ex is None:
        assert all(v is None for v in its.XSlvRelRes)
    else:
        assert ex <= 4.0 * (XRRS_STATEMENT_F64 if dtype == np.float64 else XRRS_STATEMENT_F32)
    check_cnstr(ec, g, its, dtype)
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
    b.solve()                                              # (restartable: the iteration count goes on)
    its = b.getitstat()
    res = {'X': b.X, 'Y': b.Y, 'U': b.U, 'rho': b.rho}
    ei, et, _, ec = compare(res, g, lambda f: getattr(its, f))
    print('setdict %s: %.2e %.2e' % (np.dtype(dtype).name, ei, et))
    tol_i, tol_t = (F64_TOL, F64_TOL) if dtype == np.float64 else f32_tols('setdict')
    check_cnstr(ec, g, its, dtype)
    assert rel_l2(first, g['Y_first']) <= tol_i
    assert ei <= tol_i and et <= tol_t


# ---- kernel edges of the mode against the float64 statement ----------------------------------------------------
def edge_problem(N, M, K, seed=5):
    rng = np.random.RandomState(seed + 7 * N + 13 * M + K)
    D = rng.randn(N, M)
    D /= np.sqrt(np.sum(D ** 2, axis=0, keepdims=True))
    S = rng.randn(N, K)
    return D, S, 0.1 * rng.randn(M, K), 0.05 * rng.randn(M, K)


def edge_check(N, M, K, dtype, nonneg=False, auxvar=True, lsc=False, iters=2, gamma=0.7):
    """Two iterations from a Y0 / U0 with ReturnX.  gamma = 0.7: about half the columns of X + U of these problems lie
    outside at M = 1 and all of them from M = 16 on; the statement in float64 is the reference."""
    D, S, Y0, U0 = edge_problem(N, M, K)
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0, 'Y0': Y0.astype(dtype), 'U0': U0.astype(dtype),
         'NonNegCoef': nonneg, 'AuxVarObj': auxvar, 'LinSolveCheck': lsc, 'AutoRho': {'Period': 2}, 'ReturnX': True}
    b = bpdn.BPDNProjL1(D.astype(dtype), S.astype(dtype), gamma, bpdn.BPDNProjL1.Options(o))
    nan = np.full((M, K), np.nan, dtype=dtype)
    b._dev.upload(_lib.BPDN_X, nan)
    b._dev.upload(_lib.BPDN_DTS, nan)
    b.setdict(D.astype(dtype))
    X = b.solve()
    fo = {'MaxMainIter': iters, 'RelStopTol': 0.0, 'Y0': Y0, 'U0': U0, 'NonNegCoef': nonneg, 'AuxVarObj': auxvar,
          'LinSolveCheck': lsc, 'AutoRho.Period': 2}
    r = pn.run(D, S, gamma, fo, dtype=np.float64)
    its = b.getitstat()
    tol = 1e-10 if dtype == np.float64 else 2e-4
    errs = {'X': rel_l2(X, r['X']), 'Y': rel_l2(b.Y, r['Y']), 'U': rel_l2(b.U, r['U'])}
    for f in ('ObjFun',) + ALG + (() if auxvar else ('Cnstr',)):
        errs[f] = rel_l2(getattr(its, f), r[f])
    assert np.all(np.isfinite(X)) and np.all(np.isfinite(b.Y)) and np.all(np.isfinite(b.U))
    assert max(errs.values()) <= tol, errs
    eps = np.finfo(dtype).eps
    assert np.all(np.sum(np.abs(b.Y.astype(np.float64)), axis=0) <= gamma * (1 + 8 * eps * M))
    if auxvar:       # Cnstr at a projected Y: rounding noise
        assert max(its.Cnstr) <= 1e-6 * gamma and np.all(r['Cnstr'] <= 1e-14)
    if lsc:
        assert max(its.XSlvRelRes) <= (1e-13 if dtype == np.float64 else 1e-5)
    return b


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('M', [1, 16, 31, 32, 33, 40, 132, 176])
def test_edges_m(backend, M, dtype):
    edge_check(8, M, 5, dtype, lsc=True)
    edge_check(8, M, 5, dtype, auxvar=False, nonneg=True)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('N', [1, 8, 33, 64])
def test_edges_n(backend, N, dtype):
    edge_check(N, 16, 5, dtype, lsc=True, auxvar=False)
    edge_check(N, 40, 5, dtype, nonneg=True)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('kk', ['1', '5', 'KB-1', 'KB', 'KB+1', '3KB+1'])
def test_edges_k(backend, kk, dtype):
    KB = bpdn.plan(8, 16, 5, dtype)['KB']
    assert KB in (16, 32)
    K = {'1': 1, '5': 5, 'KB-1': KB - 1, 'KB': KB, 'KB+1': KB + 1, '3KB+1': 3 * KB + 1}[kk]
    edge_check(8, 16, K, dtype, nonneg=True)
    edge_check(8, 16, K, dtype, auxvar=False, lsc=True)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_edges_narrow_block(backend, dtype):
    """M = 176: the 16-column block in float32 too, three blocks + 1."""
    edge_check(8, 176, 3 * 16 + 1, dtype, lsc=True, auxvar=False)


def test_plan_unchanged(backend):
    """The column blocks asserted in tests/test_bpdn.py::test_edges_narrow_block, and the LDS of a workgroup: two
    tiles and the 32 doubles of the reduction scratch, which also carry the thresholds of the projection mode."""
    for dtype in (np.float64, np.float32):
        assert bpdn.plan(8, 176, 5, dtype)['KB'] == 16 and bpdn.plan(172, 16, 5, dtype)['KB'] == 16
    assert bpdn.plan(8, 168, 5, np.float32)['KB'] == 32
    assert bpdn.plan(8, 168, 5, np.float32)['lds'] == 2 * 168 * 48 * 4 + 256
    assert bpdn.plan(8, 176, 5, np.float64)['lds'] == 2 * 176 * 16 * 8 + 256


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_largest_served(gpu_backend, dtype):
    edge_check(512, 512, 33, dtype, lsc=True)
    edge_check(512, 512, 33, dtype, auxvar=False, nonneg=True)


@pytest.mark.gpu
def test_above_the_grid_cap(gpu_backend):
    """More column blocks than workgroups: a workgroup loops.  M = 16, 16 MB an array."""
    N, M, K = 8, 16, 262144
    pl = bpdn.plan(N, M, K, np.float32)
    assert (K + pl['KB'] - 1) // pl['KB'] > pl['blocks']
    D, S, _, _ = edge_problem(N, M, K)
    o = {'Verbose': False, 'MaxMainIter': 2, 'RelStopTol': 0.0, 'ReturnX': True}
    b = bpdn.BPDNProjL1(D.astype(np.float32), S.astype(np.float32), 0.7, bpdn.BPDNProjL1.Options(o))
    X = b.solve()
    r = pn.run(D, S, 0.7, {'MaxMainIter': 2, 'RelStopTol': 0.0}, dtype=np.float64)
    assert rel_l2(X, r['X']) <= 2e-4 and rel_l2(b.Y, r['Y']) <= 2e-4 and rel_l2(b.U, r['U']) <= 2e-4
    assert rel_l2(b.getitstat().ObjFun, r['ObjFun']) <= 2e-4


# ---- repeatability and forms -------------------------------------------------------------------------------------
def handle_iter(dtype, N, M, K, want_x, geval_y=1, seed=3):
    """One iteration in projection mode through the handle, X and D^T S prefilled with NaN."""
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
        p.rho, p.lmbda, p.rlx, p.u_scale, p.wl1, p.c = 0.8, 0.7, 1.8, 1.0, 1.0, 0.8
        p.geval_y, p.feval_x, p.want_x, p.proj_l1 = geval_y, 1 - geval_y, int(want_x), 1
        sums = h.iter(p)
        return h.download(_lib.BPDN_Y), h.download(_lib.BPDN_U), h.download(_lib.BPDN_X), sums
    finally:
        h.close()


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_x_unrequested_same_bits_and_repeatable(backend, dtype):
    N, M = 8, 40
    K = 3 * bpdn.plan(N, M, 5, dtype)['KB'] + 1
    for gy in (1, 0):
        y1, u1, x1, s1 = handle_iter(dtype, N, M, K, True, gy)
        y0, u0, x0, s0 = handle_iter(dtype, N, M, K, False, gy)
        y2, u2, x2, s2 = handle_iter(dtype, N, M, K, True, gy)
        assert np.array_equal(y1, y0) and np.array_equal(u1, u0) and s1 == s0
        assert np.all(np.isnan(x0))                              # not requested: X is not written
        assert np.array_equal(y1, y2) and np.array_equal(u1, u2) and np.array_equal(x1, x2) and s1 == s2
        assert np.all(np.isfinite(y1)) and np.all(np.isfinite(u1)) and np.all(np.isfinite(x1))
        assert np.all(np.isfinite(s1[:_lib.OUT_L21])) and np.isfinite(s1[_lib.OUT_BPDN_CNSTR])
        if gy == 0:
            assert s1[_lib.OUT_BPDN_CNSTR] > 0.0
    with pytest.raises(_lib.BackendError):                       # the mode has no joint form
        h = _lib.BpdnHandle(8, 16, 5, dtype)
        try:
            p = _lib.BpdnParams()
            p.rho, p.c, p.proj_l1, p.joint = 1.0, 1.0, 1, 1
            h.iter(p)
        finally:
            h.close()


_FORM_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(tests)r)
from sporco_amd.admm import bpdn
import test_bpdnprojl1 as t
out = {}
out['mfma'] = np.int64(bpdn.plan(8, 16, 5, np.float32)['mfma'])
for M in (16, 40, 132, 176):
    for N in (8, 64):
        for aux in (True, False):
            K = 3 * bpdn.plan(N, M, 5, np.float32)['KB'] + 1
            D, S, Y0, U0 = t.edge_problem(N, M, K)
            o = {'Verbose': False, 'MaxMainIter': 5, 'RelStopTol': 0.0, 'ReturnX': True, 'AutoRho': {'Period': 2},
                 'AuxVarObj': aux}
            b = bpdn.BPDNProjL1(D.astype(np.float32), S.astype(np.float32), 0.7, bpdn.BPDNProjL1.Options(o))
            b.solve()
            for v in 'XYU':
                out['%%d_%%d_%%d_%%s' %% (M, N, aux, v)] = getattr(b, v)
            out['%%d_%%d_%%d_obj' %% (M, N, aux)] = np.array(b.getitstat().ObjFun)
            out['%%d_%%d_%%d_cns' %% (M, N, aux)] = np.array(b.getitstat().Cnstr)
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_mfma_form_equals_plain_form(gpu_backend, tmp_path):
    """float32 with SPORCO_AMD_BPDN_PLAIN set and unset (the switch is read when a handle is made; one fresh process
    each): X, Y, U, ObjFun and Cnstr after five iterations agree bit for bit; M = 176 is the 16-column block."""
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
    assert len(keys) == 4 * 2 * 2 * 5
    diff = [k for k in keys if not np.array_equal(res['mfma'][k], res['plain'][k])]
    assert not diff, diff


# ---- contract and refusals ---------------------------------------------------------------------------------
def test_option_defaults_equal_the_reference():
    d = load_golden('bpdnprojl1_defaults')
    mine = {}
    for k, v in bpdn.BPDNProjL1.Options.defaults.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                mine['%s.%s' % (k, kk)] = repr(vv)
        else:
            mine[k] = repr(v)
    assert mine == dict(zip((str(k) for k in d['keys']), (str(v) for v in d['values'])))
    assert bpdn.BPDNProjL1.IterationStats._fields == tuple(str(f) for f in d['fields']) == FIELDS
    assert bpdn.BPDNProjL1.hdrtxt() == tuple(str(f) for f in d['hdrtxt']) == ('Itn', 'Fnc', 'Cnstr', 'r', 's', u'ρ')
    assert bpdn.BPDNProjL1.Options()['AutoRho', 'RsdlTarget'] == 1.0
    assert bpdn.GenericBPDN.Options()['AutoRho', 'RsdlTarget'] is None
    o = bpdn.BPDNProjL1.Options({'AuxVarObj': False})
    assert o['fEvalX'] is True and o['gEvalY'] is False
    assert 'BPDNProjL1' in bpdn.__all__ and 'BPDNProjL1' in bpdn.__doc__


def test_rules_and_attributes(backend):
    g = gold('default')
    D, S = g['D'].astype(np.float32), g['S'].astype(np.float32)
    Dc, Sc = D.copy(), S.copy()
    y0 = (0.1 * np.random.RandomState(1).randn(16, 5)).astype(np.float32)
    seen = []
    b = bpdn.BPDNProjL1(D, S, 1.0, bpdn.BPDNProjL1.Options({'Verbose': False, 'MaxMainIter': 3, 'Y0': y0,
                                                            'Callback': lambda o: seen.append(o.X.copy()) and False}))
    assert b.gamma == np.float32(1.0) and b.gamma.dtype == np.float32
    assert b.rho == np.float32(1.0) and b.rho_xi == np.float32(1.0) and not hasattr(b, 'lmbda')
    assert np.array_equal(b.U, np.zeros((16, 5), np.float32))          # uinit: zero with a Y0 too
    assert np.array_equal(b.Y, y0) and b.X is None
    out = b.solve()
    assert out.dtype == np.float32 and out.shape == (16, 5) and np.array_equal(out, b.Y)
    assert len(seen) == 3 and np.array_equal(seen[-1], b.X)
    assert np.array_equal(D, Dc) and np.array_equal(S, Sc)
    v = b.getcoef_device()
    assert isinstance(v, DeviceArray) and v.shape == (16, 5) and np.array_equal(v.get(), b.Y)
    b.solve()                                                           # restartable; the view shows the new Y
    assert len(b.getitstat().ObjFun) == 6 and np.array_equal(v.get(), b.Y)
    # FastSolve: no statistics, the same iterates
    o = {'Verbose': False, 'MaxMainIter': 4, 'AutoRho': {'Enabled': False}}
    f = bpdn.BPDNProjL1(D, S, 1.0, bpdn.BPDNProjL1.Options(dict(o, FastSolve=True)))
    n = bpdn.BPDNProjL1(D, S, 1.0, bpdn.BPDNProjL1.Options(dict(o, RelStopTol=0.0)))
    assert np.array_equal(f.solve(), n.solve()) and f.itstat == [] and np.array_equal(f.X, n.X)
    # gamma = 0: Y is zero
    z = bpdn.BPDNProjL1(D, S, 0.0, bpdn.BPDNProjL1.Options({'Verbose': False, 'MaxMainIter': 2}))
    assert not np.any(z.solve())


def test_refusals(backend):
    D = np.random.RandomState(0).randn(8, 16)
    S = np.random.RandomState(1).randn(8, 5)
    P = bpdn.BPDNProjL1
    with pytest.raises(TypeError):
        P(D.astype(np.complex128), S, 1.0)
    with pytest.raises(TypeError):
        P(D, S.astype(np.complex64), 1.0)
    with pytest.raises(TypeError):
        P(D.astype(np.float16), S.astype(np.float16), 1.0)
    with pytest.raises(TypeError):
        P(D, S.astype(np.int32), 1.0)
    with pytest.raises(TypeError):                                    # the reference's float16 test_15
        P(D, S, 1.0, P.Options({'Verbose': False, 'MaxMainIter': 20, 'AutoRho': {'Enabled': True},
                                'DataType': np.float16}))
    dS = DeviceArray.from_host(S)
    with pytest.raises(TypeError):
        P(D, dS, 1.0)
    with pytest.raises(TypeError):
        P(dS, S, 1.0)
    with pytest.raises(ValueError, match='512'):
        P(np.zeros((8, 513)), S, 1.0)
    with pytest.raises(ValueError, match='512'):
        P(np.zeros((513, 16)), np.zeros((513, 2)), 1.0)
    with pytest.raises(ValueError):
        P(D, S[:, 0], 1.0)
    with pytest.raises(ValueError):
        P(D, S[:7], 1.0)
    with pytest.raises(ValueError, match='gamma'):
        P(D, S, -1.0)
    with pytest.raises(ValueError, match='gamma'):
        P(D, S, float('nan'))
    with pytest.raises(NotImplementedError):
        P(D, S, 1.0, reducer=object())
    b = P(D, S, 1.0)
    with pytest.raises(NotImplementedError):
        pickle.dumps(b)
    with pytest.raises(ValueError):
        b.setdict(D[:, :8])
