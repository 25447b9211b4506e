"""sporco_amd.admm.cmod CnstrMOD against fixtures of the unmodified reference (tests/golden/cmod_*_f64.npz,
tools/make_golden_cmod.py) and against the NumPy statement of tests/_cmod_numpy.py; the kernels of csrc/csc_cmod.h
at their edges.

Tolerances.  float64: the project's 1e-9 relative l2 on iterates, traces and the final rho.  Cnstr evaluated at Y
sits at rounding level and is compared absolutely: the float64 statement differs from the fixtures by at most
CNSTR_STATEMENT_F64, the bound is four times that; in float32 four times CNSTR_STATEMENT_F32.  float32 input against
the float64 fixture: 1e-4 on iterates and 1e-3 on traces, or four times what the NumPy statement run in float32
shows against the same fixture, whichever is larger, per case: F32_MEASURED below (test_f32_measured_figures repeats
the measurement on the CPU and asserts that the float32 statement changes rho at the fixture's iterations).  The
margin of four covers the summation order and the explicit inverse, where the statement solves with a factor.  In
float64 the statement reproduces every fixture to 1.4e-12 (`k1`; 7e-15 elsewhere); the widest float32 figure is
4.3e-5, so every float32 bound is the floor of 1e-4 / 1e-3 but `k1`'s on iterates (1.6e-4).
"""

import gc
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _cmod_numpy as cn

from sporco_amd import _lib
from sporco_amd.admm import bpdn, cmod
from sporco_amd.device import DeviceArray

CASES = ['default', 'auxvar_off', 'fixedrho', 'zeromean', 'y0', 'y0u0', 'returnx', 'k_lt_m', 'k1', 'z_none', 'zero_row']
F64_TOL = 1e-9
CNSTR_STATEMENT_F64 = 1.2e-15
CNSTR_STATEMENT_F32 = 8e-7
# case: (iterates, traces and final rho) of the float32 statement against the float64 fixture
F32_MEASURED = {'default': (7.2e-7, 4.0e-7), 'auxvar_off': (7.2e-7, 4.0e-7), 'fixedrho': (1.9e-6, 6.0e-7),
                'zeromean': (4.1e-7, 2.7e-7), 'y0': (6.6e-7, 4.8e-7), 'y0u0': (7.2e-7, 3.6e-7),
                'returnx': (7.2e-7, 4.0e-7), 'k_lt_m': (2.0e-6, 6.9e-7), 'k1': (3.9e-5, 4.3e-5),
                'z_none': (7.2e-7, 4.0e-7), 'zero_row': (7.5e-7, 5.2e-7), 'setcoef2': (2.4e-6, 7.6e-7)}
FIELDS = ('DFid',) + cn.ALG

_GOLD = {}


def gold(case):
    if case not in _GOLD:
        _GOLD[case] = load_golden('cmod_%s_f64' % case)
    return _GOLD[case]


def flat_opts(g, dtype):
    o = {}
    for k in g:
        if k.startswith('opt_'):
            v, name = float(g[k]), k[4:]
            if name in ('MaxMainIter', 'AutoRho.Period'):
                v = int(v)
            elif name in ('AuxVarObj', 'ZeroMean', 'ReturnX', 'AutoRho.Enabled'):
                v = bool(v)
            o[name] = v
        elif k in ('optarr_Y0', 'optarr_U0'):
            o[k[7:]] = g[k].astype(dtype)
    return o


def options_of(g, dtype, extra=None):
    o = {'Verbose': False}
    for k, v in flat_opts(g, dtype).items():
        if '.' in k:
            a, b = k.split('.')
            o.setdefault(a, {})[b] = v
        else:
            o[k] = v
    o.update(extra or {})
    return cmod.CnstrMOD.Options(o)


def statement(g, dtype, Z=None, **kw):
    o = flat_opts(g, dtype)
    o.pop('ReturnX', None)
    return cn.run(g['Z'] if Z is None else Z, g['S'], o, dtype=dtype, **kw)


def setcoef2_statement(g, dtype):
    r1 = statement(g, dtype)
    r = statement(g, dtype, Z=g['optarr_Z2'], Y=r1['Y'], U=r1['U'], rho=r1['rho'], k0=int(g['opt_MaxMainIter']))
    r['Y_first'] = r1['Y']
    return r


def compare(res, g, traces_of):
    """(worst iterate error, worst trace error with the final rho, Cnstr absolute error)."""
    ei = max(rel_l2(res['X'], g['X']), rel_l2(res['Y'], g['Y']), rel_l2(res['U'], g['U']))
    et = max(rel_l2(traces_of(f), g['it_' + f]) for f in FIELDS)
    et = max(et, abs(float(res['rho']) - float(g['rho_final'])) / float(g['rho_final']))
    ec = float(np.max(np.abs(np.asarray(traces_of('Cnstr'), dtype=np.float64) - g['it_Cnstr'])))
    return ei, et, ec


def f32_tols(case):
    mi, mt = F32_MEASURED[case]
    return max(4.0 * mi, 1e-4), max(4.0 * mt, 1e-3)


def rho_changes(rho):
    rho = np.asarray(rho, dtype=np.float64)
    return tuple(np.nonzero(rho[1:] != rho[:-1])[0])


def cnstr_tol(dtype):
    return 4.0 * (CNSTR_STATEMENT_F64 if dtype == np.float64 else CNSTR_STATEMENT_F32)


# ---- the statement and the fixtures (CPU only) ---------------------------------------------------------------
def test_statement_reproduces_fixtures():
    worst, worst_c = 0.0, 0.0
    for case in CASES + ['setcoef2']:
        g = gold(case)
        if case == 'setcoef2':
            r = setcoef2_statement(g, np.float64)
            assert rel_l2(r['Y_first'], g['Y_first']) <= 1e-10
        else:
            r = statement(g, np.float64)
        ei, et, ec = compare(r, g, lambda f: r[f])
        worst, worst_c = max(worst, ei, et), max(worst_c, ec)
    print('statement in float64 against the fixtures: %.2e; Cnstr %.2e' % (worst, worst_c))
    assert worst <= 1e-10
    assert worst_c <= CNSTR_STATEMENT_F64


def test_f32_measured_figures():
    """The figures of F32_MEASURED, measured again; every case follows the fixture's rho path in float32."""
    worst_c = 0.0
    for case in CASES + ['setcoef2']:
        g = gold(case)
        r = setcoef2_statement(g, np.float32) if case == 'setcoef2' else statement(g, np.float32)
        ei, et, ec = compare(r, g, lambda f: r[f])
        print("'%s': (%.1e, %.1e)," % (case, ei, et))
        assert rho_changes(r['Rho']) == rho_changes(g['it_Rho']), case
        assert ei <= F32_MEASURED[case][0] and et <= F32_MEASURED[case][1], (case, ei, et)
        worst_c = max(worst_c, ec)
    print('Cnstr %.2e' % worst_c)
    assert worst_c <= CNSTR_STATEMENT_F32


def test_fixtures_hold_their_conditions():
    for case in CASES + ['setcoef2']:
        g = gold(case)
        for f in FIELDS + ('Cnstr',):
            assert np.all(np.isfinite(g['it_' + f])) and len(g['it_' + f]) == int(g['opt_MaxMainIter']), (case, f)
        if bool(g.get('opt_AutoRho.Enabled', 1.0)):
            assert len(rho_changes(g['it_Rho'])) >= 1, case
        else:
            assert len(rho_changes(g['it_Rho'])) == 0
    assert gold('k_lt_m')['Z'].shape == (16, 5) and gold('k1')['Z'].shape == (16, 1)
    z = gold('zero_row')['Z']
    assert not np.any(z[3]) and np.all(np.any(z[np.arange(16) != 3], axis=1))
    assert float(gold('zeromean')['x_colmean_max']) > 1e-8
    assert np.max(np.abs(np.mean(gold('zeromean')['Y'], axis=0))) < 1e-14
    assert 'optarr_Y0' in gold('y0') and 'optarr_U0' not in gold('y0') and 'optarr_U0' in gold('y0u0')
    assert not np.array_equal(gold('returnx')['X'], gold('returnx')['Y'])
    for f in ('X', 'Y', 'U', 'it_DFid', 'it_Rho'):
        assert np.array_equal(gold('default')[f], gold('z_none')[f]), f
    assert float(gold('default')['rho0']) == 1.0      # the reference's default in effect, not K / 500


# ---- the class against the fixtures of the unmodified reference ----------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('case', CASES)
def test_against_reference_fixture(backend, case, dtype):
    g = gold(case)
    Z, S = g['Z'].astype(dtype), g['S'].astype(dtype)
    if case == 'z_none':
        b = cmod.CnstrMOD(None, S, (16, 40), options_of(g, dtype))
        b.setcoef(Z)
    else:
        b = cmod.CnstrMOD(Z, S, (16, Z.shape[1]), options_of(g, dtype))
    out = b.solve()
    its = b.getitstat()
    res = {'X': b.X, 'Y': b.Y, 'U': b.U, 'rho': b.rho}
    ei, et, ec = compare(res, g, lambda f: getattr(its, f))
    print('%s %s: iterates %.2e traces %.2e cnstr %.2e' % (case, np.dtype(dtype).name, ei, et, ec))
    tol_i, tol_t = (F64_TOL, F64_TOL) if dtype == np.float64 else f32_tols(case)
    assert out.dtype == dtype and out.shape == g['Y'].shape and b.X.dtype == dtype and b.U.dtype == dtype
    assert np.array_equal(out, b.X if case == 'returnx' else b.Y)
    assert np.array_equal(b.getdict(), b.Y)
    assert its._fields == ('Iter', 'DFid', 'Cnstr') + cn.ALG + ('Time',)
    assert np.array_equal(its.Iter, np.arange(len(g['it_DFid'])))
    assert ei <= tol_i and et <= tol_t, (ei, et)
    assert ec <= cnstr_tol(dtype), ec


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_second_setcoef_and_restart(backend, dtype):
    g = gold('setcoef2')
    n = int(g['opt_MaxMainIter'])
    b = cmod.CnstrMOD(g['Z'].astype(dtype), g['S'].astype(dtype), None, options_of(g, dtype, {'MaxMainIter': n // 2}))
    b.solve()
    assert b.k == n // 2
    b.solve()                                   # restartable: continues from self.k
    assert b.k == n and len(b.itstat) == n
    first = b.Y.copy()
    tol_i, tol_t = (F64_TOL, F64_TOL) if dtype == np.float64 else f32_tols('setcoef2')
    assert rel_l2(first, g['Y_first']) <= tol_i
    assert abs(float(b.rho) - float(g['rho_first'])) <= tol_t * float(g['rho_first'])
    b.itstat = []
    b.opt['MaxMainIter'] = n
    b.setcoef(g['optarr_Z2'].astype(dtype))
    assert np.array_equal(b.Y, first)           # Y and U are kept
    assert rel_l2(b.SZT, g['S'].dot(g['optarr_Z2'].T)) <= (1e-13 if dtype == np.float64 else 1e-6)
    b.solve()
    its = b.getitstat()
    ei, et, ec = compare({'X': b.X, 'Y': b.Y, 'U': b.U, 'rho': b.rho}, g, lambda f: getattr(its, f))
    print('setcoef2 %s: %.2e %.2e %.2e' % (np.dtype(dtype).name, ei, et, ec))
    assert ei <= tol_i and et <= tol_t and ec <= cnstr_tol(dtype)


# ---- kernel edges ----------------------------------------------------------------------------------------
GRAM_SHAPES = [(8, 16, 5), (33, 40, 1), (5, 176, 49), (24, 16, 33), (8, 16, 'slabs')]


def gram_problem(N, M, K, dtype):
    if K == 'slabs':
        K = 3 * cmod.plan(N, M, 1000, dtype)['slab'] + 1
        assert cmod.plan(N, M, K, dtype)['slabs'] == 4
    rng = np.random.RandomState(3 + 7 * N + 13 * M + K)
    return rng.randn(M, K).astype(dtype), rng.randn(N, K).astype(dtype), K


def run_gram(N, M, K, dtype, Z, S):
    h = _lib.CmodHandle(N, M, K, dtype)
    h.upload(_lib.CMOD_G, np.full((M, M), np.nan))
    h.upload(_lib.CMOD_SZTD, np.full((N, M), np.nan))
    h.upload(_lib.CMOD_SZT, np.full((N, M), np.nan, dtype=dtype))
    h.set_signal(S)
    h.set_coef(Z)
    res = h.download(_lib.CMOD_G), h.download(_lib.CMOD_SZTD), h.download(_lib.CMOD_SZT)
    h.close()
    return res


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('shape', GRAM_SHAPES)
def test_gram_edges(backend, shape, dtype):
    """cmod_gram + cmod_gram_reduce against the float64 product of the same inputs.  The partial sums are chains
    of K fused multiply-adds in the working precision, so the bound is K eps relative to || |Z| |Z|^T ||."""
    N, M, K = shape
    Z, S, K = gram_problem(N, M, K, dtype)
    G, SZTd, SZT = run_gram(N, M, K, dtype, Z, S)
    Z64, S64 = Z.astype(np.float64), S.astype(np.float64)
    eps = np.finfo(dtype).eps
    for got, a in ((G, Z64), (SZTd, S64), (SZT, S64)):
        ref = a.dot(Z64.T)
        assert got.shape == ref.shape and np.all(np.isfinite(got))
        bound = (K + 1) * eps * np.linalg.norm(np.abs(a).dot(np.abs(Z64.T)))
        assert np.linalg.norm(got - ref) <= bound, (np.linalg.norm(got - ref), bound)
    assert SZT.dtype == dtype and np.array_equal(SZT, SZTd.astype(dtype))
    assert np.array_equal(G, G.T)
    G2, SZTd2, SZT2 = run_gram(N, M, K, dtype, Z, S)      # two runs are bitwise equal
    assert np.array_equal(G, G2) and np.array_equal(SZTd, SZTd2) and np.array_equal(SZT, SZT2)


def iter_problem(N, M, dtype, zero_col):
    K = 37
    rng = np.random.RandomState(11 + N + 3 * M)
    Z = rng.randn(M, K)
    S = rng.randn(N, K)
    Y0 = cn.pcn(rng.randn(N, M), False)
    U0 = 0.05 * rng.randn(N, M)
    if zero_col:
        # column 2 of AX + U is exactly zero in the first iteration: Z's row 2 is zero, so S Z^T and the x step
        # leave X[:, 2] = Y[:, 2] - U[:, 2] = 0 with Y = U there (and, with RelaxParam 1, AX + U = X + U = 0 + U)
        Z[2] = 0.0
        Y0[:, 2] = 0.0
        U0[:, 2] = 0.0
    return Z.astype(dtype), S.astype(dtype), Y0.astype(dtype), U0.astype(dtype)


def run_iters(N, M, dtype, zm, zero_col, iters=2):
    Z, S, Y0, U0 = iter_problem(N, M, dtype, zero_col)
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0, 'Y0': Y0, 'U0': U0, 'ZeroMean': zm,
         'AutoRho': {'Period': 2}, 'rho': 3.0, 'RelaxParam': 1.0 if zero_col else 1.8}
    b = cmod.CnstrMOD(Z, S, None, cmod.CnstrMOD.Options(o))
    b.solve()
    fo = {'Y0': Y0, 'U0': U0, 'ZeroMean': zm, 'AutoRho.Period': 2, 'rho': 3.0, 'MaxMainIter': iters, 'RelStopTol': 0.0,
          'RelaxParam': 1.0 if zero_col else 1.8}
    return b, cn.run(Z, S, fo, dtype=np.float64), (b._dev.download(_lib.CMOD_G), b.SZT)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('zm', [False, True])
@pytest.mark.parametrize('M', [16, 40, 132])
@pytest.mark.parametrize('N', [5, 64])
def test_iter_edges(backend, N, M, zm, dtype):
    """Two iterations of cmod_rhs / cmod_iter / cmod_dfid against the float64 statement of the same (rounded)
    inputs; the bound is that of the fixture tests."""
    b, r, _ = run_iters(N, M, dtype, zm, False)
    its = b.getitstat()
    tol_i, tol_t = (F64_TOL, F64_TOL) if dtype == np.float64 else (1e-4, 1e-3)
    for v in 'XYU':
        assert rel_l2(getattr(b, v), r[v]) <= tol_i, v
    for f in FIELDS:
        assert rel_l2(getattr(its, f), r[f]) <= tol_t, f
    assert np.max(np.abs(np.array(its.Cnstr) - r['Cnstr'])) <= cnstr_tol(dtype)
    if zm:
        assert np.max(np.abs(np.mean(b.Y.astype(np.float64), axis=0))) <= 8 * np.finfo(dtype).eps


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('zm', [False, True])
@pytest.mark.parametrize('N, M', [(64, 16), (5, 40), (64, 132)])
def test_zero_column_is_divided_by_one(backend, N, M, zm, dtype):
    b, r, _ = run_iters(N, M, dtype, zm, True, iters=1)
    assert not np.any(r['Y'][:, 2]) and not np.any(b.Y[:, 2]) and np.all(np.isfinite(b.Y))
    assert not np.any(b.U[:, 2])
    others = np.arange(M) != 2
    assert rel_l2(b.Y[:, others], r['Y'][:, others]) <= (F64_TOL if dtype == np.float64 else 1e-4)


def test_two_runs_are_bitwise_equal(backend):
    a, _, (ga, sa) = run_iters(64, 132, np.float32, True, False, iters=3)
    b, _, (gb, sb) = run_iters(64, 132, np.float32, True, False, iters=3)
    for v in 'XYU':
        assert np.array_equal(getattr(a, v), getattr(b, v)), v
    assert np.array_equal(ga, gb) and np.array_equal(sa, sb)
    assert a.getitstat()[1:-1] == b.getitstat()[1:-1]


_FORM_SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_cmod as t
from sporco_amd.admm import cmod
out = {}
for i, (N, M, K) in enumerate(t.GRAM_SHAPES):
    Z, S, K = t.gram_problem(N, M, K, np.float32)
    out['plan%%d' %% i] = np.int64(cmod.plan(N, M, K)['mfma'])
    out['G%%d' %% i], out['Sd%%d' %% i], out['S%%d' %% i] = t.run_gram(N, M, K, np.float32, Z, S)
for i, (N, M) in enumerate([(5, 16), (64, 40), (64, 132)]):
    b, _, _ = t.run_iters(N, M, np.float32, True, False, iters=3)
    out['X%%d' %% i], out['Y%%d' %% i], out['U%%d' %% i] = b.X, b.Y, b.U
np.savez(sys.argv[1], **out)
'''


@pytest.mark.gpu
def test_mfma_form_equals_plain_form(tmp_path):
    """GPU only: the matrix-instruction form and the plain form (SPORCO_AMD_CMOD_PLAIN, read when a handle is made)
    give bit-identical G, S Z^T, X, Y, U at the edge shapes.  The counterpart of test_bpdn's test of the same name;
    each form runs in a process of its own."""
    here = os.path.dirname(os.path.abspath(__file__))
    res = []
    for plain in (False, True):
        env = dict(os.environ)
        env.pop('SPORCO_AMD_CMOD_PLAIN', None)
        if plain:
            env['SPORCO_AMD_CMOD_PLAIN'] = '1'
        path = str(tmp_path / ('plain.npz' if plain else 'mfma.npz'))
        subprocess.run([sys.executable, '-c', _FORM_SCRIPT % (here, os.path.dirname(here)), path], env=env, check=True,
                       timeout=120)
        res.append(np.load(path))
    assert int(res[0]['plan0']) == 1 and int(res[1]['plan0']) == 0
    for k in res[0].files:
        if not k.startswith('plan'):
            assert np.array_equal(res[0][k], res[1][k]), k


# ---- handover ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_setcoef_device_array_equals_host(backend, dtype):
    g = gold('default')
    Z, S = g['Z'].astype(dtype), g['S'].astype(dtype)
    o = {'Verbose': False, 'MaxMainIter': 5, 'RelStopTol': 0.0}
    a = cmod.CnstrMOD(Z, S, None, cmod.CnstrMOD.Options(o))
    zd, sd = DeviceArray.from_host(Z), DeviceArray.from_host(S)
    b = cmod.CnstrMOD(None, sd, (16, 40), cmod.CnstrMOD.Options(o))
    _lib.transfer_stats(reset=True)
    b.setcoef(zd)
    moved = _lib.transfer_stats(reset=True)
    assert moved['h2d_bytes'] < Z.nbytes and moved['d2h_bytes'] <= 16 * 16 * 8      # the (M, M) Gram matrix down, the solve matrix up
    a.solve()
    b.solve()
    for v in 'XYU':
        assert np.array_equal(getattr(a, v), getattr(b, v)), v
    assert a.getitstat()[1:-1] == b.getitstat()[1:-1]
    assert np.array_equal(zd.get(), Z)
    with pytest.raises(TypeError):
        b.setcoef(DeviceArray.from_host(Z.astype(np.float64 if dtype == np.float32 else np.float32)))
    with pytest.raises(ValueError):
        b.setcoef(DeviceArray.from_host(Z[:, :39]))


def test_view_keeps_its_handle_alive(backend):
    rng = np.random.RandomState(2)
    D, S = rng.randn(8, 16), rng.randn(8, 12)
    x = bpdn.BPDN(D, S, 0.1, bpdn.BPDN.Options({'Verbose': False, 'MaxMainIter': 3}))
    x.solve()
    y = x.Y.copy()
    view = x.getcoef_device()
    assert view.shape == (16, 12) and view.dtype == np.float64 and view._base is x._dev and not view._own
    del x
    gc.collect()
    assert view._base._h                        # not closed
    assert np.array_equal(view.get(), y)


# ---- contract and refusals -------------------------------------------------------------------------------------
def test_options_defaults_key_by_key():
    d = load_golden('cmod_defaults')
    got = {}

    def walk(prefix, node):
        for k, v in node.items():
            if isinstance(v, dict):
                walk(prefix + k + '.', v)
            else:
                got[prefix + k] = repr(v)
    walk('', dict(cmod.CnstrMOD.Options()))
    assert got == dict(zip(d['CnstrMOD_keys'].tolist(), d['CnstrMOD_values'].tolist()))
    assert cmod.CnstrMOD.IterationStats._fields == tuple(d['CnstrMOD_fields'].tolist())
    o = cmod.CnstrMOD.Options({'AuxVarObj': False})
    assert o['fEvalX'] is True and o['gEvalY'] is False
    o['AuxVarObj'] = True
    assert o['fEvalX'] is False and o['gEvalY'] is True


def test_contract(backend):
    g = gold('default')
    b = cmod.CnstrMOD(g['Z'], g['S'], None, cmod.CnstrMOD.Options({'Verbose': False, 'MaxMainIter': 2}))
    assert float(b.rho) == float(load_golden('cmod_defaults')['CnstrMOD_default_rho']) == 1.0
    assert b.X is None and not np.any(b.Y) and not np.any(b.U)
    b.solve()
    assert b.timer.elapsed('solve') > 0.0 and b.getitstat().Iter == [0, 1]
    y0 = gold('y0')['optarr_Y0']
    c = cmod.CnstrMOD(g['Z'], g['S'], None, cmod.CnstrMOD.Options({'Y0': y0}))
    assert np.array_equal(c.Y, y0) and np.array_equal(c.U, y0)      # uinit: a Y0 alone gives U = Y
    with pytest.raises(NotImplementedError):
        c.X = y0
    z = np.array([[1.0, -1.0], [0.0, 0.0]]).T
    assert np.array_equal(cmod.normalise(z)[:, 1], [0.0, 0.0])
    assert np.allclose(cmod.getPcn(True)(np.array([[1.0], [3.0]])), [[-np.sqrt(0.5)], [np.sqrt(0.5)]])
    assert cmod.getPcn(False) is cmod.normalise


def test_refusals(backend):
    g = gold('default')
    Z, S = g['Z'], g['S']
    C = cmod.CnstrMOD
    with pytest.raises(TypeError):
        C(Z.astype(np.complex128), S)
    with pytest.raises(TypeError):
        C(Z, S.astype(np.complex64))
    with pytest.raises(TypeError):
        C(Z.astype(np.int64), S)
    with pytest.raises(TypeError):
        C(Z.astype(np.float16), S.astype(np.float16))
    with pytest.raises(ValueError):
        C(Z[:, :39], S)
    with pytest.raises(ValueError):
        C(Z[0], S)
    with pytest.raises(ValueError):
        C(Z, S[:, :0])
    with pytest.raises(ValueError):
        C(None, S)
    with pytest.raises(ValueError):
        C(np.zeros((513, 40)), S)
    with pytest.raises(ValueError):
        C(np.zeros((16, 3)), np.zeros((513, 3)))
    with pytest.raises(NotImplementedError):
        C(Z, S, reducer=object())
    b = C(Z, S)
    with pytest.raises(NotImplementedError):
        pickle.dumps(b)
    with pytest.raises(ValueError):
        C(None, S, (16, 40)).solve()            # no coefficients yet


# ---- the bodies of the reference's tests/admm/test_cmod.py::test_06 and test_07 ----------------------------
def test_reference_test_06():
    opt = cmod.CnstrMOD.Options({'AuxVarObj': False})
    assert opt['fEvalX'] is True and opt['gEvalY'] is False
    opt['AuxVarObj'] = True
    assert opt['fEvalX'] is False and opt['gEvalY'] is True


def test_reference_test_07():
    opt = cmod.CnstrMOD.Options({'AuxVarObj': True})
    assert opt['fEvalX'] is False and opt['gEvalY'] is True
    opt['AuxVarObj'] = False
    assert opt['fEvalX'] is True and opt['gEvalY'] is False


# ---- solves at the reference's own test shape, both DataType settings it serves ------------------------------
def test_solve_at_reference_shape_and_datatype(backend):
    N, M, K = 16, 4, 8
    np.random.seed(12345)
    X = np.random.randn(M, K)
    S = np.random.randn(N, K)
    for dt in (np.float32, np.float64):
        opt = cmod.CnstrMOD.Options({'Verbose': False, 'MaxMainIter': 20, 'AutoRho': {'Enabled': True},
                                     'DataType': dt})
        b = cmod.CnstrMOD(X, S, opt=opt)
        b.solve()
        assert b.X.dtype == dt and b.Y.dtype == dt and b.U.dtype == dt
        assert b.Y.shape == (N, M) and len(b.itstat) == 20
        assert np.allclose(np.sum(b.Y.astype(np.float64) ** 2, 0), 1.0, atol=1e-5)
