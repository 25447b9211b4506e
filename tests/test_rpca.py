"""sporco_amd.admm.rpca RobustPCA and sporco_amd.prox prox_nuclear / norm_nuclear against fixtures of the unmodified
reference (tests/golden/rpca_*_f64.npz, tools/make_golden_rpca.py), against the NumPy statement of
tests/_rpca_numpy.py and against numpy.linalg.svd; the kernels of csrc/csc_rpca.h at their edges.

Tolerances.  float64: the project's 1e-9 relative l2 on iterates, traces and the final rho.  Cnstr and PrimalRsdl
shrink as a run converges, so they are compared element by element, relatively at 1e-9 with an
absolute floor of four times what the float64 Gram statement shows against the fixture (RSDL_STATEMENT_F64;
float32: RSDL_STATEMENT_F32).  float32 input against the float64 fixture: 1e-4 on iterates and 1e-3 on traces, or four
times what the float32 Gram statement measures against the same fixture, whichever is larger, per case: F32_MEASURED
below (test_f32_measured_figures repeats the measurement on the CPU and asserts that the float32 statement changes
rho at the fixture's iterations).  The margin of four covers the summation order and the matrix-instruction product.
In float64 the SVD statement reproduces every fixture to STATEMENT_SVD_F64 and the Gram statement to
STATEMENT_GRAM_F64 (test_statement_reproduces_fixtures prints both).
"""

import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _rpca_numpy as rn

from sporco_amd import _lib, prox
from sporco_amd.admm import rpca
from sporco_amd.device import DeviceArray

CASES = ['ref01', 'tall', 'wide', 'odd', 'vec', 'row', 'fixedrho', 'norelax', 'fevalx_off', 'gevaly_off', 'y0',
         'y0u0', 'lmbda']
F64_TOL = 1e-9
# the worst figures test_statement_reproduces_fixtures prints, rounded up
STATEMENT_SVD_F64 = 1e-10
STATEMENT_GRAM_F64 = 1e-9
# Cnstr / PrimalRsdl, absolute: the Gram statement against the fixtures
RSDL_STATEMENT_F64 = 4e-13
RSDL_STATEMENT_F32 = 2.1e-5
# case: (iterates, traces and final rho) of the float32 Gram statement against the float64 fixture
F32_MEASURED = {'ref01': (1.1e-5, 3.8e-6), 'tall': (2.8e-6, 2.6e-6), 'wide': (8.3e-6, 8.3e-6), 'odd': (9.3e-6, 9.4e-6),
                'vec': (4.6e-6, 5.6e-6), 'row': (7.0e-6, 7.0e-6), 'fixedrho': (8.3e-6, 5.3e-7),
                'norelax': (5.5e-6, 5.4e-6), 'fevalx_off': (4.1e-5, 4.1e-5), 'gevaly_off': (3.4e-5, 3.4e-5),
                'y0': (6.8e-6, 6.8e-6), 'y0u0': (3.8e-6, 4.8e-6), 'lmbda': (4.9e-6, 4.9e-6)}
FIELDS = ('ObjFun', 'NrmNuc', 'NrmL1', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho')
FLOORED = ('Cnstr', 'PrimalRsdl')

_GOLD = {}


def gold(case):
    if case not in _GOLD:
        _GOLD[case] = load_golden('rpca_%s_f64' % case)
    return _GOLD[case]


def flat_opts(g, dtype):
    o = {}
    for k in g:
        if k.startswith('opt_'):
            v, name = float(g[k]), k[4:]
            if name in ('MaxMainIter', 'AutoRho.Period'):
                v = int(v)
            elif name in ('fEvalX', 'gEvalY', 'AutoRho.Enabled'):
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
    return rpca.RobustPCA.Options(o)


def lmbda_of(g):
    return None if float(g['lmbda_given']) == 0.0 else float(g['lmbda_given'])


def statement(g, dtype, form):
    return rn.run(g['S'], lmbda_of(g), flat_opts(g, dtype), dtype=dtype, form=form)


def compare(res, g, traces_of):
    """(worst iterate error, worst trace error with the final rho, worst absolute error of Cnstr / PrimalRsdl,
    worst of |a - b| - 1e-9 |b| over Cnstr / PrimalRsdl)."""
    ei = max(rel_l2(res['X'], g['X']), rel_l2(res['Y'], g['Y']), rel_l2(res['U'], g['U']))
    for f in FIELDS + FLOORED:
        assert len(traces_of(f)) == len(g['it_' + f]), f
    et = max(rel_l2(traces_of(f), g['it_' + f]) for f in FIELDS)
    et = max(et, abs(float(res['rho']) - float(g['rho_final'])) / float(g['rho_final']))
    ea, ex = 0.0, 0.0
    for f in FLOORED:
        a, b = np.asarray(traces_of(f), dtype=np.float64), g['it_' + f]
        ea = max(ea, float(np.max(np.abs(a - b))))
        ex = max(ex, float(np.max(np.abs(a - b) - F64_TOL * np.abs(b))))
    return ei, et, ea, ex


def f32_tols(case):
    mi, mt = F32_MEASURED[case]
    return max(4.0 * mi, 1e-4), max(4.0 * mt, 1e-3)


def rho_changes(rho):
    rho = np.asarray(rho, dtype=np.float64)
    return tuple(np.nonzero(rho[1:] != rho[:-1])[0])


def rsdl_floor(dtype):
    return 4.0 * (RSDL_STATEMENT_F64 if dtype == np.float64 else RSDL_STATEMENT_F32)


# ---- the statement and the fixtures (CPU only) ---------------------------------------------------------------
def test_statement_reproduces_fixtures():
    worst = {'svd': 0.0, 'gram': 0.0}
    worst_a = 0.0
    for case in CASES:
        g = gold(case)
        for form in ('svd', 'gram'):
            r = statement(g, np.float64, form)
            ei, et, ea, _ = compare(r, g, lambda f: r[f])
            worst[form] = max(worst[form], ei, et, rel_l2(r['ss'], g['ss']))
            if form == 'gram':
                worst_a = max(worst_a, ea)
    print('statement in float64 against the fixtures: svd %.2e, gram %.2e; Cnstr / PrimalRsdl (gram) %.2e'
          % (worst['svd'], worst['gram'], worst_a))
    assert worst['svd'] <= STATEMENT_SVD_F64
    assert worst['gram'] <= STATEMENT_GRAM_F64
    assert worst_a <= RSDL_STATEMENT_F64


def test_f32_measured_figures():
    """The figures of F32_MEASURED, measured again; every case follows the fixture's rho path in float32."""
    worst_a = 0.0
    for case in CASES:
        g = gold(case)
        r = statement(g, np.float32, 'gram')
        ei, et, ea, _ = compare(r, g, lambda f: r[f])
        print("'%s': (%.1e, %.1e)," % (case, ei, et))
        assert rho_changes(r['Rho']) == rho_changes(g['it_Rho']), case
        assert ei <= F32_MEASURED[case][0] and et <= F32_MEASURED[case][1], (case, ei, et)
        worst_a = max(worst_a, ea)
    print('Cnstr / PrimalRsdl %.2e' % worst_a)
    assert worst_a <= RSDL_STATEMENT_F32


def test_fixtures_hold_their_conditions():
    shapes = {'ref01': (64, 64), 'tall': (300, 24), 'wide': (24, 300), 'odd': (33, 17), 'vec': (40, 1), 'row': (1, 40)}
    for case in CASES:
        g = gold(case)
        assert g['S'].shape == shapes.get(case, (33, 17)), case
        for f in FIELDS + FLOORED:
            assert np.all(np.isfinite(g['it_' + f])), (case, f)
        if case != 'ref01':
            assert len(g['it_Rho']) == int(g['opt_MaxMainIter']), case
        if bool(g.get('opt_AutoRho.Enabled', 1.0)):
            assert len(rho_changes(g['it_Rho'])) >= 1, case
        else:
            assert len(rho_changes(g['it_Rho'])) == 0
        assert g['ss'].shape == (min(g['S'].shape),)
    assert 'optarr_Y0' in gold('y0') and 'optarr_U0' not in gold('y0') and 'optarr_U0' in gold('y0u0')
    assert float(gold('norelax')['opt_RelaxParam']) == 1.0 and float(gold('lmbda')['lmbda_given']) == 0.3
    assert not bool(gold('fevalx_off')['opt_fEvalX']) and not bool(gold('gevaly_off')['opt_gEvalY'])
    assert int(gold('ref01')['opt_MaxMainIter']) == 250 and not bool(gold('ref01')['opt_gEvalY'])


# ---- the class against the fixtures of the unmodified reference ----------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('case', CASES)
def test_against_reference_fixture(backend, case, dtype):
    g = gold(case)
    b = rpca.RobustPCA(g['S'].astype(dtype), lmbda_of(g), options_of(g, dtype))
    X, Y = b.solve()
    its = b.getitstat()
    res = {'X': b.X, 'Y': b.Y, 'U': b.U, 'rho': b.rho}
    ei, et, ea, ex = compare(res, g, lambda f: getattr(its, f))
    print('%s %s: iterates %.2e traces %.2e Cnstr / PrimalRsdl abs %.2e' % (case, np.dtype(dtype).name, ei, et, ea))
    tol_i, tol_t = (F64_TOL, F64_TOL) if dtype == np.float64 else f32_tols(case)
    assert X.dtype == dtype and Y.dtype == dtype and b.U.dtype == dtype and X.shape == g['X'].shape
    assert np.array_equal(X, b.X) and np.array_equal(Y, b.Y)
    assert its._fields == ('Iter',) + rn.FIELDS + rn.ALG + ('Time',)
    assert np.array_equal(its.Iter, np.arange(len(g['it_Rho'])))
    assert b.ss.shape == g['ss'].shape and np.all(np.diff(b.ss) <= 0.0)
    assert ei <= tol_i and et <= tol_t, (ei, et)
    assert np.linalg.norm(b.ss - g['ss']) <= tol_i * max(np.linalg.norm(g['ss']), float(g['it_Rho'][-1]) ** -1)
    if dtype == np.float64:
        assert ex <= rsdl_floor(dtype), ex
    else:
        for f in FLOORED:
            a, r = np.asarray(getattr(its, f), dtype=np.float64), g['it_' + f]
            assert np.all(np.abs(a - r) <= tol_t * np.abs(r) + rsdl_floor(dtype)), f


def test_reference_test_01(backend):
    """The assertions of the reference's tests/admm/test_rpca.py::test_01, its problem by its seed and draws."""
    np.random.seed(12345)
    N, K, L = 64, 5, 10
    u = np.random.randn(N, K)
    U = np.dot(u, u.T)
    V = np.random.randn(N, N)
    t = np.sort(np.abs(V).ravel())[V.size - L]
    V[np.abs(V) < t] = 0
    D = U + V
    assert np.array_equal(D, gold('ref01')['S'])
    opt = rpca.RobustPCA.Options({'Verbose': False, 'gEvalY': False, 'MaxMainIter': 250, 'AutoRho': {'Enabled': True}})
    b = rpca.RobustPCA(D, None, opt)
    X, Y = b.solve()
    assert np.abs(b.itstat[-1].ObjFun - 321.493968419) < 1e-6
    assert np.mean(np.abs(U - X) ** 2) < 5e-6
    assert np.mean(np.abs(V - Y) ** 2) < 1e-8


# ---- kernel edges ----------------------------------------------------------------------------------------
# (R, C): the long side below one staged step of 32, not a multiple of it, a multiple; n = 1, 4, 17, 64; both layouts
GRAM_SHAPES = [(5, 1), (1, 5), (45, 4), (4, 45), (100, 17), (17, 100), (96, 64), (64, 97)]
GRAM_SHAPES_GPU = [(600, 512), (512, 600), (40000, 8), (8, 40000)]


def edge_problem(R, C, dtype):
    rng = np.random.RandomState(5 + 3 * R + 11 * C)
    return [rng.randn(R, C).astype(dtype) for _ in range(3)]


def v_of(mode, S, Y, U, us):
    if mode == _lib.RPCA_V_S:
        return S
    if mode == _lib.RPCA_V_SY:
        return S - Y
    return S - Y - S.dtype.type(us) * U


def run_gram(R, C, dtype, mode, us=1.0):
    S, Y, U = edge_problem(R, C, dtype)
    h = _lib.RpcaHandle(R, C, dtype)
    h.set_signal(S)
    h.upload(_lib.RPCA_Y, Y)
    h.upload(_lib.RPCA_U, U)
    G = h.gram(mode, us)
    plan = h.plan()
    h.close()
    return G, plan, v_of(mode, S, Y, U, us)


def check_gram(R, C, dtype):
    for mode, us in ((_lib.RPCA_V_SYU, 1.0), (_lib.RPCA_V_SYU, 0.75), (_lib.RPCA_V_SY, 1.0), (_lib.RPCA_V_S, 1.0)):
        G, plan, V = run_gram(R, C, dtype, mode, us)
        ref = rn.gram(V)
        assert G.shape == ref.shape and G.dtype == np.float64 and np.all(np.isfinite(G))
        assert np.linalg.norm(G - ref) <= 1e-13 * np.linalg.norm(ref), (mode, np.linalg.norm(G - ref) / np.linalg.norm(ref))
        G2, _, _ = run_gram(R, C, dtype, mode, us)      # two runs are bitwise equal
        assert np.array_equal(G, G2)
    return plan


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('shape', GRAM_SHAPES)
def test_gram_edges(backend, shape, dtype):
    """rpca_gram + rpca_gram_reduce in its three modes against the float64 product of the same V: the sums are
    double, so 1e-13 relative."""
    plan = check_gram(shape[0], shape[1], dtype)
    assert plan['KS'] == 32 and plan['slabs'] >= 1


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('shape', GRAM_SHAPES_GPU)
def test_gram_edges_large(gpu_backend, shape, dtype):
    """GPU only: n = 512 (64 blocks of 64 x 64) and a long side that is cut into slabs."""
    plan = check_gram(shape[0], shape[1], dtype)
    assert plan['mfma_gram'] == 1
    if max(shape) == 40000:
        assert plan['slabs'] > 1 and plan['blocks'] == 1
    else:
        assert plan['blocks'] == 8 and plan['slabs'] > 1


def iter_reference(S, Y, U, T, lmbda, rho, rlx, us, dtype):
    """One rpca_iter in float64 NumPy from the (rounded) inputs: X, Y', U' and the seven sums."""
    S, Y, U = (a.astype(np.float64) for a in (S, Y, U))
    T = T.astype(dtype).astype(np.float64)
    U = us * U
    V = S - Y - U
    X = V.dot(T) if S.shape[0] >= S.shape[1] else T.dot(V)
    AX = rlx * X - (1 - rlx) * (Y - S)
    Yn = rn.soft(S - AX - U, float(dtype(lmbda) / dtype(rho)))
    Un = U + AX + Yn - S
    sums = {_lib.OUT_R2: np.sum((X + Yn - S) ** 2), _lib.OUT_S2: np.sum((Yn - Y) ** 2), _lib.OUT_AX2: np.sum(X ** 2),
            _lib.OUT_Y2: np.sum(Yn ** 2), _lib.OUT_U2: np.sum(Un ** 2), _lib.OUT_L1: np.sum(np.abs(Yn)),
            _lib.OUT_L21: np.sum(np.abs(S - X)), _lib.OUT_C2: np.sum(S ** 2)}
    return X, Yn, Un, sums


def run_iter(R, C, dtype, rlx=1.8, us=0.75):
    S, Y, U = edge_problem(R, C, dtype)
    Y *= dtype(0.3)
    U *= dtype(0.1)
    n = min(R, C)
    rng = np.random.RandomState(R + C)
    A = rng.randn(n, n)
    T = (A + A.T) / (2.0 * np.sqrt(n))
    p = _lib.RpcaParams()
    p.rho, p.lmbda, p.rlx, p.u_scale = 0.8, 0.25, rlx, us
    h = _lib.RpcaHandle(R, C, dtype)
    h.set_signal(S)
    h.upload(_lib.RPCA_Y, Y)
    h.upload(_lib.RPCA_U, U)
    out = h.iter(p, T)
    got = [h.download(v) for v in (_lib.RPCA_X, _lib.RPCA_Y, _lib.RPCA_U)]
    h.apply(T)
    xa = h.download(_lib.RPCA_X)
    assert np.array_equal(h.download(_lib.RPCA_Y), got[1]) and np.array_equal(h.download(_lib.RPCA_U), got[2])
    plan = h.plan()
    h.close()
    return got, out, xa, plan, (S, Y, U, T)


ITER_SHAPES = [(5, 1), (1, 5), (45, 4), (4, 45), (100, 17), (17, 100), (96, 64), (64, 97), (33, 33)]


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('shape', ITER_SHAPES)
def test_iter_edges(backend, shape, dtype):
    """One rpca_iter from arbitrary Y, U and a symmetric T against float64 NumPy of the same (rounded) inputs: the
    arrays at the project's bounds, the seven sums and ||S||^2 at 1e-12 (float64) / 1e-5 (float32); the stateless
    mode stores S T (T S) and leaves Y and U alone; two runs are bitwise equal."""
    R, C = shape
    dt = np.dtype(dtype).type
    got, out, xa, plan, (S, Y, U, T) = run_iter(R, C, dt)
    X, Yn, Un, sums = iter_reference(S, Y, U, T, 0.25, 0.8, 1.8, 0.75, dt)
    tol_a, tol_s = (F64_TOL, 1e-12) if dtype == np.float64 else (1e-4, 1e-5)
    for a, r in zip(got, (X, Yn, Un)):
        assert a.dtype == dtype and rel_l2(a, r) <= tol_a
    for slot, v in sums.items():
        assert abs(out[slot] - v) <= tol_s * abs(v), (slot, out[slot], v)
    S64, T64 = S.astype(np.float64), T.astype(dtype).astype(np.float64)
    assert rel_l2(xa, S64.dot(T64) if R >= C else T64.dot(S64)) <= tol_a
    assert plan['KB'] in (16, 32) and plan['workgroups'] == -(-max(R, C) // plan['KB'])
    got2, out2, xa2, _, _ = run_iter(R, C, dt)
    assert all(np.array_equal(a, b) for a, b in zip(got, got2)) and out == out2 and np.array_equal(xa, xa2)
    # RelaxParam 1: AX is X itself
    got1, _, _, _, _ = run_iter(R, C, dt, rlx=1.0, us=1.0)
    X1, Y1, U1, _ = iter_reference(S, Y, U, T, 0.25, 0.8, 1.0, 1.0, dt)
    for a, r in zip(got1, (X1, Y1, U1)):
        assert rel_l2(a, r) <= tol_a


_FORM_SCRIPT = r'''
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_rpca as t
from sporco_amd import _lib
out = {}
for i, (R, C) in enumerate(t.GRAM_SHAPES):
    for dt in (np.float32, np.float64):
        G, plan, _ = t.run_gram(R, C, dt, _lib.RPCA_V_SYU, 0.75)
        out['G%%d_%%s' %% (i, np.dtype(dt).name)] = G
        out['plan_gram'], out['plan_iter32'] = np.int64(plan['mfma_gram']), np.int64(plan['mfma_iter'])
for i, (R, C) in enumerate(t.ITER_SHAPES):
    got, sums, xa, plan, _ = t.run_iter(R, C, np.float32)
    out['X%%d' %% i], out['Y%%d' %% i], out['U%%d' %% i], out['A%%d' %% i] = got[0], got[1], got[2], xa
    out['plan_iter32'] = np.int64(plan['mfma_iter'])
np.savez(sys.argv[1], **out)
'''


@pytest.mark.gpu
def test_matrix_form_against_plain_form(tmp_path):
    """GPU only: the matrix-instruction forms and the plain forms (SPORCO_AMD_RPCA_PLAIN, read when a handle is
    made).  The float64 Gram matrices agree to 1e-13 relative (no bit equality is promised: csrc/csc_rpca.h); the
    float32 X, Y, U of rpca_iter and the stateless X are bit-identical.  Each form runs in a process of its own."""
    here = os.path.dirname(os.path.abspath(__file__))
    res = []
    for plain in (False, True):
        env = dict(os.environ)
        env.pop('SPORCO_AMD_RPCA_PLAIN', None)
        if plain:
            env['SPORCO_AMD_RPCA_PLAIN'] = '1'
        path = str(tmp_path / ('plain.npz' if plain else 'mfma.npz'))
        subprocess.run([sys.executable, '-c', _FORM_SCRIPT % (here, os.path.dirname(here)), path], env=env, check=True,
                       timeout=120)
        res.append(np.load(path))
    assert int(res[0]['plan_gram']) == 1 and int(res[1]['plan_gram']) == 0
    assert int(res[0]['plan_iter32']) == 1 and int(res[1]['plan_iter32']) == 0
    worst, same = 0.0, True
    for k in res[0].files:
        if k.startswith('plan'):
            continue
        if k.startswith('G'):
            d = np.linalg.norm(res[0][k] - res[1][k]) / np.linalg.norm(res[1][k])
            worst, same = max(worst, d), same and np.array_equal(res[0][k], res[1][k])
            assert d <= 1e-13, (k, d)
        else:
            assert np.array_equal(res[0][k], res[1][k]), k
    print('float64 matrix form against the plain form: worst relative difference %.2e, bitwise equal: %s' % (worst, same))


# ---- prox_nuclear / norm_nuclear against numpy.linalg.svd --------------------------------------------------------
def svt_reference(V, alpha):
    Us, s, Vs = np.linalg.svd(V.astype(np.float64), full_matrices=False)
    ss = np.maximum(0, s - alpha)
    return Us.dot(np.diag(ss)).dot(Vs), ss, s


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('device_in', [False, True])
@pytest.mark.parametrize('shape', [(50, 7), (7, 50), (33, 33)])
def test_prox_nuclear(backend, shape, device_in, dtype):
    rng = np.random.RandomState(shape[0] + 2 * shape[1])
    V = rng.randn(*shape).astype(dtype)
    tol = 1e-9 if dtype == np.float64 else 1e-5
    arg = DeviceArray.from_host(V) if device_in else V
    _, _, s = svt_reference(V, 0.0)
    smax = s[0]
    for alpha in (0.5 * smax, s[min(shape) // 2]):
        X, ss = prox.prox_nuclear(arg, alpha)
        ref, rss, _ = svt_reference(V, alpha)
        assert isinstance(X, DeviceArray) == device_in and X.dtype == dtype and tuple(X.shape) == shape
        Xh = X.get() if device_in else X
        assert np.linalg.norm(Xh - ref) <= tol * np.linalg.norm(V), alpha
        assert ss.shape == (min(shape),) and np.all(np.diff(ss) <= 0.0) and np.max(np.abs(ss - rss)) <= tol * smax
    X, ss = prox.prox_nuclear(arg, 1.01 * smax)
    Xh = X.get() if device_in else X
    assert not np.any(Xh) and not np.any(ss)
    X, ss = prox.prox_nuclear(arg, 0.0)
    Xh = X.get() if device_in else X
    assert rel_l2(Xh, V) <= tol and np.max(np.abs(ss - s)) <= tol * smax
    nn = prox.norm_nuclear(arg)
    assert isinstance(nn, float) and abs(nn - np.sum(s)) <= tol * smax * min(shape)
    if device_in:
        assert np.array_equal(arg.get(), V)


def test_prox_nuclear_refusals(backend):
    V = np.random.RandomState(0).randn(6, 4)
    for fn in (lambda a: prox.prox_nuclear(a, 0.1), prox.norm_nuclear):
        with pytest.raises(TypeError):
            fn(V.astype(np.complex128))
        with pytest.raises(TypeError):
            fn(V.astype(np.float16))
        with pytest.raises(TypeError):
            fn(V.astype(np.int32))
        with pytest.raises(ValueError):
            fn(V[0])
        with pytest.raises(ValueError):
            fn(V[:, :, None])
        with pytest.raises(ValueError):
            fn(np.zeros((513, 514)))
    with pytest.raises(ValueError):
        prox.prox_nuclear(V, -1.0)
    X, _ = prox.prox_nuclear(np.zeros((513, 4)), 0.1)      # only the short side is bounded
    assert X.shape == (513, 4) and not np.any(X)


# ---- behaviour ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_reference_test_04_05(backend, dtype):
    np.random.seed(12345)
    D = np.random.randn(8, 8)
    opt = rpca.RobustPCA.Options({'Verbose': False, 'MaxMainIter': 20, 'AutoRho': {'Enabled': True}, 'DataType': dtype})
    b = rpca.RobustPCA(D, opt=opt)
    b.solve()
    assert b.X.dtype == dtype and b.Y.dtype == dtype and b.U.dtype == dtype


def test_reference_test_02(backend):
    np.random.seed(12345)
    b = rpca.RobustPCA(np.random.randn(8, 8))
    X, Y = b.solve()
    assert b.k >= 1 and np.all(np.isfinite(X)) and np.all(np.isfinite(Y))
    assert float(b.lmbda) == 8 ** -0.5


def test_restart_equals_one_run(backend):
    g = gold('odd')
    S = g['S']
    a = rpca.RobustPCA(S, None, rpca.RobustPCA.Options({'Verbose': False, 'MaxMainIter': 24, 'RelStopTol': 0.0}))
    a.solve()
    b = rpca.RobustPCA(S, None, rpca.RobustPCA.Options({'Verbose': False, 'MaxMainIter': 12, 'RelStopTol': 0.0}))
    b.solve()
    assert b.k == 12
    b.solve()
    assert b.k == 24 and len(b.itstat) == 24
    for v in 'XYU':
        assert rel_l2(getattr(b, v), getattr(a, v)) <= 1e-12, v
    assert abs(float(a.rho) - float(b.rho)) <= 1e-12 * float(a.rho)
    assert rel_l2(b.getitstat().ObjFun, a.getitstat().ObjFun) <= 1e-12


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('case', ['odd', 'wide'])
def test_device_array_signal_equals_host(backend, case, dtype):
    S = gold(case)['S'].astype(dtype)
    o = {'Verbose': False, 'MaxMainIter': 6, 'RelStopTol': 0.0}
    a = rpca.RobustPCA(S, None, rpca.RobustPCA.Options(o))
    Xa, Ya = a.solve()
    sd = DeviceArray.from_host(S)
    b = rpca.RobustPCA(sd, None, rpca.RobustPCA.Options(o))
    Xb, Yb = b.solve()
    assert isinstance(Xb, DeviceArray) and isinstance(Yb, DeviceArray) and Xb.dtype == dtype and Xb.shape == S.shape
    assert np.array_equal(Xb.get(), Xa) and np.array_equal(Yb.get(), Ya) and np.array_equal(a.U, b.U)
    assert a.getitstat()[1:-1] == b.getitstat()[1:-1]
    assert np.array_equal(sd.get(), S)
    with pytest.raises(TypeError):
        rpca.RobustPCA(DeviceArray.from_host(S), None, rpca.RobustPCA.Options({'DataType': np.float16}))


def test_callback_stops_the_run(backend):
    seen = []

    def cb(obj):
        seen.append(obj.k)
        return obj.k == 3

    b = rpca.RobustPCA(gold('odd')['S'], None, rpca.RobustPCA.Options({'Verbose': False, 'MaxMainIter': 30,
                                                                        'RelStopTol': 0.0, 'Callback': cb}))
    b.solve()
    assert seen == [0, 1, 2, 3] and len(b.itstat) == 4


def test_contract(backend):
    g = gold('y0')
    S = g['S']
    b = rpca.RobustPCA(S)
    assert float(b.lmbda) == S.shape[0] ** -0.5 and float(b.rho) == 2.0 * float(b.lmbda) + 0.1
    assert b.X is None and not np.any(b.Y) and not np.any(b.U)
    o = rpca.RobustPCA.Options()
    assert o['fEvalX'] is True and o['gEvalY'] is True and o['RelaxParam'] == 1.8
    assert dict(o['AutoRho']) == {'Enabled': True, 'Period': 1, 'Scaling': 1000.0, 'RsdlRatio': 1.2, 'RsdlTarget': 1.0,
                                  'AutoScaling': True, 'StdResiduals': False}
    assert rpca.RobustPCA.IterationStats._fields == ('Iter',) + rn.FIELDS + rn.ALG + ('Time',)
    assert rpca.RobustPCA.hdrtxt()[1:5] == ('Fnc', 'NrmNuc', u'Nrmℓ1', 'Cnstr')
    c = rpca.RobustPCA(S, None, rpca.RobustPCA.Options({'Y0': g['optarr_Y0']}))
    assert np.array_equal(c.Y, g['optarr_Y0'])
    assert np.array_equal(c.U, (c.lmbda / c.rho) * np.sign(g['optarr_Y0']))      # uinit from a Y0 alone
    with pytest.raises(NotImplementedError):
        c.X = S
    assert c.cnst_A(S) is S and c.cnst_AT(S) is S and c.cnst_B(S) is S and c.cnst_c() is c.S
    b.opt['MaxMainIter'] = 2
    b.solve()
    assert b.timer.elapsed('solve') > 0.0 and b.getitstat().Iter == [0, 1]


def test_refusals(backend):
    S = gold('odd')['S']
    C = rpca.RobustPCA
    with pytest.raises(TypeError):
        C(S.astype(np.complex128))
    with pytest.raises(TypeError):
        C(S.astype(np.float16))
    with pytest.raises(TypeError):
        C(S.astype(np.int64))
    with pytest.raises(TypeError):          # the reference's test_03
        C(S, opt=C.Options({'Verbose': False, 'MaxMainIter': 20, 'AutoRho': {'Enabled': True}, 'DataType': np.float16}))
    with pytest.raises(ValueError):
        C(S[0])
    with pytest.raises(ValueError):
        C(S[:, :, None])
    with pytest.raises(ValueError):
        C(S[:, :0])
    with pytest.raises(ValueError):
        C(np.zeros((513, 513)))
    with pytest.raises(NotImplementedError):
        C(S, reducer=object())
    with pytest.raises(NotImplementedError):
        pickle.dumps(C(S))
    assert C(np.zeros((513, 2))).Y.shape == (513, 2)      # only the short side is bounded
