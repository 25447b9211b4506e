"""sporco_amd.pgm.bpdn BPDN / WeightedBPDN against fixtures of the unmodified reference
(tests/golden/pgm_bpdn_*_f64.npz, tools/make_golden_pgm_bpdn.py) and against the NumPy statement of
tests/_pgm_bpdn_numpy.py.

Tolerances.  float64: the project's 1e-9 relative l2 on X, Y, every trace and the final L.  float32 input against
the float64 fixture: 1e-4 on iterates and 1e-3 on traces, or four times what the NumPy statement run in float32 shows
against the same fixture, whichever is larger, per case: F32_MEASURED below (test_f32_measured_figures repeats the
measurement on the CPU); the margin of four covers the summation order.  IterBTrack is compared as integers.

Every backtracking, Barzilai-Borwein, Cauchy and Monotone fixture was checked when it was made to be followed by the
float32 statement on its discrete path (IterBTrack, the iterations at which Monotone reverts and at which the
Barzilai-Borwein rule falls back); test_f32_measured_figures asserts it again, for every case and iteration.

Edge shapes run against the statement in the same dtype: 1e-9 in float64; in float32 EDGE_F32 = 2e-4 on iterates and
traces after EDGE_ITERS = 4 iterations.  (Reasoning: an iterate is a sum of at most 512 products of O(1) numbers per
product routine call, three calls a step; a float32 dot product of n terms in a different order differs by about
sqrt(n) eps = 23 * 6e-8 = 1.4e-6 relative to the operand norms, amplified by || D^T D || / L <= about 8 per step
at the L the edge problems use: 4 steps * 3 products * 1.4e-6 * 8 = 1.3e-4.)
"""

import os
import pickle

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _pgm_bpdn_numpy as pn

from sporco_amd import _lib
from sporco_amd.pgm import bpdn
from sporco_amd.pgm.backtrack import BacktrackRobust, BacktrackStandard
from sporco_amd.pgm.momentum import MomentumGenLinear, MomentumLinear, MomentumNesterov
from sporco_amd.pgm.stepsize import StepSizePolicyBB, StepSizePolicyCauchy

CASES = ['default', 'l2', 'lmbda_none', 'nonneg', 'w_atom', 'w_signal', 'w_full', 'x0', 'k1', 'tall', 'square',
         'bt_standard', 'bt_robust', 'mom_nesterov', 'mom_linear', 'mom_genlinear', 'cauchy', 'bb', 'monotone',
         'monotone_l1', 'autostop', 'wt_scalar', 'wt_n', 'wt_n1', 'wt_1k', 'wt_nk', 'wt_nk_standard', 'wt_n1_robust']
F64_TOL = 1e-9
EDGE_ITERS = 4
EDGE_F32 = 2e-4
# case: (iterates, traces and final L) of the float32 statement against the float64 fixture
F32_MEASURED = {'default': (1.2e-06, 1.1e-06), 'l2': (5.9e-07, 6e-07), 'lmbda_none': (3.9e-07, 7.3e-07),
                'nonneg': (2.7e-07, 5.8e-07), 'w_atom': (1.2e-07, 2.4e-07), 'w_signal': (4.3e-07, 1.7e-07),
                'w_full': (4.5e-07, 5.8e-07), 'x0': (3.7e-07, 6.1e-07), 'k1': (1.7e-07, 1.4e-06),
                'tall': (1.5e-07, 2.5e-07), 'square': (2.2e-07, 2.1e-07), 'bt_standard': (1.8e-07, 2.8e-06),
                'bt_robust': (1.5e-07, 7.7e-07), 'mom_nesterov': (4.3e-07, 2.7e-07), 'mom_linear': (4.6e-07, 5.1e-07),
                'mom_genlinear': (5.5e-07, 7.2e-07), 'cauchy': (1.6e-07, 5.7e-07), 'bb': (1.4e-07, 1.1e-05),
                'monotone': (1.1e-06, 8.1e-07), 'monotone_l1': (2.9e-07, 1.7e-07), 'autostop': (7.7e-08, 3.6e-08),
                'wt_scalar': (5.5e-07, 8.2e-07), 'wt_n': (6.3e-07, 7.4e-07), 'wt_n1': (6.3e-07, 7.4e-07),
                'wt_1k': (4.5e-07, 4.4e-07), 'wt_nk': (7.5e-07, 7.5e-07), 'wt_nk_standard': (3.6e-07, 1.4e-06),
                'wt_n1_robust': (2.5e-07, 6e-07), 'setdict': (1.2e-06, 3.4e-07)}
# one step from the state of pgm_bpdn_step_f64.npz: the float32 statement against the recorded float64 scalars
F32_STEP_MEASURED = {'F': 9.4e-08, 'Q': 1.2e-07, 'Rsdl': 3.6e-08, 'DFid': 9.4e-08, 'RegL1': 5.6e-09, 'ObjFun': 2.5e-08,
                     'Lfinal': 4.6e-08, 'X': 6.7e-08}

RULES = {'nesterov': MomentumNesterov, 'linear': MomentumLinear, 'genlinear': MomentumGenLinear,
         'cauchy': StepSizePolicyCauchy, 'bb': StepSizePolicyBB, 'standard': BacktrackStandard,
         'robust': BacktrackRobust}
TRACES = ('ObjFun', 'DFid', 'RegL1', 'Rsdl', 'L')
BT_TRACES = ('F_Btrack', 'Q_Btrack')

_GOLD = {}


def gold(case):
    if case not in _GOLD:
        _GOLD[case] = load_golden('pgm_bpdn_%s_f64' % case)
    return _GOLD[case]


def flat_opts(g, dtype):
    """The options and rules a fixture records, as the flat dict of tests/_pgm_bpdn_numpy.py."""
    o = {}
    for k in g:
        if k.startswith('opt_'):
            name, v = k[4:], float(g[k])
            if name == 'MaxMainIter':
                v = int(v)
            elif name in ('NonNegCoef', 'Monotone', 'AutoStop.Enabled'):
                v = bool(v)
            o[name] = v
        elif k.startswith('rule_'):
            o[k[5:]] = str(g[k]) if g[k].dtype.kind in 'US' else float(g[k])
        elif k in ('optarr_X0', 'optarr_L1Weight'):
            o[k[7:]] = g[k].astype(dtype)
    return o


def rule_objects(o):
    """Fresh rule objects of the package for the flat options ``o`` (a rule carries state)."""
    out = {}
    for slot in ('Momentum', 'StepSizePolicy', 'Backtrack'):
        if slot in o:
            par = {k.split('.')[1]: o[k] for k in o if k.startswith(slot + '.')}
            if 'maxiter' in par:
                par['maxiter'] = int(par['maxiter'])
            out[slot] = RULES[o[slot]](**par)
    return out


def options_of(o, extra=None):
    d = {'Verbose': False}
    for k, v in o.items():
        if k.split('.')[0] in ('Momentum', 'StepSizePolicy', 'Backtrack'):
            continue
        if '.' in k:
            a, b = k.split('.')
            d.setdefault(a, {})[b] = v
        else:
            d[k] = v
    d.update(rule_objects(o))
    d.update(extra or {})
    return bpdn.BPDN.Options(d)


def build(g, dtype, extra=None, D=None):
    o = flat_opts(g, dtype)
    lm = None if float(g['lmbda_given']) == 0.0 else float(g['lmbda_given'])
    D = (g['D'] if D is None else D).astype(dtype)
    if str(g['cls']) == 'WeightedBPDN':
        return bpdn.WeightedBPDN(D, g['S'].astype(dtype), lm, g['optarr_W'].astype(dtype), options_of(o, extra))
    return bpdn.BPDN(D, g['S'].astype(dtype), lm, options_of(o, extra))


def statement(g, dtype, **kw):
    lm = None if float(g['lmbda_given']) == 0.0 else float(g['lmbda_given'])
    return pn.run(g['D'], g['S'], lm, flat_opts(g, dtype), W=g.get('optarr_W'), dtype=dtype, **kw)


def setdict_statement(g, dtype):
    o = flat_opts(g, dtype)
    r1 = pn.run(g['D'], g['S'], float(g['lmbda']), o, dtype=dtype)
    r = pn.run(g['optarr_D2'], g['S'], float(g['lmbda']), o, dtype=dtype, state=r1['state'])
    r['X_first'] = r1['X']
    return r


def compare(res, g, traces_of):
    """(worst iterate error, worst trace error with the final L)."""
    ei = max(rel_l2(res['X'], g['X']), rel_l2(res['Y'], g['Y']))
    fields = TRACES + (BT_TRACES if 'it_F_Btrack' in g else ())
    et = max(rel_l2(traces_of(f), g['it_' + f]) for f in fields)
    et = max(et, abs(float(res['Lfinal']) - float(g['Lfinal'])) / float(g['Lfinal']))
    return ei, et


def f32_tols(case):
    mi, mt = F32_MEASURED[case]
    return max(4.0 * mi, 1e-4), max(4.0 * mt, 1e-3)


def discrete_path(g):
    return (tuple(int(v) for v in g['it_IterBTrack']) if 'it_IterBTrack' in g else None,
            tuple(int(v) for v in g['reverts']), tuple(int(v) for v in g['bb_fallbacks']))


def statement_path(r, g):
    return (tuple(int(v) for v in r['IterBTrack']) if 'it_IterBTrack' in g else None, tuple(r['reverts']),
            tuple(r['bb_fallbacks']) if str(g.get('rule_StepSizePolicy', '')) == 'bb' else ())


# ---- the statement and the fixtures (CPU only) ---------------------------------------------------------------
def test_statement_reproduces_fixtures():
    worst = 0.0
    for case in CASES + ['setdict']:
        g = gold(case)
        if case == 'setdict':
            r = setdict_statement(g, np.float64)
            assert rel_l2(r['X_first'], g['X_first']) <= F64_TOL
        else:
            r = statement(g, np.float64)
        ei, et = compare(r, g, lambda f: r[f])
        assert statement_path(r, g) == discrete_path(g), case
        worst = max(worst, ei, et)
    print('statement in float64 against the fixtures: %.2e' % worst)
    assert worst <= F64_TOL


def test_f32_measured_figures():
    """The figures of F32_MEASURED, measured again; every case follows the fixture's discrete path in float32,
    at every iteration."""
    for case in CASES + ['setdict']:
        g = gold(case)
        r = setdict_statement(g, np.float32) if case == 'setdict' else statement(g, np.float32)
        ei, et = compare(r, g, lambda f: r[f])
        print("'%s': (%.1e, %.1e)," % (case, ei, et))
        assert statement_path(r, g) == discrete_path(g), case
        assert len(r['ObjFun']) == len(g['it_ObjFun']), case
        assert ei <= F32_MEASURED[case][0] and et <= F32_MEASURED[case][1], (case, ei, et)


def test_fixtures_hold_their_conditions():
    for case in CASES + ['setdict']:
        g = gold(case)
        n = len(g['it_ObjFun'])
        assert n == (int(g['opt_MaxMainIter']) if case != 'autostop' else 4), case
        for f in TRACES:
            assert np.all(np.isfinite(g['it_' + f])) and len(g['it_' + f]) == n, (case, f)
        if 'rule_Backtrack' in g:
            assert g['it_IterBTrack'].max() > 1 and 'it_F_Btrack' in g, case
            assert np.all(g['it_F_Btrack'] <= g['it_Q_Btrack']), case
        else:
            assert 'it_IterBTrack' not in g, case
        assert 0.05 <= float(g['zero_share']) <= 0.95, case
    assert float(gold('default')['opt_L']) == 500.0 and float(gold('monotone')['opt_L']) == 200.0
    assert float(gold('lmbda_none')['lmbda_given']) == 0.0
    assert abs(float(gold('lmbda_none')['lmbda']) - pn.default_lmbda(gold('lmbda_none')['D'], gold('lmbda_none')['S'])) < 1e-15
    assert not np.any(gold('nonneg')['X'] < 0)
    assert gold('w_atom')['optarr_L1Weight'].shape == (16, 1)
    assert gold('w_signal')['optarr_L1Weight'].shape == (1, 5)
    assert gold('w_full')['optarr_L1Weight'].shape == (16, 5)
    assert 'optarr_X0' in gold('x0')
    assert gold('square')['D'].shape == (8, 8) and gold('tall')['D'].shape == (24, 16) and gold('k1')['S'].shape == (8, 1)
    for case, shp in (('wt_scalar', ()), ('wt_n', (8,)), ('wt_n1', (8, 1)), ('wt_1k', (1, 5)), ('wt_nk', (8, 5)),
                      ('wt_nk_standard', (8, 5)), ('wt_n1_robust', (8, 1))):
        assert gold(case)['optarr_W'].shape == shp and str(gold(case)['cls']) == 'WeightedBPDN', case
    assert len(gold('monotone_l1')['reverts']) >= 1 and bool(gold('monotone')['opt_Monotone'])
    assert len(set(gold('cauchy')['it_L'])) > 10 and len(set(gold('bb')['it_L'])) > 10
    s = gold('setdict')
    assert not np.array_equal(s['D'], s['optarr_D2']) and not np.array_equal(s['X_first'], s['X'])
    r = load_golden('pgm_bpdn_recover_f64')
    assert np.linalg.norm(r['Y'] - r['x0']) < 1e-3 and np.count_nonzero(r['x0']) == 4
    st = load_golden('pgm_bpdn_step_f64')
    assert int(st['IterBTrack']) >= 2 and float(st['F']) <= float(st['Q'])


# ---- the classes against the fixtures of the unmodified reference --------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('case', CASES)
def test_against_reference_fixture(backend, case, dtype):
    g = gold(case)
    b = build(g, dtype)
    out = b.solve()
    its = b.getitstat()
    res = {'X': b.X, 'Y': b.Y, 'Lfinal': b.L}
    ei, et = compare(res, g, lambda f: getattr(its, f))
    print('%s %s: iterates %.2e traces %.2e' % (case, np.dtype(dtype).name, ei, et))
    tol_i, tol_t = (F64_TOL, F64_TOL) if dtype == np.float64 else f32_tols(case)
    assert out.dtype == dtype and out.shape == g['X'].shape and b.Y.dtype == dtype
    assert np.array_equal(out, b.X) and np.array_equal(b.getcoef(), b.X)
    assert np.array_equal(its.Iter, np.arange(len(g['it_ObjFun'])))
    if 'it_IterBTrack' in g:
        assert [int(v) for v in its.IterBTrack] == [int(v) for v in g['it_IterBTrack']]
    else:
        assert all(v is None for v in its.IterBTrack) and all(v is None for v in its.F_Btrack)
    assert ei <= tol_i and et <= tol_t, (ei, et)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_setdict_between_solves(backend, dtype):
    g = gold('setdict')
    b = build(g, dtype)
    b.solve()
    first = b.X.copy()
    b.itstat = []
    b.setdict(g['optarr_D2'].astype(dtype))
    assert np.array_equal(b.X, first)
    b.solve()
    its = b.getitstat()
    ei, et = compare({'X': b.X, 'Y': b.Y, 'Lfinal': b.L}, g, lambda f: getattr(its, f))
    tol_i, tol_t = (F64_TOL, F64_TOL) if dtype == np.float64 else f32_tols('setdict')
    assert rel_l2(first, g['X_first']) <= tol_i
    assert ei <= tol_i and et <= tol_t, (ei, et)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_one_step_from_recorded_state(backend, dtype):
    st = load_golden('pgm_bpdn_step_f64')
    opt = bpdn.BPDN.Options({'Verbose': False, 'MaxMainIter': 1, 'RelStopTol': 0.0, 'L': float(st['L_before']),
                             'Backtrack': BacktrackStandard(gamma_u=float(st['gamma_u']), maxiter=int(st['maxiter']))})
    b = bpdn.BPDN(st['D'].astype(dtype), st['S'].astype(dtype), float(st['lmbda']), opt)
    b.X = st['X_before']
    b.Y = st['Y_before']
    b.k, b.t = int(st['k']), float(st['t'])
    b.solve()
    it = b.itstat[-1]
    assert it.Iter == int(st['k']) and it.IterBTrack == int(st['IterBTrack'])
    for name, v in (('F', it.F_Btrack), ('Q', it.Q_Btrack), ('Rsdl', it.Rsdl), ('DFid', it.DFid), ('RegL1', it.RegL1),
                    ('ObjFun', it.ObjFun), ('Lfinal', b.L)):
        e = abs(float(v) - float(st[name])) / abs(float(st[name]))
        print('%s %s: %.2e' % (name, np.dtype(dtype).name, e))
        assert e <= (F64_TOL if dtype == np.float64 else max(4.0 * F32_STEP_MEASURED[name], 1e-3)), (name, e)
    tol = F64_TOL if dtype == np.float64 else max(4.0 * F32_STEP_MEASURED['X'], 1e-4)
    assert rel_l2(b.X, st['X']) <= tol and rel_l2(b.Y, st['Y']) <= tol


def test_f32_step_measured_figures():
    st = load_golden('pgm_bpdn_step_f64')
    o = {'MaxMainIter': 1, 'RelStopTol': 0.0, 'L': float(st['L_before']), 'Backtrack': 'standard',
         'Backtrack.gamma_u': float(st['gamma_u']), 'Backtrack.maxiter': int(st['maxiter'])}
    for dtype in (np.float64, np.float32):
        s = pn.State()
        s.X, s.Y = st['X_before'].astype(dtype), st['Y_before'].astype(dtype)
        s.L, s.k, s.t, s.Tk, s.Z, s.bbx, s.bbg, s.objfn, s.reverts = dtype(st['L_before']), int(st['k']), float(st['t']), \
            0.0, None, None, None, None, []
        r = pn.run(st['D'], st['S'], float(st['lmbda']), o, dtype=dtype, state=s)
        fig = {'F': r['F_Btrack'][0], 'Q': r['Q_Btrack'][0], 'Rsdl': r['Rsdl'][0], 'DFid': r['DFid'][0],
               'RegL1': r['RegL1'][0], 'ObjFun': r['ObjFun'][0], 'Lfinal': r['Lfinal']}
        assert int(r['IterBTrack'][0]) == int(st['IterBTrack'])
        for name, v in fig.items():
            e = abs(float(v) - float(st[name])) / abs(float(st[name]))
            print("'%s': %.1e," % (name, e))
            assert e <= (F64_TOL if dtype == np.float64 else F32_STEP_MEASURED[name]), (name, e)
        e = max(rel_l2(r['X'], st['X']), rel_l2(r['Y'], st['Y']))
        print("'X': %.1e," % e)
        assert e <= (F64_TOL if dtype == np.float64 else F32_STEP_MEASURED['X'])


# ---- edges against the NumPy statement ---------------------------------------------------------------------
def edge_problem(N, M, K, seed=3):
    rng = np.random.RandomState(seed)
    D = rng.randn(N, M)
    D /= np.sqrt(np.sum(D ** 2, axis=0, keepdims=True))
    S = rng.randn(N, K)
    X0 = 0.3 * rng.randn(M, K)
    return D, S, X0


def edge_L(D):
    """A step constant for which the iteration contracts: the largest eigenvalue of D^T D."""
    return float(np.linalg.norm(D, 2) ** 2) * 1.05


def run_edge(N, M, K, dtype, o=None, W=None, cls=None, iters=EDGE_ITERS, fold=True, lmbda=0.15):
    D, S, X0 = edge_problem(N, M, K)
    oo = {'MaxMainIter': iters, 'RelStopTol': 0.0, 'L': edge_L(D), 'X0': X0}
    oo.update(o or {})
    opts = options_of({k: (v.astype(dtype) if isinstance(v, np.ndarray) else v) for k, v in oo.items()})
    if W is not None:
        b = bpdn.WeightedBPDN(D.astype(dtype), S.astype(dtype), lmbda, np.asarray(W, dtype=dtype), opts)
    else:
        b = (cls or bpdn.BPDN)(D.astype(dtype), S.astype(dtype), lmbda, opts)
    b._fold_momentum = fold
    b.solve()
    r = pn.run(D, S, lmbda, oo, W=W, dtype=dtype)
    its = b.getitstat()
    tol = F64_TOL if dtype == np.float64 else EDGE_F32
    for f in ('X', 'Y'):
        assert rel_l2(getattr(b, f), r[f]) <= tol, (f, rel_l2(getattr(b, f), r[f]))
    for f in TRACES + (BT_TRACES if oo.get('Backtrack') else ()):
        assert rel_l2(getattr(its, f), r[f]) <= tol, (f, rel_l2(getattr(its, f), r[f]))
    if oo.get('Backtrack'):
        assert [int(v) for v in its.IterBTrack] == [int(v) for v in r['IterBTrack']]
    return b, r


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('M', [1, 3, 4, 5, 15, 16, 17, 33])
def test_edge_M(backend, M, dtype):
    run_edge(8, M, 5, dtype)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('N', [1, 3, 5, 16, 17, 33])
def test_edge_N(backend, N, dtype):
    run_edge(N, 16, 5, dtype)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('K', [1, 15, 16, 17, 31, 32, 33, 65])
def test_edge_K(backend, K, dtype):
    run_edge(8, 16, K, dtype, o={'Backtrack': 'standard', 'Backtrack.gamma_u': 1.2, 'Backtrack.maxiter': 50, 'L': 0.5})


@pytest.mark.parametrize('dims', [(np.float32, 168, 8, 32), (np.float32, 8, 168, 32), (np.float32, 172, 8, 16),
                                  (np.float32, 8, 172, 16), (np.float64, 84, 8, 32), (np.float64, 8, 84, 32),
                                  (np.float64, 88, 8, 16), (np.float64, 8, 88, 16)])
def test_both_column_block_widths(backend, dims):
    """The rule of bpdn_kb (the two LDS tiles within 64 KiB: the new kernel keeps it, its extra LDS is the sums'
    scratch) just below and just above its boundary, with M and with N the larger dimension."""
    dtype, M, N, KB = dims
    assert bpdn.plan(N, M, 2 * KB + 3, dtype)['KB'] == KB
    run_edge(N, M, 2 * KB + 3, dtype, iters=2)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('shape', [(), (8,), (8, 1), (1, 5), (8, 5)])
@pytest.mark.parametrize('bt', [None, 'robust'])
def test_edge_W_shapes(backend, shape, bt, dtype):
    W = 0.5 + np.random.RandomState(5).rand(*shape)
    o = {} if bt is None else {'Backtrack': 'robust', 'Backtrack.gamma_d': 0.9, 'Backtrack.gamma_u': 2.0,
                               'Backtrack.maxiter': 50, 'L': 0.5}
    run_edge(8, 16, 5, dtype, o=o, W=W)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('shape', [(), (16, 1), (1, 5), (16, 5)])
@pytest.mark.parametrize('nonneg', [False, True])
def test_edge_L1Weight_shapes_and_nonneg(backend, shape, nonneg, dtype):
    w = 1.0 + np.random.RandomState(6).rand(*shape)
    b, r = run_edge(8, 16, 5, dtype, o={'L1Weight': w, 'NonNegCoef': nonneg})
    if nonneg:
        assert not np.any(b.X < 0) and np.any(r['X'] == 0)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('o', [{'StepSizePolicy': 'cauchy'}, {'StepSizePolicy': 'bb'}, {'Monotone': True, 'L': 1.2},
                               {'Monotone': True, 'L': 0.8, 'Backtrack': 'standard', 'Backtrack.gamma_u': 1.2,
                                'Backtrack.maxiter': 50},
                               {'Momentum': 'linear', 'Momentum.b': 2.0},
                               {'Momentum': 'genlinear', 'Momentum.a': 50.0, 'Momentum.b': 2.0}],
                         ids=['cauchy', 'bb', 'monotone', 'monotone_standard', 'linear', 'genlinear'])
def test_edge_rules(backend, o, dtype):
    run_edge(5, 17, 33, dtype, o=o, iters=6)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_momentum_folded_into_the_load_equals_a_separate_step(backend, dtype):
    """The Y tile formed on the way into the step against the Y formed by a launch of its own: the same
    operations, so the same bits."""
    a, _ = run_edge(8, 17, 33, dtype, iters=5, fold=True)
    b, _ = run_edge(8, 17, 33, dtype, iters=5, fold=False)
    assert a._pending_beta is not None and b._pending_beta is None
    assert np.array_equal(a.X, b.X) and np.array_equal(a.Y, b.Y)
    assert np.array_equal(a.getitstat().ObjFun, b.getitstat().ObjFun)
    assert np.array_equal(a.getitstat().Rsdl, b.getitstat().Rsdl)


# ---- GPU only ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_workgroup_loops_over_column_blocks(gpu_backend, dtype):
    """More column blocks than workgroups (kBpdnMaxBlocks = 1024)."""
    K = 1024 * 32 + 40
    p = bpdn.plan(4, 8, K, dtype)
    assert p['blocks'] == 1024 and p['KB'] == 32
    run_edge(4, 8, K, dtype, iters=2)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_largest_dictionary(gpu_backend, dtype):
    run_edge(512, 512, 40, dtype, iters=2)


@pytest.mark.gpu
def test_two_runs_are_bitwise_equal(gpu_backend):
    res = []
    for _ in range(2):
        b, _ = run_edge(33, 70, 100, np.float32, iters=5,
                        o={'Backtrack': 'robust', 'Backtrack.gamma_d': 0.9, 'Backtrack.gamma_u': 2.0,
                           'Backtrack.maxiter': 50, 'L': 0.5})
        its = b.getitstat()
        res.append((b.X, b.Y, np.array(its.ObjFun), np.array(its.Rsdl), np.array(its.F_Btrack)))
    for u, v in zip(*res):
        assert np.array_equal(u, v)


_FORM_SCRIPT = r"""
import sys, numpy as np
sys.path.insert(0, %(repo)r); sys.path.insert(0, %(tests)r)
from sporco_amd.pgm import bpdn
import test_pgm_bpdn as t
out = {'mfma': np.int64(bpdn.plan(8, 16, 5, np.float32)['mfma'])}
for tag, o in (('plain', {}), ('std', {'Backtrack': 'standard', 'Backtrack.gamma_u': 1.2, 'Backtrack.maxiter': 50, 'L': 0.5}),
               ('cauchy', {'StepSizePolicy': 'cauchy'})):
    for M in (16, 40, 132, 176):
        for N in (8, 64):
            K = 3 * bpdn.plan(N, M, 5, np.float32)['KB'] + 1
            b, _ = t.run_edge(N, M, K, np.float32, o=o, iters=4)
            out['%%s_%%d_%%d_X' %% (tag, M, N)] = b.X
            out['%%s_%%d_%%d_Y' %% (tag, M, N)] = b.Y
            out['%%s_%%d_%%d_obj' %% (tag, M, N)] = np.array(b.getitstat().ObjFun)
            out['%%s_%%d_%%d_rsdl' %% (tag, M, N)] = np.array(b.getitstat().Rsdl)
np.savez(sys.argv[1], **out)
"""


@pytest.mark.gpu
def test_mfma_form_equals_plain_form(gpu_backend, tmp_path):
    """float32 with SPORCO_AMD_BPDN_PLAIN set and unset (the switch is read when a handle is made; one process
    each): X, Y and the traces agree bit for bit; M = 176 is the 16-column block."""
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


# ---- sparse recovery: the reference's tests/pgm/test_bpdn.py::TestSet01::test_09 -----------------------------
def test_sparse_recovery(backend):
    r = load_golden('pgm_bpdn_recover_f64')
    opt = bpdn.BPDN.Options({'Verbose': False, 'MaxMainIter': int(r['MaxMainIter']), 'RelStopTol': float(r['RelStopTol']),
                             'Backtrack': BacktrackRobust(gamma_d=float(r['gamma_d']))})
    b = bpdn.BPDN(r['D'], r['S'], float(r['lmbda']), opt)
    b.solve()
    x1 = b.Y
    assert np.abs(b.itstat[-1].ObjFun - 0.012009) < 1e-5
    assert np.abs(b.itstat[-1].DFid - 1.9636082e-06) < 1e-5
    assert np.abs(b.itstat[-1].RegL1 - 2.401446) < 2e-4
    assert np.linalg.norm(x1 - r['x0']) < 1e-3
    assert x1.dtype == np.float64


# ---- contract and refusals ---------------------------------------------------------------------------------
def test_option_defaults_equal_the_reference():
    d = load_golden('pgm_bpdn_defaults')
    for cname in ('BPDN', 'WeightedBPDN'):
        cls = getattr(bpdn, cname)
        mine = {}
        for k, v in cls.Options.defaults.items():
            if isinstance(v, dict):
                for kk, vv in v.items():
                    mine['%s.%s' % (k, kk)] = repr(vv)
            else:
                mine[k] = type(v).__name__ if k in ('Momentum', 'StepSizePolicy', 'Backtrack') else repr(v)
        ref = dict(zip((str(k) for k in d[cname + '_keys']), (str(v) for v in d[cname + '_values'])))
        assert mine == ref, cname
        assert cls.IterationStats._fields == tuple(str(f) for f in d[cname + '_fields'])
        assert cls.IterationStats._fields == ('Iter', 'ObjFun', 'DFid', 'RegL1', 'Rsdl', 'F_Btrack', 'Q_Btrack',
                                              'IterBTrack', 'L', 'Time')
        assert cls.hdrtxt() == tuple(str(h) for h in d[cname + '_hdrtxt'])
        assert tuple(cls.hdrval()[h] for h in cls.hdrtxt()) == tuple(str(h) for h in d[cname + '_hdrval'])


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_host_methods(backend, dtype):
    D, S, X0 = edge_problem(8, 16, 5)
    W = (0.5 + np.random.RandomState(2).rand(8, 1)).astype(dtype)
    wl1 = (1.0 + np.random.RandomState(4).rand(16, 1)).astype(dtype)
    D, S, X0 = D.astype(dtype), S.astype(dtype), X0.astype(dtype)
    opt = bpdn.BPDN.Options({'Verbose': False, 'MaxMainIter': 3, 'L': 9.0, 'L1Weight': wl1, 'NonNegCoef': True})
    b = bpdn.WeightedBPDN(D, S, 0.2, W, opt)
    b.solve()
    tol = 1e-12 if dtype == np.float64 else 1e-5
    V = np.random.RandomState(8).randn(16, 5).astype(dtype)
    assert rel_l2(b.grad_f(V), D.T.dot(W * (D.dot(V) - S))) <= tol
    assert rel_l2(b.grad_f(), D.T.dot(W * (D.dot(b.Y) - S))) <= tol
    assert rel_l2(b.hessian_f(V), D.T.dot(D.dot(V))) <= tol
    P = np.sign(V) * np.maximum(0, np.abs(V) - (0.2 / 9.0) * wl1)
    P[P < 0] = 0
    assert rel_l2(b.prox_g(V), P) <= tol and b.prox_g(V).dtype == dtype
    assert abs(b.obfn_f(V) - 0.5 * np.sum(W * (D.dot(V) - S) ** 2)) <= tol * b.obfn_f(V)
    assert abs(b.obfn_f() - b.itstat[-1].DFid) <= max(tol, 1e-4 if dtype == np.float32 else 0) * b.obfn_f()
    assert abs(b.obfn_reg()[1] - np.sum(np.abs(wl1 * b.X))) <= tol * 10 * b.obfn_reg()[1]
    assert abs(b.eval_objfn()[0] - b.itstat[-1].ObjFun) == 0.0
    assert np.array_equal(b.reconstruct(), D.dot(b.X)) and np.array_equal(b.reconstruct(V), D.dot(b.X))
    assert b.X.dtype == dtype and b.Y.dtype == dtype and b.Yprv.dtype == dtype and b.Yprv.shape == (16, 5)


def test_fastsolve_reads_nothing(backend, monkeypatch):
    D, S, X0 = edge_problem(8, 16, 5)
    reads = []
    real = _lib.PgmBpdnHandle.step

    def step(self, params, read=True):
        reads.append(read)
        return real(self, params, read=read)
    monkeypatch.setattr(_lib.PgmBpdnHandle, 'step', step)
    b = bpdn.BPDN(D, S, 0.15, bpdn.BPDN.Options({'Verbose': False, 'MaxMainIter': 6, 'FastSolve': True, 'L': edge_L(D)}))
    X = b.solve()
    assert b.itstat == [] and reads == [False] * 6
    r = pn.run(D, S, 0.15, {'MaxMainIter': 6, 'RelStopTol': 0.0, 'L': edge_L(D)})
    assert rel_l2(X, r['X']) <= F64_TOL and rel_l2(b.Y, r['Y']) <= F64_TOL


def test_callback_and_restart(backend):
    D, S, X0 = edge_problem(8, 16, 5)
    o = {'Verbose': False, 'MaxMainIter': 50, 'RelStopTol': 0.0, 'L': edge_L(D)}
    b = bpdn.BPDN(D, S, 0.15, bpdn.BPDN.Options(dict(o, Callback=lambda obj: bool(obj.k > 5))))
    b.solve()
    assert len(b.itstat) == 7 and b.k == 7
    c = bpdn.BPDN(D, S, 0.15, bpdn.BPDN.Options(dict(o, MaxMainIter=4)))
    c.solve()
    c.solve()
    d = bpdn.BPDN(D, S, 0.15, bpdn.BPDN.Options(dict(o, MaxMainIter=8)))
    d.solve()
    assert np.array_equal(c.X, d.X) and np.array_equal(c.Y, d.Y)
    assert np.array_equal(c.getitstat().ObjFun, d.getitstat().ObjFun) and list(c.getitstat().Iter) == list(range(8))


def test_refusals(backend):
    D, S, _ = edge_problem(8, 16, 5)
    with pytest.raises(TypeError):
        bpdn.BPDN(D.astype(np.complex128), S)
    with pytest.raises(TypeError):
        bpdn.BPDN(D.astype(np.float16), S.astype(np.float16))
    with pytest.raises(TypeError):
        bpdn.BPDN(D, S, 0.1, bpdn.BPDN.Options({'DataType': np.float16}))
    with pytest.raises(TypeError):
        bpdn.BPDN(D.astype(np.int32), S)
    with pytest.raises(ValueError):
        bpdn.BPDN(np.zeros((8, 513)), S)
    with pytest.raises(ValueError):
        bpdn.BPDN(np.zeros((513, 8)), np.zeros((513, 2)))
    with pytest.raises(ValueError):
        bpdn.BPDN(D, S[:, 0])
    with pytest.raises(ValueError):
        bpdn.BPDN(D, S[:7])
    with pytest.raises(ValueError):
        bpdn.WeightedBPDN(D, S, 0.1, np.ones((7, 1)))
    with pytest.raises(ValueError):
        bpdn.WeightedBPDN(D, S, 0.1, np.ones((8, 4)))
    with pytest.raises(NotImplementedError):
        bpdn.BPDN(D, S, 0.1, reducer=object())
    b = bpdn.BPDN(D, S, 0.1)
    with pytest.raises(NotImplementedError):
        pickle.dumps(b)
    with pytest.raises(ValueError):
        b.setdict(D[:, :8])
    assert bpdn.WeightedBPDN(D, S, 0.1).W.size == 1
