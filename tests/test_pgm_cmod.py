"""sporco_amd.pgm.cmod CnstrMOD / WeightedCnstrMOD against fixtures of the unmodified reference
(tests/golden/pgm_cmod_*_f64.npz, tools/make_golden_pgm_cmod.py) and against the NumPy statement of
tests/_pgm_cmod_numpy.py.

Tolerances.  float64: the statement against the fixtures 1e-10, the package the project's 1e-9 relative l2 on X, Y,
every trace and the final L.  float32 input against the float64 fixture: 1e-4 on iterates and 1e-3 on traces, or four
times what the NumPy statement run in float32 shows against the same fixture, whichever is larger, per case:
F32_MEASURED below (test_f32_measured_figures repeats the measurement on the CPU); the margin of four covers the
summation order.  Cnstr sits at rounding level (X' is normalised, so Pcn(X') - X' is a rounding residue): it is
compared absolutely, in float64 at 1e-13 and in float32 at four times the statement's own figure (third entry of
F32_MEASURED).  IterBTrack is compared as integers.

Every backtracking, Barzilai-Borwein, Cauchy and Monotone fixture was checked when it was made to be followed by the
float32 statement on its discrete path (IterBTrack, the iterations at which Monotone reverts and at which the
Barzilai-Borwein rule falls back); test_f32_measured_figures asserts it again, for every case and iteration.

Edge shapes run against the statement in the same dtype: 1e-9 in float64; in float32 EDGE_F32 = 2e-4 on iterates and
traces after EDGE_ITERS = 4 iterations.  (Reasoning: G is two chained products, the first a sum of at most 512 terms,
the second of K <= 100 terms here, of O(1) numbers; a float32 dot product of n terms in a different order differs by
about sqrt(n) eps = 23 * 6e-8 = 1.4e-6 relative to the operand norms; a step moves Y by G / L with || Z Z^T || / L <=
about 4 at the L the edge problems use, and the normalisation does not amplify: 4 steps * 2 products * 1.4e-6 * 4 =
4.5e-5, doubled for the momentum term's factor below 2.)  At K of a few tens of thousands (the slab-cap case) the
second product has 4e4 terms: sqrt(n) eps = 1.2e-5 a product, and EDGE_F32_LONG = 2e-3 by the same count.
"""

import pickle

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _pgm_cmod_numpy as pn

from sporco_amd import _lib
from sporco_amd.device import DeviceArray
from sporco_amd.pgm import cmod
from sporco_amd.pgm.backtrack import BacktrackRobust, BacktrackStandard
from sporco_amd.pgm.momentum import MomentumGenLinear, MomentumLinear, MomentumNesterov
from sporco_amd.pgm.stepsize import StepSizePolicyBB, StepSizePolicyCauchy

CASES = ['default', 'l30', 'zeromean', 'nonneg', 'x0', 'dsz_only', 'tall', 'wide', 'zero_row', 'bt_standard',
         'bt_robust', 'mom_nesterov', 'mom_linear', 'mom_genlinear', 'cauchy', 'bb', 'monotone', 'autostop', 'wt_none',
         'wt_scalar', 'wt_n', 'wt_n1', 'wt_1k', 'wt_nk', 'wt_mask', 'wt_mask_standard', 'wt_n1_robust',
         'wt_nk_zeromean']
F64_TOL = 1e-9
STATEMENT_TOL = 1e-10
CNSTR_F64 = 1e-13
EDGE_ITERS = 4
EDGE_F32 = 2e-4
EDGE_F32_LONG = 2e-3
# case: (iterates, traces and final L, Cnstr absolute) of the float32 statement against the float64 fixture
F32_MEASURED = {'default': (5.9e-07, 1.1e-07, 2.8e-07), 'l30': (1.8e-07, 4.4e-08, 3.3e-07),
                'zeromean': (1.9e-07, 9.6e-08, 2.8e-07), 'nonneg': (1.4e-07, 8.9e-08, 2.7e-07),
                'x0': (1.7e-07, 1.2e-07, 3.1e-07), 'dsz_only': (1.4e-07, 1.6e-07, 1.8e-07),
                'tall': (1.5e-07, 7.6e-08, 2.8e-07), 'wide': (2.4e-07, 1.1e-07, 3.9e-07),
                'zero_row': (1.9e-07, 6.9e-08, 2.8e-07), 'bt_standard': (1.6e-07, 2.9e-06, 3.3e-07),
                'bt_robust': (2.4e-07, 5.2e-07, 3.0e-07), 'mom_nesterov': (1.5e-07, 3.0e-08, 3.3e-07),
                'mom_linear': (1.9e-07, 5.2e-08, 3.2e-07), 'mom_genlinear': (1.8e-07, 4.3e-08, 3.1e-07),
                'cauchy': (1.5e-07, 2.6e-06, 2.7e-07), 'bb': (2.0e-07, 4.3e-05, 3.2e-07),
                'monotone': (2.5e-07, 9.0e-08, 2.2e-07), 'autostop': (8.7e-08, 3.0e-08, 2.7e-07),
                'wt_none': (1.8e-07, 4.4e-08, 3.3e-07), 'wt_scalar': (2.1e-07, 7.1e-08, 3.4e-07),
                'wt_n': (2.1e-07, 2.3e-08, 3.5e-07), 'wt_n1': (2.1e-07, 2.3e-08, 3.5e-07),
                'wt_1k': (1.7e-07, 6.5e-08, 3.3e-07), 'wt_nk': (2.1e-07, 1.3e-07, 2.9e-07),
                'wt_mask': (2.7e-07, 4.8e-08, 2.7e-07), 'wt_mask_standard': (2.4e-07, 1.4e-06, 3.5e-07),
                'wt_n1_robust': (1.8e-07, 3.0e-07, 3.4e-07), 'wt_nk_zeromean': (2.2e-07, 1.1e-07, 2.8e-07)}

RULES = {'nesterov': MomentumNesterov, 'linear': MomentumLinear, 'genlinear': MomentumGenLinear,
         'cauchy': StepSizePolicyCauchy, 'bb': StepSizePolicyBB, 'standard': BacktrackStandard,
         'robust': BacktrackRobust}
TRACES = ('DFid', 'Rsdl', 'L')
BT_TRACES = ('F_Btrack', 'Q_Btrack')

_GOLD = {}


def gold(case):
    if case not in _GOLD:
        _GOLD[case] = load_golden('pgm_cmod_%s_f64' % case)
    return _GOLD[case]


def flat_opts(g, dtype):
    """The options and rules a fixture records, as the flat dict of tests/_pgm_cmod_numpy.py."""
    o = {}
    for k in g:
        if k.startswith('opt_'):
            name, v = k[4:], float(g[k])
            if name == 'MaxMainIter':
                v = int(v)
            elif name in ('NonNegCoef', 'ZeroMean', 'Monotone', 'AutoStop.Enabled'):
                v = bool(v)
            o[name] = v
        elif k.startswith('rule_'):
            o[k[5:]] = str(g[k]) if g[k].dtype.kind in 'US' else float(g[k])
        elif k == 'optarr_X0':
            o['X0'] = g[k].astype(dtype)
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
    return cmod.CnstrMOD.Options(d)


def build(g, dtype, extra=None):
    o = flat_opts(g, dtype)
    Z, S = g['Z'].astype(dtype), g['S'].astype(dtype)
    zarg = None if float(g['dsz_only']) else Z
    dsz = (Z.shape[0], S.shape[1])
    if str(g['cls']) == 'WeightedCnstrMOD':
        W = g['optarr_W'].astype(dtype) if 'optarr_W' in g else None
        c = cmod.WeightedCnstrMOD(zarg, S, W, dsz, options_of(o, extra))
    else:
        c = cmod.CnstrMOD(zarg, S, dsz, options_of(o, extra))
    if zarg is None:
        c.setcoef(Z)
    return c


def statement(g, dtype, **kw):
    return pn.run(g['Z'], g['S'], flat_opts(g, dtype), W=g.get('optarr_W'), dtype=dtype, **kw)


def compare(res, g, traces_of):
    """(worst iterate error, worst trace error with the final L, worst absolute Cnstr error)."""
    ei = max(rel_l2(res['X'], g['X']), rel_l2(res['Y'], g['Y']))
    fields = TRACES + (BT_TRACES if 'it_F_Btrack' in g else ())
    et = max(rel_l2(traces_of(f), g['it_' + f]) for f in fields)
    et = max(et, abs(float(res['Lfinal']) - float(g['Lfinal'])) / float(g['Lfinal']))
    ec = float(np.max(np.abs(np.asarray(traces_of('Cnstr')) - g['it_Cnstr'])))
    return ei, et, ec


def f32_tols(case):
    mi, mt, mc = F32_MEASURED[case]
    return max(4.0 * mi, 1e-4), max(4.0 * mt, 1e-3), 4.0 * mc


def discrete_path(g):
    return (tuple(int(v) for v in g['it_IterBTrack']) if 'it_IterBTrack' in g else None,
            tuple(int(v) for v in g['reverts']), tuple(int(v) for v in g['bb_fallbacks']))


def statement_path(r, g):
    return (tuple(int(v) for v in r['IterBTrack']) if 'it_IterBTrack' in g else None, tuple(r['reverts']),
            tuple(r['bb_fallbacks']) if str(g.get('rule_StepSizePolicy', '')) == 'bb' else ())


def solved(c):
    c.solve()
    its = c.getitstat()
    res = dict(X=c.X, Y=c.Y, Lfinal=float(c.L))
    return res, (lambda f: np.asarray(getattr(its, f), dtype=np.float64)), its


# ---- the statement and the fixtures (CPU only) ---------------------------------------------------------------
def test_statement_reproduces_fixtures():
    worst = 0.0
    for case in CASES:
        g = gold(case)
        r = statement(g, np.float64)
        ei, et, ec = compare(r, g, lambda f: r[f])
        assert statement_path(r, g) == discrete_path(g), case
        assert ec <= CNSTR_F64, (case, ec)
        worst = max(worst, ei, et)
    print('statement in float64 against the fixtures: %.2e' % worst)
    assert worst <= STATEMENT_TOL


def test_f32_measured_figures():
    """The figures of F32_MEASURED, measured again; every case follows the fixture's discrete path in float32,
    at every iteration."""
    for case in CASES:
        g = gold(case)
        r = statement(g, np.float32)
        ei, et, ec = compare(r, g, lambda f: r[f])
        print("'%s': (%.1e, %.1e, %.1e)," % (case, ei, et, ec))
        assert statement_path(r, g) == discrete_path(g), case
        assert len(r['DFid']) == len(g['it_DFid']), case
        m = F32_MEASURED[case]
        assert ei <= m[0] and et <= m[1] and ec <= m[2], (case, ei, et, ec)


def test_fixtures_hold_their_conditions():
    for case in CASES:
        g = gold(case)
        n = len(g['it_DFid'])
        assert n == (int(g['opt_MaxMainIter']) if case != 'autostop' else n) and n >= 2, case
        if case == 'autostop':
            assert n < int(g['opt_MaxMainIter'])
        if 'it_IterBTrack' in g:
            assert g['it_IterBTrack'].max() > 1, case
        if case == 'monotone':
            assert 0 < len(g['reverts']) < n, case
        if case == 'wt_mask':
            assert np.any(g['optarr_W'] == 0) and g['optarr_W'].shape == g['S'].shape
        if case == 'zero_row':
            assert np.any(np.all(g['Z'] == 0, axis=1))
        N, K = g['S'].shape
        M = g['Z'].shape[0]
        assert 8 <= N <= 24 and 4 <= M <= 32 and 8 <= K <= 100, case
    shapes = {tuple(np.shape(gold(c)['optarr_W'])) for c in CASES if 'optarr_W' in gold(c)}
    assert {(), (12,), (12, 1), (1, 40), (12, 40)} <= shapes


def test_option_defaults_equal_the_reference():
    d = load_golden('pgm_cmod_defaults')
    for cls in ('CnstrMOD', 'WeightedCnstrMOD'):
        c = getattr(cmod, cls)
        have = {}
        for k, v in c.Options.defaults.items():
            if isinstance(v, dict):
                for kk, vv in v.items():
                    have['%s.%s' % (k, kk)] = repr(vv)
            else:
                have[k] = type(v).__name__ if k in ('Momentum', 'StepSizePolicy', 'Backtrack') else repr(v)
        assert have == dict(zip((str(k) for k in d[cls + '_keys']), (str(v) for v in d[cls + '_values'])))
        assert tuple(c.IterationStats._fields) == tuple(str(f) for f in d[cls + '_fields'])
        assert tuple(c.hdrtxt()) == tuple(str(f) for f in d[cls + '_hdrtxt'])


def test_pcn_helpers():
    rng = np.random.RandomState(0)
    v = rng.randn(7, 5)
    v[:, 2] = 0.0
    assert np.allclose(np.sum(cmod.normalise(v) ** 2, 0), [1, 1, 0, 1, 1])
    assert np.allclose(np.mean(cmod.zeromean(v), 0), 0)
    assert np.array_equal(cmod.getPcn(False, False)(v), pn.get_pcn(False, False)(v))
    assert np.array_equal(cmod.getPcn(True, False)(v), pn.get_pcn(True, False)(v))
    assert np.array_equal(cmod.getPcn(False, True)(v), pn.get_pcn(False, True)(v))
    with pytest.raises(ValueError):
        cmod.getPcn(True, True)


# ---- parity with the reference -------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_f64_parity(backend, case):
    g = gold(case)
    res, tr, its = solved(build(g, np.float64))
    ei, et, ec = compare(res, g, tr)
    print('%s: iterates %.2e traces %.2e Cnstr %.2e' % (case, ei, et, ec))
    if 'it_IterBTrack' in g:
        assert [int(v) for v in its.IterBTrack] == [int(v) for v in g['it_IterBTrack']]
    assert len(its.DFid) == len(g['it_DFid'])
    assert ei <= F64_TOL and et <= F64_TOL and ec <= CNSTR_F64, (case, ei, et, ec)


@pytest.mark.parametrize('case', CASES)
def test_f32_parity(backend, case):
    g = gold(case)
    res, tr, its = solved(build(g, np.float32))
    assert res['X'].dtype == np.float32
    ei, et, ec = compare(res, g, tr)
    ti, tt, tc = f32_tols(case)
    print('%s: iterates %.2e (%.1e) traces %.2e (%.1e) Cnstr %.2e (%.1e)' % (case, ei, ti, et, tt, ec, tc))
    if 'it_IterBTrack' in g:
        assert [int(v) for v in its.IterBTrack] == [int(v) for v in g['it_IterBTrack']]
    assert len(its.DFid) == len(g['it_DFid'])
    assert ei <= ti and et <= tt and ec <= tc, (case, ei, et, ec)


# ---- edge shapes against the statement in the same dtype ----------------------------------------------------
def edge_problem(N, M, K, seed=5, mask=True):
    rng = np.random.RandomState(seed)
    Z = rng.randn(M, K) * (rng.rand(M, K) < 0.3)
    D0 = cmod.normalise(rng.randn(N, M))
    S = D0.dot(Z) + 0.05 * rng.randn(N, K)
    W = (0.5 + rng.rand(N, K)) * (rng.rand(N, K) >= 0.2) if mask else None
    L = 4.0 * max(1.0, float(np.linalg.norm(Z.dot(Z.T), 2)))
    return Z, S, W, L


def edge_check(N, M, K, dtype, tol, rule=None, zm=False):
    Z, S, W, L = edge_problem(N, M, K)
    o = {'L': L, 'MaxMainIter': EDGE_ITERS, 'RelStopTol': 0.0, 'ZeroMean': zm}
    if rule == 'standard':
        o.update({'Backtrack': 'standard', 'Backtrack.gamma_u': 1.2, 'Backtrack.maxiter': 50, 'L': L / 16.0})
    r = pn.run(Z, S, o, W=W, dtype=dtype)
    c = cmod.WeightedCnstrMOD(Z.astype(dtype), S.astype(dtype), W.astype(dtype), None, options_of(o))
    res, tr, its = solved(c)
    e = max(rel_l2(res['X'], r['X']), rel_l2(res['Y'], r['Y']), rel_l2(tr('DFid'), r['DFid']),
            rel_l2(tr('Rsdl'), r['Rsdl']))
    print('(%d, %d, %d) %s: %.2e' % (N, M, K, np.dtype(dtype).name, e))
    if rule == 'standard':
        assert [int(v) for v in its.IterBTrack] == [int(v) for v in r['IterBTrack']]
    assert e <= tol, (N, M, K, e)


EDGE_SHAPES = [(1, 1, 1), (5, 3, 31), (17, 13, 32), (65, 17, 33), (5, 65, 100), (33, 3, 100), (17, 17, 65)]


@pytest.mark.parametrize('shape', EDGE_SHAPES)
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_edge_shapes(backend, shape, dtype):
    edge_check(*shape, dtype=dtype, tol=F64_TOL if dtype == np.float64 else EDGE_F32, zm=shape[0] > 1)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_edge_backtracking(backend, dtype):
    edge_check(17, 13, 33, dtype, F64_TOL if dtype == np.float64 else EDGE_F32, rule='standard')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_largest_dictionary(gpu_backend, dtype):
    edge_check(512, 512, 64, dtype, F64_TOL if dtype == np.float64 else EDGE_F32)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_slab_cap(gpu_backend, dtype):
    """K such that the slab count reaches its cap of 512 and a slab has two steps, the last slab a short one."""
    K = 512 * 64 - 5
    p = cmod.plan(16, 16, K, dtype)
    assert p['slabs'] == 512 and p['slab'] == 64 and p['row_blocks'] == 1
    edge_check(16, 16, K, dtype, F64_TOL if dtype == np.float64 else EDGE_F32_LONG)


def run_bits(Z, S, W, L, iters=3, zm=False):
    o = cmod.CnstrMOD.Options({'L': L, 'MaxMainIter': iters, 'RelStopTol': 0.0, 'ZeroMean': zm})
    c = cmod.WeightedCnstrMOD(Z, S, W, None, o)
    c.solve()
    its = c.getitstat()
    return c.X.copy(), c.Y.copy(), np.asarray(its.DFid), np.asarray(its.Rsdl), np.asarray(its.Cnstr)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(17, 13, 100), (65, 130, 3000)])
def test_two_runs_bitwise_equal(gpu_backend, shape):
    Z, S, W, L = edge_problem(*shape)
    a = run_bits(Z.astype(np.float32), S.astype(np.float32), W.astype(np.float32), L)
    b = run_bits(Z.astype(np.float32), S.astype(np.float32), W.astype(np.float32), L)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


@pytest.mark.gpu
@pytest.mark.parametrize('shape', [(17, 13, 100), (65, 130, 3000), (40, 300, 200)])
def test_matrix_form_equals_plain_form_bitwise(gpu_backend, shape, monkeypatch):
    Z, S, W, L = (a.astype(np.float32) if isinstance(a, np.ndarray) else a for a in edge_problem(*shape))
    assert cmod.plan(shape[0], shape[1], shape[2])['mfma'] == 1
    a = run_bits(Z, S, W, L, zm=True)
    monkeypatch.setenv('SPORCO_AMD_CMOD_PLAIN', '1')
    assert cmod.plan(shape[0], shape[1], shape[2])['mfma'] == 0
    b = run_bits(Z, S, W, L, zm=True)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


# ---- behaviour -------------------------------------------------------------------------------------------------
def test_fastsolve_reads_nothing(backend):
    g = gold('l30')
    ref, _, _ = solved(build(g, np.float64))
    c = build(g, np.float64, {'FastSolve': True})
    _lib.transfer_stats(reset=True)
    c._return_min = False
    c.solve()
    st = _lib.transfer_stats()
    assert st['d2h_bytes'] == 0 and st['h2d_bytes'] == 0, st
    assert c.itstat == []
    assert rel_l2(c.X, ref['X']) == 0.0 and rel_l2(c.Y, ref['Y']) == 0.0


def test_one_read_per_step_with_fixed_l(backend):
    g = gold('l30')
    c = build(g, np.float64)
    c._return_min = False
    _lib.transfer_stats(reset=True)
    c.solve()
    st = _lib.transfer_stats()
    n = len(c.itstat)
    assert st['h2d_bytes'] == 0 and st['d2h_bytes'] == n * 8 * _lib.OUT_COUNT, st


def test_setcoef_between_solves_restart_and_callback(backend):
    g = gold('l30')
    o = flat_opts(g, np.float64)
    o['MaxMainIter'] = 6
    Z2 = np.roll(g['Z'], 1, axis=1) * 0.9
    r1 = pn.run(g['Z'], g['S'], o, dtype=np.float64)
    r2 = pn.run(Z2, g['S'], o, dtype=np.float64, state=r1['state'])
    seen = []
    c = cmod.CnstrMOD(g['Z'], g['S'], None, options_of(o, {'Callback': lambda s: seen.append(s.k) or False}))
    c.solve()
    assert rel_l2(c.X, r1['X']) <= F64_TOL
    c.setcoef(Z2)
    c.solve()
    assert seen == list(range(12))
    assert rel_l2(c.X, r2['X']) <= F64_TOL and rel_l2(c.Y, r2['Y']) <= F64_TOL
    assert rel_l2(np.asarray(c.getitstat().DFid)[6:], r2['DFid']) <= F64_TOL
    stop = cmod.CnstrMOD(g['Z'], g['S'], None, options_of(o, {'Callback': lambda s: s.k == 2}))
    stop.solve()
    assert len(stop.itstat) == 3


def test_setcoef_takes_a_device_array(backend):
    g = gold('wt_mask')
    ref, _, _ = solved(build(g, np.float64))
    o = options_of(flat_opts(g, np.float64))
    zd, sd, wd = (DeviceArray.from_host(np.ascontiguousarray(g[k])) for k in ('Z', 'S', 'optarr_W'))
    c = cmod.WeightedCnstrMOD(None, sd, wd, (g['Z'].shape[0], g['S'].shape[1]), o)
    c.setcoef(zd)
    c.solve()
    assert rel_l2(c.X, ref['X']) == 0.0


def test_host_methods(backend):
    g = gold('wt_nk')
    c = build(g, np.float64, {'MaxMainIter': 3})
    c.solve()
    Z, S, W = g['Z'], g['S'], g['optarr_W']
    V = c.Y
    assert rel_l2(c.grad_f(), (W * (V.dot(Z) - S)).dot(Z.T)) <= 1e-14
    assert rel_l2(c.hessian_f(V), V.dot(Z).dot(Z.T)) <= 1e-14
    assert abs(c.obfn_f() - c.itstat[-1].DFid) <= 1e-9 * c.itstat[-1].DFid
    assert abs(c.dfid_device() - c.obfn_f()) <= 1e-9 * c.obfn_f()
    assert np.array_equal(c.prox_g(V), cmod.normalise(V))
    assert c.obfn_cns() <= 1e-13
    assert c.getdict() is c.X and c.X.shape == (12, 16) and c.Yprv.shape == (12, 16)
    assert not hasattr(c, 'reconstruct')
    f = build(g, np.float32, {'MaxMainIter': 1, 'DataType': np.float64})
    assert f.dtype == np.float64 and f.X.dtype == np.float64


def test_refusals(backend):
    Z, S = np.ones((4, 8)), np.ones((6, 8))
    for bad in (Z.astype(np.float16), Z.astype(np.complex128), Z.astype(np.int32)):
        with pytest.raises(TypeError):
            cmod.CnstrMOD(bad, S.astype(bad.dtype))
    with pytest.raises(ValueError):
        cmod.CnstrMOD(np.ones((513, 8)), S)
    with pytest.raises(ValueError):
        cmod.CnstrMOD(Z, np.ones((513, 8)))
    with pytest.raises(ValueError):
        cmod.CnstrMOD(np.ones((4, 9)), S)
    with pytest.raises(ValueError):
        cmod.CnstrMOD(None, S)
    with pytest.raises(ValueError):
        cmod.WeightedCnstrMOD(Z, S, np.ones((5, 8)))
    with pytest.raises(ValueError):
        cmod.WeightedCnstrMOD(Z, S, np.ones((6, 8, 1)))
    with pytest.raises(ValueError):
        cmod.CnstrMOD(Z, S, None, cmod.CnstrMOD.Options({'ZeroMean': True, 'NonNegCoef': True}))
    with pytest.raises(NotImplementedError):
        cmod.CnstrMOD(Z, S, reducer=object())

    class Foreign(MomentumNesterov):
        pass
    with pytest.raises(NotImplementedError):
        cmod.CnstrMOD(Z, S, None, cmod.CnstrMOD.Options({'Momentum': Foreign()}))
    with pytest.raises(NotImplementedError):
        pickle.dumps(cmod.CnstrMOD(Z, S))
    with pytest.raises(ValueError):
        cmod.CnstrMOD(None, S, (4, 8)).solve()


# ---- the reference's own tests/pgm/test_cmod.py, cases 01-03 and 05-12, against this package -----------------
# (test_04 asks for float16, which is refused: test_refusals.)  The problem of every case: seed 12345, N = 16, M = 4,
# K = 8, X = randn(M, K), S = randn(N, K); dsz = (N, M) where the reference passes it (dsz[0] is read only without Z).
class TestReferenceSet01(object):

    def setup_method(self, method):
        np.random.seed(12345)
        self.N, self.M, self.K = 16, 4, 8
        self.X = np.random.randn(self.M, self.K)
        self.S = np.random.randn(self.N, self.K)

    def _solve(self, o, dsz=True, W=None):
        opt = cmod.CnstrMOD.Options(dict({'Verbose': False}, **o)) if o is not None else None
        if W is not None:
            b = cmod.WeightedCnstrMOD(self.X, self.S, W=W, dsz=(self.N, self.M), opt=opt)
        else:
            b = cmod.CnstrMOD(self.X, self.S, (self.N, self.M) if dsz else None, opt=opt)
        b.solve()
        return b

    def test_01(self, backend):
        self._solve(None)

    def test_02(self, backend):
        self._solve(None, dsz=False)

    def test_03(self, backend):
        b = self._solve({'MaxMainIter': 200, 'RelStopTol': 1e-4, 'L': 100.0})
        assert np.array(b.getitstat().Rsdl).min() < 1e-4

    @pytest.mark.parametrize('dt', [np.float32, np.float64])
    def test_05_06(self, backend, dt):
        b = self._solve({'MaxMainIter': 20, 'DataType': dt}, dsz=False)
        assert b.X.dtype == dt
        assert b.Y.dtype == dt

    def test_07(self, backend):
        b = self._solve({'MaxMainIter': 200, 'RelStopTol': 1e-4, 'L': 100.0, 'Momentum': MomentumLinear()})
        assert np.array(b.getitstat().Rsdl).min() < 1e-4

    def test_08(self, backend):
        b = self._solve({'MaxMainIter': 200, 'RelStopTol': 1e-4, 'L': 100.0, 'Momentum': MomentumGenLinear()})
        assert np.array(b.getitstat().Rsdl).min() < 1e-4

    def test_09(self, backend):
        b = self._solve({'MaxMainIter': 50, 'RelStopTol': 1e-4, 'L': 100.0, 'StepSizePolicy': StepSizePolicyBB()})
        assert np.array(b.getitstat().Rsdl).min() < 1e-4

    def test_10(self, backend):
        self._solve({'MaxMainIter': 100, 'RelStopTol': 1e-4, 'L': 10.0, 'StepSizePolicy': StepSizePolicyCauchy()})

    def test_11(self, backend):
        b = self._solve({'MaxMainIter': 500, 'RelStopTol': 1e-4, 'L': 250.0, 'Monotone': True})
        assert np.array(b.getitstat().Rsdl).min() < 2e-4

    def test_12(self, backend):
        W = np.abs(np.random.randn(self.N, self.K))
        b = self._solve({'MaxMainIter': 200, 'RelStopTol': 1e-4, 'L': 100.0}, W=W)
        assert np.array(b.getitstat().Rsdl).min() < 1e-4
