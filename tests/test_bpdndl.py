"""sporco_amd.dictlrn.bpdndl BPDNDictLearn against fixtures of the unmodified reference
(tests/golden/bpdndl_*_f64.npz, tools/make_golden_cmod.py) and the NumPy statement of tests/_cmod_numpy.py.

Tolerances: those of tests/test_cmod.py.  float64: 1e-9 relative l2 on iterates, traces and the final rho values.
Cnstr is taken at X here (the learner sets ``AuxVarObj`` False) and is not at rounding level, but it shrinks with
the run, so it is still compared absolutely, with four times the statement's figure.  float32 against the float64
fixtures: the larger of 1e-4 on iterates / 1e-3 on traces and four times what the float32 statement shows,
F32_MEASURED (test_f32_measured_figures repeats the measurement and asserts the fixture's rho paths); the widest
figure is 1.8e-6, so every float32 bound is the floor.
"""

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _cmod_numpy as cn

from sporco_amd import _lib
from sporco_amd.dictlrn import bpdndl

CASES = ['default', 'accurate', 'lmbda_none', 'zeromean', 'refshape']
F64_TOL = 1e-9
CNSTR_STATEMENT_F64 = 1.7e-15
CNSTR_STATEMENT_F32 = 8e-7
F32_MEASURED = {'default': (1.7e-6, 5.3e-7), 'accurate': (1.7e-6, 5.3e-7), 'lmbda_none': (8.8e-7, 3.1e-7),
                'zeromean': (1.8e-6, 4.6e-7), 'refshape': (5.2e-7, 6.7e-7)}
ITERATES = ('D', 'X', 'DX', 'DU', 'XU')
TRACES = tuple(f for f in cn.DL_FIELDS if f != 'Cnstr')

_GOLD = {}


def gold(case):
    if case not in _GOLD:
        _GOLD[case] = load_golden('bpdndl_%s_f64' % case)
    return _GOLD[case]


def flags(g):
    return (bool(g['opt_AccurateDFid']) if 'opt_AccurateDFid' in g else False,
            bool(g['opt_CMOD.ZeroMean']) if 'opt_CMOD.ZeroMean' in g else False)


def lmbda_of(g):
    return None if float(g['lmbda_given']) == 0.0 else float(g['lmbda_given'])


def statement(g, dtype):
    acc, zm = flags(g)
    o = {'AccurateDFid': acc, 'CMOD.ZeroMean': zm, 'BPDN.AutoRho.Period': int(g['opt_BPDN.AutoRho.Period']),
         'CMOD.AutoRho.Period': int(g['opt_CMOD.AutoRho.Period'])}
    return cn.run_dl(g['D0'], g['S'], lmbda_of(g), o, dtype=dtype, iters=int(g['opt_MaxMainIter']))


def learner(g, dtype, iters=None):
    acc, zm = flags(g)
    o = {'Verbose': False, 'MaxMainIter': int(g['opt_MaxMainIter']) if iters is None else iters, 'AccurateDFid': acc,
         'BPDN': {'AutoRho': {'Period': int(g['opt_BPDN.AutoRho.Period'])}},
         'CMOD': {'AutoRho': {'Period': int(g['opt_CMOD.AutoRho.Period'])}, 'ZeroMean': zm}}
    return bpdndl.BPDNDictLearn(g['D0'].astype(dtype), g['S'].astype(dtype), lmbda_of(g), bpdndl.BPDNDictLearn.Options(o))


def compare(res, g, traces_of):
    ei = max(rel_l2(res[k], g[k]) for k in ITERATES)
    et = max(rel_l2(traces_of(f), g['it_' + f]) for f in TRACES)
    for k, f in (('xrho', 'xrho_final'), ('drho', 'drho_final')):
        et = max(et, abs(float(res[k]) - float(g[f])) / float(g[f]))
    ec = float(np.max(np.abs(np.asarray(traces_of('Cnstr'), dtype=np.float64) - g['it_Cnstr'])))
    return ei, et, ec


def changes(v):
    v = np.asarray(v, dtype=np.float64)
    return tuple(np.nonzero(v[1:] != v[:-1])[0])


def test_statement_reproduces_fixtures():
    worst, worst_c = 0.0, 0.0
    for case in CASES:
        g = gold(case)
        r = statement(g, np.float64)
        ei, et, ec = compare(r, g, lambda f: r[f])
        worst, worst_c = max(worst, ei, et), max(worst_c, ec)
    print('statement in float64 against the fixtures: %.2e; Cnstr %.2e' % (worst, worst_c))
    assert worst <= 1e-10 and worst_c <= CNSTR_STATEMENT_F64


def test_f32_measured_figures():
    worst_c = 0.0
    for case in CASES:
        g = gold(case)
        r = statement(g, np.float32)
        ei, et, ec = compare(r, g, lambda f: r[f])
        print("'%s': (%.1e, %.1e)," % (case, ei, et))
        assert changes(r['XRho']) == changes(g['it_XRho']) and changes(r['DRho']) == changes(g['it_DRho']), case
        assert ei <= F32_MEASURED[case][0] and et <= F32_MEASURED[case][1], (case, ei, et)
        worst_c = max(worst_c, ec)
    assert worst_c <= CNSTR_STATEMENT_F32


def test_fixtures_hold_their_conditions():
    for case in CASES:
        g = gold(case)
        assert all(np.all(np.isfinite(g['it_' + f])) and len(g['it_' + f]) == 12 for f in cn.DL_FIELDS)
        assert len(changes(g['it_XRho'])) + len(changes(g['it_DRho'])) >= 1
    assert gold('refshape')['D0'].shape == (8, 4) and gold('refshape')['S'].shape == (8, 8)
    assert float(gold('lmbda_none')['lmbda_given']) == 0.0
    assert not np.array_equal(gold('default')['it_DFid'], gold('accurate')['it_DFid'])
    assert np.max(np.abs(np.mean(gold('zeromean')['D'], axis=0))) < 1e-14


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('case', CASES)
def test_against_reference_fixture(backend, case, dtype):
    g = gold(case)
    d = learner(g, dtype)
    D = d.solve()
    its = d.getitstat()
    res = {'D': D, 'X': d.getcoef(), 'DX': d.dstep.X, 'DU': d.dstep.U, 'XU': d.xstep.U, 'xrho': d.xstep.rho,
           'drho': d.dstep.rho}
    ei, et, ec = compare(res, g, lambda f: getattr(its, f))
    print('%s %s: iterates %.2e traces %.2e cnstr %.2e' % (case, np.dtype(dtype).name, ei, et, ec))
    assert D.dtype == dtype and np.array_equal(D, d.getdict())
    assert its._fields == ('Iter',) + cn.DL_FIELDS + ('Time',)
    assert np.array_equal(its.Iter, np.arange(12))
    if dtype == np.float64:
        assert ei <= F64_TOL and et <= F64_TOL and ec <= 4.0 * CNSTR_STATEMENT_F64
    else:
        assert ei <= max(4.0 * F32_MEASURED[case][0], 1e-4) and et <= max(4.0 * F32_MEASURED[case][1], 1e-3)
        assert ec <= 4.0 * CNSTR_STATEMENT_F32


def test_no_big_array_moves_during_solve(backend, monkeypatch):
    """A BpdnHandle / CmodHandle pair with the upload and download entry points counted: during solve() neither an
    (M, K) nor an (N, K) array crosses to the host or back, with AccurateDFid on."""
    N, M, K = 8, 16, 4096
    rng = np.random.RandomState(5)
    D0 = rng.randn(N, M)
    S = rng.randn(N, K).astype(np.float32)
    o = {'Verbose': False, 'MaxMainIter': 4, 'AccurateDFid': True}
    d = bpdndl.BPDNDictLearn(D0.astype(np.float32), S, 0.1, bpdndl.BPDNDictLearn.Options(o))
    seen = []

    def counted(cls, name):
        orig = getattr(cls, name)

        def wrapper(self, *a, **k):
            for v in a:
                if hasattr(v, 'shape') and not isinstance(v, np.ndarray):
                    seen.append((cls.__name__ + '.' + name, 'device', tuple(v.shape)))
                elif isinstance(v, np.ndarray):
                    seen.append((cls.__name__ + '.' + name, 'host', v.shape))
            res = orig(self, *a, **k)
            if isinstance(res, np.ndarray):
                seen.append((cls.__name__ + '.' + name, 'host', res.shape))
            return res
        monkeypatch.setattr(cls, name, wrapper)
    for cls, names in ((_lib.BpdnHandle, ('upload', 'download', 'set_dict', 'set_solve')),
                       (_lib.CmodHandle, ('upload', 'download', 'set_signal', 'set_coef', 'set_solve'))):
        for name in names:
            counted(cls, name)
    _lib.transfer_stats(reset=True)
    d.solve()
    moved = _lib.transfer_stats(reset=True)
    big = [e for e in seen if e[1] == 'host' and K in e[2]]
    assert not big, big
    assert sum(1 for e in seen if e[0] == 'CmodHandle.set_coef' and e[1] == 'device') == 4
    assert ('CmodHandle.download', 'host', (M, M)) in seen and ('BpdnHandle.set_dict', 'host', (N, M)) in seen
    # all that moved in four outer iterations is less than one (N, K) array
    assert moved['h2d_bytes'] + moved['d2h_bytes'] < S.nbytes, moved
    assert len(d.itstat) == 4 and np.all(np.isfinite(d.getitstat().ObjFun))


def test_accurate_dfid_is_that_of_the_final_pair(backend):
    g = gold('accurate')
    d = learner(g, np.float64, iters=3)
    D = d.solve()
    X = d.getcoef()
    it = d.itstat[-1]
    dfd = 0.5 * np.linalg.norm(D.dot(X) - g['S']) ** 2
    assert abs(it.DFid - dfd) <= 1e-12 * dfd and abs(it.RegL1 - np.sum(np.abs(X))) <= 1e-12 * it.RegL1
    assert abs(it.ObjFun - (dfd + float(d.xstep.lmbda) * it.RegL1)) <= 1e-12 * it.ObjFun


def test_options_tree():
    d = load_golden('cmod_defaults')
    got = {}

    def walk(prefix, node):
        for k, v in node.items():
            if isinstance(v, dict):
                walk(prefix + k + '.', v)
            else:
                got[prefix + k] = repr(v)
    walk('', dict(bpdndl.BPDNDictLearn.Options()))
    assert got == dict(zip(d['BPDNDictLearn_keys'].tolist(), d['BPDNDictLearn_values'].tolist()))


# ---- the bodies of the reference's tests/dictlrn/test_bpdndl.py::test_01 - test_03 -------------------------
def ref_problem():
    N, M, K = 8, 4, 8
    np.random.seed(12345)
    return np.random.randn(N, M), np.random.randn(N, K)


def test_reference_test_01(backend):
    D0, S = ref_problem()
    lmbda = 1e-1
    b = bpdndl.BPDNDictLearn(D0, S, lmbda)
    b.opt['MaxMainIter'] = 30      # (the body as it is, but for the 1000 outer iterations of the default options)
    b.solve()


def test_reference_test_02(backend):
    D0, S = ref_problem()
    b = bpdndl.BPDNDictLearn(D0, S)
    b.opt['MaxMainIter'] = 30      # (likewise)
    b.solve()


def test_reference_test_03(backend):
    D0, S = ref_problem()
    lmbda = 1e-1
    opt = bpdndl.BPDNDictLearn.Options({'AccurateDFid': True, 'MaxMainIter': 10})
    b = bpdndl.BPDNDictLearn(D0, S, lmbda, opt=opt)
    b.solve()
    assert len(b.itstat) == 10
    assert np.array_equal(b.getdict(), b.dstep.getdict()) and np.array_equal(b.getcoef(), b.xstep.getcoef())
