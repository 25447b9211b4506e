"""sporco_amd.dictlrn.wbpdndl WeightedBPDNDictLearn against fixtures of the unmodified reference
(tests/golden/wbpdndl_*_f64.npz, tools/make_golden_pgm_cmod.py) and against the NumPy statement ``learn`` of
tests/_pgm_cmod_numpy.py.

Tolerances as tests/test_pgm_cmod.py: the statement against the fixtures 1e-10; the package in float64 1e-9 relative
l2 on the dictionary, the coefficients and every outer trace; float32 input against the float64 fixture 1e-4 on the
iterates and 1e-3 on the traces, or four times what the float32 statement shows against the same fixture, whichever
is larger, per case (F32_MEASURED, measured again by test_f32_measured_figures).  Cnstr sits at rounding level and is
compared absolutely: 1e-13 in float64, four times the statement's figure in float32.
"""

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _pgm_cmod_numpy as pn

from sporco_amd import _lib
from sporco_amd.dictlrn import wbpdndl
from sporco_amd.pgm import cmod

CASES = ['default', 'fast', 'w_mask', 'accurate', 'lmbda_none', 'zeromean', 'ref_shape']
F64_TOL = 1e-9
STATEMENT_TOL = 1e-10
CNSTR_F64 = 1e-13
TRACES = tuple(f for f in pn.LEARN_FIELDS if f != 'Cnstr')
# case: (D and X, traces, Cnstr absolute) of the float32 statement against the float64 fixture
F32_MEASURED = {'default': (4.0e-07, 3.1e-06, 3.4e-07), 'fast': (3.3e-07, 3.1e-07, 3.9e-07),
                'w_mask': (3.7e-07, 3.5e-07, 3.6e-07), 'accurate': (3.7e-07, 3.5e-07, 3.6e-07),
                'lmbda_none': (4.3e-07, 2.4e-07, 3.2e-07), 'zeromean': (4.3e-07, 3.5e-07, 3.4e-07),
                'ref_shape': (2.5e-07, 7.8e-07, 1.9e-07)}

_GOLD = {}


def gold(case):
    if case not in _GOLD:
        _GOLD[case] = load_golden('wbpdndl_%s_f64' % case)
    return _GOLD[case]


def inner_opts(g, tag):
    o = {}
    for k in g:
        if k.startswith(tag):
            v = float(g[k])
            o[k[len(tag):]] = bool(v) if k[len(tag):] in ('ZeroMean', 'NonNegCoef') else v
    return o


def args_of(g, dtype):
    lm = None if float(g['lmbda_given']) == 0.0 else float(g['lmbda_given'])
    W = g['W'].astype(dtype) if 'W' in g else None
    return g['D0'].astype(dtype), g['S'].astype(dtype), lm, W


def build(g, dtype, extra=None):
    D0, S, lm, W = args_of(g, dtype)
    o = {'Verbose': False, 'MaxMainIter': int(g['iters']), 'AccurateDFid': bool(float(g['accurate'])),
         'BPDN': inner_opts(g, 'xopt_'), 'CMOD': inner_opts(g, 'dopt_')}
    o.update(extra or {})
    return wbpdndl.WeightedBPDNDictLearn(D0, S, lm, W=W, opt=wbpdndl.WeightedBPDNDictLearn.Options(o))


def statement(g, dtype):
    D0, S, lm, W = args_of(g, np.float64)
    return pn.learn(D0, S, lm, int(g['iters']), W=W, accurate=bool(float(g['accurate'])), xo=inner_opts(g, 'xopt_'),
                    do=inner_opts(g, 'dopt_'), dtype=dtype)


def compare(D, X, traces_of, g):
    ei = max(rel_l2(D, g['D']), rel_l2(X, g['X']))
    et = max(rel_l2(traces_of(f), g['it_' + f]) for f in TRACES)
    ec = float(np.max(np.abs(np.asarray(traces_of('Cnstr')) - g['it_Cnstr'])))
    return ei, et, ec


def solved(d):
    d.solve()
    its = d.getitstat()
    return d.getdict(), d.getcoef(), (lambda f: np.asarray(getattr(its, f), dtype=np.float64))


def test_statement_reproduces_fixtures():
    for case in CASES:
        g = gold(case)
        r = statement(g, np.float64)
        ei, et, ec = compare(r['D'], r['X'], lambda f: r[f], g)
        assert ei <= STATEMENT_TOL and et <= STATEMENT_TOL and ec <= CNSTR_F64, (case, ei, et, ec)


def test_f32_measured_figures():
    for case in CASES:
        g = gold(case)
        r = statement(g, np.float32)
        ei, et, ec = compare(r['D'], r['X'], lambda f: r[f], g)
        print("'%s': (%.1e, %.1e, %.1e)," % (case, ei, et, ec))
        m = F32_MEASURED[case]
        assert ei <= m[0] and et <= m[1] and ec <= m[2], (case, ei, et, ec)


def test_fixtures_hold_their_conditions():
    for case in CASES:
        g = gold(case)
        N, K = g['S'].shape
        M = g['D0'].shape[1]
        assert 8 <= N <= 24 and 4 <= M <= 32 and 8 <= K <= 100 and 12 <= int(g['iters']) <= 30, case
    assert gold('ref_shape')['D0'].shape == (8, 4) and gold('ref_shape')['S'].shape == (8, 8)
    assert gold('w_mask')['W'].shape == gold('w_mask')['S'].shape and np.any(gold('w_mask')['W'] == 0)
    assert float(gold('accurate')['accurate']) == 1.0 and float(gold('lmbda_none')['lmbda_given']) == 0.0
    assert float(gold('zeromean')['dopt_ZeroMean']) == 1.0


@pytest.mark.parametrize('case', CASES)
def test_f64_parity(backend, case):
    g = gold(case)
    D, X, tr = solved(build(g, np.float64))
    ei, et, ec = compare(D, X, tr, g)
    print('%s: iterates %.2e traces %.2e Cnstr %.2e' % (case, ei, et, ec))
    assert ei <= F64_TOL and et <= F64_TOL and ec <= CNSTR_F64, (case, ei, et, ec)


@pytest.mark.parametrize('case', CASES)
def test_f32_parity(backend, case):
    g = gold(case)
    D, X, tr = solved(build(g, np.float32))
    assert D.dtype == np.float32 and X.dtype == np.float32
    ei, et, ec = compare(D, X, tr, g)
    mi, mt, mc = F32_MEASURED[case]
    ti, tt, tc = max(4.0 * mi, 1e-4), max(4.0 * mt, 1e-3), 4.0 * mc
    print('%s: iterates %.2e (%.1e) traces %.2e (%.1e) Cnstr %.2e (%.1e)' % (case, ei, ti, et, tt, ec, tc))
    assert ei <= ti and et <= tt and ec <= tc, (case, ei, et, ec)


def test_no_big_array_moves_during_solve(backend, monkeypatch):
    """The two handles with their upload and download entry points counted: during solve() neither an (M, K) nor an
    (N, K) array crosses to the host or back, with a mask W and AccurateDFid on."""
    N, M, K = 8, 16, 4096
    rng = np.random.RandomState(5)
    D0 = rng.randn(N, M).astype(np.float32)
    S = rng.randn(N, K).astype(np.float32)
    W = (rng.rand(N, K) >= 0.3).astype(np.float32)
    o = {'Verbose': False, 'MaxMainIter': 4, 'AccurateDFid': True, 'BPDN': {'L': 20.0}, 'CMOD': {'L': 2000.0}}
    d = wbpdndl.WeightedBPDNDictLearn(D0, S, 0.1, W=W, opt=wbpdndl.WeightedBPDNDictLearn.Options(o))
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
    for cls, names in ((_lib.BpdnHandle, ('upload', 'download', 'set_dict')),
                       (_lib.CmodHandle, ('upload', 'download', 'set_signal', 'set_coef')),
                       (_lib.PgmCmodHandle, ('set_weight',))):
        for name in names:
            counted(cls, name)
    _lib.transfer_stats(reset=True)
    d.solve()
    moved = _lib.transfer_stats(reset=True)
    big = [e for e in seen if e[1] == 'host' and K in e[2]]
    assert not big, big
    assert sum(1 for e in seen if e[0] == 'CmodHandle.set_coef' and e[1] == 'device') == 4
    assert ('CmodHandle.download', 'host', (N, M)) in seen and ('BpdnHandle.set_dict', 'host', (N, M)) in seen
    # all that moved in four outer iterations is less than one (N, K) array
    assert moved['h2d_bytes'] + moved['d2h_bytes'] < S.nbytes, moved
    assert len(d.itstat) == 4 and np.all(np.isfinite(d.getitstat().ObjFun))
    # the D step read the x step's current X buffer: its data fidelity is that of the final pair
    X, D = d.getcoef(), d.getdict()
    dfd = 0.5 * np.sum(W.astype(np.float64) * (D.astype(np.float64).dot(X) - S) ** 2)
    assert abs(d.itstat[-1].DFid - dfd) <= 1e-4 * dfd


def test_options_and_stats_fields(backend):
    o = wbpdndl.WeightedBPDNDictLearn.Options()
    assert o['AccurateDFid'] is False and o['BPDN', 'MaxMainIter'] == 1 and o['CMOD', 'MaxMainIter'] == 1
    assert o['BPDN', 'L'] == 500.0 and o['CMOD', 'L'] == 500.0 and o['MaxMainIter'] == 1000
    g = gold('ref_shape')
    d = build(g, np.float64, {'MaxMainIter': 2})
    d.solve()
    assert d.itstat[-1]._fields == ('Iter', 'ObjFun', 'DFid', 'RegL1', 'Cnstr', 'XRsdl', 'XL', 'DRsdl', 'DL', 'Time')
    assert np.allclose(np.sum(d.getdict() ** 2, 0), 1.0)
    d.solve()
    assert [s.Iter for s in d.itstat] == [0, 1, 2, 3]


def test_evaluate_downloads_where_the_sum_is_not_the_l1_norm(backend):
    g = gold('accurate')
    wl1 = 1.0 + np.random.RandomState(3).rand(g['D0'].shape[1], 1)
    d = build(g, np.float64, {'MaxMainIter': 3, 'BPDN': dict(inner_opts(g, 'xopt_'), L1Weight=wl1)})
    d.solve()
    X, D = d.getcoef(), d.getdict()
    assert abs(d.itstat[-1].RegL1 - np.sum(np.abs(X))) <= 1e-12 * np.sum(np.abs(X))
    dfd = 0.5 * np.sum(g['W'] * (D.dot(X) - g['S']) ** 2)
    assert abs(d.itstat[-1].DFid - dfd) <= 1e-9 * dfd


# ---- the reference's own tests/dictlrn/test_wbpdndl.py, cases 01-03, against this package ---------------------
class TestReferenceSet01(object):

    def setup_method(self, method):
        N, M, K = 8, 4, 8
        rng = np.random.RandomState(12345)
        self.D0 = rng.randn(N, M)
        self.S = rng.randn(N, K)
        self.W = np.abs(rng.randn(N, K))

    def test_01(self, backend):
        opt = wbpdndl.WeightedBPDNDictLearn.Options({'MaxMainIter': 50})
        wbpdndl.WeightedBPDNDictLearn(self.D0, self.S, 1e-1, opt=opt).solve()

    def test_02(self, backend):
        opt = wbpdndl.WeightedBPDNDictLearn.Options({'MaxMainIter': 50})
        wbpdndl.WeightedBPDNDictLearn(self.D0, self.S, 1e-1, W=self.W, opt=opt).solve()

    def test_03(self, backend):
        opt = wbpdndl.WeightedBPDNDictLearn.Options({'AccurateDFid': True, 'MaxMainIter': 10})
        b = wbpdndl.WeightedBPDNDictLearn(self.D0, self.S, 1e-1, W=self.W, opt=opt)
        b.solve()
        assert len(b.itstat) == 10 and np.all(np.isfinite([s.ObjFun for s in b.itstat]))


def test_masked_recovery(backend):
    """A planted dictionary, 30 % of the samples masked out: the masked data fidelity falls at every one of 20 outer
    iterations.  Both inner L lie above the Lipschitz constants of their gradients (|| D^T D || <= M for unit-norm
    columns; || Z Z^T || measured on the planted code, doubled), so every inner step majorises."""
    rng = np.random.RandomState(7)
    N, M, K = 16, 24, 100
    Dp = cmod.normalise(rng.randn(N, M))
    Xp = np.zeros((M, K))
    for k in range(K):
        Xp[rng.permutation(M)[:3], k] = rng.randn(3)
    S = Dp.dot(Xp) + 0.01 * rng.randn(N, K)
    W = (rng.rand(N, K) >= 0.3).astype(np.float64)
    Ld = 2.0 * float(np.linalg.norm(Xp.dot(Xp.T), 2))
    opt = wbpdndl.WeightedBPDNDictLearn.Options({'MaxMainIter': 20, 'AccurateDFid': True, 'BPDN': {'L': float(M)},
                                                 'CMOD': {'L': Ld}})
    d = wbpdndl.WeightedBPDNDictLearn(Dp + 0.3 * rng.randn(N, M), S, 0.05, W=W, opt=opt)
    d.solve()
    dfd = np.asarray(d.getitstat().DFid)
    print(dfd)
    assert len(dfd) == 20 and np.all(np.diff(dfd) < 0), dfd
    X, D = d.getcoef(), d.getdict()
    assert abs(dfd[-1] - 0.5 * np.sum(W * (D.dot(X) - S) ** 2)) <= 1e-9 * dfd[-1]
