#!/usr/bin/env python3
"""Generate the pgm.bpdn BPDN / WeightedBPDN fixtures tests/golden/pgm_bpdn_*_f64.npz from the UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at $SPORCO_REFERENCE
(default /root/reference) with the import stand-ins of oracle/_stubs, exactly as tools/make_golden_bpdn.py does.
Nothing here is read by the test-suite; the tests read the .npz files alone.

    python tools/make_golden_pgm_bpdn.py [CASE ...]

Each file holds the seeded inputs (D, S, W where given), the options as flat keys (`opt_*`; arrays `optarr_*`; the
rule objects as `rule_Momentum`, `rule_StepSizePolicy`, `rule_Backtrack` with their parameters `rule_<Rule>.<name>`),
the class name, lmbda as given (`lmbda_given` = 0: `lmbda=None`) and as used, the final X, Y and L, the iterations
at which Monotone reverted (`reverts`, seen through a callback) and at which the Barzilai-Borwein rule fell back
(`bb_fallbacks`), and every IterationStats column but Time (`it_*`; the backtracking columns where they are not None)
of a float64 run of ITERS iterations with RelStopTol = 0.

The problem: as tools/make_golden_bpdn.py -- seed 11 (a case may name another), D = randn(N, M) with unit-norm
columns, a sparse code of three non-zeros a column, S = D X0 + 0.05 randn, then the optional X0 (0.1 randn), L1Weight
(1 + rand of its shape), W (0.5 + rand of its shape) and D2 (the `setdict` case).  8 x 16 x 5 unless the case says
otherwise.

Asserted per case, with the NumPy statement of tests/_pgm_bpdn_numpy.py: the float64 statement reproduces the run
to 1e-10; the float32 statement takes the same discrete path (IterBTrack, reverts, bb_fallbacks).  A case that
fails the second condition gets another seed here, not an excuse in the tests.  pgm_bpdn_step_f64.npz holds the
`bt_standard` problem's state after STEP_K iterations and the scalars of the next one; pgm_bpdn_recover_f64.npz the
reference's tests/pgm/test_bpdn.py::TestSet01::test_09; pgm_bpdn_defaults.npz the option defaults, key by key.
"""

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.environ.get('SPORCO_REFERENCE', '/root/reference'))
sys.path.insert(0, os.path.join(REPO, 'oracle', '_stubs'))
sys.path.insert(0, os.path.join(REPO, 'tests'))
warnings.filterwarnings('ignore')

from sporco.pgm import bpdn as ref                                              # noqa: E402
from sporco.pgm.momentum import MomentumNesterov, MomentumLinear, MomentumGenLinear    # noqa: E402
from sporco.pgm.stepsize import StepSizePolicyBB, StepSizePolicyCauchy         # noqa: E402
from sporco.pgm.backtrack import BacktrackStandard, BacktrackRobust            # noqa: E402
import _pgm_bpdn_numpy as pn                                                    # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
ITERS = 30
STEP_K = 2
LMBDA = 0.1

# name: (class, (N, M, K), lmbda, options, rules, extras, seed)
CASES = {
    'default': ('BPDN', (8, 16, 5), LMBDA, {}, {}, (), 11),
    'l2': ('BPDN', (8, 16, 5), LMBDA, {'L': 5.0}, {}, (), 11),
    'lmbda_none': ('BPDN', (8, 16, 5), None, {'L': 5.0}, {}, (), 11),
    'nonneg': ('BPDN', (8, 16, 5), LMBDA, {'L': 5.0, 'NonNegCoef': True}, {}, (), 11),
    'w_atom': ('BPDN', (8, 16, 5), LMBDA, {'L': 5.0}, {}, ('W_M1',), 11),
    'w_signal': ('BPDN', (8, 16, 5), LMBDA, {'L': 5.0}, {}, ('W_1K',), 11),
    'w_full': ('BPDN', (8, 16, 5), LMBDA, {'L': 5.0}, {}, ('W_MK',), 11),
    'x0': ('BPDN', (8, 16, 5), LMBDA, {'L': 5.0}, {}, ('X0',), 11),
    'k1': ('BPDN', (8, 16, 1), LMBDA, {'L': 5.0}, {}, (), 11),
    'tall': ('BPDN', (24, 16, 5), LMBDA, {'L': 4.0}, {}, (), 11),
    'square': ('BPDN', (8, 8, 5), LMBDA, {'L': 5.0}, {}, (), 11),
    'bt_standard': ('BPDN', (8, 16, 5), LMBDA, {'L': 0.1}, {'Backtrack': ('standard', {})}, (), 11),
    'bt_robust': ('BPDN', (8, 16, 5), LMBDA, {'L': 0.1}, {'Backtrack': ('robust', {})}, (), 11),
    'mom_nesterov': ('BPDN', (8, 16, 5), LMBDA, {'L': 3.0}, {'Momentum': ('nesterov', {})}, (), 11),
    'mom_linear': ('BPDN', (8, 16, 5), LMBDA, {'L': 5.0}, {'Momentum': ('linear', {'b': 3.0})}, (), 11),
    'mom_genlinear': ('BPDN', (8, 16, 5), LMBDA, {'L': 5.0}, {'Momentum': ('genlinear', {'a': 40.0, 'b': 2.5})}, (), 11),
    'cauchy': ('BPDN', (8, 16, 5), LMBDA, {'L': 5.0}, {'StepSizePolicy': ('cauchy', {})}, (), 11),
    'bb': ('BPDN', (8, 16, 5), LMBDA, {'L': 5.0}, {'StepSizePolicy': ('bb', {})}, (), 11),
    'monotone': ('BPDN', (8, 16, 5), LMBDA, {'L': 200.0, 'Monotone': True}, {}, (), 11),
    'monotone_l1': ('BPDN', (8, 16, 5), LMBDA, {'L': 2.5, 'Monotone': True}, {}, (), 11),
    'autostop': ('BPDN', (8, 16, 5), LMBDA, {'L': 5.0, 'AutoStop': {'Enabled': True, 'Tau0': 1.0}}, {}, (), 11),
    'wt_scalar': ('WeightedBPDN', (8, 16, 5), LMBDA, {'L': 6.0}, {}, ('Wd_0',), 11),
    'wt_n': ('WeightedBPDN', (8, 16, 5), LMBDA, {'L': 6.0}, {}, ('Wd_N',), 11),
    'wt_n1': ('WeightedBPDN', (8, 16, 5), LMBDA, {'L': 6.0}, {}, ('Wd_N1',), 11),
    'wt_1k': ('WeightedBPDN', (8, 16, 5), LMBDA, {'L': 6.0}, {}, ('Wd_1K',), 11),
    'wt_nk': ('WeightedBPDN', (8, 16, 5), LMBDA, {'L': 6.0}, {}, ('Wd_NK',), 11),
    'wt_nk_standard': ('WeightedBPDN', (8, 16, 5), LMBDA, {'L': 0.1}, {'Backtrack': ('standard', {'gamma_u': 1.3})},
                       ('Wd_NK',), 11),
    'wt_n1_robust': ('WeightedBPDN', (8, 16, 5), LMBDA, {'L': 0.1},
                     {'Backtrack': ('robust', {'gamma_d': 0.95, 'maxiter': 20})}, ('Wd_N1',), 11),
    'setdict': ('BPDN', (8, 16, 5), LMBDA, {'L': 5.0}, {}, ('D2',), 11),
}

RULES = {'nesterov': MomentumNesterov, 'linear': MomentumLinear, 'genlinear': MomentumGenLinear,
         'cauchy': StepSizePolicyCauchy, 'bb': StepSizePolicyBB, 'standard': BacktrackStandard,
         'robust': BacktrackRobust}
RULE_DEFAULTS = {'linear': {'b': 2.0}, 'genlinear': {'a': 50.0, 'b': 2.0}, 'standard': {'gamma_u': 1.2, 'maxiter': 50},
                 'robust': {'gamma_d': 0.9, 'gamma_u': 2.0, 'maxiter': 50}}


def problem(dims, extras, seed):
    N, M, K = dims
    rng = np.random.RandomState(seed)
    D = rng.randn(N, M)
    D /= np.sqrt(np.sum(D ** 2, axis=0, keepdims=True))
    X0 = np.zeros((M, K))
    for k in range(K):
        X0[rng.permutation(M)[:min(3, M)], k] = rng.randn(min(3, M))
    S = D.dot(X0) + 0.05 * rng.randn(N, K)
    arrs = {}
    if 'X0' in extras:
        arrs['X0'] = 0.1 * rng.randn(M, K)
    for tag, shp in (('W_M1', (M, 1)), ('W_1K', (1, K)), ('W_MK', (M, K))):
        if tag in extras:
            arrs['L1Weight'] = 1.0 + rng.rand(*shp)
    for tag, shp in (('Wd_0', ()), ('Wd_N', (N,)), ('Wd_N1', (N, 1)), ('Wd_1K', (1, K)), ('Wd_NK', (N, K))):
        if tag in extras:
            arrs['W'] = np.asarray(0.5 + rng.rand(*shp))
    if 'D2' in extras:
        D2 = rng.randn(N, M)
        arrs['D2'] = D2 / np.sqrt(np.sum(D2 ** 2, axis=0, keepdims=True))
    return D, S, arrs


def flat(od, rules, iters):
    """The options and rules as the flat dict of tests/_pgm_bpdn_numpy.py (arrays apart)."""
    o = {'MaxMainIter': iters, 'RelStopTol': 0.0, 'L': 500.0}
    for k, v in od.items():
        if isinstance(v, dict):
            for kk, vv in v.items():
                o['%s.%s' % (k, kk)] = vv
        else:
            o[k] = v
    for slot, (kind, par) in rules.items():
        o[slot] = kind
        full = dict(RULE_DEFAULTS.get(kind, {}))
        full.update(par)
        for kk, vv in full.items():
            o['%s.%s' % (slot, kk)] = vv
    return o


def build(cls, D, S, lmbda, od, rules, arrs, iters, reverts):
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0}
    o.update(od)
    for slot, (kind, par) in rules.items():
        o[slot] = RULES[kind](**par)
    for k in ('X0', 'L1Weight'):
        if k in arrs:
            o[k] = arrs[k]

    def cb(obj):
        # (a revert hands the previous tuple on: pgm.py:416-420)
        if obj.opt['Monotone'] and obj.k > 0 and obj.objfn is obj.objfn_prev:
            reverts.append(int(obj.k))
        return False
    o['Callback'] = cb
    c = getattr(ref, cls)
    if cls == 'BPDN':
        return c(D, S, lmbda, c.Options(o))
    return c(D, S, lmbda, arrs.get('W'), c.Options(o))


def traces(b, name):
    out = {}
    its = b.getitstat()
    for f in its._fields:
        col = getattr(its, f)
        if f == 'Time' or col[0] is None:
            continue
        v = np.asarray(col, dtype=np.float64)
        assert np.all(np.isfinite(v)), (name, f)
        out['it_' + f] = v
    return out


def bb_fallbacks(L):
    return [k for k in range(2, len(L)) if L[k] == L[k - 1]]


def check_statement(name, D, S, lmbda, o, arrs, out, state_runs=None):
    """The float64 statement reproduces the run; the float32 statement takes its discrete path."""
    oo = dict(o)
    for k in ('X0', 'L1Weight'):
        if k in arrs:
            oo[k] = arrs[k]
    for dtype in (np.float64, np.float32):
        if state_runs is None:
            r = pn.run(D, S, lmbda, oo, W=arrs.get('W'), dtype=dtype)
        else:
            r = state_runs(dtype, oo)
        if dtype == np.float64:
            for f in ('X', 'Y'):
                e = np.linalg.norm(r[f] - out[f]) / max(np.linalg.norm(out[f]), 1e-300)
                assert e <= 1e-10, (name, f, e)
            for f in pn.FIELDS:
                if 'it_' + f in out:
                    e = np.linalg.norm(r[f] - out['it_' + f]) / max(np.linalg.norm(out['it_' + f]), 1e-300)
                    assert e <= 1e-10, (name, f, e)
        if 'it_IterBTrack' in out:
            assert np.array_equal(np.asarray(r['IterBTrack']), out['it_IterBTrack']), (name, dtype, 'IterBTrack')
        assert list(r['reverts']) == list(out['reverts']), (name, dtype, r['reverts'], out['reverts'])
        if o.get('StepSizePolicy') == 'bb':
            assert list(r['bb_fallbacks']) == list(out['bb_fallbacks']), (name, dtype, r['bb_fallbacks'])
        assert len(r['ObjFun']) == len(out['it_ObjFun']), (name, dtype, 'iterations')


def record(name, cls, D, S, lmbda, od, rules, arrs, b, reverts, extra=None, iters=ITERS):
    out = traces(b, name)
    o = flat(od, rules, iters)
    for k, v in o.items():
        if isinstance(v, str):
            out['rule_' + k] = np.array(v)
        elif k.split('.')[0] in ('Momentum', 'StepSizePolicy', 'Backtrack'):
            out['rule_' + k] = np.float64(v)
        else:
            out['opt_' + k] = np.float64(v)
    out.update(D=D, S=S, cls=np.array(cls), lmbda_given=np.float64(0.0 if lmbda is None else lmbda),
               lmbda=np.float64(b.lmbda), X=np.array(b.X), Y=np.array(b.Y), Lfinal=np.float64(b.L),
               reverts=np.asarray(reverts, dtype=np.int64),
               bb_fallbacks=np.asarray(bb_fallbacks(out['it_L']) if 'StepSizePolicy' in rules else [], dtype=np.int64),
               zero_share=np.float64(np.mean(np.asarray(b.X) == 0)))
    for k, v in arrs.items():
        out['optarr_' + k] = np.asarray(v)
    out.update(extra or {})
    path = os.path.join(OUT, 'pgm_bpdn_%s_f64.npz' % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 100000, (name, size)
    print('%-34s %5.1f KB  zeros %.2f  ObjFun[-1] = %.6f  L %.4g  btrack %s reverts %s fallbacks %s'
          % (os.path.basename(path), size / 1024.0, out['zero_share'], out['it_ObjFun'][-1], out['Lfinal'],
             sorted(set(out['it_IterBTrack'].astype(int))) if 'it_IterBTrack' in out else '-', list(reverts),
             list(out['bb_fallbacks'])))
    return out, o


def defaults():
    out = {}
    for cls in ('BPDN', 'WeightedBPDN'):
        d = getattr(ref, cls).Options().__class__.defaults
        keys, vals = [], []
        for k, v in sorted(d.items()):
            if isinstance(v, dict):
                for kk, vv in sorted(v.items()):
                    keys.append('%s.%s' % (k, kk))
                    vals.append(repr(vv))
            else:
                keys.append(k)
                vals.append(type(v).__name__ if k in ('Momentum', 'StepSizePolicy', 'Backtrack') else repr(v))
        out[cls + '_keys'] = np.array(keys)
        out[cls + '_values'] = np.array(vals)
        out[cls + '_fields'] = np.array(getattr(ref, cls).IterationStats._fields)
        out[cls + '_hdrtxt'] = np.array(getattr(ref, cls).hdrtxt())
        hv = getattr(ref, cls).hdrval()
        out[cls + '_hdrval'] = np.array([hv[h] for h in getattr(ref, cls).hdrtxt()])
    np.savez_compressed(os.path.join(OUT, 'pgm_bpdn_defaults.npz'), **out)
    print('pgm_bpdn_defaults.npz  %d keys' % len(out['BPDN_keys']))


def recover():
    """tests/pgm/test_bpdn.py::TestSet01::test_09 of the reference, its inputs and what it asserts."""
    N, M, L = 64, 128, 4
    np.random.seed(12345)
    D = np.random.randn(N, M)
    x0 = np.zeros((M, 1))
    si = np.random.permutation(list(range(0, M - 1)))
    x0[si[0:L]] = np.random.randn(L, 1)
    s0 = D.dot(x0)
    lmbda = 5e-3
    opt = ref.BPDN.Options({'Verbose': False, 'MaxMainIter': 1000, 'RelStopTol': 5e-8,
                            'Backtrack': BacktrackRobust(gamma_d=0.95)})
    b = ref.BPDN(D, s0, lmbda, opt)
    b.solve()
    assert np.abs(b.itstat[-1].ObjFun - 0.012009) < 1e-5
    assert np.abs(b.itstat[-1].DFid - 1.9636082e-06) < 1e-5
    assert np.abs(b.itstat[-1].RegL1 - 2.401446) < 2e-4
    assert np.linalg.norm(b.Y - x0) < 1e-3
    path = os.path.join(OUT, 'pgm_bpdn_recover_f64.npz')
    np.savez_compressed(path, D=D, S=s0, x0=x0, lmbda=np.float64(lmbda), MaxMainIter=np.int64(1000),
                        RelStopTol=np.float64(5e-8), gamma_d=np.float64(0.95), Y=np.array(b.Y),
                        iterations=np.int64(len(b.itstat)), ObjFun=np.float64(b.itstat[-1].ObjFun),
                        DFid=np.float64(b.itstat[-1].DFid), RegL1=np.float64(b.itstat[-1].RegL1))
    print('%-34s %5.1f KB  %d iterations, |Y - x0| = %.2e'
          % (os.path.basename(path), os.path.getsize(path) / 1024.0, len(b.itstat), np.linalg.norm(b.Y - x0)))


def step():
    cls, dims, lmbda, od, rules, extras, seed = CASES['bt_standard']
    D, S, arrs = problem(dims, extras, seed)
    b = build(cls, D, S, lmbda, od, rules, arrs, STEP_K, [])
    b.solve()
    out = dict(D=D, S=S, lmbda=np.float64(lmbda), k=np.int64(b.k), t=np.float64(b.t), L_before=np.float64(b.L),
               X_before=b.X.copy(), Y_before=b.Y.copy(), gamma_u=np.float64(1.2), maxiter=np.int64(50))
    b.opt['MaxMainIter'] = 1
    b.solve()
    it = b.itstat[-1]
    out.update(X=np.array(b.X), Y=np.array(b.Y), Lfinal=np.float64(b.L), F=np.float64(it.F_Btrack),
               Q=np.float64(it.Q_Btrack), Rsdl=np.float64(it.Rsdl), DFid=np.float64(it.DFid),
               RegL1=np.float64(it.RegL1), ObjFun=np.float64(it.ObjFun), IterBTrack=np.int64(it.IterBTrack))
    assert len(b.itstat) == STEP_K + 1
    path = os.path.join(OUT, 'pgm_bpdn_step_f64.npz')
    np.savez_compressed(path, **out)
    print('%-34s %5.1f KB  IterBTrack %d' % (os.path.basename(path), os.path.getsize(path) / 1024.0, it.IterBTrack))


def run(only):
    for case, (cls, dims, lmbda, od, rules, extras, seed) in CASES.items():
        if only and case not in only:
            continue
        D, S, arrs = problem(dims, extras, seed)
        reverts = []
        b = build(cls, D, S, lmbda, od, rules, arrs, ITERS, reverts)
        extra = {}
        state_runs = None
        if case == 'setdict':
            b.solve()
            extra['X_first'] = np.array(b.X)
            b.itstat = []
            b.setdict(arrs['D2'])

            def state_runs(dtype, oo, D=D, S=S, lmbda=lmbda, D2=arrs['D2']):
                r1 = pn.run(D, S, lmbda, oo, dtype=dtype)
                return pn.run(D2, S, lmbda, oo, dtype=dtype, state=r1['state'])
        b.solve()
        for v in (b.X, b.Y):
            assert np.all(np.isfinite(v)), case
        out, o = record(case, cls, D, S, lmbda, od, rules, arrs, b, reverts, extra)
        check_statement(case, D, S, lmbda, o, arrs, out, state_runs)
        if 'Backtrack' in rules:
            assert out['it_IterBTrack'].max() > 1, case
        if case == 'monotone_l1':
            assert len(reverts) > 0, case
        if case == 'autostop':
            assert len(out['it_ObjFun']) < ITERS, case
        if case == 'nonneg':
            u = build(cls, D, S, lmbda, {k: v for k, v in od.items() if k != 'NonNegCoef'}, rules, arrs, ITERS, [])
            u.solve()
            assert np.any(u.X < 0) and not np.any(b.X < 0), case
    if not only or 'step' in only:
        step()
    if not only or 'recover' in only:
        recover()
    if not only or 'defaults' in only:
        defaults()


if __name__ == '__main__':
    run(sys.argv[1:])
