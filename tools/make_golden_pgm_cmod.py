#!/usr/bin/env python3
"""Generate the pgm.cmod CnstrMOD / WeightedCnstrMOD fixtures tests/golden/pgm_cmod_*_f64.npz and the
dictlrn.wbpdndl WeightedBPDNDictLearn fixtures tests/golden/wbpdndl_*_f64.npz from the UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at $SPORCO_REFERENCE
(default /root/reference) with the import stand-ins of oracle/_stubs, exactly as tools/make_golden_pgm_bpdn.py does.
Nothing here is read by the test-suite; the tests read the .npz files alone.

    python tools/make_golden_pgm_cmod.py [CASE ...]

Each file holds the seeded inputs (Z, S, W and X0 where given), the options as flat keys (`opt_*`; arrays `optarr_*`;
the rule objects as `rule_Momentum`, `rule_StepSizePolicy`, `rule_Backtrack` with their parameters
`rule_<Rule>.<name>`), the class name, the final X, Y and L, the iterations at which Monotone reverted (`reverts`, seen
through a callback) and at which the Barzilai-Borwein rule fell back (`bb_fallbacks`), and every IterationStats column
but Time (`it_*`; the backtracking columns where they are not None) of a float64 run of ITERS iterations with
RelStopTol = 0.

The problem: seed 11 (a case may name another), D0 = randn(N, M) with unit-norm columns, Z (M, K) with three
non-zeros a column, S = D0 Z + 0.05 randn, then the optional X0 (0.1 randn) and W (0.5 + rand of its shape; `mask`:
zero with probability 0.3).  12 x 16 x 40 unless the case says otherwise.  `dsz_only` constructs with Z = None and
dsz, then calls setcoef; `zero_row` has an all-zero row of Z.

Asserted per case, with the NumPy statement of tests/_pgm_cmod_numpy.py: the float64 statement reproduces the run to
1e-10 (Cnstr, which sits at rounding level: 1e-13 absolute); the float32 statement takes the same discrete path
(IterBTrack, reverts, bb_fallbacks).  A case that fails the second condition gets another seed or L here, not an
excuse in the tests.  pgm_cmod_defaults.npz holds the option defaults, key by key.

The learner cases (LEARN_CASES, `wbpdndl_<case>_f64.npz`): D0 = randn(N, M) as given to the class (it normalises), a
planted sparse code, S = Pcn(D0) X + 0.05 randn, lmbda (0: `lmbda=None`), the optional (N, K) mask W (zero with
probability 0.3), the inner options `xopt_*` / `dopt_*`, `accurate`, the final dictionary and coefficients and every
outer IterationStats column but Iter and Time of LEARN_ITERS outer iterations.  Asserted: the float64 statement
(`learn` of tests/_pgm_cmod_numpy.py) reproduces the run to 1e-10 (Cnstr 1e-13 absolute).
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

from sporco.pgm import cmod as ref                                              # noqa: E402
from sporco.dictlrn import wbpdndl as refdl                                     # noqa: E402
from sporco.pgm.momentum import MomentumNesterov, MomentumLinear, MomentumGenLinear    # noqa: E402
from sporco.pgm.stepsize import StepSizePolicyBB, StepSizePolicyCauchy         # noqa: E402
from sporco.pgm.backtrack import BacktrackStandard, BacktrackRobust            # noqa: E402
import _pgm_cmod_numpy as pn                                                    # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
ITERS = 20
DIMS = (12, 16, 40)
C, WC = 'CnstrMOD', 'WeightedCnstrMOD'

# name: (class, (N, M, K), options, rules, extras, seed)
CASES = {
    'default': (C, DIMS, {}, {}, (), 11),
    'l30': (C, DIMS, {'L': 30.0}, {}, (), 11),
    'zeromean': (C, DIMS, {'L': 30.0, 'ZeroMean': True}, {}, (), 11),
    'nonneg': (C, DIMS, {'L': 30.0, 'NonNegCoef': True}, {}, (), 11),
    'x0': (C, DIMS, {'L': 30.0}, {}, ('X0',), 11),
    'dsz_only': (C, (8, 4, 8), {'L': 30.0}, {}, ('dsz',), 11),
    'tall': (C, (24, 8, 100), {'L': 60.0}, {}, (), 11),
    'wide': (C, (8, 32, 60), {'L': 30.0}, {}, (), 11),
    'zero_row': (C, DIMS, {'L': 30.0}, {}, ('zero_row',), 11),
    'bt_standard': (C, DIMS, {'L': 1.0}, {'Backtrack': ('standard', {})}, (), 11),
    'bt_robust': (C, DIMS, {'L': 1.0}, {'Backtrack': ('robust', {})}, (), 11),
    'mom_nesterov': (C, DIMS, {'L': 25.0}, {'Momentum': ('nesterov', {})}, (), 11),
    'mom_linear': (C, DIMS, {'L': 30.0}, {'Momentum': ('linear', {'b': 3.0})}, (), 11),
    'mom_genlinear': (C, DIMS, {'L': 30.0}, {'Momentum': ('genlinear', {'a': 40.0, 'b': 2.5})}, (), 11),
    'cauchy': (C, DIMS, {'L': 30.0}, {'StepSizePolicy': ('cauchy', {})}, (), 11),
    'bb': (C, DIMS, {'L': 30.0}, {'StepSizePolicy': ('bb', {})}, (), 11),
    'monotone': (C, DIMS, {'L': 6.0, 'Monotone': True}, {}, (), 11),
    'autostop': (C, DIMS, {'L': 30.0, 'AutoStop': {'Enabled': True, 'Tau0': 2.0}}, {}, (), 11),
    'wt_none': (WC, DIMS, {'L': 30.0}, {}, (), 11),
    'wt_scalar': (WC, DIMS, {'L': 40.0}, {}, ('Wd_0',), 11),
    'wt_n': (WC, DIMS, {'L': 40.0}, {}, ('Wd_N',), 11),
    'wt_n1': (WC, DIMS, {'L': 40.0}, {}, ('Wd_N1',), 11),
    'wt_1k': (WC, DIMS, {'L': 40.0}, {}, ('Wd_1K',), 11),
    'wt_nk': (WC, DIMS, {'L': 40.0}, {}, ('Wd_NK',), 11),
    'wt_mask': (WC, DIMS, {'L': 30.0}, {}, ('Wd_mask',), 11),
    'wt_mask_standard': (WC, DIMS, {'L': 1.0}, {'Backtrack': ('standard', {'gamma_u': 1.3})}, ('Wd_mask',), 11),
    'wt_n1_robust': (WC, DIMS, {'L': 1.0}, {'Backtrack': ('robust', {'gamma_d': 0.95, 'maxiter': 20})}, ('Wd_N1',), 11),
    'wt_nk_zeromean': (WC, DIMS, {'L': 40.0, 'ZeroMean': True}, {}, ('Wd_NK',), 11),
}

RULES = {'nesterov': MomentumNesterov, 'linear': MomentumLinear, 'genlinear': MomentumGenLinear,
         'cauchy': StepSizePolicyCauchy, 'bb': StepSizePolicyBB, 'standard': BacktrackStandard,
         'robust': BacktrackRobust}
RULE_DEFAULTS = {'linear': {'b': 2.0}, 'genlinear': {'a': 50.0, 'b': 2.0}, 'standard': {'gamma_u': 1.2, 'maxiter': 50},
                 'robust': {'gamma_d': 0.9, 'gamma_u': 2.0, 'maxiter': 50}}


def problem(dims, extras, seed):
    N, M, K = dims
    rng = np.random.RandomState(seed)
    D0 = rng.randn(N, M)
    D0 /= np.sqrt(np.sum(D0 ** 2, axis=0, keepdims=True))
    Z = np.zeros((M, K))
    for k in range(K):
        Z[rng.permutation(M)[:min(3, M)], k] = rng.randn(min(3, M))
    if 'zero_row' in extras:
        Z[M // 2, :] = 0.0
    S = D0.dot(Z) + 0.05 * rng.randn(N, K)
    arrs = {}
    if 'X0' in extras:
        arrs['X0'] = 0.1 * rng.randn(N, M)
    for tag, shp in (('Wd_0', ()), ('Wd_N', (N,)), ('Wd_N1', (N, 1)), ('Wd_1K', (1, K)), ('Wd_NK', (N, K))):
        if tag in extras:
            arrs['W'] = np.asarray(0.5 + rng.rand(*shp))
    if 'Wd_mask' in extras:
        arrs['W'] = (rng.rand(N, K) >= 0.3).astype(np.float64)
        assert np.any(arrs['W'] == 0)
    return Z, S, arrs


def flat(od, rules, iters):
    """The options and rules as the flat dict of tests/_pgm_cmod_numpy.py (arrays apart)."""
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


def build(cls, Z, S, od, rules, arrs, extras, iters, reverts):
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0}
    o.update(od)
    for slot, (kind, par) in rules.items():
        o[slot] = RULES[kind](**par)
    if 'X0' in arrs:
        o['X0'] = arrs['X0']

    def cb(obj):
        # (a revert hands the previous tuple on: pgm.py:416-420)
        if obj.opt['Monotone'] and obj.k > 0 and obj.objfn is obj.objfn_prev:
            reverts.append(int(obj.k))
        return False
    o['Callback'] = cb
    c = getattr(ref, cls)
    dsz = (Z.shape[0], S.shape[1])
    z_arg = None if 'dsz' in extras else Z
    if cls == C:
        b = c(z_arg, S, dsz, c.Options(o))
    else:
        b = c(z_arg, S, arrs.get('W'), dsz, c.Options(o))
    if z_arg is None:
        b.setcoef(Z)
    return b


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


def check_statement(name, Z, S, o, arrs, out):
    """The float64 statement reproduces the run; the float32 statement takes its discrete path."""
    oo = dict(o)
    if 'X0' in arrs:
        oo['X0'] = arrs['X0']
    for dtype in (np.float64, np.float32):
        r = pn.run(Z, S, oo, W=arrs.get('W'), dtype=dtype)
        if dtype == np.float64:
            for f in ('X', 'Y'):
                e = np.linalg.norm(r[f] - out[f]) / max(np.linalg.norm(out[f]), 1e-300)
                assert e <= 1e-10, (name, f, e)
            for f in pn.FIELDS:
                if 'it_' + f in out:
                    if f == 'Cnstr':
                        e = np.max(np.abs(r[f] - out['it_' + f]))
                        assert e <= 1e-13, (name, f, e)
                        continue
                    e = np.linalg.norm(r[f] - out['it_' + f]) / max(np.linalg.norm(out['it_' + f]), 1e-300)
                    assert e <= 1e-10, (name, f, e)
        if 'it_IterBTrack' in out:
            assert np.array_equal(np.asarray(r['IterBTrack']), out['it_IterBTrack']), (name, dtype, 'IterBTrack')
        assert list(r['reverts']) == list(out['reverts']), (name, dtype, r['reverts'], out['reverts'])
        if o.get('StepSizePolicy') == 'bb':
            assert list(r['bb_fallbacks']) == list(out['bb_fallbacks']), (name, dtype, r['bb_fallbacks'])
        assert len(r['DFid']) == len(out['it_DFid']), (name, dtype, 'iterations')


def record(name, cls, Z, S, od, rules, arrs, extras, b, reverts, iters=ITERS):
    out = traces(b, name)
    o = flat(od, rules, iters)
    for k, v in o.items():
        if isinstance(v, str):
            out['rule_' + k] = np.array(v)
        elif k.split('.')[0] in ('Momentum', 'StepSizePolicy', 'Backtrack'):
            out['rule_' + k] = np.float64(v)
        else:
            out['opt_' + k] = np.float64(v)
    out.update(Z=Z, S=S, cls=np.array(cls), X=np.array(b.X), Y=np.array(b.Y), Lfinal=np.float64(b.L),
               dsz_only=np.float64('dsz' in extras), reverts=np.asarray(reverts, dtype=np.int64),
               bb_fallbacks=np.asarray(bb_fallbacks(out['it_L']) if 'StepSizePolicy' in rules else [], dtype=np.int64))
    for k, v in arrs.items():
        out['optarr_' + k] = np.asarray(v)
    path = os.path.join(OUT, 'pgm_cmod_%s_f64.npz' % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 100000, (name, size)
    print('%-36s %5.1f KB  DFid[0] = %.4f DFid[-1] = %.6f  L %.4g  btrack %s reverts %s fallbacks %s'
          % (os.path.basename(path), size / 1024.0, out['it_DFid'][0], out['it_DFid'][-1], out['Lfinal'],
             sorted(set(out['it_IterBTrack'].astype(int))) if 'it_IterBTrack' in out else '-', list(reverts),
             list(out['bb_fallbacks'])))
    return out, o


def defaults():
    out = {}
    for cls in (C, WC):
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
    np.savez_compressed(os.path.join(OUT, 'pgm_cmod_defaults.npz'), **out)
    print('pgm_cmod_defaults.npz  %d keys' % len(out[C + '_keys']))


LEARN_ITERS = 15
# name: ((N, M, K), lmbda, mask, accurate, x options, D options, seed)
LEARN_CASES = {
    'default': ((12, 16, 40), 0.1, False, False, {}, {}, 11),
    'fast': ((12, 16, 40), 0.1, False, False, {'L': 10.0}, {'L': 50.0}, 11),
    'w_mask': ((12, 16, 40), 0.1, True, False, {'L': 10.0}, {'L': 50.0}, 11),
    'accurate': ((12, 16, 40), 0.1, True, True, {'L': 10.0}, {'L': 50.0}, 11),
    'lmbda_none': ((12, 16, 40), None, False, False, {'L': 10.0}, {'L': 50.0}, 11),
    'zeromean': ((12, 16, 40), 0.1, True, True, {'L': 10.0}, {'L': 50.0, 'ZeroMean': True}, 11),
    'ref_shape': ((8, 4, 8), 0.1, True, False, {'L': 10.0}, {'L': 50.0}, 11),
}


def learners(only):
    for case, (dims, lmbda, mask, accurate, xo, do, seed) in LEARN_CASES.items():
        if only and ('dl_' + case) not in only and 'learn' not in only:
            continue
        N, M, K = dims
        rng = np.random.RandomState(seed)
        D0 = rng.randn(N, M)
        X0 = np.zeros((M, K))
        for k in range(K):
            X0[rng.permutation(M)[:min(3, M)], k] = rng.randn(min(3, M))
        S = ref.normalise(D0).dot(X0) + 0.05 * rng.randn(N, K)
        W = (rng.rand(N, K) >= 0.3).astype(np.float64) if mask else None
        opt = refdl.WeightedBPDNDictLearn.Options({'Verbose': False, 'MaxMainIter': LEARN_ITERS,
                                                   'AccurateDFid': accurate, 'BPDN': dict(xo), 'CMOD': dict(do)})
        b = refdl.WeightedBPDNDictLearn(D0.copy(), S, lmbda, W=W, opt=opt)
        b.solve()
        its = b.getitstat()
        out = {'it_' + f: np.asarray(getattr(its, f), dtype=np.float64) for f in pn.LEARN_FIELDS}
        for v in out.values():
            assert np.all(np.isfinite(v)) and len(v) == LEARN_ITERS, case
        out.update(D0=D0, S=S, lmbda_given=np.float64(0.0 if lmbda is None else lmbda),
                   lmbda=np.float64(b.xstep.lmbda), accurate=np.float64(accurate), iters=np.int64(LEARN_ITERS),
                   D=np.array(b.getdict()), X=np.array(b.getcoef()))
        if W is not None:
            out['W'] = W
        for tag, od in (('xopt_', xo), ('dopt_', do)):
            for k, v in od.items():
                out[tag + k] = np.float64(v)
        r = pn.learn(D0, S, lmbda, LEARN_ITERS, W=W, accurate=accurate, xo=xo, do=do, dtype=np.float64)
        for f in ('D', 'X'):
            e = np.linalg.norm(r[f] - out[f]) / max(np.linalg.norm(out[f]), 1e-300)
            assert e <= 1e-10, (case, f, e)
        for f in pn.LEARN_FIELDS:
            if f == 'Cnstr':
                assert np.max(np.abs(r[f] - out['it_' + f])) <= 1e-13, (case, f)
                continue
            e = np.linalg.norm(r[f] - out['it_' + f]) / max(np.linalg.norm(out['it_' + f]), 1e-300)
            assert e <= 1e-10, (case, f, e)
        path = os.path.join(OUT, 'wbpdndl_%s_f64.npz' % case)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size < 100000, (case, size)
        print('%-36s %5.1f KB  DFid %.4f -> %.4f  ObjFun %.4f -> %.4f  zeros %.2f'
              % (os.path.basename(path), size / 1024.0, out['it_DFid'][0], out['it_DFid'][-1], out['it_ObjFun'][0],
                 out['it_ObjFun'][-1], np.mean(out['X'] == 0)))


def run(only):
    if not only or any(a == 'learn' or a.startswith('dl_') for a in only):
        learners(only)
        if only:
            return
    for case, (cls, dims, od, rules, extras, seed) in CASES.items():
        if only and case not in only:
            continue
        Z, S, arrs = problem(dims, extras, seed)
        reverts = []
        b = build(cls, Z, S, od, rules, arrs, extras, ITERS, reverts)
        b.solve()
        for v in (b.X, b.Y):
            assert np.all(np.isfinite(v)), case
        out, o = record(case, cls, Z, S, od, rules, arrs, extras, b, reverts)
        check_statement(case, Z, S, o, arrs, out)
        if 'Backtrack' in rules:
            assert out['it_IterBTrack'].max() > 1, case
        if case == 'monotone':
            assert len(reverts) > 0, case
        if case == 'autostop':
            assert len(out['it_DFid']) < ITERS, case
        if case == 'nonneg':
            assert not np.any(b.X < 0), case
    if not only or 'defaults' in only:
        defaults()


if __name__ == '__main__':
    run(sys.argv[1:])
