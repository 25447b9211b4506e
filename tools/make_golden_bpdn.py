#!/usr/bin/env python3
"""Generate the BPDN / BPDNJoint / ElasticNet fixtures tests/golden/bpdn_*_f64.npz from the UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at $SPORCO_REFERENCE
(default /root/reference) with the import stand-ins of oracle/_stubs, exactly as tools/make_golden_spline.py
does.  Nothing here is read by the test-suite; the tests read the .npz files alone.

    python tools/make_golden_bpdn.py [CASE ...]

Each file holds the seeded inputs, the option values that differ from the defaults (`opt_*`, AutoRho keys as
`opt_AutoRho.Key`; arrays as `optarr_*`), the class name, lmbda and mu as given (`lmbda_given` = 0: `lmbda=None`),
the final X, Y, U and rho, and the per-iteration IterationStats traces (all but Time) of a float64 run of ITERS
iterations with RelStopTol = 0.

The problem: seed 11, RandomState draws in this order: D = randn(N, M) with unit-norm columns, a sparse code of
three non-zeros a column, S = D X0 + 0.05 randn, then the optional Y0 (0.1 randn), U0 (0.05 randn), L1Weight
(1 + rand of its shape) and D2 (the `setdict` case).  8 x 16 x 5 unless the case says otherwise.  AutoRho runs with
Period 4, so that a run of 30 iterations changes rho several times (`tall` and `joint_small`, 24 x 16, run 10, `square` 12
and `joint_zero` 12: run longer, their residuals reach the rounding level of float32, AutoRho then follows noise there,
and the float32 yardstick of the tests grows to 1e-3 and more; `joint_zero` uses mu = 1.0, which zeroes its rows well
inside the threshold).  Asserted per case: every trace finite; the
share of exact zeros of the final Y in [0.1, 0.95] (`joint_small`, 24 x 16 x 5 so that every row can be
used: at most 0.95); more than one value of rho where AutoRho is on; `nonneg`:
some element of the unclipped run's Y is negative; `joint_zero`: a row of Y is exactly zero, `joint_small`: none
is; `elnet_mu0` equals `default` bit for bit; `recover`: the assertions of the reference's
tests/admm/test_bpdn.py::TestSet01::test_08.  bpdn_step_f64.npz holds the `default` problem's state after
ITERS - 1 and after ITERS iterations; bpdn_defaults.npz the option defaults of the three classes, key by key.
"""

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.environ.get('SPORCO_REFERENCE', '/root/reference'))
sys.path.insert(0, os.path.join(REPO, 'oracle', '_stubs'))
warnings.filterwarnings('ignore')

from sporco.admm import bpdn as ref     # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
ITERS = 30
LMBDA = 0.1
BASE = {'AutoRho': {'Period': 4}}

# name: (class, (N, M, K), lmbda, mu, options, extras)
CASES = {
    'default': ('BPDN', (8, 16, 5), LMBDA, 0.0, {}, ()),
    'lmbda_none': ('BPDN', (8, 16, 5), None, 0.0, {}, ()),
    'auxvar_off': ('BPDN', (8, 16, 5), LMBDA, 0.0, {'AuxVarObj': False}, ()),
    'fixedrho': ('BPDN', (8, 16, 5), LMBDA, 0.0, {'AutoRho': {'Enabled': False}, 'rho': 0.7, 'RelaxParam': 1.0}, ()),
    'stdres': ('BPDN', (8, 16, 5), LMBDA, 0.0, {'AutoRho': {'Period': 1, 'StdResiduals': True}}, ()),
    'lsc': ('BPDN', (8, 16, 5), LMBDA, 0.0, {'LinSolveCheck': True}, ()),
    'nonneg': ('BPDN', (8, 16, 5), LMBDA, 0.0, {'NonNegCoef': True}, ()),
    'w_atom': ('BPDN', (8, 16, 5), LMBDA, 0.0, {}, ('W_M1',)),
    'w_signal': ('BPDN', (8, 16, 5), LMBDA, 0.0, {}, ('W_1K',)),
    'w_full': ('BPDN', (8, 16, 5), LMBDA, 0.0, {}, ('W_MK',)),
    'y0': ('BPDN', (8, 16, 5), LMBDA, 0.0, {}, ('Y0',)),
    'y0u0': ('BPDN', (8, 16, 5), LMBDA, 0.0, {}, ('Y0', 'U0')),
    'returnx': ('BPDN', (8, 16, 5), LMBDA, 0.0, {'ReturnX': True}, ()),
    'square': ('BPDN', (8, 8, 5), LMBDA, 0.0, {'MaxMainIter': 12}, ()),
    'tall': ('BPDN', (24, 16, 5), LMBDA, 0.0, {'MaxMainIter': 10}, ()),
    'k1': ('BPDN', (8, 16, 1), LMBDA, 0.0, {}, ()),
    'joint': ('BPDNJoint', (8, 16, 5), LMBDA, 0.05, {}, ()),
    'joint_zero': ('BPDNJoint', (8, 16, 5), LMBDA, 1.0, {'MaxMainIter': 12}, ()),
    'joint_small': ('BPDNJoint', (24, 16, 5), 0.02, 0.01, {'MaxMainIter': 10}, ()),
    'joint_nonneg': ('BPDNJoint', (8, 16, 5), LMBDA, 0.05, {'NonNegCoef': True}, ()),
    'elnet': ('ElasticNet', (8, 16, 5), LMBDA, 0.2, {}, ()),
    'elnet_lsc': ('ElasticNet', (8, 16, 5), LMBDA, 0.2, {'LinSolveCheck': True}, ()),
    'elnet_auxvar_off': ('ElasticNet', (8, 16, 5), LMBDA, 0.2, {'AuxVarObj': False}, ()),
    'elnet_mu0': ('ElasticNet', (8, 16, 5), LMBDA, 0.0, {}, ()),
    'setdict': ('BPDN', (8, 16, 5), LMBDA, 0.0, {}, ('D2',)),
}


def problem(dims, extras, seed=11):
    N, M, K = dims
    rng = np.random.RandomState(seed)
    D = rng.randn(N, M)
    D /= np.sqrt(np.sum(D ** 2, axis=0, keepdims=True))
    X0 = np.zeros((M, K))
    for k in range(K):
        X0[rng.permutation(M)[:min(3, M)], k] = rng.randn(min(3, M))
    S = D.dot(X0) + 0.05 * rng.randn(N, K)
    arrs = {}
    if 'Y0' in extras:
        arrs['Y0'] = 0.1 * rng.randn(M, K)
    if 'U0' in extras:
        arrs['U0'] = 0.05 * rng.randn(M, K)
    for tag, shp in (('W_M1', (M, 1)), ('W_1K', (1, K)), ('W_MK', (M, K))):
        if tag in extras:
            arrs['L1Weight'] = 1.0 + rng.rand(*shp)
    if 'D2' in extras:
        D2 = rng.randn(N, M)
        arrs['D2'] = D2 / np.sqrt(np.sum(D2 ** 2, axis=0, keepdims=True))
    return D, S, arrs


def merged(od, iters):
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0}
    for src in (BASE, od):
        for k, v in src.items():
            if isinstance(v, dict):
                o.setdefault(k, {}).update(v)
            else:
                o[k] = v
    return o


def build(cls, D, S, lmbda, mu, od, arrs, iters=ITERS):
    o = merged(od, iters)
    o.update({k: v for k, v in arrs.items() if k != 'D2'})
    c = getattr(ref, cls)
    if cls == 'BPDN':
        return c(D, S, lmbda, c.Options(o))
    return c(D, S, lmbda, mu, c.Options(o))


def traces(b, name):
    out = {}
    its = b.getitstat()
    for f in its._fields:
        if f == 'Time':
            continue
        col = getattr(its, f)
        if f == 'XSlvRelRes' and col[0] is None:
            continue
        v = np.asarray(col, dtype=np.float64)
        assert np.all(np.isfinite(v)), (name, f)
        out['it_' + f] = v
    return out


def flat_options(od, iters):
    out = {}
    for k, v in merged(od, iters).items():
        if k == 'Verbose':
            continue
        if isinstance(v, dict):
            for kk, vv in v.items():
                out['opt_%s.%s' % (k, kk)] = np.float64(vv)
        else:
            out['opt_' + k] = np.float64(v)
    return out


def record(name, cls, D, S, lmbda, mu, od, arrs, b, extra=None):
    out = traces(b, name)
    out.update(flat_options(od, ITERS))
    out.update(D=D, S=S, cls=np.array(cls), lmbda_given=np.float64(0.0 if lmbda is None else lmbda),
               lmbda=np.float64(b.lmbda), mu=np.float64(mu), rho0=np.float64(out['it_Rho'][0]),
               X=np.array(b.X), Y=np.array(b.Y), U=np.array(b.U), rho_final=np.float64(b.rho),
               zero_share=np.float64(np.mean(b.Y == 0)))
    for k, v in arrs.items():
        out['optarr_' + k] = np.asarray(v)
    out.update(extra or {})
    path = os.path.join(OUT, 'bpdn_%s_f64.npz' % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 1000000, (name, size)
    print('%-28s %6.1f KB  zero share %.3f  ObjFun[-1] = %.6f  %d rho values'
          % (os.path.basename(path), size / 1024.0, out['zero_share'], out['it_ObjFun'][-1], len(set(out['it_Rho']))))
    return out


def defaults():
    out = {}
    for cls in ('BPDN', 'BPDNJoint', 'ElasticNet'):
        d = getattr(ref, cls).Options().__class__.defaults
        keys, vals = [], []
        for k, v in sorted(d.items()):
            if isinstance(v, dict):
                for kk, vv in sorted(v.items()):
                    keys.append('%s.%s' % (k, kk))
                    vals.append(repr(vv))
            else:
                keys.append(k)
                vals.append(repr(v))
        out[cls + '_keys'] = np.array(keys)
        out[cls + '_values'] = np.array(vals)
        out[cls + '_fields'] = np.array(getattr(ref, cls).IterationStats._fields)
    np.savez_compressed(os.path.join(OUT, 'bpdn_defaults.npz'), **out)
    print('bpdn_defaults.npz  %d keys' % len(out['BPDN_keys']))


def recover():
    """tests/admm/test_bpdn.py::TestSet01::test_08 of the reference, its inputs and what it asserts."""
    N, M, L = 64, 128, 4
    np.random.seed(12345)
    D = np.random.randn(N, M)
    x0 = np.zeros((M, 1))
    si = np.random.permutation(list(range(0, M - 1)))
    x0[si[0:L]] = np.random.randn(L, 1)
    s0 = D.dot(x0)
    lmbda = 5e-3
    opt = ref.BPDN.Options({'Verbose': False, 'MaxMainIter': 500, 'RelStopTol': 5e-4})
    b = ref.BPDN(D, s0, lmbda, opt)
    b.solve()
    assert np.abs(b.itstat[-1].ObjFun - 0.012009) < 1e-5
    assert np.abs(b.itstat[-1].DFid - 1.9636082e-06) < 1e-5
    assert np.abs(b.itstat[-1].RegL1 - 2.401446) < 1e-5
    assert np.linalg.norm(b.Y - x0) < 1e-3
    path = os.path.join(OUT, 'bpdn_recover_f64.npz')
    np.savez_compressed(path, D=D, S=s0, x0=x0, lmbda=np.float64(lmbda), MaxMainIter=np.int64(500),
                        RelStopTol=np.float64(5e-4), Y=np.array(b.Y), iterations=np.int64(len(b.itstat)),
                        ObjFun=np.float64(b.itstat[-1].ObjFun), DFid=np.float64(b.itstat[-1].DFid),
                        RegL1=np.float64(b.itstat[-1].RegL1))
    print('%-28s %6.1f KB  %d iterations, |Y - x0| = %.2e'
          % (os.path.basename(path), os.path.getsize(path) / 1024.0, len(b.itstat), np.linalg.norm(b.Y - x0)))


def run(only):
    done = {}
    for case, (cls, dims, lmbda, mu, od, extras) in CASES.items():
        if only and case not in only:
            continue
        D, S, arrs = problem(dims, extras)
        b = build(cls, D, S, lmbda, mu, od, arrs)
        extra = {}
        if case == 'setdict':
            b.solve()
            extra['Y_first'] = np.array(b.Y)
            b.itstat = []
            b.setdict(arrs['D2'])
        b.solve()
        for v in (b.X, b.Y, b.U):
            assert np.all(np.isfinite(v)), case
        share = float(np.mean(b.Y == 0))
        assert (0.1 if case != 'joint_small' else 0.0) <= share <= 0.95, (case, share)
        if bool(b.opt['AutoRho', 'Enabled']):
            assert len(set(float(i.Rho) for i in b.itstat)) > 1, case
        if case in ('nonneg', 'joint_nonneg'):
            u = build(cls, D, S, lmbda, mu, {k: v for k, v in od.items() if k != 'NonNegCoef'}, arrs)
            u.solve()
            assert np.any(u.Y < 0) and not np.any(b.Y < 0), case
            extra['negative_unclipped'] = np.int64(np.sum(u.Y < 0))
        rows = np.sqrt(np.sum(np.asarray(b.Y) ** 2, axis=1))
        if case == 'joint_zero':
            assert np.any(rows == 0) and np.any(rows > 0), case
        if case == 'joint_small':
            assert np.all(rows > 0), case
        if case == 'returnx':
            assert b.getmin() is b.X
        done[case] = record(case, cls, D, S, lmbda, mu, od, arrs, b, extra)
    if 'default' in done and 'elnet_mu0' in done:
        for f in ('X', 'Y', 'U', 'it_ObjFun', 'it_Rho'):
            assert np.array_equal(done['default'][f], done['elnet_mu0'][f]), f

    if not only or 'step' in only:
        cls, dims, lmbda, mu, od, extras = CASES['default']
        D, S, arrs = problem(dims, extras)
        b = build(cls, D, S, lmbda, mu, od, arrs, ITERS - 1)
        b.solve()
        out = dict(D=D, S=S, lmbda=np.float64(lmbda), k=np.int64(ITERS - 1), Y_before=b.Y.copy(), U_before=b.U.copy(),
                   rho_before=np.float64(b.rho))
        out.update(flat_options(od, ITERS))
        b.opt['MaxMainIter'] = 1
        b.solve()
        out.update(X=np.array(b.X), Y=np.array(b.Y), U=np.array(b.U), rho_final=np.float64(b.rho))
        its = b.getitstat()
        for f in its._fields:
            if f not in ('Time', 'Iter', 'XSlvRelRes'):
                out['last_' + f] = np.float64(getattr(its, f)[-1])
        assert len(its.ObjFun) == ITERS
        path = os.path.join(OUT, 'bpdn_step_f64.npz')
        np.savez_compressed(path, **out)
        print('%-28s %6.1f KB' % (os.path.basename(path), os.path.getsize(path) / 1024.0))
    if not only or 'recover' in only:
        recover()
    if not only or 'defaults' in only:
        defaults()


if __name__ == '__main__':
    run(sys.argv[1:])
