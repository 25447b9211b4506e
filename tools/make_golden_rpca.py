#!/usr/bin/env python3
"""Generate the RobustPCA fixtures tests/golden/rpca_*_f64.npz from the UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at $SPORCO_REFERENCE
(default /root/reference) with the import stand-ins of oracle/_stubs, exactly as tools/make_golden_cmod.py does.
Nothing here is read by the test-suite; the tests read the .npz files alone.

    python tools/make_golden_rpca.py [CASE ...]

Each file holds the input S, lmbda as given (`lmbda_given`, 0 for None) and as used, the option values that differ
from the defaults (`opt_*`, AutoRho keys as `opt_AutoRho.Key`; arrays as `optarr_*`), the final X, Y, U, ss and rho
and the per-iteration IterationStats traces (all but Time) of a float64 run.

`ref01` is the problem of the reference's tests/admm/test_rpca.py::test_01, by its seed (12345, the global
generator), draws and options, 250 iterations at the default RelStopTol; its three assertions are made here too.

Every other problem: RandomState(seed), a rank-3 product A B^T of standard normal factors scaled by 1 / sqrt(3),
plus outliers of size 5 randn at 5 % of the positions (at least one), then the optional Y0 (0.5 randn at the outlier
positions) and U0 (0.05 randn); RelStopTol = 0, 24 iterations (`vec`, `row` and `fevalx_off`: 20).  AutoRho is on
with the class defaults (Period 1, AutoScaling) unless the case says otherwise: rho is then multiplied by
sqrt(r / s) after every iteration, so rounding noise in a residual feeds back into rho and U, and float32 runs
drift apart exponentially with the iteration count (at 40 iterations the float32 SVD and Gram statements of
tests/_rpca_numpy.py differed from the float64 fixture by up to 5e-4 and from each other by a factor of 13).  The
runs are kept to a length at which float32 still follows float64.  `row` (lmbda 0.2: at the default of 1 the
whole signal goes to X and the run ends at rounding level) takes a seed for which no iteration's dual residual
falls below 1e-3: where Y - Yprev nearly cancels, float32 loses the residual's digits and rho follows noise
(seeds 50, 56, 58: a smallest DualRsdl of 1e-5 and a float32 statement 2e-3 off).  `fevalx_off` stops at 20
iterations: later S - Y is numerically of rank 3 and the square roots of the near-zero eigenvalues of its Gram
matrix carry sqrt(eps) sigma_max each.  The option cases are 33 x 17.

Asserted per case: every trace finite; more than one value of rho where AutoRho is on; every file far below the
repository's file-size limit.  The 300 x 24 and 24 x 300 files hold four dense float64 arrays of 57.6 KB each and
are the largest, about 180 KB.
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

from sporco.admm import rpca as ref             # noqa: E402
import sporco.metric as sm                      # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
ITERS = 24

# name: ((R, C), seed, lmbda, options, extras)
CASES = {
    'tall': ((300, 24), 31, None, {}, ()),
    'wide': ((24, 300), 32, None, {}, ()),
    'odd': ((33, 17), 33, None, {}, ()),
    'vec': ((40, 1), 34, None, {'MaxMainIter': 20}, ()),
    'row': ((1, 40), 51, 0.2, {'MaxMainIter': 20}, ()),
    'fixedrho': ((33, 17), 36, None, {'AutoRho': {'Enabled': False}, 'rho': 0.9}, ()),
    'norelax': ((33, 17), 37, None, {'RelaxParam': 1.0}, ()),
    'fevalx_off': ((33, 17), 38, None, {'fEvalX': False, 'MaxMainIter': 20}, ()),
    'gevaly_off': ((33, 17), 39, None, {'gEvalY': False}, ()),
    'y0': ((33, 17), 40, None, {}, ('Y0',)),
    'y0u0': ((33, 17), 41, None, {}, ('Y0', 'U0')),
    'lmbda': ((33, 17), 42, 0.3, {}, ()),
}


def problem(shape, seed, extras):
    R, C = shape
    rng = np.random.RandomState(seed)
    k = min(3, R, C)
    S = rng.randn(R, k).dot(rng.randn(k, C)) / np.sqrt(3.0)
    E = np.zeros(R * C)
    idx = rng.permutation(R * C)[:max(1, (R * C) // 20)]
    E[idx] = 5.0 * rng.randn(len(idx))
    S = S + E.reshape(R, C)
    arrs = {}
    if 'Y0' in extras:
        Y0 = np.zeros(R * C)
        Y0[idx] = 0.5 * rng.randn(len(idx))
        arrs['Y0'] = Y0.reshape(R, C)
    if 'U0' in extras:
        arrs['U0'] = 0.05 * rng.randn(R, C)
    return S, arrs


def merged(od):
    o = {'Verbose': False, 'MaxMainIter': ITERS, 'RelStopTol': 0.0}
    for k, v in od.items():
        if isinstance(v, dict):
            o.setdefault(k, {}).update(v)
        else:
            o[k] = v
    return o


def traces(b, name):
    out = {}
    its = b.getitstat()
    for f in its._fields:
        if f == 'Time':
            continue
        v = np.asarray(getattr(its, f), dtype=np.float64)
        assert np.all(np.isfinite(v)), (name, f)
        out['it_' + f] = v
    return out


def flat_options(o, prefix='opt_'):
    out = {}
    for k, v in o.items():
        if k == 'Verbose':
            continue
        if isinstance(v, dict):
            for kk, vv in v.items():
                out['%s%s.%s' % (prefix, k, kk)] = np.float64(vv)
        else:
            out[prefix + k] = np.float64(v)
    return out


def save(path, out, note):
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 200000, (path, size)
    print('%-26s %6.1f KB  %s' % (os.path.basename(path), size / 1024.0, note))


def finish(case, b, S, lmbda, o, arrs, extra=None):
    for v in (b.X, b.Y, b.U):
        assert np.all(np.isfinite(v)), case
    out = traces(b, case)
    if bool(b.opt['AutoRho', 'Enabled']):
        assert len(set(out['it_Rho'])) > 1, case
    out.update(flat_options(o))
    out.update(S=S, lmbda_given=np.float64(0.0 if lmbda is None else lmbda), lmbda=np.float64(b.lmbda),
               X=np.array(b.X), Y=np.array(b.Y), U=np.array(b.U), ss=np.array(b.ss, dtype=np.float64),
               rho_final=np.float64(b.rho), rho0=np.float64(out['it_Rho'][0]))
    for k, v in arrs.items():
        out['optarr_' + k] = np.asarray(v)
    out.update(extra or {})
    save(os.path.join(OUT, 'rpca_%s_f64.npz' % case), out,
         'ObjFun[-1] = %.9f  Cnstr[-1] = %.2e  %d iterations, %d rho values'
         % (out['it_ObjFun'][-1], out['it_Cnstr'][-1], len(out['it_Rho']), len(set(out['it_Rho']))))


def run_ref01():
    np.random.seed(12345)
    N, K, L = 64, 5, 10
    u = np.random.randn(N, K)
    U = np.dot(u, u.T)
    V = np.random.randn(N, N)
    t = np.sort(np.abs(V).ravel())[V.size - L]
    V[np.abs(V) < t] = 0
    D = U + V
    o = {'Verbose': False, 'gEvalY': False, 'MaxMainIter': 250, 'AutoRho': {'Enabled': True}}
    b = ref.RobustPCA(D, None, ref.RobustPCA.Options(o))
    X, Y = b.solve()
    assert np.abs(b.itstat[-1].ObjFun - 321.493968419) < 1e-6
    assert sm.mse(U, X) < 5e-6
    assert sm.mse(V, Y) < 1e-8
    # (the low-rank factor and the positions and values of the outliers give U and V back: far smaller than both)
    nz = np.nonzero(V.ravel())[0]
    finish('ref01', b, D, None, o, {}, {'lowrank_factor': u, 'sparse_index': nz.astype(np.int64),
                                        'sparse_value': V.ravel()[nz]})


def run_cases(only):
    for case, (shape, seed, lmbda, od, extras) in CASES.items():
        if only and case not in only:
            continue
        S, arrs = problem(shape, seed, extras)
        o = merged(od)
        ro = dict(o)
        ro.update({k: v for k, v in arrs.items()})
        b = ref.RobustPCA(S, lmbda, ref.RobustPCA.Options(ro))
        b.solve()
        finish(case, b, S, lmbda, o, arrs)


if __name__ == '__main__':
    only = sys.argv[1:]
    if not only or 'ref01' in only:
        run_ref01()
    run_cases(only)
