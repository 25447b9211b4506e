#!/usr/bin/env python3
"""Generate the SplineL1 fixtures tests/golden/spline_*_f64.npz from the UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at
$SPORCO_REFERENCE (default /root/reference) with the import stand-ins of oracle/_stubs, exactly
as tools/make_golden_tvdcn.py does.  Nothing here is read by the test-suite; the tests read the
.npz files alone.

    python tools/make_golden_spline.py [CASE ...]

Each file holds the seeded inputs, the option values (as arrays), the final X, Y, U and rho, and the
per-iteration IterationStats traces (all but Time) of a float64 run of 40 iterations with
RelStopTol = 0.  A file is written only when its case holds what is asserted below, and it must stay
under 1 MB.

The problem: seed 7, RandomState draws in this order: a `rand < 0.2` hit mask and a `uniform(-1.5, 1.5)`
array that replaces the image cos(linspace(0, pi, H)) x cos(linspace(0, 1.5 pi, W)), 16 x 17 (x the trailing
axes of the case), where the mask hits; then the optional `Y0` (0.1 randn) and `U0` (0.05 randn).  `mask`
uses a DFidWeight of ones with row 3 and column 5 set to zero, `sig1d` a 1-D signal of 33 samples
(the image's first factor, cos(linspace(0, pi, 33)), axes = (0,); with its second factor the run reaches residuals
of 5e-8 within the 40 iterations and AutoRho then follows rounding noise: tests/_spline_numpy.py in float64 differed
from the reference by 7e-9 on rho there, by 1e-10 here).  lmbda = 1.0, recorded in every file as `lmbda`.
Asserted per case: every trace finite; the share of exact zeros in the final Y in [0.1, 0.9] -- both
branches of the soft threshold (recorded as `zero_share`); the cases that run with AutoRho (all but
`fixedrho`) show more than two values of rho.  spline_step_f64.npz holds the `default` problem's state after
39 and after 40 iterations.  spline_recovery_f64.npz holds the problem of the reference's
tests/admm/test_spline.py TestSet01.test_01, its clean image and the final ObjFun of the reference.
The reference cannot be built with a Y0 alone (its uinit reads an attribute that is set later): `y0warm` hands
it the U0 that its own rule states, see build().
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

from sporco.admm import spline as ref     # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
ITERS = 40
LMBDA = 1.0

# name: (trailing axes, options, extras)
CASES = {
    'default': ((), {}, ()),
    'gevalx': ((), {'gEvalY': False}, ()),
    'planes': ((3,), {}, ()),
    'planes2': ((3, 2), {}, ()),
    'fixedrho': ((), {'AutoRho': {'Enabled': False}, 'rho': 0.5, 'RelaxParam': 1.0}, ()),
    'stdres': ((), {'AutoRho': {'StdResiduals': True}}, ()),
    'lsc': ((), {'LinSolveCheck': True}, ()),
    'mask': ((), {}, ('mask',)),
    'y0warm': ((), {}, ('Y0',)),
    'y0u0': ((), {}, ('Y0', 'U0')),
    'sig1d': ((), {}, ('sig1d',)),
}


def problem(trail, extras, seed=7):
    rng = np.random.RandomState(seed)
    H, W = 16, 17
    if 'sig1d' in extras:
        shape = (33,)
        clean = np.cos(np.linspace(0, np.pi, 33))
    else:
        shape = (H, W) + tuple(trail)
        img = np.cos(np.linspace(0, np.pi, H))[:, np.newaxis] * np.cos(np.linspace(0, 1.5 * np.pi, W))[np.newaxis, :]
        clean = np.broadcast_to(img.reshape((H, W) + (1,) * len(trail)), shape)
    hit = rng.rand(*shape) < 0.2
    S = np.where(hit, rng.uniform(-1.5, 1.5, shape), clean)
    arrs = {}
    if 'mask' in extras:
        w = np.ones(shape)
        w[3] = 0.0
        w[:, 5] = 0.0
        arrs['DFidWeight'] = w
    if 'Y0' in extras:
        arrs['Y0'] = 0.1 * rng.randn(*shape)
    if 'U0' in extras:
        arrs['U0'] = 0.05 * rng.randn(*shape)
    return np.ascontiguousarray(S), arrs


def build(S, od, arrs, iters=ITERS):
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0}
    for k, v in od.items():
        if isinstance(v, dict):
            o.setdefault(k, {}).update(v)
        else:
            o[k] = v
    o.update(arrs)
    if 'Y0' in arrs and 'U0' not in arrs:
        # The reference's uinit (spline.py:176-185) reads self.Wdf before __init__ has set it, so the unmodified
        # class cannot be built with a Y0 alone (AttributeError).  Its rule, U = (Wdf / rho) sign(Y), is handed
        # to it as an explicit U0 instead, with the DFidWeight and the rho it would have used; the fixture
        # records the Y0 only.
        rho = o.get('rho', 2.0 * LMBDA + 0.1)
        o['U0'] = (np.asarray(o.get('DFidWeight', 1.0), dtype=np.float64) / rho) * np.sign(arrs['Y0'])
    axes = (0,) if S.ndim == 1 else (0, 1)
    return ref.SplineL1(S, LMBDA, ref.SplineL1.Options(o), axes=axes)


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


def options(b):
    ar = b.opt['AutoRho']
    return dict(
        opt_gEvalY=np.int64(bool(b.opt['gEvalY'])), opt_RelaxParam=np.float64(b.opt['RelaxParam']),
        opt_LinSolveCheck=np.int64(bool(b.opt['LinSolveCheck'])),
        opt_AutoRho=np.int64(bool(ar['Enabled'])), opt_AutoRho_Period=np.int64(ar['Period']),
        opt_AutoRho_Scaling=np.float64(ar['Scaling']), opt_AutoRho_RsdlRatio=np.float64(ar['RsdlRatio']),
        opt_AutoRho_AutoScaling=np.int64(bool(ar['AutoScaling'])),
        opt_AutoRho_RsdlTarget=np.float64(ar['RsdlTarget']),
        opt_StdResiduals=np.int64(bool(ar['StdResiduals'])))


def recovery():
    np.random.seed(12345)
    N, L = 64, 20
    x = np.cos(np.linspace(0, np.pi, N))[np.newaxis, :]
    y = np.cos(np.linspace(0, np.pi, N))[:, np.newaxis]
    U = x * y
    V = np.random.randn(N, N)
    t = np.sort(np.abs(V).ravel())[V.size - L]
    V[np.abs(V) < t] = 0
    D = U + V
    lmbda, iters, rel = 0.1, 250, 5e-4
    opt = ref.SplineL1.Options({'Verbose': False, 'gEvalY': False, 'MaxMainIter': iters, 'RelStopTol': rel,
                                'DFidWeight': V == 0, 'AutoRho': {'Enabled': True}})
    b = ref.SplineL1(D, lmbda, opt)
    X = b.solve()
    obj = float(b.itstat[-1].ObjFun)
    mse = float(np.mean((U - X) ** 2))
    assert abs(obj - 0.333606246) < 1e-6 and mse < 1e-6
    path = os.path.join(OUT, 'spline_recovery_f64.npz')
    np.savez_compressed(path, U=U, D=D, DFidWeight=(V == 0), lmbda=np.float64(lmbda), MaxMainIter=np.int64(iters),
                        RelStopTol=np.float64(rel), ObjFun=np.float64(obj), iterations=np.int64(len(b.itstat)),
                        mse=np.float64(mse))
    assert os.path.getsize(path) < 1000000
    print('%-24s %6.1f KB  ObjFun %.12f after %d iterations, mse %.3e'
          % (os.path.basename(path), os.path.getsize(path) / 1024.0, obj, len(b.itstat), mse))


def run(only):
    for case, (trail, od, extras) in CASES.items():
        if only and case not in only:
            continue
        name = 'spline_%s_f64' % case
        S, arrs = problem(trail, extras)
        b = build(S, od, arrs)
        rho0 = float(b.rho)
        b.solve()
        for v in (b.X, b.Y, b.U):
            assert np.all(np.isfinite(v)), name
        out = traces(b, name)
        share = float(np.mean(b.Y == 0))
        assert 0.1 <= share <= 0.9, (name, share)
        if bool(b.opt['AutoRho', 'Enabled']):
            assert len(set(out['it_Rho'])) > 2, name
        out.update(options(b))
        out.update(S=S, lmbda=np.float64(LMBDA), MaxMainIter=np.int64(ITERS), opt_rho=np.float64(rho0),
                   zero_share=np.float64(share), X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho))
        for k, v in arrs.items():
            out['optarr_' + k] = np.asarray(v)
        path = os.path.join(OUT, name + '.npz')
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size < 1000000, (name, size)
        print('%-24s %6.1f KB  zero share %.3f  ObjFun[-1] = %.6f  %d rho values'
              % (name, size / 1024.0, share, out['it_ObjFun'][-1], len(set(out['it_Rho']))))

    if only and 'step' not in only and 'recovery' not in only:
        return
    if not only or 'step' in only:
        # the `default` problem's state after 39 and after 40 iterations
        trail, od, extras = CASES['default']
        S, arrs = problem(trail, extras)
        b = build(S, od, arrs, ITERS - 1)
        b.solve()
        out = dict(S=S, lmbda=np.float64(LMBDA), k=np.int64(ITERS - 1), X_before=np.array(b.X), Y_before=b.Y.copy(),
                   U_before=b.U.copy(), rho_before=np.float64(b.rho))
        out.update(options(b))
        b.opt['MaxMainIter'] = 1
        b.solve()
        out.update(X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho))
        its = b.getitstat()
        for f in its._fields:
            if f not in ('Time', 'Iter', 'XSlvRelRes'):
                out['last_' + f] = np.float64(getattr(its, f)[-1])
        assert len(its.ObjFun) == ITERS
        for v in out.values():
            assert np.all(np.isfinite(v))
        path = os.path.join(OUT, 'spline_step_f64.npz')
        np.savez_compressed(path, **out)
        print('%-24s %6.1f KB' % (os.path.basename(path), os.path.getsize(path) / 1024.0))
    if not only or 'recovery' in only:
        recovery()


if __name__ == '__main__':
    run(sys.argv[1:])
