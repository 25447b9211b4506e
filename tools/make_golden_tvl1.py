#!/usr/bin/env python3
"""Generate the TVL1Denoise fixtures tests/golden/tvl1_*_f64.npz from the UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at
$SPORCO_REFERENCE (default /root/reference) with the import stand-ins of oracle/_stubs, exactly
as tools/make_golden_tvl2.py does.  Nothing here is read by the test-suite; the tests read the
.npz files alone.

    python tools/make_golden_tvl1.py [CASE ...]

Each file holds the seeded inputs, the option values (as arrays), the final X, Y, U and rho, and the
per-iteration IterationStats traces (all but Time) of a float64 run of 40 iterations with
RelStopTol = 0.  A file is written only when its case holds what is asserted below, and it must stay
under 1 MB.

The problem: seed 7, RandomState draws in this order: a piecewise-constant image (+1 / -1 halves, its lower
two thirds scaled by 0.5) plus 0.05 randn, 16 x 17 (x the trailing axes of the case); a `rand < 0.2` hit mask
and a `uniform(-1.5, 1.5)` array of the same shape that replaces the image where the mask hits (impulse
noise); then the optional `mask` (DFidWeight, rand < 0.7), `tvw` (TVWeight, 0.5 + rand), `Y0` (0.1 randn,
S.shape + (3,)) and `U0` (0.05 randn).  lmbda = 0.8, for `vec` 1.0 (at 0.8 its share of zero gradient-block
norms is 0.03): recorded in the file as `lmbda`.
Asserted per case: every trace finite; the share of pixels whose final gradient blocks have zero norm and
the share of zero entries of the final data block both in [0.1, 0.9] -- both branches of both shrinkages
(recorded as `zero_share`, `zero_share_data`); `autorho`, `mask` and `vec` move rho; `gstol` shows at least
three different GSIter values.  tvl1_step_f64.npz holds the `autorho` problem's state after 39 and after 40
iterations.  tvl1_recovery_f64.npz holds the problem of the reference's tests/admm/test_tvl1.py
TestSet02.test_01 (a 64 x 64 step image with 20 impulses, lmbda = 3, gEvalY off, 250 iterations), its clean
image and the final ObjFun of the reference.
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

from sporco.admm import tvl1 as ref     # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
ITERS = 40
AR = {'AutoRho': {'Enabled': True}}

# name: (trailing axes, options, caxis, lmbda, extras)
CASES = {
    'default': ((), {}, None, 0.8, ()),
    'autorho': ((), dict(AR, gEvalY=False), None, 0.8, ()),
    'mask': ((3,), dict(AR), None, 0.8, ('mask',)),
    'tvw': ((3,), {}, None, 0.8, ('tvw',)),
    'vec': ((3, 2), dict(AR), 2, 1.0, ()),
    'stdres': ((), {'AutoRho': {'StdResiduals': True}}, None, 0.8, ()),
    'relax1': ((), {'RelaxParam': 1.0, 'rho': 0.5}, None, 0.8, ()),
    'gstol': ((), {'MaxGSIter': 6, 'GSTol': 3e-2, 'rho': 0.5}, None, 0.8, ()),
    'y0warm': ((), {}, None, 0.8, ('Y0',)),
    'y0u0': ((), {}, None, 0.8, ('Y0', 'U0')),
}


def problem(trail, extras, seed=7):
    rng = np.random.RandomState(seed)
    H, W = 16, 17
    img = np.ones((H, W))
    img[:, W // 2:] = -1.0
    img[H // 3:] *= 0.5
    shape = (H, W) + tuple(trail)
    S = img.reshape((H, W) + (1,) * len(trail)) + 0.05 * rng.randn(*shape)
    hit = rng.rand(*shape) < 0.2
    S = np.where(hit, rng.uniform(-1.5, 1.5, shape), S)
    arrs = {}
    if 'mask' in extras:
        arrs['DFidWeight'] = (rng.rand(*shape) < 0.7).astype(np.float64)
    if 'tvw' in extras:
        arrs['TVWeight'] = 0.5 + rng.rand(*shape)
    if 'Y0' in extras:
        arrs['Y0'] = 0.1 * rng.randn(*(shape + (3,)))
    if 'U0' in extras:
        arrs['U0'] = 0.05 * rng.randn(*(shape + (3,)))
    return S, arrs


def build(S, lmbda, od, arrs, caxis, iters=ITERS):
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0}
    o.update({k: (dict(v) if isinstance(v, dict) else v) for k, v in od.items()})
    o.update(arrs)
    return ref.TVL1Denoise(S, lmbda, ref.TVL1Denoise.Options(o), caxis=caxis)


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


def options(b):
    ar = b.opt['AutoRho']
    return dict(
        opt_gEvalY=np.int64(bool(b.opt['gEvalY'])), opt_RelaxParam=np.float64(b.opt['RelaxParam']),
        opt_MaxGSIter=np.int64(b.opt['MaxGSIter']), opt_GSTol=np.float64(b.opt['GSTol']),
        opt_AutoRho=np.int64(bool(ar['Enabled'])), opt_AutoRho_Period=np.int64(ar['Period']),
        opt_AutoRho_Scaling=np.float64(ar['Scaling']), opt_AutoRho_RsdlRatio=np.float64(ar['RsdlRatio']),
        opt_AutoRho_AutoScaling=np.int64(bool(ar['AutoScaling'])),
        opt_AutoRho_RsdlTarget=np.float64(ar['RsdlTarget']),
        opt_StdResiduals=np.int64(bool(ar['StdResiduals'])))


def recovery():
    np.random.seed(12345)
    N, L = 64, 20
    U = np.ones((N, N))
    U[:, 0:N // 2] = -1
    V = np.random.randn(N, N)
    t = np.sort(np.abs(V).ravel())[V.size - L]
    V[np.abs(V) < t] = 0
    D = U + V
    lmbda, iters = 3.0, 250
    opt = ref.TVL1Denoise.Options({'Verbose': False, 'gEvalY': False, 'MaxMainIter': iters})
    b = ref.TVL1Denoise(D, lmbda, opt)
    X = b.solve()
    obj = float(b.itstat[-1].ObjFun)
    assert np.isfinite(obj) and np.mean((U - X) ** 2) < np.mean((U - D) ** 2)
    path = os.path.join(OUT, 'tvl1_recovery_f64.npz')
    np.savez_compressed(path, U=U, D=D, lmbda=np.float64(lmbda), MaxMainIter=np.int64(iters),
                        ObjFun=np.float64(obj), iterations=np.int64(len(b.itstat)),
                        mse=np.float64(np.mean((U - X) ** 2)))
    assert os.path.getsize(path) < 1000000
    print('%-22s %6.1f KB  ObjFun %.12f after %d iterations, mse %.3e'
          % (os.path.basename(path), os.path.getsize(path) / 1024.0, obj, len(b.itstat), np.mean((U - X) ** 2)))


def main():
    only = sys.argv[1:]      # case names to (re)write; none: all of them, the step file and the recovery file
    for case, (trail, od, caxis, lmbda, extras) in CASES.items():
        if only and case not in only:
            continue
        name = 'tvl1_%s_f64' % case
        S, arrs = problem(trail, extras)
        b = build(S, lmbda, od, arrs, caxis)
        rho0 = float(b.rho)
        b.solve()
        for v in (b.X, b.Y, b.U):
            assert np.all(np.isfinite(v)), name
        out = traces(b, name)
        nrm = np.sqrt(np.sum(b.Y[..., 0:-1] ** 2, axis=b.saxes))
        share = float(np.mean(nrm == 0))
        share_d = float(np.mean(b.Y[..., -1] == 0))
        assert 0.1 <= share <= 0.9, (name, share)
        assert 0.1 <= share_d <= 0.9, (name, share_d)
        if case in ('autorho', 'mask', 'vec'):
            assert len(set(out['it_Rho'])) > 2, name
        if case == 'gstol':
            assert len(set(out['it_GSIter'])) >= 3, (name, set(out['it_GSIter']))
        out.update(options(b))
        out.update(S=S, lmbda=np.float64(lmbda), caxis=np.int64(-1 if caxis is None else caxis),
                   MaxMainIter=np.int64(ITERS), opt_rho=np.float64(rho0), zero_share=np.float64(share),
                   zero_share_data=np.float64(share_d), X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho))
        for k, v in arrs.items():
            out['optarr_' + k] = np.asarray(v)
        path = os.path.join(OUT, name + '.npz')
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size < 1000000, (name, size)
        print('%-22s %6.1f KB  zero share %.3f / %.3f  ObjFun[-1] = %.6f  %d rho values  GSIter %s'
              % (name, size / 1024.0, share, share_d, out['it_ObjFun'][-1], len(set(out['it_Rho'])),
                 sorted(set(out['it_GSIter'].astype(int)))))

    if only:
        return
    # the `autorho` problem's state after 39 and after 40 iterations
    trail, od, caxis, lmbda, extras = CASES['autorho']
    S, arrs = problem(trail, extras)
    b = build(S, lmbda, od, arrs, caxis, ITERS - 1)
    b.solve()
    out = dict(S=S, lmbda=np.float64(lmbda), k=np.int64(ITERS - 1), X_before=np.array(b.X), Y_before=b.Y.copy(),
               U_before=b.U.copy(), rho_before=np.float64(b.rho))
    out.update(options(b))
    b.opt['MaxMainIter'] = 1
    b.solve()
    out.update(X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho))
    its = b.getitstat()
    for f in its._fields:
        if f not in ('Time', 'Iter'):
            out['last_' + f] = np.float64(getattr(its, f)[-1])
    assert len(its.ObjFun) == ITERS
    for v in out.values():
        assert np.all(np.isfinite(v))
    path = os.path.join(OUT, 'tvl1_step_f64.npz')
    np.savez_compressed(path, **out)
    print('%-22s %6.1f KB' % (os.path.basename(path), os.path.getsize(path) / 1024.0))
    recovery()


if __name__ == '__main__':
    main()
