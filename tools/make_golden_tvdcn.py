#!/usr/bin/env python3
"""Generate the TVL2Deconv / TVL1Deconv fixtures tests/golden/tvl2dcn_*_f64.npz and tvl1dcn_*_f64.npz from
the UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at
$SPORCO_REFERENCE (default /root/reference) with the import stand-ins of oracle/_stubs, exactly
as tools/make_golden_tvl1.py does.  Nothing here is read by the test-suite; the tests read the
.npz files alone.

    python tools/make_golden_tvdcn.py [l2|l1] [CASE ...]

Each file holds the seeded inputs, the option values (as arrays), the final X, Y, U and rho, and the
per-iteration IterationStats traces (all but Time) of a float64 run of 40 iterations with
RelStopTol = 0.  A file is written only when its case holds what is asserted below, and it must stay
under 1 MB.

The problem: seed 7, RandomState draws in this order: the kernel A (`rand`, 5 x 4, x 3 planes for `aplanes`;
asymmetric, positive, every plane normalised to sum 1); 0.05 randn added to the blurred image -- the
piecewise-constant image of make_golden_tvl1.py (+1 / -1 halves, its lower two thirds scaled by 0.5),
16 x 17 (x the trailing axes of the case), blurred by the reference's fftconv; for l1 a `rand < 0.2` hit mask
and a `uniform(-1.5, 1.5)` array that replaces the image where the mask hits; then the optional `tvw`
(TVWeight, 0.5 + rand), `Y0` (0.1 randn, S.shape + (blocks,)) and `U0` (0.05 randn).  `impulse` uses
A = ones((1, 1)), `mask` (l1) a DFidWeight of ones with row 3 and column 5 set to zero.  lmbda is recorded in
every file as `lmbda`.
Asserted per case: every trace finite; the share of pixels whose final gradient blocks have zero norm in
[0.1, 0.9] and, l1, the share of zero entries of the final data block in [0.1, 0.9] -- both branches of both
shrinkages (recorded as `zero_share`, `zero_share_data`); the cases that run with AutoRho (every l2 case; l1
`autorho` and `vec`) show more than two values of rho.  tvl?dcn_step_f64.npz holds the `autorho` problem's
state after 39 and after 40 iterations.  tvl?dcn_recovery_f64.npz holds the problem of the reference's
tests/admm/test_tvl2.py / test_tvl1.py TestSet02.test_02 (a 64 x 64 step image, an impulse kernel, gEvalY
off, 250 iterations), its clean image and the final ObjFun of the reference.
The reference's TVL1Deconv cannot be built with a kernel per plane (its GAf concatenates arrays whose
trailing axes differ): the l1 `aplanes` case is reported and left out.
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

from sporco.admm import tvl1 as ref1     # noqa: E402
from sporco.admm import tvl2 as ref2     # noqa: E402
from sporco.fft import fftconv           # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
ITERS = 40
AR = {'AutoRho': {'Enabled': True}}
LMBDA = {'l2': 0.05, 'l1': 0.8}

# name: (trailing axes, options, caxis, extras); `l1ar`: AutoRho is switched on for l1 (l2 has it by default)
CASES = {
    'default': ((), {}, None, ()),
    'autorho': ((), {'gEvalY': False}, None, ('l1ar',)),
    'tvw': ((3,), {}, None, ('tvw',)),
    'vec': ((3, 2), {}, 2, ('l1ar',)),
    'stdres': ((), {'AutoRho': {'StdResiduals': True}}, None, ()),
    'relax1': ((), {'RelaxParam': 1.0, 'rho': 0.5}, None, ()),
    'lsc': ((), {'LinSolveCheck': True}, None, ()),
    'y0warm': ((), {}, None, ('Y0',)),
    'y0u0': ((), {}, None, ('Y0', 'U0')),
    'aplanes': ((3,), {}, None, ('aplanes',)),
    'impulse': ((), {}, None, ('impulse',)),
    'mask': ((), {}, None, ('mask',)),      # l1 only
}


def problem(kind, trail, extras, seed=7):
    rng = np.random.RandomState(seed)
    H, W = 16, 17
    img = np.ones((H, W))
    img[:, W // 2:] = -1.0
    img[H // 3:] *= 0.5
    shape = (H, W) + tuple(trail)
    A = rng.rand(*((5, 4) + (tuple(trail) if 'aplanes' in extras else ())))
    A = A / np.sum(A, axis=(0, 1), keepdims=True)
    if 'impulse' in extras:
        A = np.ones((1, 1))
    An = A.reshape(A.shape + (1,) * (len(shape) - A.ndim))
    clean = np.broadcast_to(img.reshape((H, W) + (1,) * len(trail)), shape)
    S = fftconv(An, clean, axes=(0, 1)) + 0.05 * rng.randn(*shape)
    if kind == 'l1':
        hit = rng.rand(*shape) < 0.2
        S = np.where(hit, rng.uniform(-1.5, 1.5, shape), S)
    nb = 3 if kind == 'l1' else 2
    arrs = {}
    if 'mask' in extras:
        w = np.ones(shape)
        w[3] = 0.0
        w[:, 5] = 0.0
        arrs['DFidWeight'] = w
    if 'tvw' in extras:
        arrs['TVWeight'] = 0.5 + rng.rand(*shape)
    if 'Y0' in extras:
        arrs['Y0'] = 0.1 * rng.randn(*(shape + (nb,)))
    if 'U0' in extras:
        arrs['U0'] = 0.05 * rng.randn(*(shape + (nb,)))
    return A, np.ascontiguousarray(S), arrs


def build(kind, A, S, lmbda, od, arrs, caxis, extras, iters=ITERS):
    cls = ref1.TVL1Deconv if kind == 'l1' else ref2.TVL2Deconv
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0}
    if kind == 'l1' and 'l1ar' in extras:
        o.update({'AutoRho': {'Enabled': True}})
    for k, v in od.items():
        if isinstance(v, dict):
            o.setdefault(k, {}).update(v)
        else:
            o[k] = v
    o.update(arrs)
    return cls(A, S, lmbda, cls.Options(o), caxis=caxis)


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


def recovery(kind):
    np.random.seed(12345)
    N = 64
    U = np.ones((N, N))
    U[:, 0:N // 2] = -1
    if kind == 'l2':
        D = U + 1e-1 * np.random.randn(N, N)
        lmbda, od, A, cls, bound, mse_bound = 1e-1, {}, np.ones((1)), ref2.TVL2Deconv, 1e-3, 1e-3
    else:
        V = np.random.randn(N, N)
        t = np.sort(np.abs(V).ravel())[V.size - 20]
        V[np.abs(V) < t] = 0
        D = U + V
        lmbda, od, A, cls, bound, mse_bound = 3.0, {'rho': 10.0}, np.ones((1, 1)), ref1.TVL1Deconv, 1e-5, 1e-4
    iters = 250
    opt = cls.Options(dict({'Verbose': False, 'gEvalY': False, 'MaxMainIter': iters}, **od))
    b = cls(A, D, lmbda, opt)
    X = b.solve()
    obj = float(b.itstat[-1].ObjFun)
    mse = float(np.mean((U - X) ** 2))
    assert np.isfinite(obj) and mse < mse_bound
    path = os.path.join(OUT, 'tv%sdcn_recovery_f64.npz' % kind)
    np.savez_compressed(path, U=U, D=D, A=A, lmbda=np.float64(lmbda), MaxMainIter=np.int64(iters),
                        opt_rho=np.float64(od.get('rho', np.nan)), ObjFun=np.float64(obj),
                        iterations=np.int64(len(b.itstat)), mse=np.float64(mse), bound=np.float64(bound),
                        mse_bound=np.float64(mse_bound))
    assert os.path.getsize(path) < 1000000
    print('%-24s %6.1f KB  ObjFun %.12f after %d iterations, mse %.3e'
          % (os.path.basename(path), os.path.getsize(path) / 1024.0, obj, len(b.itstat), mse))


def run(kind, only):
    lmbda = LMBDA[kind]
    for case, (trail, od, caxis, extras) in CASES.items():
        if (only and case not in only) or (case == 'mask' and kind != 'l1'):
            continue
        name = 'tv%sdcn_%s_f64' % (kind, case)
        A, S, arrs = problem(kind, trail, extras)
        try:
            b = build(kind, A, S, lmbda, od, arrs, caxis, extras)
        except ValueError as e:
            if kind == 'l1' and case == 'aplanes':
                print('%-24s not written: the reference cannot build it (%s)' % (name, str(e).splitlines()[0][:60]))
                continue
            raise
        rho0 = float(b.rho)
        b.solve()
        for v in (b.X, b.Y, b.U):
            assert np.all(np.isfinite(v)), name
        out = traces(b, name)
        Yg = b.Y[..., 0:2]
        share = float(np.mean(np.sqrt(np.sum(Yg ** 2, axis=b.saxes)) == 0))
        assert 0.1 <= share <= 0.9, (name, share)
        share_d = -1.0
        if kind == 'l1':
            share_d = float(np.mean(b.Y[..., -1] == 0))
            assert 0.1 <= share_d <= 0.9, (name, share_d)
        if bool(b.opt['AutoRho', 'Enabled']):
            assert len(set(out['it_Rho'])) > 2, name
        out.update(options(b))
        out.update(A=A, S=S, lmbda=np.float64(lmbda), caxis=np.int64(-1 if caxis is None else caxis),
                   MaxMainIter=np.int64(ITERS), opt_rho=np.float64(rho0), zero_share=np.float64(share),
                   zero_share_data=np.float64(share_d), X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho))
        for k, v in arrs.items():
            out['optarr_' + k] = np.asarray(v)
        path = os.path.join(OUT, name + '.npz')
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size < 1000000, (name, size)
        print('%-24s %6.1f KB  zero share %.3f / %.3f  ObjFun[-1] = %.6f  %d rho values'
              % (name, size / 1024.0, share, share_d, out['it_ObjFun'][-1], len(set(out['it_Rho']))))

    if only:
        return
    # the `autorho` problem's state after 39 and after 40 iterations
    trail, od, caxis, extras = CASES['autorho']
    A, S, arrs = problem(kind, trail, extras)
    b = build(kind, A, S, lmbda, od, arrs, caxis, extras, ITERS - 1)
    b.solve()
    out = dict(A=A, S=S, lmbda=np.float64(lmbda), k=np.int64(ITERS - 1), X_before=np.array(b.X), Y_before=b.Y.copy(),
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
    path = os.path.join(OUT, 'tv%sdcn_step_f64.npz' % kind)
    np.savez_compressed(path, **out)
    print('%-24s %6.1f KB' % (os.path.basename(path), os.path.getsize(path) / 1024.0))
    recovery(kind)


def main():
    args = sys.argv[1:]
    kinds = [a for a in args if a in ('l2', 'l1')] or ['l2', 'l1']
    only = [a for a in args if a not in ('l2', 'l1')]
    for kind in kinds:
        run(kind, only)


if __name__ == '__main__':
    main()
