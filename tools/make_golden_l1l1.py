#!/usr/bin/env python3
"""Generate the ConvL1L1Grd fixtures tests/golden/l1l1_*_f64.npz from the UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at
$SPORCO_REFERENCE (default /root/reference) with the import stand-ins of oracle/_stubs, exactly
as oracle/make_golden.py does.  Nothing here is read by the test-suite; the tests read the
.npz files alone.

    python tools/make_golden_l1l1.py [CASE ...]

Each file holds the seeded inputs, the option values (as arrays), the final X, Y, U and rho,
reconstruct(), and the per-iteration IterationStats traces (all but Time and XSlvRelRes) of a
float64 run of 40 iterations with RelStopTol = 0.  A file is written only when every trace is
finite, and it must stay under 1 MB.

The problem is an impulse-noise one: D randn, normalised per filter; S = 0.3 randn with a quarter
of its entries replaced by +-4; lambda = 0.6.  Every case asserts, and stores, that the share of
non-zero entries of the final y0 and of the final y1 lies in [0.05, 0.95], so that both blocks take
both branches of the soft threshold (at lambda <= 0.3 the y0 share is 0: the block-0 shrinkage would
never act).  The autorho case asserts that rho moved.  l1l1_step_f64.npz holds the default problem's
state after 39 and after 40 iterations (one iteration of a restatement can be pinned to it).
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

from sporco.admm import cbpdn as ref     # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
ITERS = 40
LMBDA = 0.6
AUTORHO = {'Enabled': True, 'Period': 3, 'Scaling': 2.0, 'RsdlRatio': 1.2, 'AutoScaling': True, 'RsdlTarget': 1.0}

# name: (signal shape, dictionary shape, mu, masked, options)
SMALL = ((16, 17, 2), (5, 5, 6), 0.05)
CASES = {
    'default': SMALL + (False, {}),
    'mask': SMALL + (True, {}),
    'autorho': SMALL + (False, {'AutoRho': AUTORHO}),
    'fixed': SMALL + (False, {'rho': 2.0, 'RelaxParam': 1.0, 'AuxVarObj': True}),
    'gradw': SMALL + (False, {'GradWeight': np.linspace(0.5, 2.0, 6)}),
    'nonneg_nobndry': SMALL + (False, {'NonNegCoef': True, 'NoBndryCross': True}),
    'mcd': ((16, 16, 3, 2), (5, 5, 3, 4), 0.01, False, {}),
    'mcs': ((16, 16, 3, 2), (5, 5, 4), 0.01, True, {}),
}


def problem(sshape, dshape, masked, seed=7):
    rng = np.random.RandomState(seed)
    D = rng.randn(*dshape)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = 0.3 * rng.randn(*sshape)
    hit = rng.rand(*sshape) < 0.25
    S[hit] = 4.0 * np.sign(rng.randn(int(hit.sum())))
    W = (rng.rand(*sshape[:2]) >= 0.2).astype(np.float64) if masked else None
    return D, S, W


def traces(b, name):
    arrs = {}
    its = b.getitstat()
    for f in its._fields:
        if f in ('Time', 'XSlvRelRes'):
            continue
        v = np.asarray(getattr(its, f), dtype=np.float64)
        assert np.all(np.isfinite(v)), (name, f)
        arrs['it_' + f] = v
    return arrs


def build(D, S, W, mu, od, iters=ITERS):
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0}
    o.update(od)
    return ref.ConvL1L1Grd(D, S, LMBDA, mu, W, ref.ConvL1L1Grd.Options(o), dimK=1), o


def main():
    only = sys.argv[1:]      # case names to (re)write; none: all of them and the step file
    for case, (sshape, dshape, mu, masked, od) in CASES.items():
        if only and case not in only:
            continue
        name = 'l1l1_%s_f64' % case
        D, S, W = problem(sshape, dshape, masked)
        b, o = build(D, S, W, mu, od)
        b.solve()
        for v in (b.X, b.Y, b.U):
            assert np.all(np.isfinite(v)), name
        nz0, nz1 = float(np.mean(b.var_y0() != 0.0)), float(np.mean(b.var_y1() != 0.0))
        assert 0.05 <= nz0 <= 0.95 and 0.05 <= nz1 <= 0.95, (name, nz0, nz1)
        arrs = traces(b, name)
        if case == 'autorho':
            assert len(set(arrs['it_Rho'])) > 2, name
        ar = o.get('AutoRho', {})
        arrs.update(
            D=D, S=S, lmbda=np.float64(LMBDA), mu=np.float64(mu), dimK=np.int64(1), MaxMainIter=np.int64(ITERS),
            nz_y0=np.float64(nz0), nz_y1=np.float64(nz1),
            opt_AuxVarObj=np.int64(bool(o.get('AuxVarObj', False))),
            opt_NonNegCoef=np.int64(bool(o.get('NonNegCoef', False))),
            opt_NoBndryCross=np.int64(bool(o.get('NoBndryCross', False))),
            opt_rho=np.float64(o.get('rho', 1.0)), opt_RelaxParam=np.float64(o.get('RelaxParam', 1.8)),
            opt_AutoRho=np.int64(bool(ar.get('Enabled', False))),
            X=b.X, Y=b.Y, U=b.U, Y0=b.var_y0(), Y1=b.var_y1(), rho_final=np.float64(b.rho), recon=b.reconstruct())
        if W is not None:
            arrs['W'] = W
        if 'GradWeight' in o:
            arrs['optarr_GradWeight'] = np.asarray(o['GradWeight'])
        path = os.path.join(OUT, name + '.npz')
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size < 1000000, (name, size)
        print('%-26s %7.1f KB  non-zero y0 %.3f y1 %.3f  ObjFun[-1] = %.4f  Rho[-1] = %g'
              % (name, size / 1024.0, nz0, nz1, arrs['it_ObjFun'][-1], arrs['it_Rho'][-1]))

    if only:
        return
    # the default problem's state after 39 and after 40 iterations
    sshape, dshape, mu, masked, od = CASES['default']
    D, S, W = problem(sshape, dshape, masked)
    b, o = build(D, S, W, mu, od, ITERS - 1)
    b.solve()
    arrs = dict(D=D, S=S, lmbda=np.float64(LMBDA), mu=np.float64(mu), k=np.int64(ITERS - 1), Y_before=b.Y.copy(),
                U_before=b.U.copy(), rho_before=np.float64(b.rho))
    b.opt['MaxMainIter'] = 1
    b.solve()
    arrs.update(X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho))
    its = b.getitstat()
    for f in ('ObjFun', 'DFid', 'RegL1', 'RegGrad', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        arrs['last_' + f] = np.float64(getattr(its, f)[-1])
    assert len(its.ObjFun) == ITERS
    for v in arrs.values():
        assert np.all(np.isfinite(v))
    path = os.path.join(OUT, 'l1l1_step_f64.npz')
    np.savez_compressed(path, **arrs)
    print('%-26s %7.1f KB' % (os.path.basename(path), os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
