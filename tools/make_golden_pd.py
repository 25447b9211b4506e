#!/usr/bin/env python3
"""Generate the ConvProdDictBPDN / ConvProdDictBPDNJoint fixtures tests/golden/pd_*_f64.npz from the
UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at
$SPORCO_REFERENCE (default /root/reference) with the import stand-ins of oracle/_stubs, exactly
as oracle/make_golden.py does.  Nothing here is read by the test-suite; the tests read the
.npz files alone.

    python tools/make_golden_pd.py [CASE ...]

Each file holds the seeded inputs, the option values (as arrays), the final X, Y, U and rho,
reconstruct(), and the per-iteration IterationStats traces (all but Time and XSlvRelRes) of a
float64 run of 40 iterations with RelStopTol = 0.  A file is written only when every trace is
finite and |ObjFun| < 1e6, and it must stay under 1 MB.  The joint case asserts that the share of
(pixel, image, filter) positions whose channel group of the final Y is exactly zero lies in
[0.05, 0.95] and stores it; every file stores the share of non-zero entries of Y.  The cb9 case
(B 5 x 9) is run on a 16 x 16 signal: at 24 x 32 its X and U alone exceed the size limit.
pd_step_f64.npz holds a small problem's state after 39 and after 40 iterations (one iteration of
a restatement can be pinned to it).
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

from sporco.admm import pdcsc as ref     # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
ITERS = 40
LMBDA = 0.05

# name: (class, mu, signal shape, dimK, filters, shape of B, options)
BASE = ((24, 32, 5, 2), 1, 8, (5, 3))
CASES = {
    'default': ('BPDN', 0.0) + BASE + ({},),
    'joint': ('Joint', 0.05) + BASE + ({},),
    'rankdef': ('BPDN', 0.0, (24, 32, 3), 0, 8, (3, 4), {}),
    'l1w': ('BPDN', 0.0) + BASE + ({'L1Weight': 'uniform'},),
    'nonneg': ('BPDN', 0.0) + BASE + ({'NonNegCoef': True},),
    'fixedrho': ('BPDN', 0.0) + BASE + ({'rho': 2.0, 'RelaxParam': 1.0, 'AutoRho': {'Enabled': False}},),
    'auxvar': ('BPDN', 0.0) + BASE + ({'AuxVarObj': True},),
    'oddw': ('BPDN', 0.0, (16, 17, 3), 0, 6, (3, 3), {}),
    'cb9': ('BPDN', 0.0, (16, 16, 5, 2), 1, 8, (5, 9), {}),
}


def problem(sshape, K, bshape, seed=7, dsz=6):
    rng = np.random.RandomState(seed)
    D = rng.randn(dsz, dsz, K)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(*sshape)
    B = rng.randn(*bshape)
    B /= np.sqrt(np.sum(B ** 2, axis=0, keepdims=True))
    return D, B, S, rng


def traces(b, name):
    arrs = {}
    its = b.getitstat()
    for f in its._fields:
        if f in ('Time', 'XSlvRelRes'):
            continue
        v = np.asarray(getattr(its, f), dtype=np.float64)
        assert np.all(np.isfinite(v)), (name, f)
        arrs['it_' + f] = v
    assert np.all(np.abs(arrs['it_ObjFun']) < 1e6), name
    return arrs


def build(cls, D, B, S, mu, o, dimK):
    if cls == 'Joint':
        return ref.ConvProdDictBPDNJoint(D, B, S, LMBDA, mu, ref.ConvProdDictBPDNJoint.Options(o), dimK=dimK)
    return ref.ConvProdDictBPDN(D, B, S, LMBDA, ref.ConvProdDictBPDN.Options(o), dimK=dimK)


def main():
    only = sys.argv[1:]      # case names to (re)write; none: all of them and the step file
    for case, (cls, mu, sshape, dimK, K, bshape, od) in CASES.items():
        if only and case not in only:
            continue
        name = 'pd_%s_f64' % case
        D, B, S, rng = problem(sshape, K, bshape)
        od = dict(od)
        arrs = {}
        if od.get('L1Weight') == 'uniform':
            N = sshape[3] if dimK else 1
            # (values that float32 holds exactly, stored as float32: the file stays under the size limit)
            w32 = (0.5 + rng.rand(sshape[0], sshape[1], bshape[1], N, K)).astype(np.float32)
            od['L1Weight'] = w32.astype(np.float64)
            arrs['optarr_L1Weight'] = w32
        o = {'Verbose': False, 'MaxMainIter': ITERS, 'RelStopTol': 0.0}
        o.update(od)
        b = build(cls, D, B, S, mu, o, dimK)
        b.solve()
        for v in (b.X, b.Y, b.U):
            assert np.all(np.isfinite(v)), name
        zero_share = float(np.mean(np.sum(b.Y ** 2, axis=2) == 0.0))
        if case == 'joint':
            assert 0.05 <= zero_share <= 0.95, (name, zero_share)
        arrs.update(traces(b, name))
        ar = o.get('AutoRho', {})
        arrs.update(
            D=D, B=B, S=S, lmbda=np.float64(LMBDA), mu=np.float64(mu), joint=np.int64(cls == 'Joint'),
            dimK=np.int64(dimK), MaxMainIter=np.int64(ITERS), zero_share=np.float64(zero_share),
            nonzero_share=np.float64(np.mean(b.Y != 0.0)), Gamma=b.Gamma, Q=b.Q,
            opt_AuxVarObj=np.int64(bool(o.get('AuxVarObj', False))),
            opt_NonNegCoef=np.int64(bool(o.get('NonNegCoef', False))),
            opt_rho=np.float64(o.get('rho', np.nan)),
            opt_RelaxParam=np.float64(o.get('RelaxParam', 1.8)),
            opt_AutoRho=np.int64(bool(ar.get('Enabled', True))),
            X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho), recon=b.reconstruct())
        path = os.path.join(OUT, name + '.npz')
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size < 1000000, (name, size)
        print('%-20s %7.1f KB  zero groups %.3f  non-zero %.3f  min Gamma %.3g  ObjFun[-1] = %.4f  Rho[-1] = %g'
              % (name, size / 1024.0, zero_share, arrs['nonzero_share'], b.Gamma.min(), arrs['it_ObjFun'][-1],
                 arrs['it_Rho'][-1]))

    if only:
        return
    # a small problem's state after 39 and after 40 iterations
    D, B, S, rng = problem((12, 16, 4, 2), 6, (4, 3), seed=11, dsz=4)
    o = ref.ConvProdDictBPDN.Options({'Verbose': False, 'MaxMainIter': ITERS - 1, 'RelStopTol': 0.0})
    b = ref.ConvProdDictBPDN(D, B, S, LMBDA, o, dimK=1)
    b.solve()
    arrs = dict(D=D, B=B, S=S, lmbda=np.float64(LMBDA), k=np.int64(ITERS - 1), Y_before=b.Y.copy(),
                U_before=b.U.copy(), rho_before=np.float64(b.rho))
    b.opt['MaxMainIter'] = 1
    b.solve()
    arrs.update(X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho))
    its = b.getitstat()
    for f in ('ObjFun', 'DFid', 'RegL1', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        arrs['last_' + f] = np.float64(getattr(its, f)[-1])
    assert len(its.ObjFun) == ITERS
    for v in arrs.values():
        assert np.all(np.isfinite(v))
    path = os.path.join(OUT, 'pd_step_f64.npz')
    np.savez_compressed(path, **arrs)
    print('%-20s %7.1f KB' % (os.path.basename(path), os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
