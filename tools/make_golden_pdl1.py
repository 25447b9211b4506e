#!/usr/bin/env python3
"""Generate the ConvProdDictL1L1Grd / ConvProdDictL1L1GrdJoint fixtures tests/golden/pdl1_*_f64.npz
from the UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at
$SPORCO_REFERENCE (default /root/reference) with the import stand-ins of oracle/_stubs, exactly
as tools/make_golden_pd.py does.  Nothing here is read by the test-suite; the tests read the
.npz files alone.

    python tools/make_golden_pdl1.py [CASE ...]

Each file holds the seeded inputs (those of tools/make_golden_pd.py ``problem()``), the option values
(as arrays), the final X, Y (composite: block 0 first), U and rho, reconstruct(), and the
per-iteration IterationStats traces (all but Time and XSlvRelRes) of a float64 run of 40 iterations
with RelStopTol = 0, lmbda = 0.05, mu = 0.01.  A file is written only when every trace is finite and
|ObjFun| < 1e6, and it must stay under 1 MB.  Asserted here and stored (tests/test_pdl1.py re-asserts
them from the files): the share of non-zero entries of Y1 in [0.05, 0.95] for every case, of Y0 for
the cases with Cb < Cs, the share of zero channel groups of Y1 for the joint cases, at least two
distinct values of Rho for the autorho cases, a (numerically) zero eigenvalue for rankdef and cb9.
pdl1_step_f64.npz holds a small problem's state after 39 and after 40 iterations (one iteration of a
restatement can be pinned to it).
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
MU = 0.01
AUTORHO = {'Enabled': True, 'Period': 2, 'RsdlRatio': 1.2}

# name: (class, signal shape, dimK, filters, shape of B, options)
BASE = ((24, 32, 5, 2), 1, 8, (5, 3))
CASES = {
    'default': ('L1L1Grd',) + BASE + ({'LinSolveCheck': True},),
    'mask': ('L1L1Grd',) + BASE + ({'W': 'rand'},),
    'gradw': ('L1L1Grd',) + BASE + ({'GradWeight': np.linspace(0.5, 2.0, 8)},),
    'nonneg': ('L1L1Grd',) + BASE + ({'NonNegCoef': True},),
    'auxvar': ('L1L1Grd',) + BASE + ({'AuxVarObj': True},),
    'autorho': ('L1L1Grd',) + BASE + ({'AutoRho': AUTORHO},),
    'joint': ('Joint',) + BASE + ({'LinSolveCheck': True},),
    'joint_autorho': ('Joint',) + BASE + ({'AutoRho': AUTORHO},),
    'rankdef': ('L1L1Grd', (24, 32, 3), 0, 8, (3, 4), {'rho': 5.0}),
    'oddw': ('L1L1Grd', (16, 17, 3), 0, 6, (3, 3), {'rho': 5.0, 'LinSolveCheck': True}),
    'cb9': ('L1L1Grd', (16, 16, 5, 2), 1, 8, (5, 9), {'rho': 5.0}),
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


def build(cls, D, B, S, W, o, dimK):
    if cls == 'Joint':
        return ref.ConvProdDictL1L1GrdJoint(D, B, S, LMBDA, MU, ref.ConvProdDictL1L1GrdJoint.Options(o), dimK=dimK)
    return ref.ConvProdDictL1L1Grd(D, B, S, LMBDA, MU, W, ref.ConvProdDictL1L1Grd.Options(o), dimK=dimK)


def main():
    only = sys.argv[1:]      # case names to (re)write; none: all of them and the step file
    for case, (cls, sshape, dimK, K, bshape, od) in CASES.items():
        if only and case not in only:
            continue
        name = 'pdl1_%s_f64' % case
        D, B, S, rng = problem(sshape, K, bshape)
        od = dict(od)
        arrs = {}
        W = None
        if od.pop('W', None) == 'rand':
            W = (rng.rand(*sshape) > 0.2).astype(np.float64)
            arrs['optarr_W'] = W.astype(np.uint8)
        if 'GradWeight' in od:
            arrs['optarr_GradWeight'] = np.asarray(od['GradWeight'], dtype=np.float64)
        o = {'Verbose': False, 'MaxMainIter': ITERS, 'RelStopTol': 0.0}
        o.update(od)
        b = build(cls, D, B, S, W, o, dimK)
        b.solve()
        for v in (b.X, b.Y, b.U):
            assert np.all(np.isfinite(v)), name
        Y0, Y1 = b.block_sep0(b.Y), b.block_sep1(b.Y)
        Cs, Cb = bshape
        assert Y0.shape[2] == Cs and Y1.shape[2] == Cb and b.X.shape == Y1.shape
        nz0, nz1 = float(np.mean(Y0 != 0.0)), float(np.mean(Y1 != 0.0))
        zero_groups = float(np.mean(np.sum(Y1 ** 2, axis=2) == 0.0))
        assert 0.05 <= nz1 <= 0.95, (name, nz1)
        if Cb < Cs:
            assert 0.05 <= nz0 <= 0.95, (name, nz0)
        if cls == 'Joint':
            assert 0.05 <= zero_groups <= 0.95, (name, zero_groups)
        arrs.update(traces(b, name))
        if 'AutoRho' in od:
            assert len(set(arrs['it_Rho'])) >= 2, name
        if case in ('rankdef', 'cb9'):
            assert b.Gamma.min() < 1e-14 * b.Gamma.max(), name
        if o.get('LinSolveCheck'):
            assert np.array(b.getitstat().XSlvRelRes).max() < 1e-12, name
        ar = o.get('AutoRho', {})
        arrs.update(
            D=D, B=B, S=S, lmbda=np.float64(LMBDA), mu=np.float64(MU), joint=np.int64(cls == 'Joint'),
            dimK=np.int64(dimK), MaxMainIter=np.int64(ITERS), nz_y0=np.float64(nz0), nz_y1=np.float64(nz1),
            zero_groups=np.float64(zero_groups), Gamma=b.Gamma, Q=b.Q,
            opt_AuxVarObj=np.int64(bool(o.get('AuxVarObj', False))),
            opt_NonNegCoef=np.int64(bool(o.get('NonNegCoef', False))),
            opt_LinSolveCheck=np.int64(bool(o.get('LinSolveCheck', False))),
            opt_rho=np.float64(o.get('rho', 1.0)),
            opt_AutoRho=np.int64(bool(ar.get('Enabled', False))),
            opt_AutoRho_Period=np.int64(ar.get('Period', 10)),
            opt_AutoRho_RsdlRatio=np.float64(ar.get('RsdlRatio', 10.0)),
            X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho), recon=b.reconstruct())
        path = os.path.join(OUT, name + '.npz')
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size < 1000000, (name, size)
        print('%-24s %7.1f KB  nz Y0 %.3f  nz Y1 %.3f  zero groups %.3f  min Gamma %.3g  ObjFun[-1] = %.4f  '
              'Rho[-1] = %g' % (name, size / 1024.0, nz0, nz1, zero_groups, b.Gamma.min(), arrs['it_ObjFun'][-1],
                                arrs['it_Rho'][-1]))

    if only:
        return
    # a small problem's state after 39 and after 40 iterations
    D, B, S, rng = problem((12, 16, 4, 2), 6, (4, 3), seed=11, dsz=4)
    o = ref.ConvProdDictL1L1Grd.Options({'Verbose': False, 'MaxMainIter': ITERS - 1, 'RelStopTol': 0.0})
    b = ref.ConvProdDictL1L1Grd(D, B, S, LMBDA, MU, None, o, dimK=1)
    b.solve()
    arrs = dict(D=D, B=B, S=S, lmbda=np.float64(LMBDA), mu=np.float64(MU), k=np.int64(ITERS - 1),
                Y_before=b.Y.copy(), U_before=b.U.copy(), rho_before=np.float64(b.rho))
    b.opt['MaxMainIter'] = 1
    b.solve()
    arrs.update(X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho))
    its = b.getitstat()
    for f in ('ObjFun', 'DFid', 'RegL1', 'RegGrad', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        arrs['last_' + f] = np.float64(getattr(its, f)[-1])
    assert len(its.ObjFun) == ITERS
    for v in arrs.values():
        assert np.all(np.isfinite(v))
    path = os.path.join(OUT, 'pdl1_step_f64.npz')
    np.savez_compressed(path, **arrs)
    print('%-24s %7.1f KB' % (os.path.basename(path), os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
