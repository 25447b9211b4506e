#!/usr/bin/env python3
"""Generate the ConvBPDNRecTV fixtures tests/golden/rtv_*_f64.npz from the UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at
$SPORCO_REFERENCE (default /root/reference) with the import stand-ins of oracle/_stubs, exactly
as oracle/make_golden.py does.  Nothing here is read by the test-suite; the tests read the
.npz files alone.

    python tools/make_golden_rtv.py [CASE ...]

Each file holds the seeded inputs, the option values (as arrays), the final X, Y, U and rho,
reconstruct(), and the per-iteration IterationStats traces (all but Time and XSlvRelRes) of a
float64 run of 40 iterations with RelStopTol = 0.  A file is written only when every trace is
finite and |ObjFun| < 1e6, and it must stay under 1 MB.  The large-mu case (mu = 0.5) asserts that
the share of pixels whose gradient vector of the final Y is exactly zero lies in [0.05, 0.95] and
stores it: the zero branch of prox_l2 is then exercised, which mu = 0.02 does not do.
rtv_step_f64.npz holds a small problem's state after 39 and after 40 iterations (one iteration of
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

from sporco.admm import cbpdntv as ref     # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
ITERS = 40
K = 8

# name: (mu, channels of a dimK = 0 signal or None, options)
CASES = {
    'default': (0.02, None, {}),
    'tvw': (0.02, None, {'TVWeight': 'vector'}),
    'l1w': (0.02, None, {'L1Weight': 'uniform'}),
    'fixedrho': (0.02, None, {'rho': 2.0, 'RelaxParam': 1.0, 'AutoRho': {'Enabled': False}}),
    'auxvar': (0.02, None, {'AuxVarObj': True}),
    'mu0': (0.0, None, {}),
    'chan': (0.02, 3, {}),
    'bigmu': (0.5, None, {}),
}


def problem(chan):
    rng = np.random.RandomState(7)
    D = rng.randn(6, 6, K)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(24, 32, 2) if chan is None else rng.randn(24, 32, chan)
    return D, S, rng


def zero_share(Y, M):
    """Share of (pixel, signal) positions whose gradient vector -- over the channels and the two
    components -- is exactly zero."""
    return float(np.mean(np.sum(Y[..., M:] ** 2, axis=(2, 4)) == 0.0))


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


def main():
    only = sys.argv[1:]      # case names to (re)write; none: all of them and the step file
    for case, (mu, chan, od) in CASES.items():
        if only and case not in only:
            continue
        name = 'rtv_%s_f64' % case
        D, S, rng = problem(chan)
        dimK = 1 if chan is None else 0
        od = dict(od)
        arrs = {}
        if od.get('L1Weight') == 'uniform':
            od['L1Weight'] = 0.5 + rng.rand(24, 32, 1, 2, K)
            arrs['optarr_L1Weight'] = od['L1Weight']
        if od.get('TVWeight') == 'vector':
            od['TVWeight'] = 0.5 + rng.rand(K)
            arrs['optarr_TVWeight'] = od['TVWeight']
        o = {'Verbose': False, 'MaxMainIter': ITERS, 'RelStopTol': 0.0}
        o.update(od)
        b = ref.ConvBPDNRecTV(D, S, 0.05, mu, ref.ConvBPDNRecTV.Options(o), dimK=dimK)
        b.solve()
        share = zero_share(b.Y, K)
        if case == 'bigmu':
            assert 0.05 <= share <= 0.95, (name, share)
        arrs.update(traces(b, name))
        ar = o.get('AutoRho', {})
        arrs.update(
            D=D, S=S, lmbda=np.float64(0.05), mu=np.float64(mu), dimK=np.int64(dimK),
            MaxMainIter=np.int64(ITERS), zero_share=np.float64(share),
            opt_AuxVarObj=np.int64(bool(o.get('AuxVarObj', False))),
            opt_rho=np.float64(o.get('rho', np.nan)),
            opt_RelaxParam=np.float64(o.get('RelaxParam', 1.8)),
            opt_AutoRho=np.int64(bool(ar.get('Enabled', True))),
            X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho), recon=b.reconstruct(),
            y0=b.var_y0(), y1=b.var_y1())
        path = os.path.join(OUT, name + '.npz')
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size < 1000000, (name, size)
        print('%-24s %7.1f KB  mu = %-6g zero share %.3f  ObjFun[-1] = %.4f  Rho[0] = %g'
              % (name, size / 1024.0, mu, share, arrs['it_ObjFun'][-1], arrs['it_Rho'][0]))

    if only:
        return
    # a small problem's state after 39 and after 40 iterations
    rng = np.random.RandomState(11)
    D = rng.randn(4, 4, 6)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(12, 16, 2)
    tvw = 0.5 + rng.rand(6)
    o = ref.ConvBPDNRecTV.Options({'Verbose': False, 'MaxMainIter': ITERS - 1, 'RelStopTol': 0.0,
                                   'TVWeight': tvw})
    b = ref.ConvBPDNRecTV(D, S, 0.05, 0.3, o, dimK=1)
    b.solve()
    arrs = dict(D=D, S=S, lmbda=np.float64(0.05), mu=np.float64(0.3), optarr_TVWeight=tvw,
                k=np.int64(ITERS - 1), Y_before=b.Y.copy(), U_before=b.U.copy(),
                rho_before=np.float64(b.rho))
    b.opt['MaxMainIter'] = 1
    b.solve()
    arrs.update(X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho))
    its = b.getitstat()
    for f in ('ObjFun', 'DFid', 'RegL1', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        arrs['last_' + f] = np.float64(getattr(its, f)[-1])
    assert len(its.ObjFun) == ITERS
    path = os.path.join(OUT, 'rtv_step_f64.npz')
    np.savez_compressed(path, **arrs)
    print('%-24s %7.1f KB' % (os.path.basename(path), os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
