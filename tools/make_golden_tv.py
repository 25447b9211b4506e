#!/usr/bin/env python3
"""Generate the ConvBPDNScalarTV / ConvBPDNVectorTV fixtures tests/golden/tv_*_f64.npz from the
UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at
$SPORCO_REFERENCE (default /root/reference) with the import stand-ins of oracle/_stubs, exactly
as oracle/make_golden.py does.  Nothing here is read by the test-suite; the tests read the
.npz files alone.

    python tools/make_golden_tv.py [CASE ...]

Each file holds the seeded inputs, the option values (as arrays), the final X, Y, U and rho,
reconstruct(), and the per-iteration IterationStats traces (all but Time and XSlvRelRes) of a
float64 run of 40 iterations with RelStopTol = 0 (the array-L1Weight case has no traces: the
reference's own objective evaluation fails on such a weight, so it runs with FastSolve).  A file is written only when every trace is finite
and |ObjFun| < 1e6, and it must stay under 1 MB.  The large-mu case raises mu from 0.5 until the
share of exactly-zero gradient vectors of the final Y lies in [0.05, 0.95] (ConvBPDNVectorTV) or
is 1 (ConvBPDNScalarTV, whose single global norm allows only 0 or 1), and asserts that: the zero
branch of prox_l2 is then exercised, which mu = 0.02 does not do.  tv_step_{s,v}_f64.npz hold a small
problem's state after 39 and after 40 iterations (one iteration of a restatement can be pinned to
them).
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
CLASSES = {'s': ref.ConvBPDNScalarTV, 'v': ref.ConvBPDNVectorTV}

# name: (mu, channels of a dimK = 0 signal or None, options)
CASES = {
    'default': (0.02, None, {}),
    'tvw': (0.02, None, {'TVWeight': 'vector'}),
    # (the reference's obfn_reg cannot multiply an array L1Weight with the six-axis g variable
    # -- cbpdntv.py:444 raises --, so this case runs with FastSolve: iterates and rho, no traces)
    'l1w': (0.02, None, {'L1Weight': 'uniform', 'FastSolve': True}),
    'fixedrho': (0.02, None, {'rho': 2.0, 'RelaxParam': 1.0, 'AutoRho': {'Enabled': False}}),
    'auxvar': (0.02, None, {'AuxVarObj': True}),
    'mu0': (0.0, None, {}),
    'chan': (0.02, 3, {}),
    # Large mu: the generator raises mu from 0.5 (doubling, then bisecting) until the zero branch of
    # prox_l2 shows in the final Y.  ConvBPDNVectorTV has one norm per pixel, so the share of
    # exactly-zero gradient vectors must lie in [0.05, 0.95].  ConvBPDNScalarTV's prox_l2 call has
    # no axis (cbpdntv.py:319): ONE norm over the whole gradient array, so its share can only be 0
    # or 1 -- the search stops at the first mu with share 1 (every gradient vector exactly zero),
    # and that is asserted instead.
    'bigmu': ('search', None, {}),
}


def problem(chan):
    rng = np.random.RandomState(7)
    D = rng.randn(6, 6, K)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(24, 32, 2) if chan is None else rng.randn(24, 32, chan)
    return D, S, rng


def zero_share(Y, vector):
    g2 = np.sum(Y[..., 0:2] ** 2, axis=(4, 5) if vector else 5)
    return float(np.mean(g2 == 0.0))


def run(cls, D, S, mu, o, dimK):
    b = cls(D, S, 0.05, mu, ref.ConvBPDNScalarTV.Options(o), dimK=dimK)
    b.solve()
    return b


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
    only = sys.argv[1:]      # case names to (re)write; none: all of them and the step files
    for tag, cls in CLASSES.items():
        vector = tag == 'v'
        for case, (mu, chan, od) in CASES.items():
            if only and case not in only:
                continue
            name = 'tv_%s_%s_f64' % (tag, case)
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
            if mu == 'search':
                window = (0.05, 0.95) if vector else (1.0, 1.0)
                mu, lo, hi = 0.5, None, None
                for _ in range(40):
                    b = run(cls, D, S, mu, o, dimK)
                    share = zero_share(b.Y, vector)
                    print('  %s: mu = %g, zero share %.4f' % (name, mu, share))
                    if window[0] <= share <= window[1]:
                        break
                    if share < window[0]:
                        lo = mu
                    else:
                        hi = mu
                    mu = mu * 2.0 if hi is None else np.sqrt(lo * hi)
                assert window[0] <= share <= window[1], (name, mu, share)
            else:
                b = run(cls, D, S, mu, o, dimK)
                share = zero_share(b.Y, vector)
            if not o.get('FastSolve', False):
                arrs.update(traces(b, name))
            ar = o.get('AutoRho', {})
            arrs.update(
                D=D, S=S, lmbda=np.float64(0.05), mu=np.float64(mu), dimK=np.int64(dimK),
                vector=np.int64(vector), MaxMainIter=np.int64(ITERS), zero_share=np.float64(share),
                opt_AuxVarObj=np.int64(bool(o.get('AuxVarObj', False))),
                opt_rho=np.float64(o.get('rho', np.nan)),
                opt_RelaxParam=np.float64(o.get('RelaxParam', 1.8)),
                opt_AutoRho=np.int64(bool(ar.get('Enabled', True))),
                X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho), recon=b.reconstruct())
            path = os.path.join(OUT, name + '.npz')
            np.savez_compressed(path, **arrs)
            size = os.path.getsize(path)
            assert size < 1000000, (name, size)
            print('%-24s %7.1f KB  mu = %-6g zero share %.3f  ObjFun[-1] = %.4f'
                  % (name, size / 1024.0, mu, share, arrs.get('it_ObjFun', [np.nan])[-1]))

        if only:
            continue
        # a small problem's state after 39 and after 40 iterations
        rng = np.random.RandomState(11)
        D = rng.randn(4, 4, 6)
        D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
        S = rng.randn(12, 16, 2)
        tvw = 0.5 + rng.rand(6)
        o = ref.ConvBPDNScalarTV.Options({'Verbose': False, 'MaxMainIter': ITERS - 1, 'RelStopTol': 0.0,
                                          'TVWeight': tvw})
        b = cls(D, S, 0.05, 0.3, o, dimK=1)
        b.solve()
        arrs = dict(D=D, S=S, lmbda=np.float64(0.05), mu=np.float64(0.3), vector=np.int64(vector),
                    optarr_TVWeight=tvw, k=np.int64(ITERS - 1),
                    Y_before=b.Y.copy(), U_before=b.U.copy(), rho_before=np.float64(b.rho))
        b.opt['MaxMainIter'] = 1
        b.solve()
        arrs.update(X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho))
        its = b.getitstat()
        for f in ('ObjFun', 'DFid', 'RegL1', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'Rho'):
            arrs['last_' + f] = np.float64(getattr(its, f)[-1])
        assert len(its.ObjFun) == ITERS
        path = os.path.join(OUT, 'tv_step_%s_f64.npz' % tag)
        np.savez_compressed(path, **arrs)
        print('%-24s %7.1f KB' % (os.path.basename(path), os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
