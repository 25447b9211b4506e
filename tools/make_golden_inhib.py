#!/usr/bin/env python3
"""Generate the ConvBPDNInhib fixtures tests/golden/inhib_*.npz from the UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at
$SPORCO_REFERENCE (default /root/reference) with the import stand-ins of oracle/_stubs, exactly
as oracle/make_golden.py does.  Nothing here is read by the test-suite; the tests read the
.npz files alone.

    python tools/make_golden_inhib.py

Each file holds the seeded inputs, the option values (as arrays), the final X, Y, U, wml, wms and
rho, reconstruct(), and the per-iteration IterationStats traces of a float64 run.  A file is
written only when every trace is finite and |ObjFun| < 1e6.
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

from sporco.admm import cbpdnin as ref     # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
ITERS = 40
K = 8


def problem(dimN):
    rng = np.random.RandomState(7)
    if dimN == 2:
        D, S = rng.randn(6, 6, K), rng.randn(32, 40, 2)
    else:
        D, S = rng.randn(6, K), rng.randn(96, 3)
    D /= np.sqrt(np.sum(D ** 2, axis=tuple(range(dimN)), keepdims=True))
    return D, S, rng


PAIR = np.append(np.eye(K // 2), np.eye(K // 2), axis=-1)
OVER = np.zeros((3, K))
OVER[0, :4] = 1
OVER[1, 2:6] = 1
OVER[2, 5:] = 1

# name: (Wg, mu, gamma, Whn, dimN, options)
CASES = {
    'inhib_latself_f64': (PAIR, 0.5, 0.02, None, 2, {}),
    'inhib_lat_f64': (PAIR, 0.5, 0.0, None, 2, {}),
    'inhib_self_f64': (None, 0.0, 0.02, None, 2, {}),
    'inhib_nonneg_f64': (PAIR, 0.5, 0.02, None, 2, {'NonNegCoef': True}),
    'inhib_whn5_f64': (PAIR, 0.5, 0.02, 5, 2, {}),
    'inhib_signals_f64': (PAIR, 0.5, 0.02, None, 1, {}),
    'inhib_l1w_f64': (PAIR, 0.5, 0.02, None, 2, {'L1Weight': 'uniform'}),
    'inhib_nobndry_f64': (PAIR, 0.5, 0.02, None, 2, {'NoBndryCross': True}),
    'inhib_overlap_f64': (OVER, 0.5, 0.02, None, 2, {}),
    'inhib_fixedrho_f64': (PAIR, 0.5, 0.02, None, 2, {'rho': 2.0, 'RelaxParam': 1.0,
                                                    'AutoRho': {'Enabled': False}}),
    'inhib_auxvar_f64': (PAIR, 0.5, 0.02, None, 2, {'AuxVarObj': True}),
    'inhib_inactive_f64': (None, None, 0.0, None, 2, {}),
}


def main():
    for name, (Wg, mu, gamma, Whn, dimN, od) in CASES.items():
        D, S, rng = problem(dimN)
        od = dict(od)
        arrs = {}
        if od.get('L1Weight') == 'uniform':
            od['L1Weight'] = 0.5 + rng.rand(32, 40, 1, 2, K)
            arrs['optarr_L1Weight'] = od['L1Weight']
        o = {'Verbose': False, 'MaxMainIter': ITERS, 'RelStopTol': 0.0}
        o.update(od)
        b = ref.ConvBPDNInhib(D, S, Wg=Wg, Whn=Whn, lmbda=0.05, mu=mu, gamma=gamma,
                              opt=ref.ConvBPDNInhib.Options(o), dimK=1, dimN=dimN)
        b.solve()
        its = b.getitstat()
        for f in its._fields:
            if f in ('Time', 'XSlvRelRes'):
                continue
            v = np.asarray(getattr(its, f), dtype=np.float64)
            assert np.all(np.isfinite(v)), (name, f)
            arrs['it_' + f] = v
        assert np.all(np.abs(arrs['it_ObjFun']) < 1e6), name
        ar = o.get('AutoRho', {})
        arrs.update(
            D=D, S=S, lmbda=np.float64(0.05), mu=np.float64(b.mu), gamma=np.float64(b.gamma),
            Whn=np.int64(0 if Whn is None else Whn), dimN=np.int64(dimN), dimK=np.int64(1),
            MaxMainIter=np.int64(ITERS),
            opt_NonNegCoef=np.int64(bool(o.get('NonNegCoef', False))),
            opt_NoBndryCross=np.int64(bool(o.get('NoBndryCross', False))),
            opt_AuxVarObj=np.int64(bool(o.get('AuxVarObj', False))),
            opt_rho=np.float64(o.get('rho', np.nan)),
            opt_RelaxParam=np.float64(o.get('RelaxParam', 1.8)),
            opt_AutoRho=np.int64(bool(ar.get('Enabled', True))),
            X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho), recon=b.reconstruct(),
            wml=np.asarray(b.wml, dtype=np.float64), wms=np.asarray(b.wms, dtype=np.float64))
        if Wg is not None:
            arrs['Wg'] = Wg
        path = os.path.join(OUT, name + '.npz')
        np.savez_compressed(path, **arrs)
        print('%-24s %7.1f KB  ObjFun[-1] = %.4f' % (name, os.path.getsize(path) / 1024.0,
                                                      arrs['it_ObjFun'][-1]))


if __name__ == '__main__':
    main()
