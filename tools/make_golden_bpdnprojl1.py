#!/usr/bin/env python3
"""Generate the BPDNProjL1 fixtures tests/golden/bpdnprojl1_*_f64.npz from the UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at $SPORCO_REFERENCE
(default /root/reference) with the import stand-ins of oracle/_stubs, exactly as tools/make_golden_bpdn.py does.
Nothing here is read by the test-suite; the tests read the .npz files alone.

    python tools/make_golden_bpdnprojl1.py [CASE ...]

Each file holds the seeded inputs D and S, gamma, the option values that differ from the defaults (`opt_*`, AutoRho
keys as `opt_AutoRho.Key`; arrays as `optarr_*`), the final X, Y, U and rho, and the per-iteration IterationStats
traces (all but Time) of a float64 run of ITERS iterations with RelStopTol = 0.

The problem is that of tools/make_golden_bpdn.py (seed 11: D = randn(N, M) with unit-norm columns, a sparse code of
three non-zeros a column, S = D X0 + 0.05 randn, then the optional Y0, U0 and D2), 8 x 16 x 5 unless the case says
otherwise.  gamma = 1.0 puts every column of the least-squares solution outside its ball; AutoRho runs with Period 2.
Asserted per case: every trace finite; more than one value of rho where AutoRho is on; every column of Y within its
ball; `nonneg`: some element of the unclipped run's Y is negative; `inside`: no column of any X + U ever left the ball
(Y equals X to rounding at the end and Cnstr is zero throughout); `mixed`: at the last iteration some columns of X
lie inside and some outside (gamma = 4.5, between the l1 norms of the unconstrained columns).  `k1` has the shape of
the reference's test_14 with gamma = 2.5: at gamma = 1 its single column settles on one entry, the dual residual is
exactly zero from the third iteration on and AutoRho drives rho to 1e15, where the traces are rounding noise.
bpdnprojl1_defaults.npz holds the option defaults and the IterationStats fields.
"""

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.environ.get('SPORCO_REFERENCE', '/root/reference'))
sys.path.insert(0, os.path.join(REPO, 'oracle', '_stubs'))
sys.path.insert(0, HERE)
warnings.filterwarnings('ignore')

from sporco.admm import bpdn as ref     # noqa: E402
from make_golden_bpdn import problem     # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
ITERS = 24
GAMMA = 1.0
BASE = {'AutoRho': {'Period': 2}}

# name: ((N, M, K), gamma, options, extras)
CASES = {
    'default': ((8, 16, 5), GAMMA, {}, ()),
    'auxvar_off': ((8, 16, 5), GAMMA, {'AuxVarObj': False}, ()),
    'fixedrho': ((8, 16, 5), GAMMA, {'AutoRho': {'Enabled': False}, 'rho': 0.7, 'RelaxParam': 1.0}, ()),
    'stdres': ((8, 16, 5), GAMMA, {'AutoRho': {'StdResiduals': True}}, ()),
    'lsc': ((8, 16, 5), GAMMA, {'LinSolveCheck': True}, ()),
    'nonneg': ((8, 16, 5), GAMMA, {'NonNegCoef': True}, ()),
    'inside': ((8, 16, 5), 100.0, {}, ()),
    'mixed': ((8, 16, 5), 4.5, {}, ()),
    'y0': ((8, 16, 5), GAMMA, {}, ('Y0',)),
    'y0u0': ((8, 16, 5), GAMMA, {}, ('Y0', 'U0')),
    'returnx': ((8, 16, 5), GAMMA, {'ReturnX': True}, ()),
    'square': ((8, 8, 5), GAMMA, {}, ()),
    'tall': ((24, 16, 5), GAMMA, {}, ()),
    'k1': ((8, 16, 1), 2.5, {}, ()),
    'setdict': ((8, 16, 5), GAMMA, {}, ('D2',)),
}


def merged(od, iters):
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0}
    for src in (BASE, od):
        for k, v in src.items():
            if isinstance(v, dict):
                o.setdefault(k, {}).update(v)
            else:
                o[k] = v
    return o


def build(D, S, gamma, od, arrs, iters=ITERS):
    o = merged(od, iters)
    o.update({k: v for k, v in arrs.items() if k != 'D2'})
    return ref.BPDNProjL1(D, S, gamma, ref.BPDNProjL1.Options(o))


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


def flat_options(od, iters):
    out = {}
    for k, v in merged(od, iters).items():
        if k == 'Verbose':
            continue
        if isinstance(v, dict):
            for kk, vv in v.items():
                out['opt_%s.%s' % (k, kk)] = np.float64(vv)
        else:
            out['opt_' + k] = np.float64(v)
    return out


def defaults():
    d = ref.BPDNProjL1.Options().__class__.defaults
    keys, vals = [], []
    for k, v in sorted(d.items()):
        if isinstance(v, dict):
            for kk, vv in sorted(v.items()):
                keys.append('%s.%s' % (k, kk))
                vals.append(repr(vv))
        else:
            keys.append(k)
            vals.append(repr(v))
    np.savez_compressed(os.path.join(OUT, 'bpdnprojl1_defaults.npz'), keys=np.array(keys), values=np.array(vals),
                        fields=np.array(ref.BPDNProjL1.IterationStats._fields),
                        hdrtxt=np.array(ref.BPDNProjL1.hdrtxt()))
    print('bpdnprojl1_defaults.npz  %d keys' % len(keys))


def run(only):
    for case, (dims, gamma, od, extras) in CASES.items():
        if only and case not in only:
            continue
        D, S, arrs = problem(dims, extras)
        b = build(D, S, gamma, od, arrs)
        extra = {}
        if case == 'setdict':
            b.solve()
            extra['Y_first'] = np.array(b.Y)
            b.itstat = []
            b.setdict(arrs['D2'])
        b.solve()
        for v in (b.X, b.Y, b.U):
            assert np.all(np.isfinite(v)), case
        if bool(b.opt['AutoRho', 'Enabled']):
            assert len(set(float(i.Rho) for i in b.itstat)) > 1, case
        l1y, l1x = np.sum(np.abs(b.Y), axis=0), np.sum(np.abs(b.X), axis=0)
        assert np.all(l1y <= gamma * (1 + 1e-12)), case
        if case == 'nonneg':
            u = build(D, S, gamma, {k: v for k, v in od.items() if k != 'NonNegCoef'}, arrs)
            u.solve()
            assert np.any(u.Y < 0) and not np.any(b.Y < 0), case
            extra['negative_unclipped'] = np.int64(np.sum(u.Y < 0))
        if case == 'inside':
            assert np.all(l1y < 0.5 * gamma) and all(i.Cnstr == 0.0 for i in b.itstat), case
        if case == 'mixed':
            assert np.any(l1x < 0.99 * gamma) and np.any(l1x > (1 + 1e-6) * gamma), (case, l1x)
        if case == 'returnx':
            assert b.getmin() is b.X
        out = traces(b, case)
        out.update(flat_options(od, ITERS))
        out.update(D=D, S=S, gamma=np.float64(gamma), rho0=np.float64(out['it_Rho'][0]), X=np.array(b.X),
                   Y=np.array(b.Y), U=np.array(b.U), rho_final=np.float64(b.rho))
        for k, v in arrs.items():
            out['optarr_' + k] = np.asarray(v)
        out.update(extra)
        path = os.path.join(OUT, 'bpdnprojl1_%s_f64.npz' % case)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size < 100000, (case, size)
        print('%-32s %5.1f KB  ObjFun[-1] = %.6f  Cnstr[-1] = %.2e  %d rho values  l1(X) %s'
              % (os.path.basename(path), size / 1024.0, out['it_ObjFun'][-1], out['it_Cnstr'][-1],
                 len(set(out['it_Rho'])), np.round(l1x, 2)))
    if not only or 'defaults' in only:
        defaults()


if __name__ == '__main__':
    run(sys.argv[1:])
