#!/usr/bin/env python3
"""Generate the ConvBPDNProjL1 fixtures tests/golden/projl1_*_f64.npz from the UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at
$SPORCO_REFERENCE (default /root/reference) with the import stand-ins of oracle/_stubs, exactly
as tools/make_golden_ball.py does.  Nothing here is read by the test-suite; the tests read the
.npz files alone.

    python tools/make_golden_projl1.py [CASE ...]

Each file holds the seeded inputs, the option values (as arrays), the final X, Y, U and rho,
reconstruct(), and the per-iteration IterationStats traces (all but Time and XSlvRelRes) of a
float64 run of 40 iterations with RelStopTol = 0.  A file is written only when every trace is
finite, and it must stay under 1 MB.

The problem: seed 7, D randn normalised per filter, S randn with the two images scaled by
(small, 1.0), gamma = 4.  Every case records, per image, the share of the 40 iterations whose y step
projected (|| AX + U ||_1 > gamma over the image; AX + U is U + Y after the dual update) and asserts that
one image has a share >= 0.9 and one a share in [0.02, 0.5], and that every trace is finite.  The small
scale is 0.02 unless a case names another one (recorded in the file as `small_scale`): it is adjusted
per case until the reference alone meets the window.  The autorho case asserts that rho moved.
projl1_step_f64.npz holds the `fixed` problem's state after 39 and after 40 iterations.  The y0warm case
is a single image started from a Y0 (one regime: the share assertions do not apply).
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
GAMMA = 4.0

# name: (signal shape, dictionary shape, options, small scale)
SMALL = ((16, 17, 2), (5, 5, 6))
CASES = {
    'default': SMALL + ({}, 0.02),
    'fixed': SMALL + ({'AutoRho': {'Enabled': False}}, 0.02),
    'autorho': SMALL + ({'AutoRho': {'Period': 3, 'Scaling': 2.0}}, 0.02),
    'auxvar': SMALL + ({'rho': 2.0, 'RelaxParam': 1.0, 'AuxVarObj': True, 'AutoRho': {'Enabled': False}}, 0.02),
    'nonneg_nobndry': SMALL + ({'NonNegCoef': True, 'NoBndryCross': True}, 0.017),
    'mcd': ((16, 16, 3, 2), (5, 5, 3, 4), {}, 0.0068),
    'mcs': ((16, 16, 3, 2), (5, 5, 4), {}, 0.006),
    'y0warm': ((16, 17), (5, 5, 6), {}, 1.0),
}


def problem(sshape, dshape, small, seed=7):
    rng = np.random.RandomState(seed)
    D = rng.randn(*dshape)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(*sshape)
    if len(sshape) > 2:
        S = S * np.asarray((small, 1.0)).reshape((1,) * (len(sshape) - 1) + (2,))
    return D, S, rng


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


class Active(object):
    """Callback: per image, whether this iteration's y step projected."""

    def __init__(self):
        self.hits = []
        self.rho = None

    def __call__(self, b):
        # (U was divided by the factor rho moved by, after the dual update: admm.py:573)
        rsf = 1.0 if self.rho is None else float(b.rho) / self.rho
        self.rho = float(b.rho)
        v = b.U * rsf + b.Y
        n1 = np.sum(np.abs(v), axis=b.cri.axisN + (b.cri.axisC, b.cri.axisM))
        self.hits.append(n1 > GAMMA)
        return False


def build(D, S, od, dimK, iters=ITERS, cb=None):
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0, 'Callback': cb}
    o.update(od)
    return ref.ConvBPDNProjL1(D, S, GAMMA, ref.ConvBPDNProjL1.Options(o), dimK=dimK), o


def main():
    only = sys.argv[1:]      # case names to (re)write; none: all of them and the step file
    for case, (sshape, dshape, od, small) in CASES.items():
        if only and case not in only:
            continue
        name = 'projl1_%s_f64' % case
        D, S, rng = problem(sshape, dshape, small)
        od = dict(od)
        dimK = 1 if len(sshape) > 2 else 0
        if case == 'y0warm':
            od['Y0'] = 0.1 * rng.randn(sshape[0], sshape[1], 1, 1, dshape[-1])
        act = Active()
        b, o = build(D, S, od, dimK, cb=act)
        b.solve()
        for v in (b.X, b.Y, b.U):
            assert np.all(np.isfinite(v)), name
        share = np.mean(np.asarray(act.hits, dtype=np.float64), axis=0).ravel()
        if case != 'y0warm':      # (a single image has one regime)
            assert np.any(share >= 0.9) and np.any((share >= 0.02) & (share <= 0.5)), (name, share)
        arrs = traces(b, name)
        if case == 'autorho':
            assert len(set(arrs['it_Rho'])) > 2, name
        ar = b.opt['AutoRho']
        arrs.update(
            D=D, S=S, gamma=np.float64(GAMMA), dimK=np.int64(dimK), MaxMainIter=np.int64(ITERS),
            active_share=share, small_scale=np.float64(small),
            opt_AuxVarObj=np.int64(bool(b.opt['AuxVarObj'])),
            opt_NonNegCoef=np.int64(bool(b.opt['NonNegCoef'])),
            opt_NoBndryCross=np.int64(bool(b.opt['NoBndryCross'])),
            opt_rho=np.float64(o.get('rho', 1.0)), opt_RelaxParam=np.float64(b.opt['RelaxParam']),
            opt_AutoRho=np.int64(bool(ar['Enabled'])), opt_AutoRho_Period=np.int64(ar['Period']),
            opt_AutoRho_Scaling=np.float64(ar['Scaling']), opt_AutoRho_RsdlRatio=np.float64(ar['RsdlRatio']),
            opt_AutoRho_AutoScaling=np.int64(bool(ar['AutoScaling'])),
            opt_AutoRho_RsdlTarget=np.float64(ar['RsdlTarget']),
            X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho), recon=b.reconstruct())
        if 'Y0' in od:
            arrs['optarr_Y0'] = np.asarray(od['Y0'])
        path = os.path.join(OUT, name + '.npz')
        np.savez_compressed(path, **arrs)
        size = os.path.getsize(path)
        assert size < 1000000, (name, size)
        print('%-30s %7.1f KB  active share %s  ObjFun[-1] = %.4f  Cnstr[-1] = %.3e  Rho[-1] = %g'
              % (name, size / 1024.0, np.round(share, 3), arrs['it_ObjFun'][-1], arrs['it_Cnstr'][-1],
                 arrs['it_Rho'][-1]))

    if only:
        return
    # the `fixed` problem's state after 39 and after 40 iterations
    sshape, dshape, od, small = CASES['fixed']
    D, S, _ = problem(sshape, dshape, small)
    b, o = build(D, S, od, 1, ITERS - 1)
    b.solve()
    arrs = dict(D=D, S=S, gamma=np.float64(GAMMA), k=np.int64(ITERS - 1), Y_before=b.Y.copy(),
                U_before=b.U.copy(), rho_before=np.float64(b.rho), opt_RelaxParam=np.float64(b.opt['RelaxParam']))
    b.opt['MaxMainIter'] = 1
    b.solve()
    arrs.update(X=b.X, Y=b.Y, U=b.U, rho_final=np.float64(b.rho))
    its = b.getitstat()
    for f in ('ObjFun', 'Cnstr', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        arrs['last_' + f] = np.float64(getattr(its, f)[-1])
    assert len(its.ObjFun) == ITERS
    for v in arrs.values():
        assert np.all(np.isfinite(v))
    path = os.path.join(OUT, 'projl1_step_f64.npz')
    np.savez_compressed(path, **arrs)
    print('%-30s %7.1f KB' % (os.path.basename(path), os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()
