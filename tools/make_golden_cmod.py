#!/usr/bin/env python3
"""Generate the CnstrMOD / BPDNDictLearn fixtures tests/golden/cmod_*_f64.npz and bpdndl_*_f64.npz from the
UNMODIFIED reference.

TEST INFRASTRUCTURE ONLY, for the authoring machine: the reference package is looked up at $SPORCO_REFERENCE
(default /root/reference) with the import stand-ins of oracle/_stubs, exactly as tools/make_golden_bpdn.py does.
Nothing here is read by the test-suite; the tests read the .npz files alone.

    python tools/make_golden_cmod.py [CASE ...]

Each file holds the seeded inputs, the option values that differ from the defaults (`opt_*`, AutoRho keys as
`opt_AutoRho.Key`; arrays as `optarr_*`), the final X, Y, U and rho and the per-iteration IterationStats traces (all
but Time) of a float64 run with RelStopTol = 0.

The CnstrMOD problem: seed 23, RandomState draws in this order: D = randn(N, M) with unit-norm columns, a sparse
code Z of three non-zeros a column drawn as 0.2 randn (at this scale the default rho is well below its balance
and AutoRho moves it), S = D Z + 0.05 randn, then the optional Y0 (randn with unit-norm columns), U0
(0.05 randn) and Z2 (another sparse code, drawn as randn so that rho moves again; the second `setcoef`).  8 x 16 x 40 unless the case says otherwise, 30
iterations (`k1`: 16; run longer, its float32 residuals reach rounding level and AutoRho follows noise),
AutoRho with Period 4.  `zero_row`: row 3 of Z is set to zero before S is formed.  `z_none`: the object is
made with Z = None and dsz, `setcoef` follows.  `setcoef2`: a solve, `setcoef(Z2)`, a second solve; `Y_first` is the
state between them.

The BPDNDictLearn problem: seed 29, D0 = randn(N, M), a sparse code of three non-zeros a column through a
unit-norm dictionary, S = D X + 0.05 randn; 8 x 16 x 40, 12 outer iterations, both inner AutoRho periods 4;
`refshape`: N, M, K = 8, 4, 8 as in the reference's tests/dictlrn/test_bpdndl.py.

Asserted per case: every trace finite; more than one value of rho where AutoRho is on; `zeromean`: the
unprojected iterate X has a column whose mean is not zero while Y's column means are; every file far below the
repository's file-size limit.  cmod_defaults.npz holds the option defaults of both classes, key by key, and the
IterationStats fields.
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

from sporco.admm import cmod as ref             # noqa: E402
from sporco.dictlrn import bpdndl as refdl      # noqa: E402

OUT = os.path.join(REPO, 'tests', 'golden')
ITERS = 30
DL_ITERS = 12
BASE = {'AutoRho': {'Period': 4}}

# name: ((N, M, K), options, extras)
CASES = {
    'default': ((8, 16, 40), {}, ()),
    'auxvar_off': ((8, 16, 40), {'AuxVarObj': False}, ()),
    'fixedrho': ((8, 16, 40), {'AutoRho': {'Enabled': False}, 'rho': 0.7, 'RelaxParam': 1.0}, ()),
    'zeromean': ((8, 16, 40), {'ZeroMean': True}, ()),
    'y0': ((8, 16, 40), {}, ('Y0',)),
    'y0u0': ((8, 16, 40), {}, ('Y0', 'U0')),
    'returnx': ((8, 16, 40), {'ReturnX': True}, ()),
    'k_lt_m': ((8, 16, 5), {}, ()),
    'k1': ((8, 16, 1), {'MaxMainIter': 16}, ()),
    'z_none': ((8, 16, 40), {}, ('ZNONE',)),
    'setcoef2': ((8, 16, 40), {}, ('Z2',)),
    'zero_row': ((8, 16, 40), {}, ('ZROW',)),
}

# name: ((N, M, K), lmbda, options)
DL_CASES = {
    'default': ((8, 16, 40), 0.1, {}),
    'accurate': ((8, 16, 40), 0.1, {'AccurateDFid': True}),
    'lmbda_none': ((8, 16, 40), None, {}),
    'zeromean': ((8, 16, 40), 0.1, {'CMOD': {'ZeroMean': True}}),
    'refshape': ((8, 4, 8), 0.1, {}),
}


def sparse_code(rng, M, K):
    Z = np.zeros((M, K))
    for k in range(K):
        Z[rng.permutation(M)[:min(3, M)], k] = rng.randn(min(3, M))
    return Z


def problem(dims, extras, seed=23):
    N, M, K = dims
    rng = np.random.RandomState(seed)
    D = rng.randn(N, M)
    D /= np.sqrt(np.sum(D ** 2, axis=0, keepdims=True))
    Z = 0.2 * sparse_code(rng, M, K)
    if 'ZROW' in extras:
        Z[3] = 0.0
    S = D.dot(Z) + 0.05 * rng.randn(N, K)
    arrs = {}
    if 'Y0' in extras:
        Y0 = rng.randn(N, M)
        arrs['Y0'] = Y0 / np.sqrt(np.sum(Y0 ** 2, axis=0, keepdims=True))
    if 'U0' in extras:
        arrs['U0'] = 0.05 * rng.randn(N, M)
    if 'Z2' in extras:
        arrs['Z2'] = sparse_code(rng, M, K)
    return Z, S, arrs


def merged(od, iters):
    o = {'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0}
    for src in (BASE, od):
        for k, v in src.items():
            if isinstance(v, dict):
                o.setdefault(k, {}).update(v)
            else:
                o[k] = v
    return o


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


def flat_options(o, prefix='opt_'):
    out = {}
    for k, v in o.items():
        if k == 'Verbose':
            continue
        if isinstance(v, dict):
            for kk, vv in v.items():
                if isinstance(vv, dict):
                    for k3, v3 in vv.items():
                        out['%s%s.%s.%s' % (prefix, k, kk, k3)] = np.float64(v3)
                else:
                    out['%s%s.%s' % (prefix, k, kk)] = np.float64(vv)
        else:
            out[prefix + k] = np.float64(v)
    return out


def save(path, out, note):
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 100000, (path, size)
    print('%-30s %6.1f KB  %s' % (os.path.basename(path), size / 1024.0, note))


def run_cmod(only):
    for case, (dims, od, extras) in CASES.items():
        if only and case not in only:
            continue
        Z, S, arrs = problem(dims, extras)
        o = merged(od, ITERS)
        o.update({k: v for k, v in arrs.items() if k in ('Y0', 'U0')})
        opt = ref.CnstrMOD.Options(o)
        extra = {}
        if 'ZNONE' in extras:
            b = ref.CnstrMOD(None, S, (dims[1], dims[2]), opt)
            b.setcoef(Z)
        else:
            b = ref.CnstrMOD(Z, S, (dims[1], dims[2]), opt)
        if case == 'setcoef2':
            b.solve()
            extra['Y_first'] = np.array(b.Y)
            extra['rho_first'] = np.float64(b.rho)
            b.itstat = []
            b.setcoef(arrs['Z2'])
        res = b.solve()
        for v in (b.X, b.Y, b.U):
            assert np.all(np.isfinite(v)), case
        if bool(b.opt['AutoRho', 'Enabled']):
            assert len(set(float(i.Rho) for i in b.itstat)) > 1, case
        if case == 'zeromean':
            # (X approaches the constraint set as the run converges: far above rounding is what is asked)
            assert np.max(np.abs(np.mean(b.X, axis=0))) > 1e-8, case
            assert np.max(np.abs(np.mean(b.Y, axis=0))) < 1e-14, case
            extra['x_colmean_max'] = np.float64(np.max(np.abs(np.mean(b.X, axis=0))))
        if case == 'returnx':
            assert res is b.X
        if case == 'zero_row':
            assert not np.any(Z[3]) and not np.any(Z.dot(Z.T)[3])
        out = traces(b, case)
        out.update(flat_options(merged(od, ITERS)))
        out.update(Z=Z, S=S, X=np.array(b.X), Y=np.array(b.Y), U=np.array(b.U), rho_final=np.float64(b.rho),
                   rho0=np.float64(out['it_Rho'][0]))
        for k, v in arrs.items():
            out['optarr_' + k] = np.asarray(v)
        out.update(extra)
        save(os.path.join(OUT, 'cmod_%s_f64.npz' % case), out,
             'DFid[-1] = %.6f  Cnstr[-1] = %.2e  %d rho values' % (out['it_DFid'][-1], out['it_Cnstr'][-1],
                                                                    len(set(out['it_Rho']))))


def dl_problem(dims, seed=29):
    N, M, K = dims
    rng = np.random.RandomState(seed)
    D0 = rng.randn(N, M)
    Dt = rng.randn(N, M)
    Dt /= np.sqrt(np.sum(Dt ** 2, axis=0, keepdims=True))
    S = Dt.dot(sparse_code(rng, M, K)) + 0.05 * rng.randn(N, K)
    return D0, S


def dl_options(od, iters):
    o = {'Verbose': False, 'MaxMainIter': iters, 'BPDN': {'AutoRho': {'Period': 4}}, 'CMOD': {'AutoRho': {'Period': 4}}}
    for k, v in od.items():
        if isinstance(v, dict):
            o[k].update(v)
        else:
            o[k] = v
    return o


def run_dl(only):
    for case, (dims, lmbda, od) in DL_CASES.items():
        if only and ('dl_' + case) not in only:
            continue
        D0, S = dl_problem(dims)
        o = dl_options(od, DL_ITERS)
        d = refdl.BPDNDictLearn(D0, S, lmbda, refdl.BPDNDictLearn.Options(o))
        D1 = d.solve()
        out = traces(d, case)
        assert len(out['it_ObjFun']) == DL_ITERS
        assert len(set(out['it_XRho'])) > 1 or len(set(out['it_DRho'])) > 1, case
        if case == 'zeromean':
            assert np.max(np.abs(np.mean(d.dstep.X, axis=0))) > 1e-8
            assert np.max(np.abs(np.mean(D1, axis=0))) < 1e-14
        out.update(flat_options(o))
        out.update(D0=D0, S=S, lmbda_given=np.float64(0.0 if lmbda is None else lmbda),
                   lmbda=np.float64(d.xstep.lmbda), D=np.array(D1), X=np.array(d.getcoef()),
                   DX=np.array(d.dstep.X), DU=np.array(d.dstep.U), XU=np.array(d.xstep.U),
                   xrho_final=np.float64(d.xstep.rho), drho_final=np.float64(d.dstep.rho))
        save(os.path.join(OUT, 'bpdndl_%s_f64.npz' % case), out,
             'ObjFun[-1] = %.6f  %d / %d rho values' % (out['it_ObjFun'][-1], len(set(out['it_XRho'])),
                                                       len(set(out['it_DRho']))))


def defaults():
    out = {}
    for name, cls in (('CnstrMOD', ref.CnstrMOD), ('BPDNDictLearn', refdl.BPDNDictLearn)):
        keys, vals = [], []

        def walk(prefix, d):
            for k, v in sorted(d.items()):
                if isinstance(v, dict):
                    walk(prefix + k + '.', v)
                else:
                    keys.append(prefix + k)
                    vals.append(repr(v))
        walk('', dict(cls.Options()))
        out[name + '_keys'] = np.array(keys)
        out[name + '_values'] = np.array(vals)
    out['CnstrMOD_fields'] = np.array(ref.CnstrMOD.IterationStats._fields)
    Z, S, _ = problem((8, 16, 40), ())
    out['CnstrMOD_default_rho'] = np.float64(ref.CnstrMOD(Z, S, (16, 40)).rho)
    save(os.path.join(OUT, 'cmod_defaults.npz'), out, '%d + %d keys' % (len(out['CnstrMOD_keys']),
                                                                       len(out['BPDNDictLearn_keys'])))


if __name__ == '__main__':
    only = sys.argv[1:]
    run_cmod(only)
    run_dl(only)
    if not only or 'defaults' in only:
        defaults()
