"""sporco_amd.admm.pdcsc.ConvProdDictL1L1Grd / ConvProdDictL1L1GrdJoint against the reference's fixtures
(tests/golden/pdl1_*_f64.npz, float64 runs of the unmodified reference written by
tools/make_golden_pdl1.py) and, for what no fixture reaches, against the NumPy restatement of
tests/_pdl1_numpy.py, which is itself pinned to the reference first.

Tolerances are the project's: float64 1e-9 relative l2 on X, Y, U, reconstruct(), every trace and
the final rho; float32 input 1e-4 on X, Y and reconstruct() and 1e-3 on the traces, both against
the float64 reference.
"""

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _pdl1_numpy as pln

CASES = ['default', 'mask', 'gradw', 'nonneg', 'auxvar', 'autorho', 'joint', 'joint_autorho', 'rankdef', 'oddw', 'cb9']
FIXTURES = ['pdl1_%s_f64' % n for n in CASES]
TRACES = ('ObjFun', 'DFid', 'RegL1', 'RegGrad', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho')
FIELDS = ('Iter', 'ObjFun', 'DFid', 'RegL1', 'RegGrad', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho',
          'XSlvRelRes', 'Time')


def fields_of(joint):
    return tuple('RegL21' if f == 'RegL1' else f for f in FIELDS) if joint else FIELDS


def traces_of(g):
    return tuple('RegL21' if f == 'RegL1' else f for f in TRACES) if bool(g['joint']) else TRACES


def autorho_of(g):
    if not bool(g['opt_AutoRho']):
        return None
    return dict(pln.AUTORHO_DEFAULT, Period=int(g['opt_AutoRho_Period']), RsdlRatio=float(g['opt_AutoRho_RsdlRatio']))


def options_of(g, extra=None):
    o = {'Verbose': False, 'MaxMainIter': int(g['MaxMainIter']), 'RelStopTol': 0.0, 'rho': float(g['opt_rho'])}
    if bool(g['opt_AuxVarObj']):
        o['AuxVarObj'] = True
    if bool(g['opt_NonNegCoef']):
        o['NonNegCoef'] = True
    if bool(g['opt_LinSolveCheck']):
        o['LinSolveCheck'] = True
    ar = autorho_of(g)
    if ar is not None:
        o['AutoRho'] = {'Enabled': True, 'Period': ar['Period'], 'RsdlRatio': ar['RsdlRatio']}
    if 'optarr_GradWeight' in g:
        o['GradWeight'] = g['optarr_GradWeight']
    o.update(extra or {})
    return o


def build(g, dtype=np.float64, extra=None):
    from sporco_amd.admm import pdcsc
    o = options_of(g, extra)
    if 'GradWeight' in o and np.ndim(o['GradWeight']):
        o['GradWeight'] = np.asarray(o['GradWeight']).astype(dtype)
    D, B, S = g['D'].astype(dtype), g['B'].astype(dtype), g['S'].astype(dtype)
    if bool(g['joint']):
        return pdcsc.ConvProdDictL1L1GrdJoint(D, B, S, float(g['lmbda']), float(g['mu']),
                                              pdcsc.ConvProdDictL1L1GrdJoint.Options(o), dimK=int(g['dimK']))
    W = g['optarr_W'].astype(dtype) if 'optarr_W' in g else None
    return pdcsc.ConvProdDictL1L1Grd(D, B, S, float(g['lmbda']), float(g['mu']), W, pdcsc.ConvProdDictL1L1Grd.Options(o),
                                     dimK=int(g['dimK']))


def signal5(g):
    S = g['S']
    return S.reshape(S.shape[:2] + ((S.shape[2], S.shape[3], 1) if int(g['dimK']) else (S.shape[2], 1, 1)))


def restated(g, maxiter=None, **kw):
    """The restatement's solve of a fixture's problem."""
    D, S5 = g['D'], signal5(g)
    kw.setdefault('D', D.reshape(D.shape[:2] + (1, 1, -1)))
    kw.setdefault('B', g['B'])
    return pln.admm_pdl1(kw.pop('D'), kw.pop('B'), S5, float(g['lmbda']), float(g['mu']),
                         int(g['MaxMainIter']) if maxiter is None else maxiter,
                         W=g['optarr_W'].astype(np.float64).reshape(S5.shape) if 'optarr_W' in g else 1.0,
                         wg=g['optarr_GradWeight'] if 'optarr_GradWeight' in g else 1.0, rho=float(g['opt_rho']),
                         auxvar=bool(g['opt_AuxVarObj']), ar=autorho_of(g), joint=bool(g['joint']),
                         nonneg=bool(g['opt_NonNegCoef']), check=bool(g['opt_LinSolveCheck']), **kw)


def check(b, g, tol, tol_tr, with_u=True):
    its = b.getitstat()
    figs = {v: rel_l2(getattr(b, v), g[v]) for v in (('X', 'Y', 'U') if with_u else ('X', 'Y'))}
    figs['recon'] = rel_l2(b.reconstruct(), g['recon'])
    trs = {f: rel_l2(getattr(its, f), g['it_' + f]) for f in traces_of(g)}
    print(figs, trs, 'rho', float(b.rho), float(g['rho_final']))
    for v, e in figs.items():
        assert e < tol, (v, e)
    for f, e in trs.items():
        assert e < tol_tr, (f, e)
    assert abs(float(b.rho) - float(g['rho_final'])) <= tol_tr * float(g['rho_final'])
    # shapes: the composite Y / U, block 0 with the signal's Cs channels, block 1 and X with Cb
    Cs, Cb = g['B'].shape
    H, W = g['S'].shape[:2]
    assert b.X.shape == g['X'].shape and b.Y.shape == g['Y'].shape and b.U.shape == g['U'].shape
    assert b.Y.shape == (H, W, b.y0I + b.y1I) and b.Y.shape == b.yshp
    assert b.block_sep0(b.Y).shape == signal5(g).shape and b.block_sep0(b.Y).shape[2] == Cs
    assert b.block_sep1(b.Y).shape == g['X'].shape and b.block_sep1(b.Y).shape[2] == Cb
    assert rel_l2(b.block_cat(b.block_sep0(b.Y), b.block_sep1(b.Y)), b.Y) == 0.0
    assert b.reconstruct().shape == g['recon'].shape and g['recon'].shape[2] == Cs


# ---- 1. the restatement and the fixtures -------------------------------------------------------------
def test_numpy_restatement_pinned_to_fixtures():
    """The algebra as built -- the mixed right-hand side, the diagonal-plus-rank-one solve, the block-0
    constraint spectrum as its by-product, the overridden dual residual -- reproduces every fixture, and
    one iteration from the reference's state after 39 iterations reproduces its state after 40 (float64,
    1e-9)."""
    for name in FIXTURES:
        g = load_golden(name)
        r = restated(g)
        for v in ('X', 'Y', 'U', 'recon'):
            assert rel_l2(r[v], g[v]) < 1e-9, (name, v)
        for f in traces_of(g):
            assert rel_l2(r[f], g['it_' + f]) < 1e-9, (name, f)
        assert abs(r['rho'] - float(g['rho_final'])) < 1e-9 * float(g['rho_final'])
        assert rel_l2(r['Gamma'], g['Gamma']) < 1e-9
        if bool(g['opt_LinSolveCheck']):
            assert r['XSlvRelRes'].max() < 1e-12
    g = load_golden('pdl1_step_f64')
    D, S, B = g['D'], g['S'], g['B']
    H, W = S.shape[:2]
    S5 = S.reshape(S.shape + (1,))
    shpX = (H, W, B.shape[1], S.shape[3], D.shape[2])
    Y0, Y1 = pln.block_sep(g['Y_before'], S5.shape, shpX)
    U0, U1 = pln.block_sep(g['U_before'], S5.shape, shpX)
    st = dict(Y0=Y0, Y1=Y1, U0=U0, U1=U1, rho=float(g['rho_before']))
    r = pln.admm_pdl1(D.reshape(D.shape[:2] + (1, 1, -1)), B, S5, float(g['lmbda']), float(g['mu']), 1, state=st,
                      k0=int(g['k']))
    for v in ('X', 'Y', 'U'):
        assert rel_l2(r[v], g[v]) < 1e-9, v
    assert abs(r['rho'] - float(g['rho_final'])) < 1e-9 * float(g['rho_final'])
    for f in ('ObjFun', 'DFid', 'RegL1', 'RegGrad', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert abs(r[f][-1] - float(g['last_' + f])) <= 1e-9 * abs(float(g['last_' + f])), f


def test_fixtures_take_both_branches():
    """What tools/make_golden_pdl1.py asserted when it wrote the files, from the files: both branches of
    the block-1 threshold in every case, of the block-0 threshold where Cb < Cs, of the l2,1 shrinkage
    in the joint cases; a rho that moves in the autorho cases; a (numerically) zero eigenvalue in the
    rank-deficient ones."""
    for name in FIXTURES:
        g = load_golden(name)
        Cs, Cb = g['B'].shape
        shp0, shp1 = signal5(g).shape, g['X'].shape
        Y0, Y1 = pln.block_sep(g['Y'], shp0, shp1)
        nz0, nz1 = np.mean(Y0 != 0.0), np.mean(Y1 != 0.0)
        assert 0.05 <= nz1 <= 0.95 and nz1 == float(g['nz_y1']), (name, nz1)
        assert nz0 == float(g['nz_y0'])
        if Cb < Cs:
            assert 0.05 <= nz0 <= 0.95, (name, nz0)
        if bool(g['joint']):
            share = np.mean(np.sum(Y1 ** 2, axis=2) == 0.0)
            assert 0.05 <= share <= 0.95 and share == float(g['zero_groups']), (name, share)
        if bool(g['opt_AutoRho']):
            assert len(set(g['it_Rho'])) >= 2, name
    for name in ('pdl1_rankdef_f64', 'pdl1_cb9_f64'):
        g = load_golden(name)
        assert g['Gamma'].min() < 1e-14 * g['Gamma'].max()


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f64(backend, name):
    g = load_golden(name)
    b = build(g, np.float64)
    b.solve()
    check(b, g, 1e-9, 1e-9)
    assert b.getitstat()._fields == fields_of(bool(g['joint']))
    assert rel_l2(b.Gamma, g['Gamma']) < 1e-9 and b.Q.shape == g['Q'].shape and b.B.shape == g['B'].shape
    if bool(g['opt_LinSolveCheck']):
        x = np.array(b.getitstat().XSlvRelRes)
        print('XSlvRelRes max', x.max())
        assert x.max() < 1e-4
    # which form of pdl1_solve ran: read back from the handle
    iters = int(g['MaxMainIter'])
    assert b._solve_form_counts() == ((0, iters) if name in ('pdl1_oddw_f64', 'pdl1_cb9_f64') else (iters, 0))


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f32(backend, name):
    g = load_golden(name)
    b = build(g, np.float32)
    b.solve()
    assert b.X.dtype == np.float32 and b.Y.dtype == np.float32 and b.Gamma.dtype == np.float64
    check(b, g, 1e-4, 1e-3, with_u=False)
    if bool(g['opt_LinSolveCheck']):
        assert np.array(b.getitstat().XSlvRelRes).max() < 1e-4


# ---- 2. the reference's own two tests (tests/admm/test_pdcsc.py 03, 04) --------------------------------
@pytest.mark.parametrize('joint', [False, True], ids=['l1l1grd', 'joint'])
def test_reference_scenarios(backend, joint):
    from sporco_amd.admm import pdcsc
    np.random.seed(12345)
    D = np.random.randn(5, 5, 4)
    B = np.random.randn(3, 4)
    s = np.random.randn(16, 17, 3)
    if joint:
        opt = pdcsc.ConvProdDictL1L1GrdJoint.Options({'LinSolveCheck': True, 'MaxMainIter': 200})
        b = pdcsc.ConvProdDictL1L1GrdJoint(D, B, s, 1e-1, 1e-2, opt=opt, dimK=0)
    else:
        opt = pdcsc.ConvProdDictL1L1Grd.Options({'LinSolveCheck': True, 'MaxMainIter': 200, 'rho': 5e-1})
        b = pdcsc.ConvProdDictL1L1Grd(D, B, s, 1e-1, 1e-2, opt=opt, dimK=0)
    b.solve()
    its = b.getitstat()
    assert its._fields == fields_of(joint)
    assert np.array(its.XSlvRelRes).max() < 1e-4
    assert b.X.shape == (16, 17, 4, 1, 4) and np.all(np.isfinite(b.X))
    assert b.Y.shape == (16, 17, 3 + 16) and b.reconstruct().shape == (16, 17, 3, 1)


# ---- 3. kernel forms ------------------------------------------------------------------------------------
def test_generic_form_forced_on_a_wave_shape(backend, monkeypatch):
    """K = 8, Cb = 3 takes the wave form; the same problem with the generic form forced (the handle's
    switch, read when it is made) agrees with it to 1e-9."""
    g = load_golden('pdl1_default_f64')
    a = build(g, extra={'MaxMainIter': 10})
    a.solve()
    monkeypatch.setenv('SPORCO_AMD_PDL1_GENERIC', '1')
    b = build(g, extra={'MaxMainIter': 10})
    monkeypatch.delenv('SPORCO_AMD_PDL1_GENERIC')
    b.solve()
    assert a._solve_form_counts() == (10, 0) and b._solve_form_counts() == (0, 10)
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(b, v), getattr(a, v)) < 1e-9, v
    assert rel_l2(b.reconstruct(), a.reconstruct()) < 1e-9
    ia, ib = a.getitstat(), b.getitstat()
    for f in TRACES:
        assert rel_l2(getattr(ib, f), getattr(ia, f)) < 1e-9, f
    assert np.array(ib.XSlvRelRes).max() < 1e-12 and np.array(ia.XSlvRelRes).max() < 1e-12


# 64 x 64, K = 64 (32 lanes a system, two systems a wave), Cs = 3, Cb = 6, N = 2, a mask and a per-filter
# GradWeight: a size no fixture reaches, against the restatement (computed once)
_BIG = {}
BIG_ITERS, BIG_LMBDA, BIG_MU = 10, 0.05, 0.01


def _big_problem():
    if not _BIG:
        rng = np.random.RandomState(21)
        D = rng.randn(6, 6, 64)
        D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
        S = rng.randn(64, 64, 3, 2)
        B = rng.randn(3, 6)
        B /= np.sqrt(np.sum(B ** 2, axis=0, keepdims=True))
        W = (rng.rand(64, 64, 3, 2) > 0.2).astype(np.float64)
        wg = np.linspace(0.5, 2.0, 64)
        ref = pln.admm_pdl1(D.reshape(6, 6, 1, 1, 64), B, S.reshape(64, 64, 3, 2, 1), BIG_LMBDA, BIG_MU, BIG_ITERS,
                            W=W.reshape(64, 64, 3, 2, 1), wg=wg)
        _BIG.update(D=D, S=S, B=B, W=W, wg=wg, ref=ref)
    return _BIG


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,tol', [(np.float64, 1e-9), (np.float32, 1e-4)], ids=['f64', 'f32'])
def test_gpu_full_wave(gpu_backend, dtype, tol):
    from sporco_amd.admm import pdcsc
    p = _big_problem()
    ref = p['ref']
    # (both branches of both thresholds are taken: the bounds of tests/test_pdcsc.py _run_form)
    assert 0.02 < np.mean(ref['Y1'] != 0.0) < 0.98 and 0.02 < np.mean(ref['Y0'] != 0.0) < 0.98
    o = pdcsc.ConvProdDictL1L1Grd.Options({'Verbose': False, 'MaxMainIter': BIG_ITERS, 'RelStopTol': 0.0,
                                           'GradWeight': p['wg'].astype(dtype)})
    b = pdcsc.ConvProdDictL1L1Grd(p['D'].astype(dtype), p['B'].astype(dtype), p['S'].astype(dtype), BIG_LMBDA, BIG_MU,
                                  p['W'].astype(dtype), o, dimK=1)
    b.solve()
    assert b._solve_form_counts() == (BIG_ITERS, 0)
    figs = {v: rel_l2(getattr(b, v), ref[v]) for v in ('X', 'Y')}
    figs['recon'] = rel_l2(b.reconstruct(), ref['recon'])
    its = b.getitstat()
    trs = {f: rel_l2(getattr(its, f), ref[f]) for f in TRACES}
    print(figs, trs)
    for v, e in figs.items():
        assert e < tol, (v, e)
    for f, e in trs.items():
        assert e < tol, (f, e)


# ---- 4. setdict, warm start, options ---------------------------------------------------------------------
@pytest.mark.parametrize('which', ['B', 'D'])
def test_setdict_between_two_solves(backend, which):
    """10 iterations, setdict(B=) or setdict(D=), 10 more: the state carries over, the tables and the
    dictionary spectrum are the new ones (against the restatement continued from its own state)."""
    g = load_golden('pdl1_oddw_f64')
    rng = np.random.RandomState(3)
    D2, B2 = rng.randn(*g['D'].shape), rng.randn(*g['B'].shape)
    b = build(g, extra={'MaxMainIter': 10})
    b.solve()
    r = restated(g, maxiter=10)
    if which == 'B':
        b.setdict(B=B2)
        r2 = restated(g, maxiter=10, B=B2, state=r['state'], k0=10)
        assert rel_l2(b.Gamma, r2['Gamma']) < 1e-12
    else:
        b.setdict(D=D2.reshape(b.cri.shpD))
        r2 = restated(g, maxiter=10, D=D2.reshape(D2.shape[:2] + (1, 1, -1)), state=r['state'], k0=10)
    b.solve()
    for v in ('X', 'Y', 'U', 'recon'):
        assert rel_l2(b.reconstruct() if v == 'recon' else getattr(b, v), r2[v]) < 1e-9, v
    its = b.getitstat()
    assert len(its.ObjFun) == 20
    for f in TRACES:
        assert rel_l2(np.array(getattr(its, f))[10:], r2[f]) < 1e-9, f


def test_warm_start_composite(backend):
    """Y0 / U0 in the composite shape: 20 iterations, then 20 more from the uploaded arrays, equal 40 in
    one go."""
    g = load_golden('pdl1_default_f64')
    a = build(g, extra={'MaxMainIter': 20})
    a.solve()
    assert a.Y.shape == g['Y'].shape
    b = build(g, extra={'MaxMainIter': 20, 'Y0': a.Y, 'U0': a.U})
    assert rel_l2(b.Y, a.Y) == 0.0 and rel_l2(b.U, a.U) == 0.0
    b.solve()
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(b, v), g[v]) < 1e-9, v
    assert rel_l2(b.getitstat().ObjFun, g['it_ObjFun'][20:]) < 1e-9
    assert rel_l2(b.reconstruct(g['X']), g['recon']) < 1e-9
    with pytest.raises(ValueError):
        build(g, extra={'Y0': a.Y[..., :-1]})


def test_nobndrycross_and_highmemsolve(backend):
    """NoBndryCross acts on block 1 (against the restatement); HighMemSolve changes nothing."""
    g = load_golden('pdl1_oddw_f64')
    a = build(g, extra={'MaxMainIter': 8, 'NoBndryCross': True, 'HighMemSolve': True})
    a.solve()
    r = restated(g, maxiter=8, nobndry=True)
    dH, dW = g['D'].shape[:2]
    Y1 = a.block_sep1(a.Y)
    assert np.all(Y1[-(dH - 1):] == 0.0) and np.all(Y1[:, -(dW - 1):] == 0.0) and np.any(Y1 != 0.0)
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(a, v), r[v]) < 1e-9, v
    b = build(g, extra={'MaxMainIter': 8, 'HighMemSolve': True})
    c = build(g, extra={'MaxMainIter': 8})
    b.solve()
    c.solve()
    assert rel_l2(b.Y, c.Y) == 0.0


def test_joint_defaults_and_weights(backend):
    """opt=None constructs (the reference fails on opt['L21Weight']); a scalar L21Weight scales the
    threshold and the RegL21 term; L1Weight is ignored; an array L21Weight is refused."""
    from sporco_amd.admm import pdcsc
    g = load_golden('pdl1_oddw_f64')
    D, B, S = g['D'], g['B'], g['S']
    b = pdcsc.ConvProdDictL1L1GrdJoint(D, B, S, 0.05, 0.01, dimK=0)
    assert b.X.shape == g['X'].shape and float(b.wl21) == 1.0
    o = {'Verbose': False, 'MaxMainIter': 8, 'RelStopTol': 0.0, 'rho': 5.0}
    a = pdcsc.ConvProdDictL1L1GrdJoint(D, B, S, 0.05, 0.01, pdcsc.ConvProdDictL1L1GrdJoint.Options(
        dict(o, L21Weight=2.0, L1Weight=7.0)), dimK=0)
    a.solve()
    S5 = signal5(g)
    r = pln.admm_pdl1(D.reshape(D.shape[:2] + (1, 1, -1)), B, S5, 0.05, 0.01, 8, rho=5.0, joint=True, wl21=2.0)
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(a, v), r[v]) < 1e-9, v
    its = a.getitstat()
    for f in ('ObjFun', 'RegL21', 'DFid', 'RegGrad', 'PrimalRsdl', 'DualRsdl'):
        assert rel_l2(getattr(its, f), r[f]) < 1e-9, f
    with pytest.raises(NotImplementedError):
        pdcsc.ConvProdDictL1L1GrdJoint(D, B, S, 0.05, 0.01, pdcsc.ConvProdDictL1L1GrdJoint.Options(
            dict(o, L21Weight=np.ones((16, 17, 1, 6)))), dimK=0)


# ---- 5. refusals ------------------------------------------------------------------------------------
def test_refusals(backend):
    import pickle
    from sporco_amd.admm import cbpdn, pdcsc
    from sporco_amd.device import DeviceArray
    rng = np.random.RandomState(0)
    D, B, S = rng.randn(4, 4, 6), rng.randn(3, 2), rng.randn(12, 12, 3)
    for cls in (pdcsc.ConvProdDictL1L1Grd, pdcsc.ConvProdDictL1L1GrdJoint):
        args = (0.1, 0.01)
        opt = cls.Options({'MaxMainIter': 2})
        with pytest.raises(ValueError, match='Only single-channel convolutional dictionaries are supported'):
            cls(rng.randn(4, 4, 3, 6), B, S, *args, opt=opt, dimK=0)
        with pytest.raises(NotImplementedError):
            cls(rng.randn(4, 6), B, rng.randn(32, 3), *args, opt=opt, dimN=1)
        with pytest.raises(NotImplementedError):
            cls(rng.randn(3, 3, 3, 6), B, rng.randn(8, 8, 8, 3), *args, opt=opt, dimN=3)
        with pytest.raises(NotImplementedError):
            cls(D.astype(complex), B, S.astype(complex), *args, opt=opt)
        with pytest.raises(NotImplementedError):
            cls(D, B, S, *args, opt=opt, reducer=object())
        with pytest.raises(NotImplementedError):
            cls(D, B, S, *args, opt=opt, resident=True)
        with pytest.raises(NotImplementedError):
            cls(D, B, DeviceArray((12, 12, 3), np.float64), *args, opt=opt)
        with pytest.raises(NotImplementedError):
            cbpdn.AddMaskSim(cls, D, S, np.ones((12, 12)), *args, opt=opt)
        with pytest.raises(NotImplementedError):
            cls(D, rng.randn(3, 17), S, *args, opt=opt, dimK=0)
        b = cls(D, B, S, *args, opt=opt, dimK=0)
        with pytest.raises(NotImplementedError):
            pickle.dumps(b)
        with pytest.raises(NotImplementedError):
            b._set_ams(np.ones((12, 12, 1, 1, 1)))
        b.rhochange()
        b.solve()
        assert b.X.shape == (12, 12, 2, 1, 6) and b.Y.shape == (12, 12, 3 + 12)
    assert set(('ConvProdDictL1L1Grd', 'ConvProdDictL1L1GrdJoint')) <= set(pdcsc.__all__)
