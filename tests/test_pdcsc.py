"""sporco_amd.admm.pdcsc.ConvProdDictBPDN / ConvProdDictBPDNJoint against the reference's fixtures
(tests/golden/pd_*_f64.npz, float64 runs of the unmodified reference written by
tools/make_golden_pd.py) and, for the kernel forms and at the GPU size, against the NumPy restatement
of tests/_pd_numpy.py, which is itself pinned to the reference first.

Tolerances are the project's: float64 1e-9 relative l2 on X, Y, U, reconstruct(), every trace and
the final rho; float32 input 1e-4 on X, Y and reconstruct() and 1e-3 on the traces, both against
the float64 reference.
"""

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _pd_numpy as pdn

CASES = ['default', 'joint', 'rankdef', 'l1w', 'nonneg', 'fixedrho', 'auxvar', 'oddw', 'cb9']
FIXTURES = ['pd_%s_f64' % n for n in CASES]
TRACES = ('ObjFun', 'DFid', 'RegL1', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho')
FIELDS = ('Iter', 'ObjFun', 'DFid', 'RegL1', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho', 'XSlvRelRes',
          'Time')
FIELDS_JOINT = FIELDS[:4] + ('RegL21',) + FIELDS[4:]


def traces_of(g):
    return TRACES + (('RegL21',) if bool(g['joint']) else ())


def options_of(g, extra=None):
    o = {'Verbose': False, 'MaxMainIter': int(g['MaxMainIter']), 'RelStopTol': 0.0,
         'RelaxParam': float(g['opt_RelaxParam'])}
    if bool(g['opt_AuxVarObj']):
        o['AuxVarObj'] = True
    if bool(g['opt_NonNegCoef']):
        o['NonNegCoef'] = True
    if not np.isnan(g['opt_rho']):
        o['rho'] = float(g['opt_rho'])
    if not bool(g['opt_AutoRho']):
        o['AutoRho'] = {'Enabled': False}
    if 'optarr_L1Weight' in g:
        o['L1Weight'] = g['optarr_L1Weight']
    o.update(extra or {})
    return o


def build(g, dtype=np.float64, extra=None):
    from sporco_amd.admm import pdcsc
    o = options_of(g, extra)
    if 'L1Weight' in o and np.ndim(o['L1Weight']):
        o['L1Weight'] = np.asarray(o['L1Weight']).astype(dtype)
    D, B, S = g['D'].astype(dtype), g['B'].astype(dtype), g['S'].astype(dtype)
    if bool(g['joint']):
        return pdcsc.ConvProdDictBPDNJoint(D, B, S, float(g['lmbda']), float(g['mu']),
                                           pdcsc.ConvProdDictBPDNJoint.Options(o), dimK=int(g['dimK']))
    return pdcsc.ConvProdDictBPDN(D, B, S, float(g['lmbda']), pdcsc.ConvProdDictBPDN.Options(o), dimK=int(g['dimK']))


def signal5(g):
    S = g['S']
    return S.reshape(S.shape[:2] + ((S.shape[2], S.shape[3], 1) if int(g['dimK']) else (S.shape[2], 1, 1)))


def restated(g, **kw):
    """The restatement's solve of a fixture's problem."""
    D = g['D']
    return pdn.admm_pd(D.reshape(D.shape[:2] + (1, 1, -1)), g['B'], signal5(g), float(g['lmbda']),
                       int(g['MaxMainIter']), mu=float(g['mu']), joint=bool(g['joint']),
                       wl1=g['optarr_L1Weight'].astype(np.float64) if 'optarr_L1Weight' in g else 1.0,
                       rho=None if np.isnan(g['opt_rho']) else float(g['opt_rho']),
                       rlx=float(g['opt_RelaxParam']), auto_rho=bool(g['opt_AutoRho']),
                       gevaly=bool(g['opt_AuxVarObj']), fevalx=not bool(g['opt_AuxVarObj']),
                       nonneg=bool(g['opt_NonNegCoef']), **kw)


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
    # shapes: the channel axis of the coefficient maps is Cb, that of the reconstruction Cs
    assert b.X.shape == g['X'].shape and b.Y.shape == g['Y'].shape and b.U.shape == g['U'].shape
    assert b.X.shape[2] == g['B'].shape[1] and b.cri.shpX == g['X'].shape
    assert b.reconstruct().shape == g['recon'].shape and g['recon'].shape[2] == g['B'].shape[0]


# ---- 1. the restatement and the fixtures -------------------------------------------------------------
def test_numpy_restatement_pinned_to_fixtures():
    """The algebra as built -- mix, scaled rank-one solve, mix back, fidelity through B Q -- reproduces
    every fixture, and one iteration from the reference's state after 39 iterations reproduces its
    state after 40 (float64, 1e-9)."""
    for name in FIXTURES:
        g = load_golden(name)
        r = restated(g)
        for v in ('X', 'Y', 'U', 'recon'):
            assert rel_l2(r[v], g[v]) < 1e-9, (name, v)
        for f in traces_of(g):
            assert rel_l2(r[f], g['it_' + f]) < 1e-9, (name, f)
        assert abs(r['rho'] - float(g['rho_final'])) < 1e-9 * float(g['rho_final'])
        gam, Q = pdn.eig(g['B'])
        assert rel_l2(gam, g['Gamma']) < 1e-9
    g = load_golden('pd_step_f64')
    D, S, B = g['D'], g['S'], g['B']
    H, W = S.shape[:2]
    Df = np.fft.rfftn(D.reshape(D.shape[:2] + (1, 1, -1)), s=(H, W), axes=(0, 1))
    Sf = np.fft.rfftn(S.reshape(S.shape + (1,)), axes=(0, 1))
    gam, Q = pdn.eig(B)
    st = dict(Y=g['Y_before'], U=g['U_before'], rho=float(g['rho_before']))
    lm = float(g['lmbda'])
    rec = pdn.iterate(st, Df, Sf, B, gam, Q, 1.0, lm, 0.0, 1.8, False, True, True, int(g['k']), (H, W),
                      rho_xi=pdn.default_rho_xi(lm))
    for v in ('X', 'Y', 'U'):
        assert rel_l2(st[v], g[v]) < 1e-9, v
    assert abs(st['rho'] - float(g['rho_final'])) < 1e-9 * float(g['rho_final'])
    for f in ('ObjFun', 'DFid', 'RegL1', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert abs(rec[f] - float(g['last_' + f])) <= 1e-9 * abs(float(g['last_' + f])), f


def test_fixtures_take_both_branches():
    """The joint fixture exercises both branches of the l2,1 shrinkage (share of exactly-zero channel
    groups of the final Y inside [0.05, 0.95], and the one stored), the default one both branches of
    the soft threshold, and the rank-deficient ones have a (numerically) zero eigenvalue."""
    g = load_golden('pd_joint_f64')
    share = np.mean(np.sum(g['Y'] ** 2, axis=2) == 0.0)
    assert 0.05 <= share <= 0.95 and share == float(g['zero_share']), share
    g = load_golden('pd_default_f64')
    assert 0.05 <= np.mean(g['Y'] != 0.0) <= 0.95
    for name in ('pd_rankdef_f64', 'pd_cb9_f64'):
        g = load_golden(name)
        assert g['B'].shape[1] > g['B'].shape[0] and g['Gamma'].min() < 1e-14 * g['Gamma'].max()


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f64(backend, name):
    g = load_golden(name)
    b = build(g, np.float64)
    b.solve()
    check(b, g, 1e-9, 1e-9)
    assert b.getitstat()._fields == (FIELDS_JOINT if bool(g['joint']) else FIELDS)
    assert rel_l2(b.Gamma, g['Gamma']) < 1e-9 and b.Q.shape == g['Q'].shape and b.B.shape == g['B'].shape


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f32(backend, name):
    g = load_golden(name)
    b = build(g, np.float32)
    b.solve()
    assert b.Y.dtype == np.float32 and b.Gamma.dtype == np.float64
    check(b, g, 1e-4, 1e-3, with_u=False)


# ---- 2. options ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['pd_default_f64', 'pd_rankdef_f64', 'pd_cb9_f64'])
def test_linsolvecheck(backend, name):
    """The eigen-channel rank-one solves solve the reference's system, a zero eigenvalue included, in
    the wave form (default, rankdef) and in the generic form (cb9)."""
    g = load_golden(name)
    b = build(g, np.float64, extra={'LinSolveCheck': True})
    b.solve()
    x = np.array(b.getitstat().XSlvRelRes)
    print('XSlvRelRes max', x.max())
    assert x.max() < 1e-9
    check(b, g, 1e-9, 1e-9)
    wave, generic = b._solve_form_counts()
    assert (wave, generic) == ((0, 40) if name == 'pd_cb9_f64' else (40, 0))


@pytest.mark.parametrize('joint', [False, True], ids=['bpdn', 'joint'])
def test_identity_b_equals_convbpdn(backend, joint):
    """B = I: the product dictionary is the plain multi-channel problem."""
    from sporco_amd.admm import cbpdn, pdcsc
    rng = np.random.RandomState(5)
    D = rng.randn(5, 5, 6)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(16, 17, 3, 2)
    o = {'Verbose': False, 'MaxMainIter': 15, 'RelStopTol': 0.0}
    if joint:
        a = pdcsc.ConvProdDictBPDNJoint(D, np.eye(3), S, 0.05, 0.03, pdcsc.ConvProdDictBPDNJoint.Options(o), dimK=1)
        c = cbpdn.ConvBPDNJoint(D, S, 0.05, 0.03, cbpdn.ConvBPDNJoint.Options(o), dimK=1)
    else:
        a = pdcsc.ConvProdDictBPDN(D, np.eye(3), S, 0.05, pdcsc.ConvProdDictBPDN.Options(o), dimK=1)
        c = cbpdn.ConvBPDN(D, S, 0.05, cbpdn.ConvBPDN.Options(o), dimK=1)
    a.solve()
    c.solve()
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(a, v), getattr(c, v)) < 1e-9, v
    assert rel_l2(a.reconstruct(), c.reconstruct()) < 1e-9
    ia, ic = a.getitstat(), c.getitstat()
    for f in TRACES + (('RegL21',) if joint else ()):
        assert rel_l2(getattr(ia, f), getattr(ic, f)) < 1e-9, f


def test_setdict(backend):
    g = load_golden('pd_oddw_f64')
    rng = np.random.RandomState(3)
    D2 = rng.randn(*g['D'].shape)
    B2 = rng.randn(*g['B'].shape)
    for kw, g2 in (({'B': B2}, dict(g, B=B2)), ({'D': D2}, dict(g, D=D2)), ({'D': D2, 'B': B2}, dict(g, D=D2, B=B2))):
        b = build(g, extra={'MaxMainIter': 10})
        if 'D' in kw:
            kw = dict(kw, D=D2.reshape(b.cri.shpD))
        b.setdict(**kw)
        b.solve()
        c = build(g2, extra={'MaxMainIter': 10})
        c.solve()
        for v in ('X', 'Y', 'U'):
            assert rel_l2(getattr(b, v), getattr(c, v)) < 1e-12, (sorted(kw), v)
        assert rel_l2(b.reconstruct(), c.reconstruct()) < 1e-12
        assert rel_l2(b.getitstat().ObjFun, c.getitstat().ObjFun) < 1e-12
        assert rel_l2(b.Gamma, c.Gamma) < 1e-12


def test_second_solve_continues(backend):
    """20 + 20 iterations equal 40."""
    g = load_golden('pd_default_f64')
    b = build(g, extra={'MaxMainIter': 20})
    b.solve()
    b.solve()
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(b, v), g[v]) < 1e-9, v
    its = b.getitstat()
    assert len(its.ObjFun) == 40
    for f in TRACES:
        assert rel_l2(getattr(its, f), g['it_' + f]) < 1e-9, f


def test_warm_start_and_returnx(backend):
    """Y0 / U0: 20 iterations, then 20 more from the uploaded arrays, equal 40 in one go."""
    g = load_golden('pd_fixedrho_f64')
    a = build(g, extra={'MaxMainIter': 20})
    a.solve()
    b = build(g, extra={'MaxMainIter': 20, 'Y0': a.Y, 'U0': a.U, 'ReturnX': True})
    X = b.solve()
    assert rel_l2(X, b.X) == 0.0
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(b, v), g[v]) < 1e-9, v
    assert rel_l2(b.getitstat().ObjFun, g['it_ObjFun'][20:]) < 1e-9
    assert rel_l2(b.reconstruct(g['Y']), g['recon']) < 1e-9


def test_nobndrycross_and_highmemsolve(backend):
    """NoBndryCross zeroes the boundary band of Y in every channel of the coefficient maps;
    HighMemSolve changes nothing."""
    g = load_golden('pd_oddw_f64')
    a = build(g, extra={'MaxMainIter': 8, 'NoBndryCross': True, 'HighMemSolve': True})
    a.solve()
    dH, dW = g['D'].shape[:2]
    assert np.all(a.Y[-(dH - 1):] == 0.0) and np.all(a.Y[:, -(dW - 1):] == 0.0) and np.any(a.Y != 0.0)
    b = build(g, extra={'MaxMainIter': 8, 'HighMemSolve': True})
    c = build(g, extra={'MaxMainIter': 8})
    b.solve()
    c.solve()
    assert rel_l2(b.Y, c.Y) == 0.0


# ---- 3. the reference's own two tests (tests/admm/test_pdcsc.py 01, 02) --------------------------------
@pytest.mark.parametrize('joint', [False, True], ids=['bpdn', 'joint'])
def test_reference_scenarios(backend, joint):
    from sporco_amd.admm import pdcsc
    np.random.seed(12345)
    D = np.random.randn(5, 5, 4)
    B = np.random.randn(3, 4)
    s = np.random.randn(16, 17, 3)
    if joint:
        opt = pdcsc.ConvProdDictBPDNJoint.Options({'LinSolveCheck': True})
        b = pdcsc.ConvProdDictBPDNJoint(D, B, s, 1e-1, 1e-2, opt=opt, dimK=0)
    else:
        opt = pdcsc.ConvProdDictBPDN.Options({'LinSolveCheck': True})
        b = pdcsc.ConvProdDictBPDN(D, B, s, 1e-1, opt=opt, dimK=0)
    X = b.solve()
    assert X.shape == (16, 17, 4, 1, 4) and np.all(np.isfinite(X))
    its = b.getitstat()
    assert its._fields == (FIELDS_JOINT if joint else FIELDS)
    assert np.array(its.XSlvRelRes).max() < 1e-4
    assert b.reconstruct().shape == (16, 17, 3, 1)


# ---- 4. kernel forms: against the restatement, computed once per module ----------------------------------
# (K, Cb, N): the wave form with G = K / 2 = 1, 4, 32 and 64 lanes a system, the generic form by an
# odd K, by a K / 2 that is no power of two and by the channel count; every Cb of {1, 3, 8, 9} and both
# N of {1, 3} occur in either form where the form admits them.  Cs = 4 throughout, so B is rank
# deficient for Cb = 8, 9.
FORM_CASES = [(2, 1, 1), (2, 3, 3), (8, 3, 3), (8, 8, 1), (8, 1, 3), (64, 3, 1), (64, 8, 3), (128, 3, 1), (128, 1, 3),
              (128, 8, 1), (7, 3, 1), (7, 8, 3), (6, 3, 3), (6, 1, 1), (8, 9, 3), (2, 9, 1), (64, 9, 1), (7, 9, 3), (6, 9, 3),
              (128, 9, 1)]
FORM_ITERS, FORM_LMBDA = 10, 0.05
GRID_THREADS = 4096 * 256      # csrc: grid_for caps a grid at kMaxPartialBlocks blocks of kThreads
_FORM = {}


def expect_wave(K, Cb):
    g = K // 2
    return K % 2 == 0 and g & (g - 1) == 0 and 1 <= g <= 64 and Cb <= 8


def _form_problem(K, Cb, N, shape=(16, 24), Cs=4, iters=FORM_ITERS):
    key = (K, Cb, N, iters) + shape
    if key not in _FORM:
        H, W = shape
        rng = np.random.RandomState(11)
        D = rng.randn(5, 5, K)
        D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
        S = rng.randn(H, W, Cs, N)
        B = rng.randn(Cs, Cb)
        B /= np.sqrt(np.sum(B ** 2, axis=0, keepdims=True))
        ref = pdn.admm_pd(D.reshape(5, 5, 1, 1, K), B, S.reshape(H, W, Cs, N, 1), FORM_LMBDA, iters)
        _FORM[key] = (D, B, S, ref)
    return _FORM[key]


def _run_form(K, Cb, N, dtype, tol, tol_tr, iters=FORM_ITERS, **kw):
    from sporco_amd import _lib
    from sporco_amd.admm import pdcsc
    D, B, S, ref = _form_problem(K, Cb, N, iters=iters, **kw)
    assert len(set(ref['Rho'])) > 1 and 0.02 < np.mean(ref['Y'] != 0.0) < 0.98
    o = pdcsc.ConvProdDictBPDN.Options({'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0})
    b = pdcsc.ConvProdDictBPDN(D.astype(dtype), B.astype(dtype), S.astype(dtype), FORM_LMBDA, o, dimK=1)
    b.solve()
    # which kernel ran: read back from the handle, so that a dispatch mistake cannot pass as agreement of
    # the generic kernel with itself (the device's filter count is K itself at these shapes)
    assert b._dev.query(_lib.QUERY_DEVICE_FILTERS) == K
    assert b._solve_form_counts() == ((iters, 0) if expect_wave(K, Cb) else (0, iters))
    figs = {v: rel_l2(getattr(b, v), ref[v]) for v in ('X', 'Y')}
    figs['recon'] = rel_l2(b.reconstruct(), ref['recon'])
    its = b.getitstat()
    trs = {f: rel_l2(getattr(its, f), ref[f]) for f in TRACES}
    print((K, Cb, N), figs, trs)
    for v, e in figs.items():
        assert e < tol, (v, e)
    for f, e in trs.items():
        assert e < tol_tr, (f, e)


@pytest.mark.parametrize('dtype,tol,tol_tr', [(np.float64, 1e-9, 1e-9), (np.float32, 1e-4, 1e-4)], ids=['f64', 'f32'])
@pytest.mark.parametrize('K,Cb,N', FORM_CASES)
def test_kernel_forms(backend, K, Cb, N, dtype, tol, tol_tr):
    _run_form(K, Cb, N, dtype, tol, tol_tr)


@pytest.mark.gpu
def test_gpu_full_wave(gpu_backend):
    """The wave form with full waves: G = 32 lanes a system, two systems a wave, 64 x 49 x 2 systems
    (784 blocks: below the grid cap, every lane makes one trip of the grid-stride loop)."""
    assert 64 * 49 * 2 * 32 < GRID_THREADS
    _run_form(64, 6, 2, np.float32, 1e-4, 1e-4, shape=(64, 96), Cs=3)


@pytest.mark.gpu
def test_gpu_grid_stride_wraps(gpu_backend):
    """The size at which the grid-stride loop of the wave form wraps: 128 x 81 frequency pixels x 2
    images x G = 64 lanes are 1 327 104 lanes on the capped grid of 4096 x 256 threads, so a quarter of
    the threads make a second trip and a block's partial sums (DFid) accumulate over trips.  3
    iterations (rho moves in the third) keep the float64 restatement of this size to a few seconds."""
    assert 128 * 81 * 2 * 64 > GRID_THREADS
    _run_form(128, 2, 2, np.float32, 1e-4, 1e-4, iters=3, shape=(128, 160), Cs=3)


# ---- 5. refusals ------------------------------------------------------------------------------------
def test_refusals(backend):
    import pickle
    from sporco_amd.admm import cbpdn, pdcsc
    from sporco_amd.device import DeviceArray
    rng = np.random.RandomState(0)
    D, B, S = rng.randn(4, 4, 6), rng.randn(3, 2), rng.randn(12, 12, 3)
    for cls, args in ((pdcsc.ConvProdDictBPDN, (0.1,)), (pdcsc.ConvProdDictBPDNJoint, (0.1, 0.01))):
        opt = cls.Options({'MaxMainIter': 2})
        with pytest.raises(ValueError):
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
        assert not b._fused_ok() and not b._device_loop_ok()
        b.rhochange()
        b.solve()
        assert b.X.shape == (12, 12, 2, 1, 6)


def test_xstep_override_passes_through(backend):
    g = load_golden('pd_oddw_f64')
    a, b = build(g, extra={'MaxMainIter': 8}), build(g, extra={'MaxMainIter': 8})
    b.xstep = lambda: type(b).xstep(b)
    a.solve()
    b.solve()
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(a, v), getattr(b, v)) < 1e-12, v
