"""sporco_amd.admm.cbpdn.ConvL1L1Grd against the reference's fixtures (tests/golden/l1l1_*_f64.npz,
float64 runs of the unmodified reference written by tools/make_golden_l1l1.py) and, at the GPU
sizes, against the NumPy restatement of tests/_l1l1_numpy.py, which is itself pinned to the
reference first.

Tolerances are the project's: float64 1e-9 relative l2 on X, Y, U, reconstruct(), every trace and
the final rho; float32 input 1e-4 on X, Y and reconstruct() and 1e-3 on the traces, both against
the float64 reference -- except the float32 DualRsdl trace, see F32_DUAL_MEASURED.
"""

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _l1l1_numpy as ln

CASES = ['default', 'mask', 'autorho', 'fixed', 'gradw', 'nonneg_nobndry', 'mcd', 'mcs']
FIXTURES = ['l1l1_%s_f64' % n for n in CASES]
TRACES = ('ObjFun', 'DFid', 'RegL1', 'RegGrad', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho')
FIELDS = ('Iter', 'ObjFun', 'DFid', 'RegL1', 'RegGrad', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho',
          'XSlvRelRes', 'Time')
AUTORHO = {'Enabled': True, 'Period': 3, 'Scaling': 2.0, 'RsdlRatio': 1.2, 'AutoScaling': True, 'RsdlTarget': 1.0}

# DualRsdl is a norm of differences of successive iterates, and the float32 error of the iterates is
# not small against it late in a run.  Measured, not taken from the library: the NumPy restatement run
# in float32 against each float64 fixture, worst relative error of an entry of the DualRsdl trace --
# 5.95e-4 (gradw; default 5.6e-4, autorho 1.1e-4, the others below 6e-5); as a relative l2 error of the
# whole trace the worst is 2.2e-6 (mcd).  Allowed: four times the measured value (summation order),
# never below the project's 1e-3.
F32_DUAL_MEASURED = 5.95e-4
F32_DUAL_TOL = max(4.0 * F32_DUAL_MEASURED, 1e-3)
F32_DUAL_TOL_L2 = max(4.0 * 2.2e-6, 1e-3)


def options_of(g, extra=None):
    o = {'Verbose': False, 'MaxMainIter': int(g['MaxMainIter']), 'RelStopTol': 0.0, 'rho': float(g['opt_rho']),
         'RelaxParam': float(g['opt_RelaxParam'])}
    if bool(g['opt_AuxVarObj']):
        o['AuxVarObj'] = True
    if bool(g['opt_NonNegCoef']):
        o['NonNegCoef'] = True
    if bool(g['opt_NoBndryCross']):
        o['NoBndryCross'] = True
    if bool(g['opt_AutoRho']):
        o['AutoRho'] = dict(AUTORHO)
    if 'optarr_GradWeight' in g:
        o['GradWeight'] = g['optarr_GradWeight']
    o.update(extra or {})
    return o


def build(g, dtype=np.float64, extra=None, **over):
    from sporco_amd.admm import cbpdn
    o = options_of(g, extra)
    if 'GradWeight' in o and np.ndim(o['GradWeight']):
        o['GradWeight'] = np.asarray(o['GradWeight']).astype(dtype)
    W = over.pop('W', g['W'].astype(dtype) if 'W' in g else None)
    mu = over.pop('mu', float(g['mu']))
    D = over.pop('D', g['D']).astype(dtype)
    assert not over
    return cbpdn.ConvL1L1Grd(D, g['S'].astype(dtype), float(g['lmbda']), mu, W, cbpdn.ConvL1L1Grd.Options(o),
                             dimK=int(g['dimK']))


def five(g):
    """D, S and W of a fixture in the restatement's five-dimensional layout."""
    D, S = g['D'], g['S']
    D5 = D.reshape(D.shape[:2] + ((D.shape[2], 1, D.shape[3]) if D.ndim == 4 else (1, 1, D.shape[2])))
    S5 = S.reshape(S.shape[:2] + ((S.shape[2], S.shape[3], 1) if S.ndim == 4 else (1, S.shape[2], 1)))
    W5 = g['W'].reshape(g['W'].shape + (1, 1, 1)) if 'W' in g else 1.0
    return D5, S5, W5


def restated(g, dtype=np.float64, **kw):
    """The restatement's solve of a fixture's problem."""
    D5, S5, W5 = five(g)
    ar = dict(AUTORHO) if bool(g['opt_AutoRho']) else None
    args = dict(W=W5, wg=g['optarr_GradWeight'] if 'optarr_GradWeight' in g else 1.0, rho=float(g['opt_rho']),
                rlx=float(g['opt_RelaxParam']), auxvar=bool(g['opt_AuxVarObj']), ar=ar,
                nonneg=bool(g['opt_NonNegCoef']), nobndry=bool(g['opt_NoBndryCross']), dtype=dtype)
    args.update(kw)
    return ln.admm_l1l1(D5, S5, float(g['lmbda']), float(g['mu']), int(g['MaxMainIter']), **args)


def check(b, g, tol, tol_tr, with_u=True, f32=False):
    its = b.getitstat()
    figs = {v: rel_l2(getattr(b, v), g[v]) for v in (('X', 'Y', 'U') if with_u else ('X', 'Y'))}
    figs['recon'] = rel_l2(b.reconstruct(), g['recon'])
    trs = {f: rel_l2(getattr(its, f), g['it_' + f]) for f in TRACES}
    dual = np.max(np.abs(np.asarray(its.DualRsdl) - g['it_DualRsdl']) / np.abs(g['it_DualRsdl']))
    print(figs, trs, 'DualRsdl worst entry', dual, 'rho', float(b.rho), float(g['rho_final']))
    for v, e in figs.items():
        assert e < tol, (v, e)
    for f, e in trs.items():
        assert e < (F32_DUAL_TOL_L2 if f32 and f == 'DualRsdl' else tol_tr), (f, e)
    assert dual < (F32_DUAL_TOL if f32 else tol_tr)
    assert abs(float(b.rho) - float(g['rho_final'])) <= tol_tr * float(g['rho_final'])
    assert b.X.shape == g['X'].shape and b.Y.shape == g['Y'].shape and b.U.shape == g['U'].shape
    assert b.var_y0().shape == g['Y0'].shape and b.var_y1().shape == g['Y1'].shape
    assert b.reconstruct().shape == g['recon'].shape


def same_run(a, b, tol=1e-9, traces=TRACES):
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(a, v), getattr(b, v)) < tol, v
    ia, ib = a.getitstat(), b.getitstat()
    for f in traces:
        assert rel_l2(getattr(ia, f), getattr(ib, f)) < tol, f


# ---- 1. the restatement and the fixtures -------------------------------------------------------------
def test_numpy_restatement_pinned_to_fixtures():
    """The iteration as built reproduces every fixture, and one iteration from the reference's state
    after 39 iterations reproduces its state after 40 (float64, 1e-9)."""
    for name in FIXTURES:
        g = load_golden(name)
        r = restated(g)
        for v in ('X', 'Y', 'U', 'recon'):
            assert rel_l2(r[v].reshape(g[v].shape), g[v]) < 1e-9, (name, v)
        for f in TRACES:
            assert rel_l2(r[f], g['it_' + f]) < 1e-9, (name, f)
        assert abs(r['rho'] - float(g['rho_final'])) < 1e-9 * float(g['rho_final'])
    g = load_golden('l1l1_step_f64')
    D5, S5, _ = five(dict(g, dimK=1))
    H, W = S5.shape[:2]
    Df = np.fft.rfftn(D5, s=(H, W), axes=(0, 1))
    Yb, Ub = g['Y_before'], g['U_before']
    st = dict(Y0=Yb[..., :1], Y1=Yb[..., 1:], U0=Ub[..., :1], U1=Ub[..., 1:], rho=np.float64(g['rho_before']))
    one = np.float64(1.0)
    rec = ln.iterate(st, Df, S5, one, one, one, float(g['lmbda']), float(g['mu']), 1.8, False, None, int(g['k']),
                     (H, W), D5.shape[:2])
    assert rel_l2(st['X'], g['X']) < 1e-9
    assert rel_l2(ln.block_cat(st['Y0'], st['Y1']), g['Y']) < 1e-9
    assert rel_l2(ln.block_cat(st['U0'], st['U1']), g['U']) < 1e-9
    for f in ('ObjFun', 'DFid', 'RegL1', 'RegGrad', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert abs(rec[f] - float(g['last_' + f])) <= 1e-9 * abs(float(g['last_' + f])), f


def test_fixtures_take_both_branches():
    """Both blocks of every fixture take both branches of the soft threshold: the share of non-zero
    entries of the final y0 and y1 lies in [0.05, 0.95] (and is the one stored); rho moves in the
    autorho fixture."""
    for name in FIXTURES:
        g = load_golden(name)
        for blk in ('Y0', 'Y1'):
            share = float(np.mean(g[blk] != 0.0))
            assert 0.05 <= share <= 0.95 and share == float(g['nz_' + blk.lower()]), (name, blk, share)
    assert len(set(load_golden('l1l1_autorho_f64')['it_Rho'])) > 2


def test_f32_dual_tolerance_is_the_measured_one():
    """The constant above is what the restatement gives in float32 (the measurement, repeated on two
    fixtures: the worst one and a multi-channel one)."""
    worst = 0.0
    for name in ('l1l1_gradw_f64', 'l1l1_mcd_f64'):
        g = load_golden(name)
        r = restated(g, np.float32)
        worst = max(worst, float(np.max(np.abs(r['DualRsdl'] - g['it_DualRsdl']) / np.abs(g['it_DualRsdl']))))
    print('float32 restatement, worst DualRsdl entry error', worst)
    assert 0.5 * F32_DUAL_MEASURED < worst < 1.5 * F32_DUAL_MEASURED


# ---- 2, 3. the fixtures ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f64(backend, name):
    g = load_golden(name)
    b = build(g, np.float64)
    b.solve()
    check(b, g, 1e-9, 1e-9)
    assert b.getitstat()._fields == FIELDS
    assert all(v is None for v in b.getitstat().XSlvRelRes)


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f32(backend, name):
    g = load_golden(name)
    b = build(g, np.float32)
    b.solve()
    assert b.X.dtype == np.float32 and b.Y.dtype == np.float32 and b.U.dtype == np.float32
    check(b, g, 1e-4, 1e-3, with_u=False, f32=True)


# ---- 4. LinSolveCheck -----------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['l1l1_default_f64', 'l1l1_gradw_f64', 'l1l1_mcd_f64'])
def test_linsolvecheck(backend, name):
    g = load_golden(name)
    b = build(g, np.float64, extra={'LinSolveCheck': True})
    b.solve()
    x = np.array(b.getitstat().XSlvRelRes)
    print('XSlvRelRes max', x.max())
    assert x.max() < 1e-9
    check(b, g, 1e-9, 1e-9)


# ---- 5. equivalences that need no fixture ---------------------------------------------------------------
def test_mu_zero_ignores_gradweight(backend):
    """mu = 0: the gradient term is gone whatever its weights.  (RegGrad itself is defined with the
    weights inside -- GHGf = Wgrd sum_i |G_i|^2, cbpdn.py:2657, :2737 -- so its trace scales with them:
    it is compared after dividing by the scalar weight, and ObjFun, which multiplies it by mu = 0,
    as it stands.)"""
    g = load_golden('l1l1_default_f64')
    a = build(g, mu=0.0, extra={'MaxMainIter': 12})
    b = build(g, mu=0.0, extra={'MaxMainIter': 12, 'GradWeight': np.linspace(0.5, 2.0, 6)})
    c = build(g, mu=0.0, extra={'MaxMainIter': 12, 'GradWeight': 3.0})
    for s in (a, b, c):
        s.solve()
    rest = tuple(f for f in TRACES if f != 'RegGrad')
    same_run(a, b, traces=rest)
    same_run(a, c, traces=rest)
    assert rel_l2(np.array(c.getitstat().RegGrad) / 3.0, a.getitstat().RegGrad) < 1e-9
    assert np.all(np.array(b.getitstat().RegGrad) > 0.0)


def test_scalar_gradweight_folds_into_mu(backend):
    """GradWeight = c with mu equals GradWeight = 1 with c mu (RegGrad then differs by the factor c,
    mu RegGrad and so ObjFun do not)."""
    g = load_golden('l1l1_default_f64')
    c = 2.5
    a = build(g, extra={'MaxMainIter': 12, 'GradWeight': c})
    b = build(g, mu=c * float(g['mu']), extra={'MaxMainIter': 12})
    a.solve()
    b.solve()
    same_run(a, b, traces=tuple(f for f in TRACES if f != 'RegGrad'))
    assert rel_l2(np.array(a.getitstat().RegGrad), c * np.array(b.getitstat().RegGrad)) < 1e-9


@pytest.mark.parametrize('name', ['l1l1_default_f64', 'l1l1_mcd_f64'])
def test_mask_of_ones_is_no_mask(backend, name):
    g = load_golden(name)
    a = build(g, extra={'MaxMainIter': 12})
    b = build(g, W=np.ones(g['S'].shape[:2]), extra={'MaxMainIter': 12})
    a.solve()
    b.solve()
    same_run(a, b)


def test_mask_of_zeros_passes_block0_through(backend):
    """W = 0: the block-0 prox is the identity, y0 = ax + u0 - s, so u0 stays zero and DFid = 0."""
    g = load_golden('l1l1_default_f64')
    b = build(g, W=np.zeros(g['S'].shape[:2]), extra={'MaxMainIter': 8, 'RelaxParam': 1.0})
    b.solve()
    its = b.getitstat()
    assert np.all(np.array(its.DFid) == 0.0)
    S5 = five(g)[1]
    ax0 = b.reconstruct().reshape(S5.shape)
    assert rel_l2(b.var_y0(), ax0 - S5) < 1e-9
    assert np.max(np.abs(b.block_sep0(b.U))) < 1e-12 * np.max(np.abs(S5))
    r = restated(dict(g, MaxMainIter=8), W=np.zeros(S5.shape[:2] + (1, 1, 1)), rlx=1.0)
    assert rel_l2(b.Y, r['Y']) < 1e-9 and rel_l2(its.ObjFun, r['ObjFun']) < 1e-9


# ---- 6. solver state ---------------------------------------------------------------------------------------
def test_second_solve_continues(backend):
    """20 + 20 iterations equal 40."""
    g = load_golden('l1l1_autorho_f64')
    b = build(g, extra={'MaxMainIter': 20})
    b.solve()
    b.solve()
    check(b, g, 1e-9, 1e-9)
    assert len(b.getitstat().ObjFun) == 40


def test_warm_start(backend):
    """Y0 / U0 (concatenated blocks): 20 iterations, then 20 more from the uploaded arrays."""
    g = load_golden('l1l1_fixed_f64')
    a = build(g, extra={'MaxMainIter': 20})
    a.solve()
    b = build(g, extra={'MaxMainIter': 20, 'Y0': a.Y, 'U0': a.U, 'ReturnVar': 'X'})
    X = b.solve()
    assert rel_l2(X, b.X) == 0.0
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(b, v), g[v]) < 1e-9, v
    for f in TRACES:
        assert rel_l2(getattr(b.getitstat(), f), g['it_' + f][20:]) < 1e-9, f


@pytest.mark.parametrize('name', ['l1l1_default_f64', 'l1l1_mcd_f64'])
def test_setdict(backend, name):
    g = load_golden(name)
    rng = np.random.RandomState(3)
    D2 = rng.randn(*g['D'].shape)
    b = build(g, extra={'MaxMainIter': 10})
    b.setdict(D2.reshape(b.cri.shpD))
    b.solve()
    c = build(g, D=D2, extra={'MaxMainIter': 10})
    c.solve()
    same_run(b, c, tol=1e-12)


def test_nobndrycross_and_highmemsolve(backend):
    """NoBndryCross zeroes the boundary band of y1 only; HighMemSolve changes nothing."""
    g = load_golden('l1l1_nonneg_nobndry_f64')
    a = build(g, extra={'MaxMainIter': 8, 'HighMemSolve': True})
    a.solve()
    dH, dW = g['D'].shape[:2]
    y0, y1 = a.var_y0(), a.var_y1()
    assert np.all(y1[-(dH - 1):] == 0.0) and np.all(y1[:, -(dW - 1):] == 0.0) and np.any(y1 != 0.0)
    assert np.all(y1 >= 0.0)
    assert np.any(y0[-(dH - 1):] != 0.0) and np.any(y0[:, -(dW - 1):] != 0.0) and np.any(y0 < 0.0)
    c = build(g, extra={'MaxMainIter': 8})
    c.solve()
    assert rel_l2(a.Y, c.Y) == 0.0 and rel_l2(a.U, c.U) == 0.0


def test_refusals(backend):
    import pickle
    from sporco_amd.admm import cbpdn
    from sporco_amd.device import DeviceArray
    cls = cbpdn.ConvL1L1Grd
    rng = np.random.RandomState(0)
    D, S = rng.randn(4, 4, 6), rng.randn(12, 12, 2)
    opt = cls.Options({'MaxMainIter': 2})
    assert opt['GradWeight'] == 1.0 and opt['rho'] == 1.0 and not opt['AutoRho', 'Enabled']
    with pytest.raises(NotImplementedError):
        cls(rng.randn(4, 6), rng.randn(32, 3), 0.1, 0.01, opt=opt, dimN=1)
    with pytest.raises(NotImplementedError):
        cls(rng.randn(3, 3, 3, 6), rng.randn(8, 8, 8, 3), 0.1, 0.01, opt=opt, dimN=3)
    with pytest.raises(NotImplementedError):
        cls(D.astype(complex), S.astype(complex), 0.1, 0.01, opt=opt)
    with pytest.raises(NotImplementedError):
        cls(D, S, 0.1, 0.01, opt=opt, reducer=object())
    with pytest.raises(NotImplementedError):
        cls(D, S, 0.1, 0.01, opt=opt, resident=True)
    with pytest.raises(NotImplementedError):
        cls(D, DeviceArray((12, 12, 2), np.float64), 0.1, 0.01, opt=opt)
    with pytest.raises(ValueError):
        cls(D, S, 0.1, 0.01, opt=cls.Options({'GradWeight': np.ones(5)}))
    with pytest.raises(ValueError):
        cls(D, S, 0.1, 0.01, opt=cls.Options({'ReturnVar': 'Z'}))
    b = cls(D, S, 0.1, 0.01, opt=opt)
    with pytest.raises(NotImplementedError):
        pickle.dumps(b)
    b.rhochange()
    assert b.solve().shape == (12, 12, 1, 2, 6) and b.GHGf.shape == (12, 7, 1, 1, 1)
    # the parent's entry point keeps refusing the gradient flag
    from sporco_amd import _lib
    p = b._params()
    p.flags = _lib.FLAG_GRADREG
    with pytest.raises(Exception):
        b._dev.mdcpl_iter(p)


# ---- 7. the reference's own two tests (tests/admm/test_cbpdn.py 31, 32) ------------------------------------
def test_reference_scenario_31(backend):
    from sporco_amd.admm import cbpdn
    np.random.seed(12345)
    D = np.random.randn(5, 5, 3, 4)
    s = np.random.randn(16, 16, 3, 2)
    b = cbpdn.ConvL1L1Grd(D, s, 1e-1, 1e-2)
    b.opt['MaxMainIter'] = 30         # (the default is 1000; RelStopTol stays the default)
    Y1 = b.solve()
    assert Y1.shape == (16, 16, 1, 2, 4) and Y1.dtype == np.float64 and np.all(np.isfinite(Y1))
    assert np.all(np.isfinite(b.X)) and np.all(np.isfinite(b.U)) and b.getitstat()._fields == FIELDS


def test_reference_scenario_32(backend):
    from sporco_amd.admm import cbpdn
    np.random.seed(12345)
    D = np.random.randn(5, 5, 4)
    s = np.random.randn(16, 16, 2)
    dt = np.float32
    opt = cbpdn.ConvL1L1Grd.Options({'Verbose': False, 'LinSolveCheck': True, 'MaxMainIter': 20,
                                     'AutoRho': {'Enabled': True}, 'DataType': dt})
    b = cbpdn.ConvL1L1Grd(D, s, 1e-1, 1e-2, opt=opt)
    b.solve()
    assert b.X.dtype == dt and b.Y.dtype == dt and b.U.dtype == dt
    assert np.all(np.isfinite(b.X)) and np.all(np.isfinite(b.Y)) and np.all(np.isfinite(b.U))
    assert len(b.getitstat().ObjFun) == 20 and np.max(b.getitstat().XSlvRelRes) < 1e-4


# ---- 8. the parent class computes what it computed -----------------------------------------------------
def test_parent_class_bitwise_unchanged():
    """ConvBPDNMaskDcpl on the existing mask-decoupling fixtures, on the simulator: bit for bit the
    arrays that the simulator build of the commit before ConvL1L1Grd gave
    (tests/golden/l1l1_parent_mdcpl.npz, tools/record_maskdcpl_parent.py)."""
    from conftest import use_backend
    from sporco_amd.admm import cbpdn
    from test_maskdcpl import CASES as MD_CASES
    use_backend('hostsim')
    rec = load_golden('l1l1_parent_mdcpl')
    for name in sorted(MD_CASES):
        g = load_golden(name)
        optd = dict(MD_CASES[name])
        if 'wl1' in g:
            optd['L1Weight'] = g['wl1']
        b = cbpdn.ConvBPDNMaskDcpl(g['D'], g['S'], float(g['lmbda']), g['W'], cbpdn.ConvBPDNMaskDcpl.Options(optd))
        b.solve()
        for v in ('X', 'Y', 'U'):
            want = rec['%s.%s' % (name, v)]
            got = getattr(b, v)
            assert got.dtype == want.dtype and np.all(got == want), (name, v)
        assert np.asarray(b.rho) == rec[name + '.rho']
        its = b.getitstat()
        for f in ('ObjFun', 'DFid', 'RegL1', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho'):
            assert np.all(np.asarray(getattr(its, f), dtype=np.float64) == rec['%s.it_%s' % (name, f)]), (name, f)
        if optd.get('LinSolveCheck'):
            assert np.all(np.asarray(its.XSlvRelRes, dtype=np.float64) == rec[name + '.it_XSlvRelRes']), name


# ---- 9. GPU-only sizes: against the restatement, computed once per module ---------------------------------
GRID_THREADS = 4096 * 256      # csrc: grid_for caps a grid at kMaxPartialBlocks blocks of kThreads
_GPU = {}


def _gpu_problem(H, W, K, N, masked, iters, lmbda):
    key = (H, W, K, N, masked, iters, lmbda)
    if key not in _GPU:
        rng = np.random.RandomState(11)
        D = rng.randn(5, 5, K)
        D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
        S = 0.3 * rng.randn(H, W, N)
        hit = rng.rand(H, W, N) < 0.25
        S[hit] = 4.0 * np.sign(rng.randn(int(hit.sum())))
        Wm = (rng.rand(H, W) >= 0.2).astype(np.float64) if masked else None
        ref = ln.admm_l1l1(D.reshape(5, 5, 1, 1, K), S.reshape(H, W, 1, N, 1), lmbda, 0.05, iters,
                           W=Wm.reshape(H, W, 1, 1, 1) if masked else 1.0)
        _GPU[key] = (D, S, Wm, ref)
    return _GPU[key]


def _run_gpu(H, W, K, N, masked, iters=10, lmbda=0.6, shares=('Y0', 'Y1')):
    from sporco_amd.admm import cbpdn
    D, S, Wm, ref = _gpu_problem(H, W, K, N, masked, iters, lmbda)
    # both branches of the soft threshold, each by at least 1 % of the entries (with 64 filters the
    # coefficient maps of ten iterations are sparser than the fixtures': 2.5 % of 1.3 M entries)
    for blk in shares:
        assert 0.01 <= np.mean(ref[blk] != 0.0) <= 0.99, (blk, np.mean(ref[blk] != 0.0))
    o = cbpdn.ConvL1L1Grd.Options({'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0})
    f4 = np.float32
    b = cbpdn.ConvL1L1Grd(D.astype(f4), S.astype(f4), lmbda, 0.05, None if Wm is None else Wm.astype(f4), o, dimK=1)
    b.solve()
    its = b.getitstat()
    figs = {v: rel_l2(getattr(b, v), ref[v]) for v in ('X', 'Y')}
    trs = {f: rel_l2(getattr(its, f), ref[f]) for f in TRACES}
    print((H, W, K, N), figs, trs)
    for v, e in figs.items():
        assert e < 1e-4, (v, e)
    for f, e in trs.items():
        assert e < 1e-3, (f, e)


@pytest.mark.gpu
def test_gpu_grid_stride_wraps(gpu_backend):
    """128 x 160, K = 64, N = 1: the X-sized arrays have more elements than a capped grid has threads, so
    the kernels that take one element a thread make a second trip (the transforms' glue, block 0 does
    not: it is signal sized).  lambda = 1.1: with 64 filters the share of non-zero entries of y0 after ten
    iterations is 0 at 0.6 and 0.11 here (y1: 0.025)."""
    assert 128 * 160 * 64 > GRID_THREADS
    _run_gpu(128, 160, 64, 1, False, lmbda=1.1)


@pytest.mark.gpu
def test_gpu_dual_kernel_wraps(gpu_backend):
    """The same with N = 4: 128 x 81 frequency pixels x 4 images x 32 filter pairs are 1 327 104 threads
    of work for l1l1_dual (and the solve) on the capped grid, and the 16-byte epilogue wraps as well, so a
    block's partial sums accumulate over trips.  4 iterations keep the float64 restatement of this size
    to a few seconds; y0 is still all zero then (the case above and the fixtures cover its shrinkage), so
    the share condition is asked of y1 alone, at the 0.9 % it has: this case is about indexing."""
    assert 128 * 81 * 4 * 32 > GRID_THREADS and 128 * 160 * 4 * 64 // 4 > GRID_THREADS
    D, S, Wm, ref = _gpu_problem(128, 160, 64, 4, False, 4, 0.6)
    assert 0.005 <= np.mean(ref['Y1'] != 0.0) <= 0.99
    _run_gpu(128, 160, 64, 4, False, iters=4, shares=())


@pytest.mark.gpu
def test_gpu_odd_k_images_mask(gpu_backend):
    """32 x 48, K = 7, N = 3, masked: odd K (one filter a thread, nine systems under a wave), N > 1
    and the broadcast of the block-0 values across a wave."""
    _run_gpu(32, 48, 7, 3, True)
