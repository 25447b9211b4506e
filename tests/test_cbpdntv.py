"""sporco_amd.admm.cbpdntv.ConvBPDNScalarTV / ConvBPDNVectorTV against the reference's fixtures
(tests/golden/tv_*_f64.npz, float64 runs of the unmodified reference written by
tools/make_golden_tv.py) and, where no reference exists, against the NumPy restatement of
tests/_tv_numpy.py, which is itself pinned to the reference first.

Tolerances are the project's: float64 1e-9 relative l2 on X, Y, U, reconstruct() and every trace;
float32 input 1e-4 on X and Y and 1e-3 on the traces, both against the float64 reference.  The
array-L1Weight fixtures hold no traces (the reference's own objective evaluation raises on such a
weight, cbpdntv.py:444): their traces are compared with the pinned restatement.
"""

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _tv_numpy as tvn

CASES = ['default', 'tvw', 'l1w', 'fixedrho', 'auxvar', 'mu0', 'chan', 'bigmu']
FIXTURES = ['tv_%s_%s_f64' % (c, n) for c in 'sv' for n in CASES]
TRACES = ('ObjFun', 'DFid', 'RegL1', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho')


def options_of(g, extra=None):
    o = {'Verbose': False, 'MaxMainIter': int(g['MaxMainIter']), 'RelStopTol': 0.0,
         'RelaxParam': float(g['opt_RelaxParam'])}
    if bool(g['opt_AuxVarObj']):
        o['AuxVarObj'] = True
    if not np.isnan(g['opt_rho']):
        o['rho'] = float(g['opt_rho'])
    if not bool(g['opt_AutoRho']):
        o['AutoRho'] = {'Enabled': False}
    for key in ('L1Weight', 'TVWeight'):
        if 'optarr_' + key in g:
            o[key] = g['optarr_' + key]
    o.update(extra or {})
    return o


def build(g, dtype=np.float64, extra=None):
    from sporco_amd.admm import cbpdntv
    cls = cbpdntv.ConvBPDNVectorTV if int(g['vector']) else cbpdntv.ConvBPDNScalarTV
    return cls(g['D'].astype(dtype), g['S'].astype(dtype), float(g['lmbda']), float(g['mu']),
               cbpdntv.ConvBPDNScalarTV.Options(options_of(g, extra)), dimK=int(g['dimK']))


def restated(g, exact=True):
    """The pinned restatement's solve of a fixture's problem (its traces, where the fixture has
    none)."""
    D, S = g['D'], g['S']
    S5 = S.reshape(S.shape[:2] + ((1, S.shape[2], 1) if int(g['dimK']) else (S.shape[2], 1, 1)))
    wtv = g['optarr_TVWeight'].reshape(1, 1, 1, 1, -1) if 'optarr_TVWeight' in g else 1.0
    return tvn.admm_tv(D.reshape(D.shape[:2] + (1, 1, -1)), S5, float(g['lmbda']), float(g['mu']),
                       int(g['MaxMainIter']), vector=bool(g['vector']), wtv=wtv,
                       wl1=g['optarr_L1Weight'] if 'optarr_L1Weight' in g else 1.0,
                       rho=None if np.isnan(g['opt_rho']) else float(g['opt_rho']),
                       rlx=float(g['opt_RelaxParam']), auto_rho=bool(g['opt_AutoRho']),
                       gevaly=bool(g['opt_AuxVarObj']), fevalx=not bool(g['opt_AuxVarObj']), exact=exact)


def check(b, g, tol, tol_tr, with_u=True):
    its = b.getitstat()
    figs = {v: rel_l2(getattr(b, v), g[v]) for v in (('X', 'Y', 'U') if with_u else ('X', 'Y'))}
    figs['recon'] = rel_l2(b.reconstruct(), g['recon'])
    if 'it_ObjFun' in g:
        trs = {f: rel_l2(getattr(its, f), g['it_' + f]) for f in TRACES}
    else:
        r = restated(g, exact=False)
        trs = {f: rel_l2(getattr(its, f), r[f]) for f in TRACES}
    print(figs, trs, 'rho', float(b.rho), float(g['rho_final']))
    for v, e in figs.items():
        assert e < tol, (v, e)
    for f, e in trs.items():
        assert e < tol_tr, (f, e)
    assert abs(float(b.rho) - float(g['rho_final'])) <= tol_tr * float(g['rho_final'])
    assert np.shape(b.Y) == np.shape(g['Y']) and np.shape(b.U) == np.shape(g['U'])


# ---- 1. the fixtures ---------------------------------------------------------------------------------
def test_bigmu_fixtures_take_the_zero_branch():
    """The large-mu fixtures exercise the zero branch of prox_l2: a share of exactly-zero gradient
    vectors in [0.05, 0.95] for vector TV; all of them for scalar TV, whose one global norm allows
    only none or all."""
    for name, lo, hi in (('tv_v_bigmu_f64', 0.05, 0.95), ('tv_s_bigmu_f64', 1.0, 1.0)):
        g = load_golden(name)
        Y = g['Y']
        share = np.mean(np.sum(Y[..., 0:2] ** 2, axis=(4, 5) if int(g['vector']) else 5) == 0.0)
        assert lo <= share <= hi and share == float(g['zero_share']), (name, share)
        assert np.linalg.norm(g['X']) > 0 and np.all(np.abs(g['it_ObjFun']) < 1e6)


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f64(backend, name):
    g = load_golden(name)
    b = build(g, np.float64)
    b.solve()
    check(b, g, 1e-9, 1e-9)
    assert rel_l2(b.getcoef(), g['Y'][..., -1]) < 1e-9
    assert rel_l2(b.var_y0(), g['Y'][..., 0:2]) < 1e-9 and b.var_y1().shape == g['X'].shape + (1,)


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f32(backend, name):
    g = load_golden(name)
    b = build(g, np.float32)
    b.solve()
    assert b.Y.dtype == np.float32
    check(b, g, 1e-4, 1e-3, with_u=False)


@pytest.mark.parametrize('name', ['tv_s_tvw_f64', 'tv_v_tvw_f64'])
def test_per_filter_weight_is_the_references_arithmetic(backend, name):
    """With different TVWeights per filter the reference's x step (linalg.solvedbi_sm with a diagonal
    that varies along the filter axis) does not solve its system; the class reproduces the reference
    (restatement with exact=False), and LinSolveCheck shows the residual.  Equal weights given as an
    array take the exact solve, as a scalar does."""
    g = load_golden(name)
    b = build(g, np.float64, extra={'LinSolveCheck': True})
    b.solve()
    r = restated(g, exact=False)
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(b, v), r[v]) < 1e-9, v
    its = b.getitstat()
    for f in TRACES:
        assert rel_l2(getattr(its, f), r[f]) < 1e-9, f
    assert 1e-6 < np.array(its.XSlvRelRes).max() < 1.0
    e = build(g, np.float64, extra={'LinSolveCheck': True, 'TVWeight': np.full(8, 0.7), 'MaxMainIter': 5})
    e.solve()
    assert np.array(e.getitstat().XSlvRelRes).max() < 1e-9
    f = build(g, np.float64, extra={'TVWeight': 0.7, 'MaxMainIter': 5})
    f.solve()
    assert rel_l2(e.X, f.X) < 1e-12


def test_returnx_and_host_operators(backend):
    g = load_golden('tv_s_tvw_f64')
    b = build(g, extra={'ReturnX': True, 'MaxMainIter': 5})
    X = b.solve()
    assert rel_l2(X, b.X) == 0.0
    rng = np.random.RandomState(0)
    V = rng.randn(*b.Y.shape)
    # <A x, v> = <x, A^T v> for the host-side operators, and A0 is the gradient part of A
    assert abs(np.sum(b.cnst_A(b.X) * V) - np.sum(b.X * b.cnst_AT(V))) < 1e-10 * np.linalg.norm(V) * np.linalg.norm(b.X)
    assert rel_l2(b.cnst_A0(b.X), b.cnst_A(b.X)[..., 0:2]) == 0.0
    assert rel_l2(b.cnst_A0T(V), np.stack([V[..., 0] - np.roll(V[..., 0], -1, 0),
                                           V[..., 1] - np.roll(V[..., 1], -1, 1)], -1) * b.Wtv[..., None]) < 1e-15
    assert b.obfn_reg()[1:] == (b.getitstat().RegL1[-1], b.getitstat().RegTV[-1])
    assert b.obfn_dfd() == b.getitstat().DFid[-1]


def test_warm_start(backend):
    """Y0 / U0: 20 iterations, then 20 more from the uploaded blocks, equal 40 in one go."""
    g = load_golden('tv_v_fixedrho_f64')
    a = build(g, extra={'MaxMainIter': 20})
    a.solve()
    b = build(g, extra={'MaxMainIter': 20, 'Y0': a.Y, 'U0': a.U})
    b.solve()
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(b, v), g[v]) < 1e-9, v


# ---- 2. the scenarios of the reference's own test file (tests/admm/test_cbpdntv.py 01, 02, 04, 05) ----
@pytest.mark.parametrize('vector', [False, True], ids=['scalar', 'vector'])
@pytest.mark.parametrize('chan', [1, 3])
def test_reference_scenarios(backend, vector, chan):
    from sporco_amd.admm import cbpdntv
    N, Nd, M = 16, 5, 4
    np.random.seed(12345)
    D = np.random.randn(Nd, Nd, M)
    s = np.random.randn(N, N) if chan == 1 else np.random.randn(N, N, chan)
    cls = cbpdntv.ConvBPDNVectorTV if vector else cbpdntv.ConvBPDNScalarTV
    opt = cls.Options({'Verbose': False, 'MaxMainIter': 20, 'LinSolveCheck': True})
    b = cls(D, s, 1e-1, 1e-2, opt=opt, dimK=0)
    X = b.solve()
    assert X.shape == (N, N, chan, 1, M) and np.all(np.isfinite(X))
    its = b.getitstat()
    assert its._fields == ('Iter', 'ObjFun', 'DFid', 'RegL1', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal',
                           'EpsDual', 'Rho', 'XSlvRelRes', 'Time')
    assert b.Y.shape == (N, N, chan, 1, M, 3) and b.U.shape == b.Y.shape
    assert b.reconstruct().shape == (N, N, chan, 1)
    print('XSlvRelRes', its.XSlvRelRes[-1])
    assert np.array(its.XSlvRelRes).max() < 1e-5
    assert float(b.rho_xi) == 1.0


# ---- 3. the kernels alone through the C ABI -------------------------------------------------------------
def test_numpy_restatement_pinned_to_fixture():
    """One iteration of the restatement from the reference's state after 39 iterations reproduces
    the reference's state after 40 (float64, 1e-12); its whole solve reproduces the fixtures.  The
    restatement runs here with the reference's own x-step arithmetic (_tv_numpy.xstep, exact=False);
    the fixtures with one TVWeight per filter cannot be reproduced otherwise."""
    for tag in 'sv':
        g = load_golden('tv_step_%s_f64' % tag)
        D, S = g['D'], g['S']
        H, W = S.shape[:2]
        Df = np.fft.rfftn(D.reshape(D.shape[:2] + (1, 1, -1)), s=(H, W), axes=(0, 1))
        Sf = np.fft.rfftn(S.reshape(H, W, 1, -1, 1), axes=(0, 1))
        st = dict(Y=g['Y_before'], U=g['U_before'], rho=float(g['rho_before']))
        rec = tvn.iterate(st, Df, Sf, g['optarr_TVWeight'].reshape(1, 1, 1, 1, -1), 1.0, float(g['lmbda']),
                          float(g['mu']), 1.8, bool(g['vector']), False, True, True, int(g['k']), (H, W), exact=False)
        for v in ('X', 'Y', 'U'):
            assert rel_l2(st[v], g[v]) < 1e-12, (tag, v)
        assert abs(st['rho'] - float(g['rho_final'])) < 1e-12 * float(g['rho_final'])
        for f in ('ObjFun', 'DFid', 'RegL1', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'Rho'):
            assert abs(rec[f] - float(g['last_' + f])) <= 1e-12 * abs(float(g['last_' + f])), (tag, f)
    for name in ('tv_s_default_f64', 'tv_v_tvw_f64', 'tv_s_tvw_f64', 'tv_v_chan_f64', 'tv_s_auxvar_f64', 'tv_s_l1w_f64'):
        g = load_golden(name)
        r = restated(g, exact=False)
        for v in ('X', 'Y', 'U'):
            assert rel_l2(r[v], g[v]) < 1e-10, (name, v)
        if 'it_ObjFun' in g:
            for f in ('ObjFun', 'RegL1', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'Rho'):
                assert rel_l2(r[f], g['it_' + f]) < 1e-10, (name, f)


ABI_SHAPES = [(2, 2, 1, 1, 1), (5, 7, 1, 2, 5), (16, 40, 3, 1, 64), (9, 33, 1, 1, 100), (8, 8, 1, 1, 300)]


@pytest.mark.parametrize('dtype', [np.float64, np.float32], ids=['f64', 'f32'])
@pytest.mark.parametrize('vector', [False, True], ids=['scalar', 'vector'])
@pytest.mark.parametrize('shape', ABI_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_tv_kernels_abi(backend, shape, vector, dtype):
    from sporco_amd import _lib
    H, W, C, N, K = shape
    rng = np.random.RandomState(H * 1000 + W * 10 + K)
    tol, tol_s = (1e-12, 1e-10) if dtype == np.float64 else (1e-5, 1e-4)
    s = _lib.Solver(H, W, C, N, K, dtype)
    s.set_signal(np.zeros((H, W, C, N), dtype=dtype))
    s.set_dict(rng.randn(1, 1, K).astype(dtype))
    s.profile(True)
    calls = 0
    for wtv, wl1, rlx, us, gevaly in ((0.7, None, 1.8, 1.0, False),
                                      (0.5 + rng.rand(K), 0.5 + rng.rand(H, W, C, N, K), 1.0, 0.8, True),
                                      (0.5 + rng.rand(K), None, 1.8, 1.25, True)):
        s.set_l1_weight(None if wl1 is None else wl1.astype(dtype))
        s.tv_setup(wtv, vector)
        w5 = np.asarray(wtv, dtype=np.float64).reshape(1, 1, 1, 1, -1)
        l5 = 1.0 if wl1 is None else wl1.astype(dtype).astype(np.float64)
        X = rng.randn(H, W, C, N, K).astype(dtype)
        Y = rng.randn(H, W, C, N, K, 3).astype(dtype)
        U = rng.randn(H, W, C, N, K, 3).astype(dtype)
        P0 = rng.randn(H, W, C, N, K).astype(dtype)
        s.upload(_lib.VAR_X, X)
        s.upload(_lib.VAR_TVY, np.ascontiguousarray(np.moveaxis(Y, -1, 0)))
        s.upload(_lib.VAR_TVU, np.ascontiguousarray(np.moveaxis(U, -1, 0)))
        s.upload(_lib.VAR_Y, P0)
        # vector TV: the threshold at the median pixel norm -- about half of the gradient vectors shrink
        # to zero, both branches of prox_l2 in one call; scalar TV has ONE norm (the whole array): half
        # of it in the first two calls, beyond it (everything shrinks to zero) in the third
        p = _lib.AdmmParams()
        p.rho, p.lmbda, p.rlx, p.u_scale = 2.0, 1.5, rlx, us
        v0 = tvn.cnst_A(X.astype(np.float64), w5)[..., 0:2]
        v0 = (v0 if rlx == 1.0 else rlx * v0 + (1 - rlx) * Y[..., 0:2]) + us * U[..., 0:2].astype(np.float64)
        if vector:
            p.mu = p.rho * float(np.median(np.sqrt(np.sum(v0 ** 2, axis=(4, 5)))))
        else:
            p.mu = p.rho * float(np.linalg.norm(v0)) * (0.5 if calls < 2 else 1.5)
        p.flags = _lib.FLAG_GEVAL_Y if gevaly else 0
        p.dH = p.dW = 1
        out = s.tv_ystep(p)
        r = tvn.tv_ystep(X.astype(np.float64), Y.astype(np.float64), U.astype(np.float64), w5, l5, p.lmbda,
                         p.mu, p.rho, rlx, vector, gevaly, u_scale=us)
        Yd = np.moveaxis(s.download(_lib.VAR_TVY), 0, -1)
        Ud = np.moveaxis(s.download(_lib.VAR_TVU), 0, -1)
        zero = np.mean(np.sum(r['Y'][..., 0:2] ** 2, axis=(4, 5) if vector else 5) == 0.0)
        print('zero share', zero)
        assert (0.2 < zero < 0.8 or H * W * K < 8) if vector else zero == (0.0 if calls < 2 else 1.0)
        assert rel_l2(Yd, r['Y']) < tol and rel_l2(Ud, r['U']) < tol
        for slot, key in ((_lib.OUT_R2, 'r2'), (_lib.OUT_AX2, 'ax2'), (_lib.OUT_Y2, 'y2'), (_lib.OUT_L1, 'l1'),
                          (_lib.OUT_L21, 'tv')):
            assert abs(out[slot] - r[key]) <= tol_s * max(abs(r[key]), 1.0), (key, out[slot], r[key])
        out = s.tv_adjoint(0.5)
        a = tvn.tv_adjoint(Yd.astype(np.float64), Ud.astype(np.float64), w5, P0.astype(np.float64), u_scale=0.5)
        Pd, Qd = s.download(_lib.VAR_Y), s.download(_lib.VAR_U)
        assert rel_l2(Pd, a['P']) < tol and rel_l2(Qd, a['Q']) < tol
        assert abs(out[_lib.OUT_S2] - a['s2']) <= tol_s * max(a['s2'], 1.0)
        assert abs(out[_lib.OUT_U2] - a['u2']) <= tol_s * max(a['u2'], 1.0)
        if dtype == np.float64:
            # the adjoint identity between the two kernels' outputs: <A x, y> = <x, A^T y>, AXnr = Y + (AXnr - Y)
            AX = tvn.cnst_A(X.astype(np.float64), w5)
            lhs, rhs = np.sum(AX * Yd), np.sum(X.astype(np.float64) * Pd)
            assert abs(lhs - rhs) <= 1e-10 * np.linalg.norm(AX) * np.linalg.norm(Yd)
        calls += 1
    prof = s.profile_read()
    assert prof['tv_ystep'][1] == calls and prof['tv_adjoint'][1] == calls


# ---- 4. GPU sizes: against the restatement, computed once per module ------------------------------------
_GPU = {}


def _gpu_problem(key):
    if key not in _GPU:
        H, W, K, N, dt = {'fused': (128, 128, 32, 2, np.float32), 'mr': (160, 128, 16, 1, np.float32),
                          'generic': (48, 40, 5, 3, np.float64)}[key]
        rng = np.random.RandomState(11)
        D = rng.randn(8, 8, K)
        D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
        S = rng.randn(H, W, N)
        refs = {v: tvn.admm_tv(D.reshape(8, 8, 1, 1, K), S.reshape(H, W, 1, N, 1), 0.05, 0.02, 10, vector=v)
                for v in (False, True)}
        _GPU[key] = (D.astype(dt), S.astype(dt), refs)
    return _GPU[key]


@pytest.mark.gpu
@pytest.mark.parametrize('vector', [False, True], ids=['scalar', 'vector'])
@pytest.mark.parametrize('key,tol', [('fused', 1e-4), ('mr', 1e-4), ('generic', 1e-9)])
def test_gpu_sizes(gpu_backend, key, tol, vector):
    from sporco_amd.admm import cbpdn, cbpdntv
    D, S, refs = _gpu_problem(key)
    ref = refs[vector]
    cls = cbpdntv.ConvBPDNVectorTV if vector else cbpdntv.ConvBPDNScalarTV
    b = cls(D, S, 0.05, 0.02, cls.Options({'Verbose': False, 'MaxMainIter': 10, 'RelStopTol': 0.0}), dimK=1)
    gr = cbpdn.ConvBPDNGradReg(D, S, 0.05, 0.02, cbpdn.ConvBPDNGradReg.Options({'MaxMainIter': 1}), dimK=1)
    print(key, 'fused rows / cols:', b._dev.uses_fused_rows(), b._dev.uses_fused_cols())
    assert b._dev.uses_fused_rows() == gr._dev.uses_fused_rows()
    assert b._dev.uses_fused_cols() == gr._dev.uses_fused_cols()
    b.profile(True)
    b.solve()
    prof = b.profile_read()
    assert prof['tv_ystep'][1] == 10 and prof['tv_adjoint'][1] == 10
    figs = {v: rel_l2(getattr(b, v), ref[v]) for v in ('X', 'Y')}
    its = b.getitstat()
    trs = {f: rel_l2(getattr(its, f), ref[f]) for f in TRACES}
    print(key, figs, trs)
    for v, e in figs.items():
        assert e < tol, (v, e)
    for f, e in trs.items():
        assert e < (tol if tol < 1e-6 else 1e-3), (f, e)


# ---- 5. refusals ------------------------------------------------------------------------------------
def test_refusals(backend):
    import pickle
    from sporco_amd.admm import cbpdn, cbpdntv
    from sporco_amd.device import DeviceArray
    rng = np.random.RandomState(0)
    D, S = rng.randn(4, 4, 6), rng.randn(12, 12)
    for cls in (cbpdntv.ConvBPDNScalarTV, cbpdntv.ConvBPDNVectorTV):
        opt = cls.Options({'MaxMainIter': 2})
        with pytest.raises(NotImplementedError):
            cls(rng.randn(4, 6), rng.randn(32), 0.1, 0.01, opt, dimN=1)
        with pytest.raises(NotImplementedError):
            cls(rng.randn(3, 3, 3, 6), rng.randn(8, 8, 8), 0.1, 0.01, opt, dimN=3)
        with pytest.raises(NotImplementedError):
            cls(rng.randn(4, 4, 3, 6), rng.randn(12, 12, 3), 0.1, 0.01, opt)
        with pytest.raises(NotImplementedError):
            cls(D.astype(complex), S.astype(complex), 0.1, 0.01, opt)
        with pytest.raises(NotImplementedError):
            cls(D, S, 0.1, 0.01, opt, reducer=object())
        with pytest.raises(NotImplementedError):
            cls(D, S, 0.1, 0.01, opt, resident=True)
        with pytest.raises(NotImplementedError):
            cls(D, DeviceArray((12, 12), np.float64), 0.1, 0.01, opt)
        with pytest.raises(NotImplementedError):
            cbpdn.AddMaskSim(cls, D, S, np.ones((12, 12)), 0.1, 0.01, opt)
        for key in ('NonNegCoef', 'NoBndryCross'):
            with pytest.raises(NotImplementedError):
                cls(D, S, 0.1, 0.01, cls.Options({key: True}))
        b = cls(D, S, 0.1, 0.01, opt)
        with pytest.raises(NotImplementedError):
            pickle.dumps(b)
        b.ystep = lambda: None
        with pytest.raises(NotImplementedError):
            b.solve()


# ---- 6. linearity and robustness -------------------------------------------------------------------------
def test_xstep_override_passes_through(backend):
    g = load_golden('tv_s_default_f64')
    a, b = build(g, extra={'MaxMainIter': 12}), build(g, extra={'MaxMainIter': 12})
    b.xstep = lambda: type(b).xstep(b)
    a.solve()
    b.solve()
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(a, v), getattr(b, v)) < 1e-12, v
    assert rel_l2(a.getitstat().ObjFun, b.getitstat().ObjFun) < 1e-12


@pytest.mark.parametrize('vector', [False, True], ids=['scalar', 'vector'])
def test_zero_tv_weight_keeps_the_gradient_blocks(backend, vector):
    """mu = 0 with TVWeight = 0: the gradient blocks stay in the constraint (and in the residuals)
    with A0 = 0, so Y's gradient blocks equal A0 X = 0 within the primal residual."""
    g = load_golden('tv_v_mu0_f64' if vector else 'tv_s_mu0_f64')
    b = build(g, extra={'TVWeight': 0.0})
    b.solve()
    its = b.getitstat()
    A0X = b.cnst_A0(b.X)
    rn = max(np.linalg.norm(b.cnst_A(b.X)), np.linalg.norm(b.Y))
    assert np.all(A0X == 0.0)
    assert np.linalg.norm(b.var_y0() - A0X) <= its.PrimalRsdl[-1] * rn * (1 + 1e-9)
    assert np.all(np.isfinite(its.ObjFun)) and its.RegTV[-1] == 0.0
