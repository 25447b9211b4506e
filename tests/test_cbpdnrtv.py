"""sporco_amd.admm.cbpdntv.ConvBPDNRecTV against the reference's fixtures (tests/golden/rtv_*_f64.npz,
float64 runs of the unmodified reference written by tools/make_golden_rtv.py) and, at the GPU
sizes, against the NumPy restatement of tests/_rtv_numpy.py, which is itself pinned to the
reference first.

Tolerances are the project's: float64 1e-9 relative l2 on X, Y, U, reconstruct(), every trace and
the final rho; float32 input 1e-4 on X, Y and reconstruct() and 1e-3 on the traces, both against
the float64 reference.
"""

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _rtv_numpy as rtn

CASES = ['default', 'tvw', 'l1w', 'fixedrho', 'auxvar', 'mu0', 'chan', 'bigmu']
FIXTURES = ['rtv_%s_f64' % n for n in CASES]
TRACES = ('ObjFun', 'DFid', 'RegL1', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho')
FIELDS = ('Iter', 'ObjFun', 'DFid', 'RegL1', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho',
          'XSlvRelRes', 'Time')


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
    return cbpdntv.ConvBPDNRecTV(g['D'].astype(dtype), g['S'].astype(dtype), float(g['lmbda']), float(g['mu']),
                                 cbpdntv.ConvBPDNRecTV.Options(options_of(g, extra)), dimK=int(g['dimK']))


def restated(g, **kw):
    """The restatement's solve of a fixture's problem."""
    D, S = g['D'], g['S']
    S5 = S.reshape(S.shape[:2] + ((1, S.shape[2], 1) if int(g['dimK']) else (S.shape[2], 1, 1)))
    return rtn.admm_rtv(D.reshape(D.shape[:2] + (1, 1, -1)), S5, float(g['lmbda']), float(g['mu']),
                        int(g['MaxMainIter']), wtv=g['optarr_TVWeight'] if 'optarr_TVWeight' in g else 1.0,
                        wl1=g['optarr_L1Weight'] if 'optarr_L1Weight' in g else 1.0,
                        rho=None if np.isnan(g['opt_rho']) else float(g['opt_rho']),
                        rlx=float(g['opt_RelaxParam']), auto_rho=bool(g['opt_AutoRho']),
                        gevaly=bool(g['opt_AuxVarObj']), fevalx=not bool(g['opt_AuxVarObj']), **kw)


def check(b, g, tol, tol_tr, with_u=True):
    its = b.getitstat()
    figs = {v: rel_l2(getattr(b, v), g[v]) for v in (('X', 'Y', 'U') if with_u else ('X', 'Y'))}
    figs['recon'] = rel_l2(b.reconstruct(), g['recon'])
    trs = {f: rel_l2(getattr(its, f), g['it_' + f]) for f in TRACES}
    print(figs, trs, 'rho', float(b.rho), float(g['rho_final']))
    for v, e in figs.items():
        assert e < tol, (v, e)
    for f, e in trs.items():
        assert e < tol_tr, (f, e)
    assert abs(float(b.rho) - float(g['rho_final'])) <= tol_tr * float(g['rho_final'])
    assert np.shape(b.Y) == np.shape(g['Y']) and np.shape(b.U) == np.shape(g['U'])


# ---- 1. the restatement and the fixtures -------------------------------------------------------------
def test_numpy_restatement_pinned_to_fixtures():
    """The algebra as built -- closed-form rank-one / rank-two solve, stencils, frequency-domain
    residual norms -- reproduces every fixture, and one iteration from the reference's state after 39
    iterations reproduces its state after 40 (float64, 1e-9)."""
    for name in FIXTURES:
        g = load_golden(name)
        r = restated(g)
        for v in ('X', 'Y', 'U', 'recon'):
            assert rel_l2(r[v], g[v]) < 1e-9, (name, v)
        for f in TRACES:
            assert rel_l2(r[f], g['it_' + f]) < 1e-9, (name, f)
        assert abs(r['rho'] - float(g['rho_final'])) < 1e-9 * float(g['rho_final'])
    g = load_golden('rtv_step_f64')
    D, S = g['D'], g['S']
    H, W = S.shape[:2]
    Df = np.fft.rfftn(D.reshape(D.shape[:2] + (1, 1, -1)), s=(H, W), axes=(0, 1))
    Sf = np.fft.rfftn(S.reshape(H, W, 1, -1, 1), axes=(0, 1))
    st = dict(Y=g['Y_before'], U=g['U_before'], rho=float(g['rho_before']))
    rec = rtn.iterate(st, Df, Sf, g['optarr_TVWeight'], 1.0, float(g['lmbda']), float(g['mu']), 1.8, False, True,
                      True, int(g['k']), (H, W))
    for v in ('X', 'Y', 'U'):
        assert rel_l2(st[v], g[v]) < 1e-9, v
    assert abs(st['rho'] - float(g['rho_final'])) < 1e-9 * float(g['rho_final'])
    for f in ('ObjFun', 'DFid', 'RegL1', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert abs(rec[f] - float(g['last_' + f])) <= 1e-9 * abs(float(g['last_' + f])), f


def test_bigmu_fixture_takes_the_zero_branch():
    """The large-mu fixture exercises both branches of prox_l2: the share of pixels whose gradient
    vector of the final Y is exactly zero lies in [0.05, 0.95] and is the one stored."""
    g = load_golden('rtv_bigmu_f64')
    M = g['D'].shape[-1]
    share = np.mean(np.sum(g['Y'][..., M:] ** 2, axis=(2, 4)) == 0.0)
    assert 0.05 <= share <= 0.95 and share == float(g['zero_share']), share
    assert float(g['it_Rho'][0]) == 1.0      # (the reference's effective default rho)


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f64(backend, name):
    g = load_golden(name)
    b = build(g, np.float64)
    b.solve()
    check(b, g, 1e-9, 1e-9)
    # block shapes and views
    M = g['D'].shape[-1]
    assert b.Y.shape == g['X'].shape[:4] + (M + 2,)
    assert rel_l2(b.getcoef(), g['y0']) < 1e-9 and b.var_y0().shape == g['y0'].shape
    assert rel_l2(b.var_y1(), g['y1']) < 1e-9 and b.var_y1().shape == g['y1'].shape
    assert rel_l2(b.var_yx(), g['y0']) < 1e-9 and rel_l2(b.Y[b.var_yx_idx()], g['y0']) < 1e-9
    assert rel_l2(b.block_cat(b.block_sep0(b.Y), b.block_sep1(b.Y)), b.Y) == 0.0


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f32(backend, name):
    g = load_golden(name)
    b = build(g, np.float32)
    b.solve()
    assert b.Y.dtype == np.float32
    check(b, g, 1e-4, 1e-3, with_u=False)


# ---- 2. options ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['rtv_default_f64', 'rtv_tvw_f64'])
def test_linsolvecheck(backend, name):
    """The closed forms solve the reference's rank-3 system: scalar (rank one) and per-filter (rank
    two) TVWeight."""
    g = load_golden(name)
    b = build(g, np.float64, extra={'LinSolveCheck': True})
    b.solve()
    x = np.array(b.getitstat().XSlvRelRes)
    print('XSlvRelRes max', x.max())
    assert x.max() < 1e-9
    check(b, g, 1e-9, 1e-9)


def test_equal_weights_as_array_equal_the_scalar(backend):
    g = load_golden('rtv_default_f64')
    e = build(g, extra={'TVWeight': np.full(8, 0.7), 'MaxMainIter': 10})
    e.solve()
    f = build(g, extra={'TVWeight': 0.7, 'MaxMainIter': 10})
    f.solve()
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(e, v), getattr(f, v)) < 1e-12, v
    assert rel_l2(e.getitstat().ObjFun, f.getitstat().ObjFun) < 1e-12


def test_returnx_and_objective_accessors(backend):
    g = load_golden('rtv_tvw_f64')
    b = build(g, extra={'ReturnX': True, 'MaxMainIter': 5})
    X = b.solve()
    assert rel_l2(X, b.X) == 0.0 and X.shape == g['X'].shape
    assert b.obfn_reg()[1:] == (b.getitstat().RegL1[-1], b.getitstat().RegTV[-1])
    assert b.obfn_dfd() == b.getitstat().DFid[-1]


def test_warm_start(backend):
    """Y0 / U0: 20 iterations, then 20 more from the uploaded blocks, equal 40 in one go."""
    g = load_golden('rtv_fixedrho_f64')
    a = build(g, extra={'MaxMainIter': 20})
    a.solve()
    b = build(g, extra={'MaxMainIter': 20, 'Y0': a.Y, 'U0': a.U})
    b.solve()
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(b, v), g[v]) < 1e-9, v
    its = b.getitstat()
    assert rel_l2(its.DualRsdl, g['it_DualRsdl'][20:]) < 1e-9 and rel_l2(its.ObjFun, g['it_ObjFun'][20:]) < 1e-9


def test_setdict(backend):
    g = load_golden('rtv_default_f64')
    b = build(g, extra={'MaxMainIter': 10})
    rng = np.random.RandomState(3)
    D2 = rng.randn(*g['D'].shape)
    b.setdict(D2.reshape(b.cri.shpD))
    b.solve()
    g2 = dict(g, D=D2)
    c = build(g2, extra={'MaxMainIter': 10})
    c.solve()
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(b, v), getattr(c, v)) < 1e-12, v


def test_std_residuals(backend):
    """AutoRho with StdResiduals: the un-normalised residual form (admm.py:473-476)."""
    g = load_golden('rtv_default_f64')
    b = build(g, extra={'MaxMainIter': 12, 'AutoRho': {'StdResiduals': True}})
    b.solve()
    r = restated(dict(g, MaxMainIter=12), std_residuals=True)
    its = b.getitstat()
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(b, v), r[v]) < 1e-9, v
    for f in ('PrimalRsdl', 'DualRsdl', 'Rho', 'ObjFun'):
        assert rel_l2(getattr(its, f), r[f]) < 1e-9, f


@pytest.mark.parametrize('name', ['rtv_tvw_f64', 'rtv_chan_f64'])
def test_host_operators_adjoint_identity(backend, name):
    """<A x, y> = <x, A^T y> for the host-side cnst_A / cnst_AT on random arrays, and A x of the
    final X is what the device's primal residual saw."""
    g = load_golden(name)
    b = build(g, extra={'MaxMainIter': 3})
    b.solve()
    rng = np.random.RandomState(0)
    X, V = rng.randn(*b.X.shape), rng.randn(*b.Y.shape)
    AX, ATV = b.cnst_A(X), b.cnst_AT(V)
    assert AX.shape == V.shape and ATV.shape == X.shape
    assert abs(np.sum(AX * V) - np.sum(X * ATV)) < 1e-12 * np.linalg.norm(AX) * np.linalg.norm(V)
    assert rel_l2(b.cnst_A0(X), X) == 0.0 and rel_l2(b.cnst_A0T(X), X) == 0.0
    assert b.cnst_A1(X).shape == X.shape[:4] + (1, 2) and b.cnst_A1T(b.block_sep1(V)).shape == X.shape + (2,)
    assert rel_l2(b.cnst_B(V), -V) == 0.0 and b.cnst_c() == 0.0
    its = b.getitstat()
    A = b.cnst_A(b.X)
    assert abs(np.linalg.norm(A - b.Y) / max(np.linalg.norm(A), np.linalg.norm(b.Y)) - its.PrimalRsdl[-1]) \
        < 1e-9 * its.PrimalRsdl[-1]


# ---- 3. the scenarios of the reference's own test file (tests/admm/test_cbpdntv.py 03, 06; 09 is the
# multi-channel dictionary, refused below) ----------------------------------------------------------------
@pytest.mark.parametrize('chan', [1, 3])
def test_reference_scenarios(backend, chan):
    from sporco_amd.admm import cbpdntv
    N, Nd, M = 16, 5, 4
    np.random.seed(12345)
    D = np.random.randn(Nd, Nd, M)
    s = np.random.randn(N, N) if chan == 1 else np.random.randn(N, N, chan)
    opt = cbpdntv.ConvBPDNRecTV.Options({'Verbose': False, 'MaxMainIter': 20, 'LinSolveCheck': True})
    b = cbpdntv.ConvBPDNRecTV(D, s, 1e-1, 1e-2, opt=opt, dimK=0)
    X = b.solve()
    assert X.shape == (N, N, chan, 1, M) and np.all(np.isfinite(X))
    its = b.getitstat()
    assert its._fields == FIELDS
    assert b.Y.shape == (N, N, chan, 1, M + 2) and b.U.shape == b.Y.shape
    assert b.reconstruct().shape == (N, N, chan, 1)
    assert np.array(its.XSlvRelRes).max() < 1e-5
    assert float(b.rho_xi) == 1.0 and its.Rho[0] == 1.0


# ---- 4. GPU sizes: against the restatement, computed once per module ------------------------------------
GPU_SHAPES = {'fused': (128, 128), 'mr': (160, 192), 'generic': (30, 42)}
# variant: (K, C, per-filter TVWeight, array L1Weight, mu).  mu was chosen on the CPU (the restatement)
# so that after 5 iterations the share of exactly-zero gradient vectors lies inside [0.05, 0.95] for
# every shape and AutoRho has moved rho: the joint norm over three channels needs a larger mu, the
# per-filter weights 0.5 + rand a smaller one
GPU_VARIANTS = {'k8': (8, 1, False, False, 0.35), 'k5': (5, 1, False, False, 0.35), 'c3': (8, 3, False, False, 1.5),
                'tvw': (8, 1, True, False, 0.1), 'l1w': (8, 1, False, True, 0.35)}
GPU_LMBDA, GPU_ITERS = 0.05, 5
_GPU = {}


def _gpu_problem(key, variant):
    if (key, variant) not in _GPU:
        H, W = GPU_SHAPES[key]
        K, C, tvw, l1w, mu = GPU_VARIANTS[variant]
        N = 2
        rng = np.random.RandomState(11)
        D = rng.randn(6, 6, K)
        D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
        S = rng.randn(H, W, C, N)
        opts = {}
        if tvw:
            opts['TVWeight'] = 0.5 + rng.rand(K)
        if l1w:
            opts['L1Weight'] = 0.5 + rng.rand(H, W, 1, N, K)
        ref = rtn.admm_rtv(D.reshape(6, 6, 1, 1, K), S.reshape(H, W, C, N, 1), GPU_LMBDA, mu, GPU_ITERS,
                           wtv=opts.get('TVWeight', 1.0), wl1=opts.get('L1Weight', 1.0))
        ref['zero_share'] = float(np.mean(np.sum(ref['Y'][..., K:] ** 2, axis=(2, 4)) == 0.0))
        _GPU[(key, variant)] = (D, S, opts, ref, mu)
    return _GPU[(key, variant)]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype,tol,tol_tr', [(np.float64, 1e-9, 1e-9), (np.float32, 1e-4, 1e-3)], ids=['f64', 'f32'])
@pytest.mark.parametrize('variant', list(GPU_VARIANTS))
@pytest.mark.parametrize('key', list(GPU_SHAPES))
def test_gpu_sizes(gpu_backend, key, variant, dtype, tol, tol_tr):
    from sporco_amd.admm import cbpdntv
    D, S, opts, ref, mu = _gpu_problem(key, variant)
    print(key, variant, 'zero share', ref['zero_share'], 'rho trace', ref['Rho'])
    assert 0.05 <= ref['zero_share'] <= 0.95
    assert len(set(ref['Rho'])) > 1          # (AutoRho period 1: rho moves)
    o = dict(opts)
    if 'L1Weight' in o:
        o['L1Weight'] = o['L1Weight'].astype(dtype)
    o.update({'Verbose': False, 'MaxMainIter': GPU_ITERS, 'RelStopTol': 0.0})
    b = cbpdntv.ConvBPDNRecTV(D.astype(dtype), S.astype(dtype), GPU_LMBDA, mu, cbpdntv.ConvBPDNRecTV.Options(o),
                              dimK=1)
    b.profile(True)
    b.solve()
    prof = b.profile_read()
    assert prof['rtv_solve'][1] == GPU_ITERS and prof['rtv_ystep'][1] == GPU_ITERS
    K = D.shape[-1]
    figs = {v: rel_l2(getattr(b, v), ref[v]) for v in ('X', 'Y')}
    figs['recon'] = rel_l2(b.reconstruct(), ref['recon'])
    its = b.getitstat()
    trs = {f: rel_l2(getattr(its, f), ref[f]) for f in TRACES}
    print(key, variant, figs, trs)
    for v, e in figs.items():
        assert e < tol, (v, e)
    for f, e in trs.items():
        assert e < tol_tr, (f, e)
    # a padded filter slot (odd K on a register-kernel shape) contributes exactly nothing
    assert b.Y.shape[-1] == K + 2


# ---- 5. refusals ------------------------------------------------------------------------------------
def test_refusals(backend):
    import pickle
    from sporco_amd.admm import cbpdn, cbpdntv
    from sporco_amd.device import DeviceArray
    rng = np.random.RandomState(0)
    D, S = rng.randn(4, 4, 6), rng.randn(12, 12)
    cls = cbpdntv.ConvBPDNRecTV
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
    for name in ('ystep', 'relax_AX', 'ustep'):
        c = cls(D, S, 0.1, 0.01, opt)
        setattr(c, name, lambda: None)
        with pytest.raises(NotImplementedError):
            c.solve()


def test_xstep_override_passes_through(backend):
    g = load_golden('rtv_default_f64')
    a, b = build(g, extra={'MaxMainIter': 8}), build(g, extra={'MaxMainIter': 8})
    b.xstep = lambda: type(b).xstep(b)
    a.solve()
    b.solve()
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(a, v), getattr(b, v)) < 1e-12, v
