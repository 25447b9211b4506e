"""sporco_amd.admm.cbpdnin.ConvBPDNInhib against the reference's fixtures (tests/golden/inhib_*.npz,
float64 runs of the unmodified reference written by tools/make_golden_inhib.py) and, where no
reference exists, against the NumPy restatement of tests/_inhib_numpy.py.

Tolerances are the project's: float64 1e-9 relative l2 on X, Y, U, wml, wms, every trace and
reconstruct(); float32 input 1e-4 on the coefficient maps (and the inhibition weights, which are
a smoothed linear image of |X|) and 1e-3 on the traces, both against the float64 reference.
"""

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _inhib_numpy as inh

FIXTURES = ['inhib_latself_f64', 'inhib_lat_f64', 'inhib_self_f64', 'inhib_nonneg_f64',
            'inhib_whn5_f64', 'inhib_signals_f64', 'inhib_l1w_f64', 'inhib_nobndry_f64',
            'inhib_overlap_f64', 'inhib_fixedrho_f64', 'inhib_auxvar_f64', 'inhib_inactive_f64']
TRACES = ('ObjFun', 'DFid', 'RegL1', 'RegLat', 'RegSelf', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal',
          'EpsDual', 'Rho')


def options_of(g, extra=None):
    o = {'Verbose': False, 'MaxMainIter': int(g['MaxMainIter']), 'RelStopTol': 0.0,
         'NonNegCoef': bool(g['opt_NonNegCoef']), 'NoBndryCross': bool(g['opt_NoBndryCross']),
         'RelaxParam': float(g['opt_RelaxParam'])}
    if bool(g['opt_AuxVarObj']):
        o['AuxVarObj'] = True
    if not np.isnan(g['opt_rho']):
        o['rho'] = float(g['opt_rho'])
    if not bool(g['opt_AutoRho']):
        o['AutoRho'] = {'Enabled': False}
    if 'optarr_L1Weight' in g:
        o['L1Weight'] = g['optarr_L1Weight']
    o.update(extra or {})
    return o


def build(g, dtype=np.float64, extra=None, staged=False):
    from sporco_amd.admm import cbpdnin
    b = cbpdnin.ConvBPDNInhib(g['D'].astype(dtype), g['S'].astype(dtype), Wg=g.get('Wg'),
                              Whn=int(g['Whn']) or None, lmbda=float(g['lmbda']), mu=float(g['mu']),
                              gamma=float(g['gamma']),
                              opt=cbpdnin.ConvBPDNInhib.Options(options_of(g, extra)),
                              dimK=int(g['dimK']), dimN=int(g['dimN']))
    if staged:
        b.xstep = lambda: type(b).xstep(b)       # a pass-through override: the step-by-step path
        assert not b._fused_ok()
    return b


def check(b, g, tol, tol_tr, with_u=True):
    its = b.getitstat()
    figs = {v: rel_l2(getattr(b, v), g[v]) for v in (('X', 'Y', 'U') if with_u else ('X', 'Y'))}
    for v in ('wml', 'wms'):
        figs[v] = rel_l2(np.asarray(getattr(b, v), dtype=np.float64) + 0.0 * g[v], g[v])
    figs['recon'] = rel_l2(b.reconstruct(), g['recon'])
    trs = {f: rel_l2(getattr(its, f), g['it_' + f]) for f in TRACES}
    print(figs, trs, 'rho', float(b.rho), float(g['rho_final']))
    for v, e in figs.items():
        assert e < tol, (v, e)
    for f, e in trs.items():
        assert e < tol_tr, (f, e)
    assert abs(float(b.rho) - float(g['rho_final'])) <= tol_tr * float(g['rho_final'])


# ---- 1. the fixtures: float64 and float32, fused-capable iteration and staged path -----------------
@pytest.mark.parametrize('staged', [False, True], ids=['fused', 'staged'])
@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f64(backend, name, staged):
    g = load_golden(name)
    b = build(g, np.float64, staged=staged)
    b.solve()
    check(b, g, 1e-9, 1e-9)
    assert b.wml is not None and np.shape(b.X) == np.shape(g['X'])


@pytest.mark.parametrize('staged', [False, True], ids=['fused', 'staged'])
@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f32(backend, name, staged):
    g = load_golden(name)
    b = build(g, np.float32, staged=staged)
    b.solve()
    assert b.Y.dtype == np.float32
    check(b, g, 1e-4, 1e-3, with_u=False)


def test_gevaly_false_is_the_default(backend):
    """The reference's default evaluates the regularisers at X (gEvalY False)."""
    g = load_golden('inhib_latself_f64')
    b = build(g, extra={'gEvalY': False})
    b.solve()
    check(b, g, 1e-9, 1e-9)


def test_fused_and_staged_agree(backend):
    g = load_golden('inhib_latself_f64')
    a, b = build(g, extra={'MaxMainIter': 12}), build(g, extra={'MaxMainIter': 12}, staged=True)
    a.solve()
    b.solve()
    for v in ('X', 'Y', 'U', 'wml', 'wms'):
        assert rel_l2(getattr(a, v), getattr(b, v)) < 1e-12, v
    assert rel_l2(a.getitstat().ObjFun, b.getitstat().ObjFun) < 1e-12


# ---- 2. the scenarios of the reference's own test file ----------------------------------------------
def _scenarios():
    pair = np.append(np.eye(16), np.eye(16), axis=-1)
    return [
        (dict(), (8, 8), (4, 4, 32), (8, 8, 1, 1, 32)),
        (dict(Wg=pair, lmbda=0.1), (8, 8), (4, 4, 32), (8, 8, 1, 1, 32)),
        (dict(Wg=pair, lmbda=0.1), (8, 8, 3), (4, 4, 32), (8, 8, 1, 3, 32)),   # (three signals)
        (dict(lmbda=0.1, gamma=0.01), (8, 8), (4, 4, 32), (8, 8, 1, 1, 32)),
        (dict(lmbda=0.1, mu=0.01), (8, 8), (4, 4, 32), (8, 8, 1, 1, 32)),
        (dict(Wg=pair, lmbda=0.1, mu=0.01, gamma=0.01, dimN=1), (64,), (4, 32), (64, 1, 1, 32)),
    ]


@pytest.mark.parametrize('idx', range(6))
def test_reference_scenarios(backend, idx):
    from sporco_amd.admm import cbpdnin
    kw, sshape, dshape, xshape = _scenarios()[idx]
    np.random.seed(12345)
    D = np.random.randn(*dshape)
    s = np.random.randn(*sshape)
    opt = cbpdnin.ConvBPDNInhib.Options({'Verbose': False, 'MaxMainIter': 10})
    b = cbpdnin.ConvBPDNInhib(D, s, opt=opt, **kw)
    X = b.solve()
    assert X.shape == xshape and np.all(np.isfinite(X))
    its = b.getitstat()
    assert its._fields[1:6] == ('ObjFun', 'DFid', 'RegL1', 'RegLat', 'RegSelf')
    assert np.all(np.isfinite(its.ObjFun))
    for w in (b.wml, b.wms):
        assert np.ndim(w) == 0 or np.shape(w) == xshape


# ---- 3. inhib_update alone through the C ABI --------------------------------------------------------
def test_numpy_update_pinned_to_fixture():
    """The restatement reproduces the reference's last update: weights of iteration 40 from those
    of a 39-iteration run cannot be read from the fixture, so the whole solve is restated and
    pinned instead (float64, 1e-12)."""
    for name in ('inhib_latself_f64', 'inhib_overlap_f64', 'inhib_whn5_f64', 'inhib_auxvar_f64',
                 'inhib_nonneg_f64'):
        g = load_golden(name)
        th, tw = inh.window_taps(int(g['Whn']) or g['D'].shape[0])
        r = inh.admm_inhib(g['D'].reshape(6, 6, 1, 1, 8), g['S'].reshape(32, 40, 1, 2, 1), g['Wg'], th,
                           tw, float(g['lmbda']), float(g['mu']), float(g['gamma']),
                           int(g['MaxMainIter']), nonneg=bool(g['opt_NonNegCoef']),
                           gevaly=bool(g['opt_AuxVarObj']), fevalx=not bool(g['opt_AuxVarObj']))
        for v in ('X', 'Y', 'U', 'wml', 'wms'):
            assert rel_l2(r[v], g[v]) < 1e-12, (name, v)
        for f in ('ObjFun', 'RegL1', 'RegLat', 'RegSelf', 'Rho'):
            assert rel_l2(r[f], g['it_' + f]) < 1e-12, (name, f)


ABI_CASES = [
    # H, W, C, N, K, taps (rows, cols), groups, dtype
    (15, 17, 1, 2, 6, (3, 3), 'pair', np.float64),
    (15, 17, 2, 1, 5, (9, 9), 'over', np.float64),          # K not a multiple of 4
    (21, 19, 1, 2, 7, (17, 17), 'pair', np.float64),
    (15, 17, 1, 1, 6, (15, 15), 'over', np.float64),        # Whn = min(H, W): wraps on every side
    (12, 10, 1, 2, 8, (10, 10), 'pair', np.float64),        # even tap count
    (1, 50, 1, 3, 6, (1, 9), 'pair', np.float64),           # folded dimN = 1
    (15, 17, 1, 2, 6, (9, 5), None, np.float64),            # self term only, different tap counts
    (15, 17, 1, 2, 6, (9, 9), 'pair', np.float32),
    (16, 24, 1, 2, 40, (5, 5), 'pair', np.float32),
]


@pytest.mark.parametrize('case', ABI_CASES, ids=lambda c: '%dx%dx%dx%dx%d-%s-%s-%s' % (
    c[:5] + ('x'.join(map(str, c[5])), c[6], np.dtype(c[7]).name)))
def test_inhib_update_abi(backend, case):
    from scipy import signal
    from sporco_amd import _lib
    H, W, C, N, K, (nh, nw), groups, dtype = case
    rng = np.random.RandomState(H * 1000 + W * 10 + K)
    shp = (H, W, C, N, K)
    # a non-symmetric window: scipy's periodic Tukey taps, as the class uses them
    th = np.ones(1) if nh == 1 else np.sqrt(signal.get_window(('tukey', 0.5), nh))
    tw = np.sqrt(signal.get_window(('tukey', 0.5), nw)) if nh > 1 else signal.get_window(('tukey', 0.5), nw)
    if groups == 'pair':
        Wg = np.zeros((K // 2, K))
        for m in range(K // 2):
            Wg[m, m] = Wg[m, m + K // 2] = 1.0
    elif groups == 'over':
        Wg = np.zeros((2, K))
        Wg[0, :K // 2 + 1] = 1.0
        Wg[1, K // 2 - 1:] = 1.0
    else:
        Wg = None
    X = (rng.randn(*shp) * (rng.rand(*shp) < 0.3)).astype(dtype)
    Y = (rng.randn(*shp) * (rng.rand(*shp) < 0.3)).astype(dtype)
    wl1 = (0.5 + rng.rand(*shp)).astype(dtype)
    lmbda, mu, gamma, smooth = 0.07, 0.5 if Wg is not None else 0.0, 0.03, 0.9
    s = _lib.Solver(H, W, C, N, K, dtype)
    s.set_signal(np.zeros((H, W, C, N), dtype=dtype))
    s.set_dict(rng.randn(1, 1, K).astype(dtype))
    s.set_l1_weight(wl1)
    s.inhib_setup(Wg, th, tw, True, lmbda)
    s.profile(True)
    tol = 1e-12 if dtype == np.float64 else 2e-6      # (float32: a few units of 2^-24 over <= 17^2 taps)
    def compare(out, r):
        if Wg is not None:
            assert rel_l2(s.download(_lib.VAR_WML), r['wml']) < tol
        assert rel_l2(s.download(_lib.VAR_WMS), r['wms']) < tol
        for slot, key in ((_lib.OUT_L1, 'rl'), (_lib.OUT_L21, 'rm'), (_lib.OUT_RGR, 'rg')):
            assert abs(out[slot] - r[key]) <= tol * max(abs(r[key]), 1.0), (key, out[slot], r[key])

    # two updates in a row (the second smooths real previous weights), sums against Y
    wml, wms = None, None
    w64 = wl1.astype(np.float64)
    for it in range(2):
        s.upload(_lib.VAR_X, X)
        s.upload(_lib.VAR_Y, Y)
        out = s.inhib_update(lmbda, mu, gamma, smooth, _lib.FLAG_GEVAL_Y)
        r = inh.inhib_update(X, Y, w64, wml, wms, Wg, th, tw, lmbda, mu, gamma, smooth)
        compare(out, r)
        wml, wms = r['wml'], r['wms']
        X = (X + 0.5 * rng.randn(*shp) * (rng.rand(*shp) < 0.2)).astype(dtype)
    # a fresh set-up starts from zero weights again; sums against X
    s.inhib_setup(Wg, th, tw, True, lmbda)
    s.upload(_lib.VAR_X, X)
    out = s.inhib_update(lmbda, mu, gamma, smooth, 0)
    compare(out, inh.inhib_update(X, X, w64, None, None, Wg, th, tw, lmbda, mu, gamma, smooth))
    prof = s.profile_read()
    assert prof['inhib_update'][1] == 3


def test_thresholds_reach_the_ystep(backend):
    """After an update the staged y step shrinks with T / rho = (lmbda wl1 + mu wml + gamma wms) / rho."""
    from sporco_amd import _lib
    H, W, C, N, K = 9, 11, 1, 2, 6
    rng = np.random.RandomState(3)
    shp = (H, W, C, N, K)
    th, tw = inh.window_taps(5)
    Wg = np.append(np.eye(3), np.eye(3), axis=-1)
    X, V = rng.randn(*shp), rng.randn(*shp)
    s = _lib.Solver(H, W, C, N, K, np.float64)
    s.set_signal(np.zeros((H, W, C, N)))
    s.set_dict(rng.randn(1, 1, K))
    s.inhib_setup(Wg, th, tw, True, 0.2)
    s.upload(_lib.VAR_X, X)
    s.inhib_update(0.2, 0.5, 0.1, 0.9, 0)
    r = inh.inhib_update(X, X, 1.0, None, None, Wg, th, tw, 0.2, 0.5, 0.1, 0.9)
    s.upload(_lib.VAR_AX, V)
    s.upload(_lib.VAR_U, np.zeros(shp))
    p = _lib.AdmmParams()
    p.rho, p.lmbda, p.mu, p.rlx, p.u_scale, p.flags, p.dH, p.dW = 2.0, 1.0, 0.0, 1.0, 1.0, 0, 1, 1
    s.admm_ystep(p)
    want = np.sign(V) * np.maximum(np.abs(V) - r['T'] / 2.0, 0.0)
    assert rel_l2(s.download(_lib.VAR_Y), want) < 1e-12


# ---- 4. refusals ------------------------------------------------------------------------------------
def test_refusals(backend):
    from sporco_amd.admm import cbpdn, cbpdnin
    rng = np.random.RandomState(0)
    D, S = rng.randn(4, 4, 6), rng.randn(12, 12)
    Wg = np.append(np.eye(3), np.eye(3), axis=-1)
    opt = cbpdnin.ConvBPDNInhib.Options({'MaxMainIter': 2})
    with pytest.raises(NotImplementedError):
        cbpdnin.ConvBPDNInhib(rng.randn(3, 3, 3, 6), rng.randn(8, 8, 8), Wg=Wg, lmbda=0.1, opt=opt, dimN=3)
    with pytest.raises(NotImplementedError):
        cbpdnin.ConvBPDNInhib(D, S, Wg=Wg, lmbda=0.1, opt=opt, reducer=object())
    with pytest.raises(NotImplementedError):
        cbpdnin.ConvBPDNInhib(D.astype(complex), S.astype(complex), Wg=Wg, lmbda=0.1, opt=opt)
    with pytest.raises(NotImplementedError):
        cbpdn.AddMaskSim(cbpdnin.ConvBPDNInhib, D, S, np.ones((12, 12)), Wg=np.append(Wg, np.zeros((3, 1)), 1),
                         lmbda=0.1, opt=opt)
    with pytest.raises(NotImplementedError):
        cbpdnin.ConvBPDNInhib(rng.randn(4, 4, 3, 6), rng.randn(12, 12, 3), Wg=Wg, lmbda=0.1, opt=opt)
    with pytest.raises(ValueError):
        cbpdnin.ConvBPDNInhib(D, S, Wg=Wg, Whn=13, lmbda=0.1, opt=opt)
    with pytest.raises(ValueError):
        cbpdnin.ConvBPDNInhib(D, S, Wg=np.eye(5), lmbda=0.1, opt=opt)
    b = cbpdnin.ConvBPDNInhib(D, S, Wg=Wg, lmbda=0.1, opt=opt)
    assert not b._device_loop_ok()


# ---- 5. the profile shows the kernel -----------------------------------------------------------------
def test_profile_slot(backend):
    g = load_golden('inhib_latself_f64')
    b = build(g, extra={'MaxMainIter': 7})
    b.profile(True)
    b.solve()
    assert b.profile_read()['inhib_update'][1] == 7
    g = load_golden('inhib_inactive_f64')
    b = build(g, extra={'MaxMainIter': 7})
    b.profile(True)
    b.solve()
    assert b.profile_read()['inhib_update'][1] == 0
    assert b.getitstat().RegLat[-1] == 0.0 and b.getitstat().RegSelf[-1] == 0.0


# ---- GPU sizes: against the restatement, computed once per module ------------------------------------
_GPU = {}


def _gpu_problem(key):
    if key not in _GPU:
        H, W, K, N, dt, iters = {'fused': (256, 256, 32, 2, np.float32, 10),
                                 'mr': (240, 320, 16, 2, np.float32, 10),
                                 'generic': (200, 200, 8, 2, np.float64, 10)}[key]
        rng = np.random.RandomState(11)
        D = rng.randn(8, 8, K)
        D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
        S = rng.randn(H, W, N)
        Wg = np.append(np.eye(K // 2), np.eye(K // 2), axis=-1)
        th, tw = inh.window_taps(8)
        ref = inh.admm_inhib(D.reshape(8, 8, 1, 1, K), S.reshape(H, W, 1, N, 1), Wg, th, tw, 0.05, 0.5, 0.02,
                             iters)
        _GPU[key] = (D.astype(dt), S.astype(dt), Wg, iters, ref)
    return _GPU[key]


@pytest.mark.gpu
@pytest.mark.parametrize('key,tol', [('fused', 1e-4), ('mr', 1e-4), ('generic', 1e-9)])
def test_gpu_sizes(gpu_backend, key, tol):
    from sporco_amd.admm import cbpdnin
    D, S, Wg, iters, ref = _gpu_problem(key)
    opt = cbpdnin.ConvBPDNInhib.Options({'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0})
    b = cbpdnin.ConvBPDNInhib(D, S, Wg=Wg, lmbda=0.05, mu=0.5, gamma=0.02, opt=opt, dimK=1)
    if key != 'generic':
        assert b._dev.uses_fused_rows()
    else:
        assert not b._dev.uses_fused_rows()
    b.profile(True)
    b.solve()
    assert b.profile_read()['inhib_update'][1] == iters
    figs = {v: rel_l2(getattr(b, v), ref[v]) for v in ('X', 'Y', 'wml', 'wms')}
    figs['ObjFun'] = rel_l2(b.getitstat().ObjFun, ref['ObjFun'])
    print(key, figs)
    for v, e in figs.items():
        assert e < (tol if v != 'ObjFun' or tol < 1e-6 else 1e-3), (v, e)
