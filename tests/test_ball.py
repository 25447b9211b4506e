"""sporco_amd.admm.cbpdn.ConvMinL1InL2Ball and sporco_amd.prox.proj_l2 against the reference's fixtures
(tests/golden/ball_*_f64.npz, float64 runs of the unmodified reference written by
tools/make_golden_ball.py) and, at the GPU sizes, against the NumPy restatement of tests/_ball_numpy.py,
which is itself pinned to the reference first.

Tolerances are the project's: float64 1e-9 relative l2 on X, Y, U, reconstruct(), every trace and the
final rho; float32 input 1e-4 on X, Y and reconstruct() and 1e-3 on the traces, both against the float64
reference -- except the float32 DualRsdl trace and Cnstr, see F32_DUAL_MEASURED and F32_CNSTR_MEASURED.
Cnstr is a difference of near-equal norms late in a run (and exactly 0 under AuxVarObj): it is compared
absolutely, |delta| <= tol * epsilon.
"""

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _ball_numpy as bn

CASES = ['default', 'fixed', 'autorho', 'auxvar', 'l1w_nonneg_nobndry', 'mcd', 'mcs', 'y0warm']
FIXTURES = ['ball_%s_f64' % n for n in CASES]
TRACES = ('ObjFun', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho')       # (Cnstr: absolutely)
FIELDS = ('Iter', 'ObjFun', 'Cnstr', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho', 'XSlvRelRes', 'Time')

# Measured, not taken from the library: the NumPy restatement run in float32 against each float64
# fixture (test_f32_tolerances_are_the_measured_ones repeats the measurement).
#   DualRsdl, worst relative error of an entry of the trace: 9.5e-5 (y0warm; the others between
#   1.4e-6 and 1.8e-5); as a relative l2 error of the whole trace the worst is 1.1e-6 (autorho).
#   Cnstr, worst |delta| / epsilon of an entry: 6.9e-7 (default; the others between 2.9e-8 and 5.5e-7).
# Allowed: four times the measured value (summation order), never below the project's 1e-3.
F32_DUAL_MEASURED = 9.5e-5
F32_CNSTR_MEASURED = 6.9e-7
F32_DUAL_TOL = max(4.0 * F32_DUAL_MEASURED, 1e-3)
F32_CNSTR_TOL = max(4.0 * F32_CNSTR_MEASURED, 1e-3)


def autorho_of(g):
    if not bool(g['opt_AutoRho']):
        return None
    return {'Period': int(g['opt_AutoRho_Period']), 'Scaling': float(g['opt_AutoRho_Scaling']),
            'RsdlRatio': float(g['opt_AutoRho_RsdlRatio']), 'AutoScaling': bool(g['opt_AutoRho_AutoScaling']),
            'RsdlTarget': float(g['opt_AutoRho_RsdlTarget'])}


def options_of(g, dtype, extra=None):
    o = {'Verbose': False, 'MaxMainIter': int(g['MaxMainIter']), 'RelStopTol': 0.0, 'rho': float(g['opt_rho']),
         'RelaxParam': float(g['opt_RelaxParam'])}
    for key in ('AuxVarObj', 'NonNegCoef', 'NoBndryCross'):
        if bool(g['opt_' + key]):
            o[key] = True
    ar = autorho_of(g)
    o['AutoRho'] = dict(ar, Enabled=True) if ar else {'Enabled': False}
    if 'optarr_L1Weight' in g:
        o['L1Weight'] = g['optarr_L1Weight'].astype(dtype)
    if 'optarr_Y0' in g:
        o['Y0'] = g['optarr_Y0'].astype(dtype)
    o.update(extra or {})
    return o


def build(g, dtype=np.float64, extra=None, **over):
    from sporco_amd.admm import cbpdn
    o = options_of(g, dtype, extra)
    D = over.pop('D', g['D']).astype(dtype)
    eps = over.pop('epsilon', float(g['epsilon']))
    assert not over
    return cbpdn.ConvMinL1InL2Ball(D, g['S'].astype(dtype), eps, cbpdn.ConvMinL1InL2Ball.Options(o),
                                   dimK=int(g['dimK']))


def five(D, S, dimK=1):
    """D and S in the restatement's five-dimensional layout."""
    D5 = D.reshape(D.shape[:2] + ((D.shape[2], 1, D.shape[3]) if D.ndim == 4 else (1, 1, D.shape[2])))
    if S.ndim == 2:
        S5 = S.reshape(S.shape + (1, 1, 1))
    elif S.ndim == 4:
        S5 = S.reshape(S.shape + (1,))
    else:
        S5 = S.reshape(S.shape[:2] + ((1, S.shape[2], 1) if dimK == 1 else (S.shape[2], 1, 1)))
    return D5, S5


def warm_state(g, S5, dtype=np.float64):
    """The state a Y0 without U0 starts from: U0 = sign(block 0) / rho, U1 = block 1 - S."""
    Y = g['optarr_Y0'].astype(dtype)
    rho = dtype(g['opt_rho'])
    return dict(Y0=Y[..., :1], Y1=Y[..., 1:], U0=(np.sign(Y[..., :1]) / rho).astype(dtype),
                U1=(Y[..., 1:] - S5.astype(dtype)).astype(dtype), rho=rho)


def restated(g, dtype=np.float64, **kw):
    """The restatement's solve of a fixture's problem."""
    D5, S5 = five(g['D'], g['S'], int(g['dimK']))
    args = dict(wl1=g['optarr_L1Weight'] if 'optarr_L1Weight' in g else 1.0, rho=float(g['opt_rho']),
                rlx=float(g['opt_RelaxParam']), auxvar=bool(g['opt_AuxVarObj']), ar=autorho_of(g),
                nonneg=bool(g['opt_NonNegCoef']), nobndry=bool(g['opt_NoBndryCross']), dtype=dtype)
    if 'optarr_Y0' in g:
        args['state'] = warm_state(g, S5, np.dtype(dtype).type)
    args.update(kw)
    return bn.admm_ball(D5, S5, float(g['epsilon']), int(g['MaxMainIter']), **args)


def check(b, g, tol, tol_tr, with_u=True, f32=False):
    its = b.getitstat()
    eps = float(g['epsilon'])
    figs = {v: rel_l2(getattr(b, v), g[v]) for v in (('X', 'Y', 'U') if with_u else ('X', 'Y'))}
    figs['recon'] = rel_l2(b.reconstruct(), g['recon'])
    trs = {f: rel_l2(getattr(its, f), g['it_' + f]) for f in TRACES}
    dual = np.max(np.abs(np.asarray(its.DualRsdl) - g['it_DualRsdl']) / np.abs(g['it_DualRsdl']))
    cn = np.max(np.abs(np.asarray(its.Cnstr) - g['it_Cnstr'])) / eps
    print(figs, trs, 'DualRsdl worst entry', dual, 'Cnstr worst |delta| / eps', cn, 'rho', float(b.rho),
          float(g['rho_final']))
    for v, e in figs.items():
        assert e < tol, (v, e)
    for f, e in trs.items():
        assert e < tol_tr, (f, e)
    assert dual < (F32_DUAL_TOL if f32 else tol_tr)
    assert cn <= (F32_CNSTR_TOL if f32 else tol_tr)
    assert abs(float(b.rho) - float(g['rho_final'])) <= tol_tr * float(g['rho_final'])
    assert b.X.shape == g['X'].shape and b.Y.shape == g['Y'].shape and b.U.shape == g['U'].shape
    assert b.var_y0().shape == g['Y0'].shape and b.var_y1().shape == g['Y1'].shape
    assert b.reconstruct().shape == g['recon'].shape


def same_run(a, b, tol=1e-9, traces=TRACES + ('Cnstr',)):
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(a, v), getattr(b, v)) < tol, v
    ia, ib = a.getitstat(), b.getitstat()
    for f in traces:
        assert rel_l2(getattr(ia, f), getattr(ib, f)) < tol, f


# ---- 1. the restatement and the fixtures -------------------------------------------------------------
def test_numpy_restatement_pinned_to_fixtures():
    """The iteration as built reproduces every fixture, and one iteration from the reference's state
    after 39 iterations reproduces its state after 40 (float64, 1e-9; Cnstr absolutely)."""
    for name in FIXTURES:
        g = load_golden(name)
        r = restated(g)
        for v in ('X', 'Y', 'U', 'recon'):
            assert rel_l2(r[v].reshape(g[v].shape), g[v]) < 1e-9, (name, v)
        for f in TRACES:
            assert rel_l2(r[f], g['it_' + f]) < 1e-9, (name, f)
        assert np.max(np.abs(r['Cnstr'] - g['it_Cnstr'])) <= 1e-9 * float(g['epsilon']), name
        assert abs(r['rho'] - float(g['rho_final'])) < 1e-9 * float(g['rho_final'])
        assert np.array_equal(np.mean(r['active'], axis=0), g['active_share'].ravel()), name
    g = load_golden('ball_step_f64')
    D5, S5 = five(g['D'], g['S'])
    H, W = S5.shape[:2]
    Df = np.fft.rfftn(D5, s=(H, W), axes=(0, 1))
    Yb, Ub = g['Y_before'], g['U_before']
    st = dict(Y0=Yb[..., :1], Y1=Yb[..., 1:], U0=Ub[..., :1], U1=Ub[..., 1:], rho=np.float64(g['rho_before']))
    rec = bn.iterate(st, Df, S5, np.float64(1.0), float(g['epsilon']), 1.8, False, None, int(g['k']), (H, W),
                     D5.shape[:2])
    assert rel_l2(st['X'], g['X']) < 1e-9
    assert rel_l2(bn.block_cat(st['Y0'], st['Y1']), g['Y']) < 1e-9
    assert rel_l2(bn.block_cat(st['U0'], st['U1']), g['U']) < 1e-9
    for f in ('ObjFun', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert abs(rec[f] - float(g['last_' + f])) <= 1e-9 * abs(float(g['last_' + f])), f
    assert abs(rec['Cnstr'] - float(g['last_Cnstr'])) <= 1e-9 * float(g['epsilon'])


def test_fixtures_take_both_branches():
    """Both branches of the projection are taken, differently per plane: a plane projected in at least
    90 % of the iterations and one in 2 % to 50 % of them (a single image has one regime); the
    non-zero share of the final y1 lies in [0.05, 0.95]; rho moves in the autorho fixture."""
    for name in FIXTURES:
        g = load_golden(name)
        sh = g['active_share']
        if g['S'].ndim > 2:
            assert np.any(sh >= 0.9) and np.any((sh >= 0.02) & (sh <= 0.5)), (name, sh)
        share = float(np.mean(g['Y1'] != 0.0))
        assert 0.05 <= share <= 0.95 and share == float(g['nz_y1']), (name, share)
    assert len(set(load_golden('ball_autorho_f64')['it_Rho'])) > 2


def test_f32_tolerances_are_the_measured_ones():
    """The constants above are what the restatement gives in float32 (the measurement, repeated on
    the two worst fixtures)."""
    dual = cn = 0.0
    for name in ('ball_y0warm_f64', 'ball_default_f64'):
        g = load_golden(name)
        r = restated(g, np.float32)
        dual = max(dual, float(np.max(np.abs(r['DualRsdl'] - g['it_DualRsdl']) / np.abs(g['it_DualRsdl']))))
        cn = max(cn, float(np.max(np.abs(r['Cnstr'] - g['it_Cnstr']))) / float(g['epsilon']))
    print('float32 restatement: worst DualRsdl entry error', dual, 'worst Cnstr |delta| / eps', cn)
    assert 0.5 * F32_DUAL_MEASURED < dual < 1.5 * F32_DUAL_MEASURED
    assert 0.5 * F32_CNSTR_MEASURED < cn < 1.5 * F32_CNSTR_MEASURED


# ---- 2, 3. the fixtures ---------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f64(backend, name):
    g = load_golden(name)
    b = build(g, np.float64)
    b.solve()
    check(b, g, 1e-9, 1e-9)
    assert b.getitstat()._fields == FIELDS
    assert all(v is None for v in b.getitstat().XSlvRelRes)
    assert b.epsilon.dtype == np.float64


@pytest.mark.parametrize('name', FIXTURES)
def test_fixture_f32(backend, name):
    g = load_golden(name)
    b = build(g, np.float32)
    b.solve()
    assert b.X.dtype == np.float32 and b.Y.dtype == np.float32 and b.U.dtype == np.float32
    assert b.epsilon.dtype == np.float32
    check(b, g, 1e-4, 1e-3, with_u=False, f32=True)


# ---- 4. prox.proj_l2 ---------------------------------------------------------------------------------
def np_proj_l2(v, gamma, axis):
    d = np.sqrt(np.sum(v ** 2, axis=axis, keepdims=True))
    return np.where(d <= gamma, v, gamma * v / np.where(d == 0, 1, d))


@pytest.mark.parametrize('dtype,tol', [(np.float64, 1e-12), (np.float32, 1e-6)])
@pytest.mark.parametrize('shape,axis', [((7, 9, 5), None), ((3, 10, 4), 1), ((3, 10, 5), -2), ((4, 3, 8), (1,)),
                                        ((6, 7, 1), (0, 1)), ((6, 7, 6), (0, 1)), ((5, 4, 300), (0, 1)),
                                        ((5, 4, 3, 4), (0, 1)), ((2, 3, 4, 5), (1, 2)), ((40, 52), None),
                                        ((40, 52, 2), (1, 0))])
def test_proj_l2(backend, shape, axis, dtype, tol):
    """Against the NumPy expression: every plane scaled independently, planes inside and outside the
    ball in one call (the planes' norms straddle gamma: they are scaled by 0.2 ... 1.8 of it)."""
    from sporco_amd import prox
    rng = np.random.RandomState(5)
    v = rng.randn(*shape)
    ax = axis if axis is None else (tuple(axis) if isinstance(axis, tuple) else (axis,))
    d = np.sqrt(np.sum(v ** 2, axis=ax, keepdims=True))
    gamma = 2.5
    scale = gamma * np.linspace(0.2, 1.8, d.size).reshape(d.shape) / d
    v = (v * scale).astype(dtype)
    want = np_proj_l2(v.astype(np.float64), gamma, ax)
    d = np.sqrt(np.sum(v.astype(np.float64) ** 2, axis=ax, keepdims=True))
    if d.size > 1:
        assert np.any(d < gamma) and np.any(d > gamma)
    got = prox.proj_l2(v, gamma, axis=axis)
    assert got.dtype == dtype and got.shape == v.shape
    assert rel_l2(got, want) < tol
    inside = np.broadcast_to(d <= gamma, v.shape)
    assert np.array_equal(got[inside], v[inside])          # (a plane inside the ball is returned bit for bit)


def test_proj_l2_edges(backend):
    """A plane of zeros stays zero; a plane whose norm is exactly gamma is returned as it is; both beside
    a plane that is scaled, in the same call."""
    from sporco_amd import prox
    v = np.zeros((2, 2, 3))
    v[:, :, 1] = [[3.0, 0.0], [0.0, 4.0]]        # norm exactly 5
    v[:, :, 2] = [[6.0, 0.0], [8.0, 0.0]]        # norm 10
    got = prox.proj_l2(v, 5.0, axis=(0, 1))
    assert np.all(got[:, :, 0] == 0.0) and np.array_equal(got[:, :, 1], v[:, :, 1])
    assert np.max(np.abs(got[:, :, 2] - 0.5 * v[:, :, 2])) < 1e-12 * 10
    assert np.array_equal(prox.proj_l2(np.zeros(5), 1.0), np.zeros(5))
    assert rel_l2(prox.proj_l2(np.array([3.0, 4.0], dtype=np.float32), 1.0), [0.6, 0.8]) < 1e-6
    with pytest.raises(NotImplementedError):
        prox.proj_l2(v, 5.0, axis=(0, 2))
    with pytest.raises(NotImplementedError):
        prox.proj_l2(v, np.ones(3), axis=(0, 1))
    with pytest.raises(NotImplementedError):
        prox.proj_l2(v.astype(complex), 5.0)
    with pytest.raises(NotImplementedError):
        prox.proj_l2(v, 5.0, axis='x')


# ---- 5. behaviour -------------------------------------------------------------------------------------------
def test_options_defaults_and_fields(backend):
    from sporco_amd.admm import cbpdn
    cls = cbpdn.ConvMinL1InL2Ball
    opt = cls.Options()
    want = {'AuxVarObj': False, 'fEvalX': True, 'gEvalY': False, 'RelaxParam': 1.8, 'rho': 1.0, 'L1Weight': 1.0,
            'NonNegCoef': False, 'ReturnVar': 'Y1'}
    for key, val in want.items():
        assert opt[key] == val, key
    ar = {'Enabled': True, 'Period': 10, 'AutoScaling': True, 'Scaling': 1000.0, 'RsdlRatio': 1.2, 'RsdlTarget': 1.0}
    for key, val in ar.items():
        assert opt['AutoRho', key] == val, key
    assert not cbpdn.ConvBPDNMaskDcpl.Options()['AutoRho', 'Enabled']      # (the parent's stay its own)
    assert cls.hdrtxt_objfn == ('Fnc', 'Cnstr')
    rng = np.random.RandomState(0)
    b = cls(rng.randn(4, 4, 3), rng.randn(12, 12), 1.0, cls.Options({'MaxMainIter': 2}))
    b.solve()
    assert b.getitstat()._fields == FIELDS
    assert float(b.lmbda) == 1.0


def test_refusals(backend):
    import pickle
    from sporco_amd.admm import cbpdn
    from sporco_amd.device import DeviceArray
    cls = cbpdn.ConvMinL1InL2Ball
    rng = np.random.RandomState(0)
    D, S = rng.randn(4, 4, 6), rng.randn(12, 12, 2)
    opt = cls.Options({'MaxMainIter': 2})
    with pytest.raises(NotImplementedError):
        cls(rng.randn(4, 6), rng.randn(32, 3), 1.0, opt=opt, dimN=1)
    with pytest.raises(NotImplementedError):
        cls(rng.randn(3, 3, 3, 6), rng.randn(8, 8, 8, 3), 1.0, opt=opt, dimN=3)
    with pytest.raises(NotImplementedError):
        cls(D.astype(complex), S.astype(complex), 1.0, opt=opt)
    with pytest.raises(NotImplementedError):
        cls(D, S, 1.0, opt=opt, reducer=object())
    with pytest.raises(NotImplementedError):
        cls(D, S, 1.0, opt=opt, resident=True)
    with pytest.raises(NotImplementedError):
        cls(D, DeviceArray((12, 12, 2), np.float64), 1.0, opt=opt)
    with pytest.raises(ValueError):
        cls(D, S, 1.0, opt=cls.Options({'ReturnVar': 'Z'}))
    with pytest.raises(ValueError):
        cls(D, S, -1.0, opt=opt)
    b = cls(D, S, 1.0, opt=opt)
    with pytest.raises(NotImplementedError):
        pickle.dumps(b)


def test_y0_without_u0(backend):
    """The reference's rule, where its shapes fit (a single image), and a ValueError naming the shapes
    where they do not (several images; a multi-channel dictionary)."""
    from sporco_amd.admm import cbpdn
    cls = cbpdn.ConvMinL1InL2Ball
    g = load_golden('ball_y0warm_f64')
    b = build(g, extra={'MaxMainIter': 1})
    assert rel_l2(b.U, g['optarr_U0']) < 1e-15
    assert rel_l2(b.Y, g['optarr_Y0']) == 0.0
    rng = np.random.RandomState(1)
    with pytest.raises(ValueError, match=r'\(12, 12, 2, 1, 1\).*\(12, 12, 1, 2, 6\)'):
        cls(rng.randn(4, 4, 6), rng.randn(12, 12, 2), 1.0, cls.Options({'Y0': rng.randn(12, 12, 1, 2, 7)}), dimK=1)
    with pytest.raises(ValueError, match=r'\(12, 12, 3, 1, 1\).*\(12, 12, 1, 1, 4\)'):
        cls(rng.randn(4, 4, 3, 4), rng.randn(12, 12, 3), 1.0, cls.Options({'Y0': rng.randn(12, 12, 1, 1, 7)}), dimK=0)
    # (with a U0 beside it, the Y0 is taken as it is, whatever the shapes)
    Y0 = rng.randn(12, 12, 1, 2, 7)
    c = cls(rng.randn(4, 4, 6), rng.randn(12, 12, 2), 1.0, cls.Options({'Y0': Y0, 'U0': 0 * Y0}), dimK=1)
    assert rel_l2(c.Y, Y0) == 0.0 and np.all(c.U == 0.0)


@pytest.mark.parametrize('name', ['ball_fixed_f64', 'ball_mcd_f64'])
def test_setdict_mid_run(backend, name):
    """setdict after 10 iterations, 10 more: equal to a fresh solver with the new dictionary,
    warm-started from the first one's blocks through Y0 / U0."""
    g = load_golden(name)
    rng = np.random.RandomState(3)
    D2 = rng.randn(*g['D'].shape)
    a = build(g, extra={'MaxMainIter': 10})
    a.solve()
    Y, U, rho = a.Y.copy(), a.U.copy(), float(a.rho)
    a.setdict(D2.reshape(a.cri.shpD))
    a.solve()
    c = build(g, D=D2, extra={'MaxMainIter': 10, 'Y0': Y, 'U0': U, 'rho': rho})
    c.solve()
    for v in ('X', 'Y', 'U'):
        assert rel_l2(getattr(a, v), getattr(c, v)) < 1e-12, v
    ia, ic = a.getitstat(), c.getitstat()
    for f in ('ObjFun', 'Cnstr', 'PrimalRsdl', 'DualRsdl'):
        assert rel_l2(np.array(getattr(ia, f))[10:], getattr(ic, f)) < 1e-12, f
    assert rel_l2(a.reconstruct(), c.reconstruct()) < 1e-12


@pytest.mark.parametrize('name', ['ball_default_f64', 'ball_mcd_f64'])
def test_linsolvecheck(backend, name):
    g = load_golden(name)
    b = build(g, np.float64, extra={'LinSolveCheck': True})
    b.solve()
    x = np.array(b.getitstat().XSlvRelRes, dtype=np.float64)
    print('XSlvRelRes max', x.max())
    assert np.all(np.isfinite(x)) and x.max() < 1e-5
    check(b, g, 1e-9, 1e-9)


def test_returnvar_and_blocks(backend):
    g = load_golden('ball_mcs_f64')
    for rv, want in (('X', 'X'), ('Y0', 'Y0'), ('Y1', 'Y1')):
        b = build(g, extra={'ReturnVar': rv, 'HighMemSolve': True})
        out = b.solve()
        assert rel_l2(out, g[want]) < 1e-9 and out.shape == g[want].shape
    # every plane of y0 lies in its ball
    d = np.sqrt(np.sum(b.var_y0() ** 2, axis=(0, 1)))
    assert np.all(d <= float(g['epsilon']) * (1 + 1e-12))


def test_two_runs_agree_bit_for_bit(backend):
    g = load_golden('ball_mcs_f64')
    a, b = build(g, np.float32), build(g, np.float32)
    a.solve()
    b.solve()
    assert np.array_equal(a.Y, b.Y) and np.array_equal(a.U, b.U)
    for f in TRACES + ('Cnstr',):
        assert np.array_equal(getattr(a.getitstat(), f), getattr(b.getitstat(), f)), f


# ---- 6. the reference's test_22 as a property -----------------------------------------------------------
def test_recovers_the_bpdn_solution(backend):
    """ConvBPDN solved to RelStopTol 1e-5, epsilon set to its residual norm: ConvMinL1InL2Ball with rho 200,
    RelaxParam 1 and AutoRho off recovers X within 1e-3 relative and the l1 norm within 1e-3 absolute
    (the reference's tests/admm/test_cbpdn.py:410-436, its own bounds)."""
    from sporco_amd.admm import cbpdn
    rng = np.random.RandomState(22)
    N, M, Nd = 32, 4, 8
    D = rng.randn(Nd, Nd, M)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1)))
    X0 = np.zeros((N, N, M))
    xp = np.abs(rng.randn(N, N, M)) > 3
    X0[xp] = rng.randn(int(xp.sum()))
    S = np.sum(np.fft.irfft2(np.fft.rfft2(D, s=(N, N), axes=(0, 1)) * np.fft.rfft2(X0, axes=(0, 1)), s=(N, N),
                             axes=(0, 1)), axis=2)
    opt = cbpdn.ConvBPDN.Options({'Verbose': False, 'MaxMainIter': 500, 'RelStopTol': 1e-5, 'rho': 5e-1,
                                  'AutoRho': {'Enabled': False}})
    bp = cbpdn.ConvBPDN(D, S, 1e-3, opt)
    Xp = bp.solve()
    epsilon = np.linalg.norm(bp.reconstruct(Xp).squeeze() - S)
    opt = cbpdn.ConvMinL1InL2Ball.Options({'Verbose': False, 'MaxMainIter': 500, 'RelStopTol': 1e-5, 'rho': 2e2,
                                           'RelaxParam': 1.0, 'AutoRho': {'Enabled': False}})
    bc = cbpdn.ConvMinL1InL2Ball(D, S, epsilon, opt)
    Xc = bc.solve()
    ex = np.linalg.norm(Xp - Xc) / np.linalg.norm(Xp)
    el = abs(np.linalg.norm(Xp.ravel(), 1) - np.linalg.norm(Xc.ravel(), 1))
    print('epsilon', epsilon, 'iterations', len(bp.getitstat().ObjFun), len(bc.getitstat().ObjFun), 'X', ex, 'l1', el)
    assert ex < 1e-3
    assert el < 1e-3


# ---- 7. the register-resident kernels against the generic chain -----------------------------------------
FUSED_SCALES = (0.2, 1.0, 0.6)


@pytest.mark.parametrize('H,K,N', [(128, 8, 3), pytest.param(512, 64, 2, marks=pytest.mark.gpu)])
def test_fused_iteration_vs_generic_chain(backend, H, K, N, monkeypatch):
    """On the fast-path shapes (float32, 128 / 256 / 512, even K <= 64) the x step, block 1 and the dual
    residual run on the register-resident kernels, block 0 on ball_norms / ball_y0step either way: same
    iterates and statistics as the generic chain, and (128 x 128) as the float64 restatement."""
    from sporco_amd.admm import cbpdn
    rng = np.random.RandomState(11)
    D = rng.randn(8, 8, K).astype(np.float32)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = (rng.randn(H, H, N) * np.asarray(FUSED_SCALES[:N])).astype(np.float32)
    eps = 0.5 * H / 16 * 4.0         # (between the images' norms, 0.2 H and H, 0.6 H: both branches)
    cls = cbpdn.ConvMinL1InL2Ball
    optd = {'MaxMainIter': 5, 'RelStopTol': 0.0, 'AutoRho': {'Period': 2}}

    def run(generic):
        if generic:
            monkeypatch.setenv('SPORCO_AMD_MD_GENERIC', '1')
        else:
            monkeypatch.delenv('SPORCO_AMD_MD_GENERIC', raising=False)
        b = cls(D, S, eps, cls.Options(optd), dimK=1)
        b._dev.profile(True)
        Y1 = b.solve()
        prof = {k for k, v in b._dev.profile_read().items() if v[1]}
        return b, Y1, prof

    bf, Yf, pf = run(False)
    bg, Yg, pg = run(True)
    assert {'rows_fwd', 'fused_cols_sm', 'rows_inv_post', 'ball_norms', 'ball_y0step'} <= pf and 'sm_solve' not in pf
    assert {'sm_solve', 'ball_norms', 'ball_y0step'} <= pg and not ({'rows_fwd', 'fused_cols_sm', 'rows_inv_post'} & pg)
    assert rel_l2(Yf, Yg) < 1e-4 and rel_l2(bf.X, bg.X) < 1e-4 and rel_l2(bf.U, bg.U) < 1e-4
    assert rel_l2(bf.var_y0(), bg.var_y0()) < 1e-3
    assert rel_l2(bf.reconstruct(), bg.reconstruct()) < 1e-4
    for f in TRACES:
        assert rel_l2(getattr(bf.getitstat(), f), getattr(bg.getitstat(), f)) < 1e-4, f
    assert np.max(np.abs(np.array(bf.getitstat().Cnstr) - bg.getitstat().Cnstr)) <= 1e-4 * eps
    if H <= 128:
        D5, S5 = five(D.astype(np.float64), S.astype(np.float64))
        r = bn.admm_ball(D5, S5, eps, 5, ar=dict(bn.AUTORHO_DEFAULT, Period=2))
        assert np.any(r['active']) and not np.all(r['active'])
        compare_f32(bf, r, eps)


def compare_f32(b, r, eps):
    """A float32 run against the float64 restatement: X, Y 1e-4, traces 1e-3, with the measured
    exceptions."""
    its = b.getitstat()
    figs = {'X': rel_l2(b.X, r['X']), 'Y': rel_l2(b.Y, r['Y'])}
    trs = {f: rel_l2(getattr(its, f), r[f]) for f in TRACES}
    dual = np.max(np.abs(np.asarray(its.DualRsdl) - r['DualRsdl']) / np.abs(r['DualRsdl']))
    cn = np.max(np.abs(np.asarray(its.Cnstr) - r['Cnstr'])) / eps
    print(figs, trs, 'DualRsdl worst entry', dual, 'Cnstr worst |delta| / eps', cn)
    for v, e in figs.items():
        assert e < 1e-4, (v, e)
    for f, e in trs.items():
        assert e < 1e-3, (f, e)
    assert dual < F32_DUAL_TOL and cn <= F32_CNSTR_TOL


# ---- 8. GPU-only sizes: the smallest at which the plane-interleaved reduction can still go wrong -------------
#   inner = 1 (odd K, a single plane); inner = 6 (divides neither a wave nor a workgroup); inner = 300 (more
#   planes than a workgroup has threads); block 0 beyond one capped grid of 4096 x 256 threads.
GPU_SHAPES = {
    'inner1': ((64, 80), 7, 'single'),
    'inner6': ((32, 48, 3, 2), 4, 'mcs'),
    'inner300': ((16, 16, 300), 2, 'alt'),
    'capped_grid': ((256, 264, 17), 2, 'alt'),
}
_GPU_CACHE = {}


def gpu_problem(name):
    """Inputs and the float64 restatement of 10 iterations, computed once per module."""
    if name not in _GPU_CACHE:
        sshape, K, kind = GPU_SHAPES[name]
        rng = np.random.RandomState(31)
        D = rng.randn(5, 5, K)
        D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
        S = rng.randn(*sshape)
        big = np.sqrt(sshape[0] * sshape[1])          # (the norm of a unit-variance image)
        if kind == 'single':
            eps, dimK = 0.9 * big, 0          # (outside the ball at first, inside once x explains the image)
        else:
            S = S * np.where(np.arange(sshape[-1]) % 2 == 0, 0.2, 1.0)
            eps, dimK = 0.25 * big, 1
        D5, S5 = five(D, S, dimK)
        r = bn.admm_ball(D5, S5, eps, 10)
        _GPU_CACHE[name] = (D, S, eps, dimK, r)
    return _GPU_CACHE[name]


@pytest.mark.gpu
@pytest.mark.parametrize('name', sorted(GPU_SHAPES))
def test_gpu_sizes(gpu_backend, name):
    from sporco_amd.admm import cbpdn
    D, S, eps, dimK, r = gpu_problem(name)
    if name == 'capped_grid':
        assert S.size > 4096 * 256
    act = r['active']
    assert np.any(act) and not np.all(act), name        # (both branches of the projection occur)
    cls = cbpdn.ConvMinL1InL2Ball
    b = cls(D.astype(np.float32), S.astype(np.float32), eps, cls.Options({'MaxMainIter': 10, 'RelStopTol': 0.0}),
            dimK=dimK)
    b.solve()
    compare_f32(b, r, eps)
