"""What tests/test_tvl2dcn.py and tests/test_tvl1dcn.py share: the two classes differ in their block count, their
fixtures and a few options, not in what is checked.  ``kind`` is 'l2' or 'l1' throughout."""

import pickle

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _tvdcn_numpy as tn

from sporco_amd import _lib
from sporco_amd.admm import tvl1, tvl2
from sporco_amd.device import DeviceArray

CLS = {'l2': tvl2.TVL2Deconv, 'l1': tvl1.TVL1Deconv}
NBLK = {'l2': 2, 'l1': 3}
PLAN = {'l2': tvl2.plan_deconv, 'l1': tvl1.plan_deconv}
LMBDA = {'l2': 0.05, 'l1': 0.8}
# (the reference cannot build TVL1Deconv with a kernel per plane: tools/make_golden_tvdcn.py)
CASES = {'l2': ['default', 'autorho', 'tvw', 'vec', 'stdres', 'relax1', 'lsc', 'y0warm', 'y0u0', 'aplanes', 'impulse'],
         'l1': ['default', 'autorho', 'tvw', 'vec', 'stdres', 'relax1', 'lsc', 'y0warm', 'y0u0', 'impulse', 'mask']}
TRACES = ('ObjFun', 'DFid', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho')
F64_TOL = 1e-9
XRRS_ABS = 1e-12

_GOLD = {}


def gold(kind, case):
    key = 'tv%sdcn_%s_f64' % (kind, case)
    if key not in _GOLD:
        _GOLD[key] = load_golden(key)
    return _GOLD[key]


def autorho_of(g):
    return {'Enabled': bool(g['opt_AutoRho']), 'Period': int(g['opt_AutoRho_Period']),
            'Scaling': float(g['opt_AutoRho_Scaling']), 'RsdlRatio': float(g['opt_AutoRho_RsdlRatio']),
            'AutoScaling': bool(g['opt_AutoRho_AutoScaling']), 'RsdlTarget': float(g['opt_AutoRho_RsdlTarget']),
            'StdResiduals': bool(g['opt_StdResiduals'])}


def caxis_of(g):
    return None if 'caxis' not in g or int(g['caxis']) < 0 else int(g['caxis'])


def options_of(kind, g, dtype, extra=None):
    o = {'Verbose': False, 'MaxMainIter': int(g['MaxMainIter']) if 'MaxMainIter' in g else 1, 'RelStopTol': 0.0,
         'rho': float(g['opt_rho']) if 'opt_rho' in g else float(g['rho_before']),
         'RelaxParam': float(g['opt_RelaxParam']), 'gEvalY': bool(g['opt_gEvalY']),
         'LinSolveCheck': bool(g['opt_LinSolveCheck']), 'AutoRho': autorho_of(g)}
    for key in ('DFidWeight', 'TVWeight', 'Y0', 'U0'):
        if 'optarr_' + key in g:
            o[key] = g['optarr_' + key].astype(dtype)
    o.update(extra or {})
    return CLS[kind].Options(o)


def tolerances(dtype, f32_tols):
    return (F64_TOL, F64_TOL) if dtype == np.float64 else f32_tols


def compare(b, X, g, dtype, case, f32_tols):
    its = b.getitstat()
    tol_i, tol_t = tolerances(dtype, f32_tols)
    errs = {'X': rel_l2(X, g['X']), 'Y': rel_l2(b.Y, g['Y']), 'U': rel_l2(b.U, g['U'])}
    terr = {f: rel_l2(getattr(its, f), g['it_' + f]) for f in TRACES}
    terr['rho'] = abs(float(b.rho) - float(g['rho_final'])) / float(g['rho_final'])
    print('%s %s: iterates %s traces %s' % (case, np.dtype(dtype).name,
                                           {k: '%.2e' % v for k, v in errs.items()},
                                           {k: '%.2e' % v for k, v in terr.items()}))
    assert X.dtype == dtype and b.Y.dtype == dtype and b.Y.shape == g['Y'].shape
    assert max(errs.values()) <= tol_i, errs
    assert max(terr.values()) <= tol_t, terr
    assert np.array_equal(its.Iter, np.arange(len(g['it_ObjFun'])))
    if 'it_XSlvRelRes' in g:
        # (it sits at 1e-16 in float64 and at 1e-8 in float32: an absolute comparison)
        xr = np.asarray(its.XSlvRelRes, dtype=np.float64)
        print('XSlvRelRes: max %.2e (fixture %.2e)' % (xr.max(), g['it_XSlvRelRes'].max()))
        assert np.max(np.abs(xr - g['it_XSlvRelRes'])) <= (XRRS_ABS if dtype == np.float64 else 1e-5)
    else:
        assert all(v is None for v in its.XSlvRelRes)


def check_fixture(kind, case, dtype, f32_tols):
    g = gold(kind, case)
    b = CLS[kind](g['A'].astype(dtype), g['S'].astype(dtype), float(g['lmbda']), options_of(kind, g, dtype),
                  caxis=caxis_of(g))
    X = b.solve()
    compare(b, X, g, dtype, case, f32_tols)


def check_fixture_conditions(kind):
    """What the generator asserted, read back."""
    for case in CASES[kind]:
        g = gold(kind, case)
        assert 0.1 <= float(g['zero_share']) <= 0.9, case
        if kind == 'l1':
            assert 0.1 <= float(g['zero_share_data']) <= 0.9, case
        assert float(g['lmbda']) == LMBDA[kind]
        assert g['S'].shape[:2] == (16, 17) and len(g['it_ObjFun']) == 40
        if int(g['opt_AutoRho']):
            assert len(set(g['it_Rho'])) > 2, case
    assert int(gold(kind, 'autorho')['opt_AutoRho']) and int(gold(kind, 'vec')['opt_AutoRho'])
    if kind == 'l2':
        assert int(gold(kind, 'default')['opt_AutoRho'])
    else:
        w = gold(kind, 'mask')['optarr_DFidWeight']
        assert np.all(w[3] == 0) and np.all(w[:, 5] == 0) and np.sum(w == 0) == 16 + 17 - 1
    assert gold(kind, 'impulse')['A'].shape == (1, 1) and gold(kind, 'default')['A'].shape == (5, 4)


def measured_figures(kind):
    """The NumPy statement in float64 reproduces every fixture; in float32 its worst errors are returned."""
    wi = wt = 0.0
    for case in CASES[kind]:
        g = gold(kind, case)
        o64 = tn.from_golden(kind, g)
        for k in ('X', 'Y', 'U'):
            assert rel_l2(o64[k], g[k]) <= F64_TOL, (case, k)
        for f in TRACES:
            assert rel_l2(o64[f], g['it_' + f]) <= F64_TOL, (case, f)
        if 'it_XSlvRelRes' in g:
            assert np.max(np.abs(o64['XSlvRelRes'] - g['it_XSlvRelRes'])) <= XRRS_ABS
        assert abs(o64['rho'] - float(g['rho_final'])) <= F64_TOL * float(g['rho_final'])
        o = tn.from_golden(kind, g, dtype=np.float32)
        ei = max(rel_l2(o[k], g[k]) for k in ('X', 'Y', 'U'))
        et = max(max(rel_l2(o[f], g['it_' + f]) for f in TRACES),
                 abs(o['rho'] - float(g['rho_final'])) / float(g['rho_final']))
        print('%-8s float32 statement: iterates %.2e traces %.2e' % (case, ei, et))
        wi, wt = max(wi, ei), max(wt, et)
    print('worst: iterates %.3e traces %.3e' % (wi, wt))
    return wi, wt


def check_one_step(kind, dtype, f32_tols):
    g = load_golden('tv%sdcn_step_f64' % kind)
    opt = options_of(kind, g, dtype, {'Y0': g['Y_before'].astype(dtype), 'U0': g['U_before'].astype(dtype),
                                      'MaxMainIter': 1})
    b = CLS[kind](g['A'].astype(dtype), g['S'].astype(dtype), float(g['lmbda']), opt)
    X = b.solve()
    ti, tt = tolerances(dtype, f32_tols)
    assert rel_l2(X, g['X']) <= ti and rel_l2(b.Y, g['Y']) <= ti
    # (the recorded run changed rho at the end of its iteration 40, a fresh object does not in its first:
    # rho U is what both agree on)
    assert rel_l2(b.U.astype(np.float64) * float(b.rho), g['U'] * float(g['rho_final'])) <= ti
    its = b.getitstat()
    for f in ('ObjFun', 'DFid', 'RegTV', 'PrimalRsdl', 'DualRsdl'):
        assert abs(getattr(its, f)[-1] - float(g['last_' + f])) <= tt * abs(float(g['last_' + f])), f


# ---- against the NumPy statement at shapes chosen from the kernels' plan ------------------------------------
_PROBLEMS = {}
AR = {'Enabled': True, 'Period': 1, 'Scaling': 1000.0, 'RsdlRatio': 1.2, 'AutoScaling': True, 'RsdlTarget': 1.0}


def problem(kind, shape, aplanes=False, seed=3):
    key = (kind, tuple(shape), aplanes, seed)
    if key not in _PROBLEMS:
        rng = np.random.RandomState(seed)
        H, W = shape[:2]
        img = np.ones((H, W))
        img[:, W // 2:] = -1.0
        img[H // 3:] *= 0.5
        A = rng.rand(*((min(3, H), min(2, W)) + (tuple(shape[2:]) if aplanes else ())))
        A /= np.sum(A, axis=(0, 1), keepdims=True)
        S = img.reshape((H, W) + (1,) * (len(shape) - 2)) + 0.3 * rng.randn(*shape)
        if kind == 'l1':
            S = np.where(rng.rand(*shape) < 0.2, rng.uniform(-1.5, 1.5, shape), S)
        _PROBLEMS[key] = (A, np.ascontiguousarray(S))
    return _PROBLEMS[key]


def check_edge(kind, shape, caxis=None, aplanes=False, dtype=np.float64, f32_tols=None, expect=None):
    """5 iterations with AutoRho against the statement in float64; ``expect``: plan entries the shape was
    chosen for."""
    A, S = problem(kind, shape, aplanes)
    pl = PLAN[kind](shape, dtype, caxis)
    print(shape, caxis, pl)
    for k, v in (expect or {}).items():
        assert pl[k] == v, (k, pl)
    lmbda = 0.2 if kind == 'l2' else 0.8
    # (a start far from balance, so that AutoRho moves rho at every shape within five iterations)
    o = {'Verbose': False, 'MaxMainIter': 5, 'RelStopTol': 0.0, 'AutoRho': {'Enabled': True}, 'LinSolveCheck': True,
         'rho': 20.0}
    b = CLS[kind](A.astype(dtype), S.astype(dtype), lmbda, CLS[kind].Options(o), caxis=caxis)
    X = b.solve()
    ref = tn.tv_deconv(kind, A, S, lmbda, 5, rho=20.0, caxis=caxis, ar=AR, lin_solve_check=True)
    ti, tt = tolerances(dtype, f32_tols)
    its = b.getitstat()
    errs = {'X': rel_l2(X, ref['X']), 'Y': rel_l2(b.Y, ref['Y']), 'U': rel_l2(b.U, ref['U'])}
    terr = {f: rel_l2(getattr(its, f), ref[f]) for f in TRACES}
    print({k: '%.2e' % v for k, v in errs.items()}, {k: '%.2e' % v for k, v in terr.items()})
    assert len(set(ref['Rho'])) > 2      # (AutoRho moved rho: the pending rescale of U is exercised)
    assert max(errs.values()) <= ti, errs
    assert max(terr.values()) <= tt, terr
    assert max(its.XSlvRelRes) <= (1e-12 if dtype == np.float64 else 1e-5)


def edge_shapes(kind):
    """(shape, caxis, aplanes, expected plan entries): chosen from the plan of the float64 kernels.  A strip is
    256 items, a segment at least 8 rows; with one plane and an item of one element a strip covers TW = 256
    columns."""
    pl = PLAN[kind]((8, 300), np.float64)
    TW, R = pl['TW'], pl['R']
    assert (pl['V'], TW, R) == (1, 256, 8)
    out = []
    for H in (2, R, R + 1):
        for W, strips in ((TW - 1, 1), (TW, 1), (TW + 1, 2), (2 * TW + 1, 3)):
            # (an even row of at least 512 elements is taken two at a time: W = 256 then has one strip of 128 items)
            out.append(((H, W), None, False, {'strips': strips, 'nseg': 2 if H > R else 1, 'V': 1}))
    out += [((9, 86, 3), None, False, {'V': 1, 'strips': 2}),        # W P = 258
            ((9, 171, 3), None, False, {'V': 1, 'strips': 3}),       # W P = 513: odd
            ((5, 52, 5), None, False, {'V': 1, 'strips': 2}),        # W P = 260
            ((9, 86, 3), None, True, {'V': 1}),                      # a kernel per plane
            ((4, 512), None, False, {'V': 2, 'strips': 1}),          # 16-byte accesses in float64, P = 1
            ((4, 300, 2), None, False, {'V': 2, 'strips': 2}),       # ... and P = 2
            ((9, 10, 3, 2), 2, False, {'V': 3}),                     # vector TV: 3 channels x 2 images
            ((6, 7, 5), 2, False, {'V': 5}),                         # ... 5 channels
            ((7, 6, 3, 2), 2, True, {'V': 3}),
            ((2, 2), None, False, {'V': 1, 'strips': 1, 'nseg': 1})]
    return out


# ---- contract -------------------------------------------------------------------------------------------------
def small(kind, dtype=np.float64, trail=()):
    A, S = problem(kind, (12, 13) + trail)
    return A.astype(dtype), S.astype(dtype)


def base_opts(**kw):
    o = {'Verbose': False, 'MaxMainIter': 12, 'RelStopTol': 0.0, 'AutoRho': {'Enabled': True}}
    o.update(kw)
    return o


def check_bitwise_repeatable(kind, dtype):
    A, S = small(kind, dtype, (3,))
    runs = []
    for _ in range(2):
        b = CLS[kind](A, S, LMBDA[kind], CLS[kind].Options(base_opts()))
        X = b.solve()
        runs.append((X, b.Y, b.U, np.asarray(b.getitstat().ObjFun), np.asarray(b.getitstat().DualRsdl)))
    for u, v in zip(*runs):
        assert np.array_equal(u, v)


def check_solve_twice(kind):
    A, S = small(kind)
    c = CLS[kind]
    b1 = c(A, S, LMBDA[kind], c.Options(base_opts(MaxMainIter=6)))
    b1.solve()
    assert b1.k == 6
    X1 = b1.solve()
    b2 = c(A, S, LMBDA[kind], c.Options(base_opts(MaxMainIter=12)))
    X2 = b2.solve()
    assert b1.k == 12 and len(b1.itstat) == 12
    assert np.array_equal(X1, X2) and np.array_equal(b1.U, b2.U)
    assert np.array_equal(b1.getitstat().ObjFun, b2.getitstat().ObjFun)


def check_callback_and_fastsolve(kind):
    A, S = small(kind)
    c = CLS[kind]
    b = c(A, S, LMBDA[kind], c.Options(base_opts(Callback=lambda o: o.k == 3)))
    b.solve()
    assert len(b.itstat) == 4
    ref = c(A, S, LMBDA[kind], c.Options(base_opts()))
    Xr = ref.solve()
    # FastSolve: no statistics; with AutoRho the residuals are still formed, so the iterates are the same
    f = c(A, S, LMBDA[kind], c.Options(base_opts(FastSolve=True)))
    Xf = f.solve()
    assert f.itstat == [] and np.array_equal(Xf, Xr)
    # ... and without AutoRho no residual is formed at all
    r0 = c(A, S, LMBDA[kind], c.Options(base_opts(AutoRho={'Enabled': False})))
    f0 = c(A, S, LMBDA[kind], c.Options(base_opts(AutoRho={'Enabled': False}, FastSolve=True)))
    assert np.array_equal(r0.solve(), f0.solve()) and f0.itstat == []


def check_surface(kind):
    c = CLS[kind]
    A, S = small(kind, np.float64, (3,))
    opt = c.Options()
    assert opt['RelaxParam'] == 1.8 and opt['gEvalY'] is True and opt['LinSolveCheck'] is False
    ar = opt['AutoRho']
    assert (ar['Period'], ar['AutoScaling'], ar['Scaling'], ar['RsdlRatio'], ar['RsdlTarget']) == (1, True, 1000.0, 1.2, 1.0)
    assert ar['Enabled'] is (kind == 'l2')
    assert ('DFidWeight' in c.Options.defaults) is (kind == 'l1')
    for key in ('MaxGSIter', 'GSTol'):
        assert key not in c.Options.defaults
    assert c.IterationStats._fields == ('Iter', 'ObjFun', 'DFid', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal',
                                        'EpsDual', 'Rho', 'XSlvRelRes', 'Time')
    lm = LMBDA[kind]
    b = c(A, S, lm, c.Options({'Verbose': False, 'MaxMainIter': 3}))
    assert abs(float(b.rho) - (2 * lm + 0.1)) < 1e-12 and b.rho.dtype == np.float64
    X = b.solve()
    nb = NBLK[kind]
    assert X.shape == S.shape and b.Y.shape == S.shape + (nb,) and b.U.shape == S.shape + (nb,)
    assert b.getmin() is not None and np.array_equal(b.getmin(), X) and b.itstat[-1].XSlvRelRes is None
    assert b.timer.elapsed('solve') > 0 and b.A.shape == A.shape + (1,) and b.lmbda == lm and b.Wtv.shape == ()
    Hh, Ww = S.shape[:2]
    Wf = Ww // 2 + 1
    assert b.Af.shape == (Hh, Wf, 1) and b.Sf.shape == (Hh, Wf, 3) and b.Xf.shape == (Hh, Wf, 3)
    assert b.Gf.shape == (Hh, Wf, 1, 2) and b.GHGf.shape == (Hh, Wf, 1)
    assert rel_l2(b.AHAf, np.abs(b.Af) ** 2) < 1e-12 and rel_l2(b.AHSf, np.conj(b.Af) * b.Sf) < 1e-12
    kk, ll = np.arange(Hh)[:, None, None], np.arange(Wf)[None, :, None]
    assert rel_l2(b.GHGf, (2 - 2 * np.cos(2 * np.pi * kk / Hh)) + (2 - 2 * np.cos(2 * np.pi * ll / Ww))) < 1e-12
    assert rel_l2(np.fft.irfftn(b.Xf, s=(Hh, Ww), axes=(0, 1)), X) < 1e-12
    if kind == 'l1':
        assert b.GAf.shape == (Hh, Wf, 1, 3) and b.Wdf.shape == ()
    # the constraint on host arrays: A^T is the exact transpose of A, c and B as the reference has them
    rng = np.random.RandomState(5)
    x, v = rng.randn(*S.shape), rng.randn(*(S.shape + (nb,)))
    assert abs(np.sum(b.cnst_A(x) * v) - np.sum(x * b.cnst_AT(v))) <= 1e-10
    assert np.array_equal(b.cnst_B(v), -v) and b.cnst_c().shape == S.shape + (nb,)
    assert np.array_equal(b.cnst_c()[..., -1], S if kind == 'l1' else np.zeros_like(S))
    assert rel_l2(b.cnst_A(x)[..., 0], x - np.roll(x, 1, axis=0)) < 1e-15      # circular, unlike Denoise
    # the 1-D and (1, 1) impulse kernels of the reference's tests and *_den examples
    for imp in (np.ones((1)), np.ones((1, 1))):
        bi = c(imp, S, lm, c.Options({'Verbose': False, 'MaxMainIter': 2}))
        bi.solve()
        assert rel_l2(bi.Af, np.ones_like(bi.Af)) < 1e-15
    # weights
    wt = 0.5 + rng.rand(*S.shape)
    bw = c(A, S, lm, c.Options({'Verbose': False, 'MaxMainIter': 2, 'TVWeight': wt}))
    bw.solve()
    assert bw.Wtv.shape == S.shape


def check_refusals(kind):
    c = CLS[kind]
    A, S = small(kind)
    lm = LMBDA[kind]
    S3 = np.stack([S] * 3, axis=-1)
    with pytest.raises(NotImplementedError):
        c(A, S + 0j, lm)
    with pytest.raises(NotImplementedError):
        c(A + 0j, S, lm)
    with pytest.raises(NotImplementedError):
        c(A, S3, lm, axes=(0, 1, 2))
    with pytest.raises(NotImplementedError):
        c(A, S3, lm, caxis=1)
    with pytest.raises(NotImplementedError):
        c(A, S, lm, caxis=2)
    with pytest.raises(NotImplementedError):
        c(A, np.zeros((6, 6, 9)), lm, caxis=2)
    with pytest.raises(NotImplementedError):
        c(A, np.zeros((6, 6, 2, 2, 2)), lm)
    with pytest.raises(NotImplementedError):
        c(np.ones((1, 1)), np.zeros((1, 8)), lm)
    with pytest.raises(NotImplementedError):
        c(np.ones((1, 1)), np.zeros((8, 1)), lm)
    with pytest.raises(NotImplementedError):
        c(A, S3, lm, c.Options({'TVWeight': np.ones(S3.shape)}), caxis=2)
    with pytest.raises(NotImplementedError):
        c(np.ones((S.shape[0] + 1, 2)), S, lm)
    with pytest.raises(NotImplementedError):
        c(np.ones((2, 2, 3, 1)), np.zeros((6, 6, 3, 2)), lm)
    with pytest.raises(NotImplementedError):
        c(np.ones((2, 2, 2)), S3, lm)
    with pytest.raises(TypeError):
        c(A, S.astype(np.float16), lm)
    with pytest.raises(TypeError):
        c(A, S.astype(np.int32), lm)
    with pytest.raises(NotImplementedError):
        c(A, S, lm, reducer=object())
    with pytest.raises(NotImplementedError):
        pickle.dumps(c(A, S, lm))


def check_device_input(kind):
    g = gold(kind, 'mask' if kind == 'l1' else 'default')
    A, img, lmbda = g['A'].astype(np.float32), g['S'].astype(np.float32), float(g['lmbda'])
    c = CLS[kind]
    o = {'Verbose': False, 'MaxMainIter': 40, 'gEvalY': False, 'AutoRho': {'Enabled': True}}
    msk = g['optarr_DFidWeight'].astype(np.float32) if kind == 'l1' else None
    bh = c(A, img, lmbda, c.Options(dict(o, DFidWeight=msk) if kind == 'l1' else o))
    slh = bh.solve()

    imgd, Ad = DeviceArray.from_host(img), DeviceArray.from_host(A)
    mskd = DeviceArray.from_host(msk) if kind == 'l1' else None
    _lib.transfer_stats(reset=True)
    b = c(Ad, imgd, lmbda, c.Options(dict(o, DFidWeight=mskd) if kind == 'l1' else o))
    sl = b.solve()
    st = _lib.transfer_stats()
    assert st['h2d_bytes'] == 0 and st['d2h_bytes'] <= 40 * _lib.OUT_COUNT * 8     # (the sums only, one read each)
    assert isinstance(sl, DeviceArray) and isinstance(b.getmin(), DeviceArray)
    assert np.array_equal(sl.get(), slh)
    assert np.array_equal(b.getitstat().ObjFun, bh.getitstat().ObjFun)
    assert np.array_equal(b.getitstat().PrimalRsdl, bh.getitstat().PrimalRsdl)


def check_four_classes_alive():
    """A TVL2Denoise, a TVL1Denoise, a TVL2Deconv and a TVL1Deconv alive in one process, stepped in turn, each
    still give their own fixture."""
    g = {'d2': load_golden('tvl2_default_f64'), 'd1': load_golden('tvl1_default_f64'),
         'c2': gold('l2', 'default'), 'c1': gold('l1', 'default')}

    def den_opts(cls, gg):
        return cls.Options({'Verbose': False, 'MaxMainIter': 10, 'RelStopTol': 0.0, 'rho': float(gg['opt_rho']),
                            'RelaxParam': float(gg['opt_RelaxParam']), 'gEvalY': bool(gg['opt_gEvalY']),
                            'MaxGSIter': int(gg['opt_MaxGSIter']), 'GSTol': float(gg['opt_GSTol']),
                            'AutoRho': autorho_of(gg)})
    objs = {'d2': tvl2.TVL2Denoise(g['d2']['S'], float(g['d2']['lmbda']), den_opts(tvl2.TVL2Denoise, g['d2'])),
            'd1': tvl1.TVL1Denoise(g['d1']['S'], float(g['d1']['lmbda']), den_opts(tvl1.TVL1Denoise, g['d1'])),
            'c2': tvl2.TVL2Deconv(g['c2']['A'], g['c2']['S'], float(g['c2']['lmbda']),
                                  options_of('l2', g['c2'], np.float64, {'MaxMainIter': 10})),
            'c1': tvl1.TVL1Deconv(g['c1']['A'], g['c1']['S'], float(g['c1']['lmbda']),
                                  options_of('l1', g['c1'], np.float64, {'MaxMainIter': 10}))}
    for _ in range(4):
        for b in objs.values():
            b.solve()
    for key, b in objs.items():
        assert rel_l2(b.X, g[key]['X']) <= F64_TOL and rel_l2(b.U, g[key]['U']) <= F64_TOL, key
        assert rel_l2(b.getitstat().ObjFun, g[key]['it_ObjFun']) <= F64_TOL, key


def check_recovery(kind):
    g = load_golden('tv%sdcn_recovery_f64' % kind)
    c = CLS[kind]
    o = {'Verbose': False, 'gEvalY': False, 'MaxMainIter': int(g['MaxMainIter'])}
    if np.isfinite(float(g['opt_rho'])):
        o['rho'] = float(g['opt_rho'])
    b = c(g['A'], g['D'], float(g['lmbda']), c.Options(o))
    X = b.solve()
    print('ObjFun %.12f after %d iterations (reference %.12f after %d)'
          % (b.itstat[-1].ObjFun, len(b.itstat), float(g['ObjFun']), int(g['iterations'])))
    assert abs(b.itstat[-1].ObjFun - float(g['ObjFun'])) < float(g['bound'])
    assert np.mean((g['U'] - X) ** 2) < float(g['mse_bound'])
