"""sporco_amd.admm.tvl1.TVL1Denoise against fixtures of the unmodified reference (tests/golden/tvl1_*_f64.npz,
tools/make_golden_tvl1.py) and against the NumPy statement of tests/_tvl1_numpy.py.

Tolerances.  float64: the project's 1e-9 relative l2 on iterates and traces, GSIter exactly.  float32 input
against the float64 fixture: the project's 1e-4 on iterates and 1e-3 on traces, or four times what the NumPy
statement run in float32 shows against the same fixtures, whichever is larger (the margin of four covers the
summation order: NumPy's pairwise sums against the kernel's per-workgroup partials).

Measured (test_f32_measured_figures repeats the measurement on the CPU), worst case over the fixtures of the
NumPy statement in float32 against the float64 fixture:
  iterates X, Y, U, relative l2:   2.69e-6 (`autorho`; `mask` 1.3e-6, `gstol` 1.3e-6, `vec` 1.2e-6, every other
                                   case <= 7.3e-7)
  traces and the final rho:        2.80e-6 (`gstol`; `autorho` 2.6e-6, `mask` 1.3e-6, `vec` 1.1e-6, every other
                                   case <= 3.4e-7)
Four times either lies far below the project's 1e-4 / 1e-3, which therefore apply unchanged.
`gstol` in float32: GSIter is compared only at iterations where the fixture's GSRelRes after some sweep is
not within the float32 margin F32_TRACE_TOL (relative) of GSTol -- there a float32 run may legitimately
stop one sweep earlier or later; such iterations, and every later one (the iterates have then taken another
path), are left out of the GSIter comparison, and at most a quarter of the iterations may be.  With
GSTol = 3e-2 the fixture leaves out none.
"""

import pickle

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _tvl1_numpy as tn

from sporco_amd import _lib
from sporco_amd.admm import tvl1, tvl2
from sporco_amd.device import DeviceArray

CASES = ['default', 'autorho', 'mask', 'tvw', 'vec', 'stdres', 'relax1', 'gstol', 'y0warm', 'y0u0']
TRACES = ('ObjFun', 'DFid', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho', 'GSRelRes')

F32_ITER_MEASURED = 2.7e-6
F32_TRACE_MEASURED = 2.9e-6
F32_ITER_TOL = max(4.0 * F32_ITER_MEASURED, 1e-4)
F32_TRACE_TOL = max(4.0 * F32_TRACE_MEASURED, 1e-3)
F64_TOL = 1e-9

_GOLD = {}


def gold(case):
    if case not in _GOLD:
        _GOLD[case] = load_golden('tvl1_%s_f64' % case)
    return _GOLD[case]


def autorho_of(g):
    return {'Enabled': bool(g['opt_AutoRho']), 'Period': int(g['opt_AutoRho_Period']),
            'Scaling': float(g['opt_AutoRho_Scaling']), 'RsdlRatio': float(g['opt_AutoRho_RsdlRatio']),
            'AutoScaling': bool(g['opt_AutoRho_AutoScaling']), 'RsdlTarget': float(g['opt_AutoRho_RsdlTarget']),
            'StdResiduals': bool(g['opt_StdResiduals'])}


def caxis_of(g):
    return None if 'caxis' not in g or int(g['caxis']) < 0 else int(g['caxis'])


def options_of(g, dtype, extra=None, cls=tvl1.TVL1Denoise):
    o = {'Verbose': False, 'MaxMainIter': int(g['MaxMainIter']) if 'MaxMainIter' in g else 1, 'RelStopTol': 0.0,
         'rho': float(g['opt_rho']) if 'opt_rho' in g else float(g['rho_before']),
         'RelaxParam': float(g['opt_RelaxParam']), 'gEvalY': bool(g['opt_gEvalY']),
         'MaxGSIter': int(g['opt_MaxGSIter']), 'GSTol': float(g['opt_GSTol']), 'AutoRho': autorho_of(g)}
    for key in ('DFidWeight', 'TVWeight', 'Y0', 'U0'):
        if 'optarr_' + key in g:
            o[key] = g['optarr_' + key].astype(dtype)
    o.update(extra or {})
    return cls.Options(o)


def restate(g, dtype=np.float64, iters=None, **kw):
    ar = autorho_of(g)
    args = dict(rho=float(g['opt_rho']), rlx=float(g['opt_RelaxParam']), caxis=caxis_of(g),
                geval_y=bool(g['opt_gEvalY']), ar=ar if ar['Enabled'] else None, std_residuals=ar['StdResiduals'],
                max_gs=int(g['opt_MaxGSIter']), gs_tol=float(g['opt_GSTol']), dtype=dtype)
    for key, name in (('DFidWeight', 'wdf'), ('TVWeight', 'wtv'), ('Y0', 'Y0'), ('U0', 'U0')):
        if 'optarr_' + key in g:
            args[name] = g['optarr_' + key]
    args.update(kw)
    return tn.tvl1_denoise(g['S'], float(g['lmbda']), int(g['MaxMainIter']) if iters is None else iters, **args)


def gs_comparable(g, margin):
    """Iterations of a GSTol > 0 fixture whose GSIter a run of lower precision must reproduce: up to the
    first one where a sweep's relative residual (re-run in float64 by the NumPy statement) lies within
    ``margin`` (relative) of GSTol."""
    gst = float(g['opt_GSTol'])
    n = len(g['it_GSIter'])
    rec = []

    def spy(ax, b):
        v = spy.rrs(ax, b)
        rec.append(v)
        return v
    spy.rrs = tn.rrs
    tn.rrs = spy
    try:
        out = restate(g)
    finally:
        tn.rrs = spy.rrs
    assert np.array_equal(out['GSIter'], g['it_GSIter'])
    keep, pos = np.ones(n, bool), 0
    for k in range(n):
        ng = int(g['it_GSIter'][k])
        vals = rec[pos:pos + ng]
        pos += ng
        if any(abs(v - gst) <= margin * gst for v in vals):
            keep[k:] = False
            break
    return keep


def compare(b, X, g, dtype, case):
    its = b.getitstat()
    if dtype == np.float64:
        tol_i = tol_t = F64_TOL
    else:
        tol_i, tol_t = F32_ITER_TOL, F32_TRACE_TOL
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
    gsi = np.asarray(its.GSIter)
    if dtype == np.float64 or float(g['opt_GSTol']) == 0.0:
        assert np.array_equal(gsi, g['it_GSIter'])
    else:
        keep = gs_comparable(g, F32_TRACE_TOL)
        assert np.sum(~keep) <= len(keep) // 4, np.sum(~keep)
        assert np.array_equal(gsi[keep], g['it_GSIter'][keep])


# ---- the class against the fixtures of the unmodified reference ----------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('case', CASES)
def test_against_reference_fixture(backend, case, dtype):
    g = gold(case)
    b = tvl1.TVL1Denoise(g['S'].astype(dtype), float(g['lmbda']), options_of(g, dtype), caxis=caxis_of(g))
    X = b.solve()
    compare(b, X, g, dtype, case)


def test_fixtures_take_both_branches():
    """What the generator asserted, read back: both shrinkages take both branches in every fixture."""
    for case in CASES:
        g = gold(case)
        for k in ('zero_share', 'zero_share_data'):
            assert 0.1 <= float(g[k]) <= 0.9, (case, k)
        assert float(g['lmbda']) == (1.0 if case == 'vec' else 0.8)
    assert all(len(set(gold(c)['it_Rho'])) > 2 for c in ('autorho', 'mask', 'vec'))
    assert sorted(set(gold('gstol')['it_GSIter'].astype(int))) == [1, 2, 3, 4, 5, 6]


def test_f32_measured_figures():
    """The figures of the header, measured again: the NumPy statement in float32 against each float64 fixture
    (and in float64: it states the reference's arithmetic)."""
    wi = wt = 0.0
    for case in CASES:
        g = gold(case)
        o64 = restate(g)
        for k in ('X', 'Y', 'U'):
            assert rel_l2(o64[k], g[k]) <= F64_TOL, (case, k)
        for f in TRACES:
            assert rel_l2(o64[f], g['it_' + f]) <= F64_TOL, (case, f)
        assert np.array_equal(o64['GSIter'], g['it_GSIter'])
        assert abs(o64['rho'] - float(g['rho_final'])) <= F64_TOL * float(g['rho_final'])
        o = restate(g, np.float32)
        ei = max(rel_l2(o[k], g[k]) for k in ('X', 'Y', 'U'))
        et = max(max(rel_l2(o[f], g['it_' + f]) for f in TRACES),
                 abs(o['rho'] - float(g['rho_final'])) / float(g['rho_final']))
        print('%-8s float32 statement: iterates %.2e traces %.2e' % (case, ei, et))
        wi, wt = max(wi, ei), max(wt, et)
    print('worst: iterates %.3e traces %.3e' % (wi, wt))
    assert wi <= F32_ITER_MEASURED and wt <= F32_TRACE_MEASURED
    # the gstol fixture leaves no iteration out of the float32 GSIter comparison
    keep = gs_comparable(gold('gstol'), F32_TRACE_TOL)
    print('gstol: %d of %d iterations left out' % (np.sum(~keep), len(keep)))
    assert np.sum(~keep) == 0


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_one_step_from_recorded_state(backend, dtype):
    g = load_golden('tvl1_step_f64')
    opt = options_of(g, dtype, {'Y0': g['Y_before'].astype(dtype), 'U0': g['U_before'].astype(dtype),
                                'MaxMainIter': 1})
    b = tvl1.TVL1Denoise(g['S'].astype(dtype), float(g['lmbda']), opt)
    b.X = g['X_before'].astype(dtype)
    X = b.solve()
    ti, tt = (F64_TOL, F64_TOL) if dtype == np.float64 else (F32_ITER_TOL, F32_TRACE_TOL)
    assert rel_l2(X, g['X']) <= ti and rel_l2(b.Y, g['Y']) <= ti
    # (the recorded run changed rho at the end of its iteration 40, a fresh object does not in its first:
    # rho U is what both agree on)
    assert rel_l2(b.U.astype(np.float64) * float(b.rho), g['U'] * float(g['rho_final'])) <= ti
    its = b.getitstat()
    for f in ('ObjFun', 'DFid', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'GSRelRes'):
        assert abs(getattr(its, f)[-1] - float(g['last_' + f])) <= tt * abs(float(g['last_' + f])), f
    assert its.GSIter[-1] == int(g['last_GSIter'])


# ---- against the NumPy statement at shapes chosen from the kernel's plan --------------------------------------
_PROBLEMS = {}


def problem(shape, seed=3, mask=False):
    """A piecewise-constant image with a little Gaussian and 20 % impulse noise; the optional mask has a
    fully masked border row and column."""
    key = (tuple(shape), seed, mask)
    if key not in _PROBLEMS:
        rng = np.random.RandomState(seed)
        H, W = shape[:2]
        img = np.ones((H, W))
        img[:, W // 2:] = -1.0
        img[H // 3:] *= 0.5
        S = img.reshape((H, W) + (1,) * (len(shape) - 2)) + 0.05 * rng.randn(*shape)
        S = np.where(rng.rand(*shape) < 0.2, rng.uniform(-1.5, 1.5, shape), S)
        wdf = 1.0
        if mask:
            wdf = (rng.rand(*shape) < 0.7).astype(np.float64)
            wdf[0] = 0.0
            wdf[:, -1] = 0.0
        _PROBLEMS[key] = (S, wdf)
    return _PROBLEMS[key]


def run_both(shape, caxis=None, mask=False, max_gs=2, iters=5, tvw=False, lmbda=0.8, rlx=1.8):
    S, wdf = problem(shape, mask=mask)
    wtv = 1.0
    if tvw:
        wtv = 0.5 + np.random.RandomState(5).rand(*shape)
    ar = {'Enabled': True, 'Period': 1, 'Scaling': 1000.0, 'RsdlRatio': 1.2, 'AutoScaling': True, 'RsdlTarget': 1.0}
    opt = tvl1.TVL1Denoise.Options({'Verbose': False, 'MaxMainIter': iters, 'RelStopTol': 0.0, 'DFidWeight': wdf,
                                    'TVWeight': wtv, 'MaxGSIter': max_gs, 'AutoRho': ar, 'RelaxParam': rlx})
    b = tvl1.TVL1Denoise(S, lmbda, opt, caxis=caxis)
    X = b.solve()
    ref = tn.tvl1_denoise(S, lmbda, iters, rlx=rlx, wdf=wdf, wtv=wtv, caxis=caxis, ar=ar, max_gs=max_gs)
    its = b.getitstat()
    errs = [rel_l2(X, ref['X']), rel_l2(b.Y, ref['Y']), rel_l2(b.U, ref['U'])]
    errs += [rel_l2(getattr(its, f), ref[f]) for f in TRACES]
    assert max(errs) <= F64_TOL, errs
    assert len(set(its.Rho)) > 1          # (the pending factor on U reached all three blocks)
    return b


def strip_and_segment():
    """TW (columns a strip covers) and R (rows of a segment) of the small float64 plan, P = 1."""
    pl = tvl1.plan((16, 16), np.float64)
    return pl['TW'], pl['R']


def test_plan_is_that_of_tvl2(backend):
    for shape, dt, cx in (((16, 16), np.float64, None), ((33, 1024), np.float32, None), ((4, 5, 3, 2), np.float64, 2)):
        assert tvl1.plan(shape, dt, caxis=cx) == tvl2.plan(shape, dt, caxis=cx)


@pytest.mark.parametrize('dw', [-1, 0, 1, 'two'])
@pytest.mark.parametrize('hsel', ['two', 'R', 'R+1'])
def test_strip_and_segment_borders(backend, dw, hsel):
    TW, R = strip_and_segment()
    W = 2 * TW + 1 if dw == 'two' else TW + dw
    H = {'two': 2, 'R': R, 'R+1': R + 1}[hsel]
    run_both((H, W), mask=(dw == 1))


@pytest.mark.parametrize('P', [1, 3, 5])
@pytest.mark.parametrize('max_gs', [1, 3])
def test_planes_and_sweeps(backend, P, max_gs):
    TW, R = strip_and_segment()
    # (P = 3, 5: a row of W P elements that is no multiple of the access width; two strips; two segments)
    W = TW // P + 2
    shape = (R + 3, W) if P == 1 else (R + 3, W, P)
    run_both(shape, mask=True, max_gs=max_gs, tvw=(P == 3))


def test_vector_accesses(backend):
    """Rows wide enough for 16-byte accesses (V = 2 in float64), P = 1 and P = 2: the elements of an item are
    neighbouring pixels, or a pixel's two planes."""
    TW, R = strip_and_segment()
    assert tvl1.plan((R + 1, 4 * TW), np.float64)['V'] == 2
    run_both((R + 1, 4 * TW), mask=True)
    assert tvl1.plan((3, 2 * TW, 2), np.float64)['V'] == 2
    run_both((3, 2 * TW, 2), mask=True, rlx=1.0)


def test_vector_tv_channels_and_images(backend):
    TW, R = strip_and_segment()
    run_both((R + 1, TW // 2 + 3, 3, 2), caxis=2, mask=True, lmbda=1.0)
    run_both((5, 7, 5), caxis=2, lmbda=1.0)            # (more than four channels: the wider item)


@pytest.mark.gpu
@pytest.mark.parametrize('shape,caxis', [((257, 131, 3), None), ((257, 131, 3), 2), ((64, 1031), None),
                                         ((40, 520, 8), None)])
def test_gpu_sizes(gpu_backend, shape, caxis):
    run_both(shape, caxis=caxis, mask=True, lmbda=1.0 if caxis else 0.8)


@pytest.mark.gpu
def test_gpu_float32_vector_access(gpu_backend):
    """16-byte float32 accesses (V = 4) against the float64 statement, at the float32 tolerances."""
    S, wdf = problem((33, 1024), mask=True)
    opt = tvl1.TVL1Denoise.Options({'Verbose': False, 'MaxMainIter': 5, 'RelStopTol': 0.0,
                                    'DFidWeight': wdf.astype(np.float32)})
    b = tvl1.TVL1Denoise(S.astype(np.float32), 0.8, opt)
    assert b._dev.plan()['V'] == 4
    X = b.solve()
    ref = tn.tvl1_denoise(S.astype(np.float32), 0.8, 5, wdf=wdf)
    assert max(rel_l2(X, ref['X']), rel_l2(b.Y, ref['Y']), rel_l2(b.U, ref['U'])) <= F32_ITER_TOL
    assert rel_l2(b.getitstat().ObjFun, ref['ObjFun']) <= F32_TRACE_TOL


# ---- the solver contract --------------------------------------------------------------------------------------
def small(dtype=np.float64, **o):
    g = gold('mask')
    opt = options_of(g, dtype, o)
    return tvl1.TVL1Denoise(g['S'].astype(dtype), float(g['lmbda']), opt), g


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_two_runs_bitwise_equal(backend, dtype):
    a, _ = small(dtype)
    b, _ = small(dtype)
    Xa, Xb = a.solve(), b.solve()
    assert np.array_equal(Xa, Xb) and np.array_equal(a.Y, b.Y) and np.array_equal(a.U, b.U)
    for f in TRACES + ('GSIter',):
        assert np.array_equal(getattr(a.getitstat(), f), getattr(b.getitstat(), f)), f


def test_solve_twice_continues(backend):
    a, g = small(MaxMainIter=20)
    a.solve()
    X = a.solve()
    b, _ = small()
    Xb = b.solve()
    assert np.array_equal(X, Xb) and np.array_equal(a.U, b.U) and float(a.rho) == float(b.rho)
    assert np.array_equal(a.getitstat().ObjFun, b.getitstat().ObjFun)
    assert list(a.getitstat().Iter) == list(range(40))
    assert rel_l2(X, g['X']) <= F64_TOL


def test_callback_stops(backend):
    seen = []

    def cb(obj):
        seen.append(obj.k)
        return obj.k == 3
    b, _ = small(Callback=cb)
    b.solve()
    assert seen == [0, 1, 2, 3] and len(b.itstat) == 4


def test_fastsolve(backend):
    a, g = small(FastSolve=True)
    X = a.solve()
    assert a.itstat == []
    assert rel_l2(X, g['X']) <= F64_TOL           # (AutoRho is on: the residuals are still formed)
    gd = gold('default')
    b = tvl1.TVL1Denoise(gd['S'], float(gd['lmbda']), tvl1.TVL1Denoise.Options(
        {'FastSolve': True, 'MaxMainIter': 40, 'Verbose': False}))
    assert rel_l2(b.solve(), gd['X']) <= F64_TOL and b.itstat == []


def test_defaults_and_attributes(backend):
    o = tvl1.TVL1Denoise.Options()
    assert (o['gEvalY'], o['RelaxParam'], o['DFidWeight'], o['TVWeight'], o['GSTol'], o['MaxGSIter']) == \
        (True, 1.8, 1.0, 1.0, 0.0, 2)
    ar = o['AutoRho']
    assert (ar['Enabled'], ar['Period'], ar['AutoScaling'], ar['Scaling'], ar['RsdlRatio'], ar['RsdlTarget']) == \
        (False, 1, True, 1000.0, 1.2, 1.0)
    S = gold('default')['S']
    b = tvl1.TVL1Denoise(S, 0.8)
    assert abs(float(b.rho) - 1.7) < 1e-15 and float(b.lmbda) == 0.8          # rho = 2 lmbda + 0.1
    assert tvl1.TVL1Denoise.IterationStats._fields == (
        'Iter', 'ObjFun', 'DFid', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho', 'GSIter',
        'GSRelRes', 'Time')
    assert np.array_equal(b.X, S) and np.array_equal(b.getmin(), S)          # X starts at S
    assert b.Y.shape == S.shape + (3,) and b.U.shape == S.shape + (3,) and not b.Y.any() and not b.U.any()
    assert np.array_equal(b.S, S) and float(b.Wdf) == 1.0 and float(b.Wtv) == 1.0
    assert b.itstat == [] and b.timer is not None
    assert np.array_equal(b.cnst_c()[..., 2], S) and not b.cnst_c()[..., :2].any()
    V = np.random.RandomState(0).randn(*(S.shape + (3,)))
    assert abs(np.sum(b.cnst_A(S) * V) - np.sum(S * b.cnst_AT(V))) < 1e-10          # A^T is A's transpose
    b32 = tvl1.TVL1Denoise(S, 0.8, tvl1.TVL1Denoise.Options({'DataType': np.float32}))
    assert b32.X.dtype == np.float32
    with pytest.raises(ValueError):
        b.Y = np.zeros(S.shape + (2,))


def test_refusals(backend):
    S = gold('default')['S']
    T = tvl1.TVL1Denoise
    with pytest.raises(NotImplementedError, match='real'):
        T(S + 1j * S, 0.8)
    with pytest.raises(NotImplementedError, match='axes'):
        T(np.zeros((4, 5, 6)), 0.8, axes=(0, 1, 2))
    with pytest.raises(NotImplementedError, match='axes'):
        T(S, 0.8, axes=(1,))
    with pytest.raises(NotImplementedError, match='caxis'):
        T(np.zeros((4, 5, 3, 2)), 0.8, caxis=3)
    with pytest.raises(NotImplementedError, match='caxis'):
        T(S, 0.8, caxis=2)
    with pytest.raises(NotImplementedError, match='at least 2'):
        T(np.zeros((1, 9)), 0.8)
    with pytest.raises(NotImplementedError, match='at least 2'):
        T(np.zeros((9, 1, 3)), 0.8)
    with pytest.raises(TypeError):
        T(S.astype(np.float16), 0.8)
    with pytest.raises(TypeError):
        T(S.astype(np.int32), 0.8)
    with pytest.raises(NotImplementedError, match='reducer'):
        T(S, 0.8, reducer=lambda x: x)
    with pytest.raises(NotImplementedError, match='TVWeight'):
        T(np.zeros((4, 5, 3, 2)), 0.8, T.Options({'TVWeight': np.ones((4, 5, 3, 2))}), caxis=2)
    with pytest.raises(NotImplementedError, match='channels'):
        T(np.zeros((4, 5, 9)), 0.8, caxis=2)
    with pytest.raises(NotImplementedError, match='trailing'):
        T(np.zeros((4, 5, 3, 2, 2)), 0.8)
    with pytest.raises(NotImplementedError, match='pickling'):
        pickle.dumps(T(S, 0.8))


def test_mode_is_per_handle(backend):
    """A TVL2Denoise made after (and beside) a TVL1Denoise in the same process still gives its own fixture."""
    g1 = gold('default')
    a = tvl1.TVL1Denoise(g1['S'], float(g1['lmbda']), options_of(g1, np.float64))
    g2 = load_golden('tvl2_default_f64')
    b = tvl2.TVL2Denoise(g2['S'], float(g2['lmbda']), options_of(g2, np.float64, cls=tvl2.TVL2Denoise))
    Xb = b.solve()
    Xa = a.solve()
    assert b.Y.shape == g2['Y'].shape and a.Y.shape == g1['Y'].shape
    assert max(rel_l2(Xb, g2['X']), rel_l2(b.Y, g2['Y']), rel_l2(b.U, g2['U'])) <= F64_TOL
    for f in TRACES:
        assert rel_l2(getattr(b.getitstat(), f), g2['it_' + f]) <= F64_TOL, f
    assert max(rel_l2(Xa, g1['X']), rel_l2(a.Y, g1['Y']), rel_l2(a.U, g1['U'])) <= F64_TOL


# ---- device arrays -----------------------------------------------------------------------------------------------
def test_device_input_and_example_chain(backend):
    """Device arrays in, sl = TVL1Denoise(...).solve(), sh = mskp * (imgwp - sl): nothing crosses to the host
    but the sums of each iteration."""
    g = gold('mask')
    img, msk, lmbda = g['S'].astype(np.float32), g['optarr_DFidWeight'].astype(np.float32), float(g['lmbda'])
    o = {'Verbose': False, 'MaxMainIter': 40, 'gEvalY': False, 'AutoRho': {'Enabled': True}}
    bh = tvl1.TVL1Denoise(img, lmbda, tvl1.TVL1Denoise.Options(dict(o, DFidWeight=msk)))
    slh = bh.solve()
    shh = msk * (img - slh)

    imgwp, mskp = DeviceArray.from_host(img), DeviceArray.from_host(msk)
    _lib.transfer_stats(reset=True)
    opt = tvl1.TVL1Denoise.Options(dict(o, DFidWeight=mskp))
    b = tvl1.TVL1Denoise(imgwp, lmbda, opt)
    sl = b.solve()
    sh = mskp * (imgwp - sl)
    st = _lib.transfer_stats()
    assert st['h2d_bytes'] == 0 and st['d2h_bytes'] <= 40 * _lib.OUT_COUNT * 8     # (the sums only, one read each)
    assert isinstance(sl, DeviceArray) and isinstance(b.getmin(), DeviceArray) and isinstance(sh, DeviceArray)
    assert np.array_equal(sl.get(), slh) and np.array_equal(sh.get(), shh)
    assert np.array_equal(b.getitstat().ObjFun, bh.getitstat().ObjFun)
    assert np.array_equal(b.getitstat().PrimalRsdl, bh.getitstat().PrimalRsdl)      # (||S|| formed on the device)


# ---- recovery: the reference's tests/admm/test_tvl1.py TestSet02.test_01 ------------------------------------------
def test_recovery(backend):
    g = load_golden('tvl1_recovery_f64')
    U, D = g['U'], g['D']
    opt = tvl1.TVL1Denoise.Options({'Verbose': False, 'gEvalY': False, 'MaxMainIter': int(g['MaxMainIter'])})
    b = tvl1.TVL1Denoise(D, float(g['lmbda']), opt)
    X = b.solve()
    print('ObjFun %.12f after %d iterations (reference %.12f after %d)'
          % (b.itstat[-1].ObjFun, len(b.itstat), float(g['ObjFun']), int(g['iterations'])))
    assert len(b.itstat) == int(g['iterations'])
    # (the reference's own bound on this value in its test)
    assert abs(b.itstat[-1].ObjFun - float(g['ObjFun'])) < 1e-6
    assert np.mean((U - X) ** 2) < np.mean((U - D) ** 2)
