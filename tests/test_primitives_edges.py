"""Every kernel form and launch edge of the stateless primitives -- linalg.inner, linalg.solvedbi_sm(_c),
prox.prox_l1 / prox_sl1l2 / prox_l2 / proj_l2, fft.rfl2norm2, signal.tikhonov_filter, fft.fftconv --
against the float64 NumPy expressions of tests/_prims_numpy.py (written from the definitions; pinned
to the reference's recorded outputs in section 0).  The same kernels sit under every solver class.

What the launchers decide, and where it is tested here (the rules are restated in this file from the
launchers' source, never read back from the library):

* grid_for caps every grid at 4096 workgroups of 256 threads: above CAP = 1 048 576 work items a kernel
  walks its grid-stride loop a second time.  Every such case is GPU-only (`above_cap` tests).
* launch_sm_solve: the wave form (groups of K/2 lanes, shuffle reduction, tail wave padded with `valid`
  flags) for K/2 a power of two <= 64, the generic form (one thread a system) for every other K.
* launch_inner: sixteen lanes an output for K >= 16 (strided tail when K % 16 != 0), else one thread.
* prox_l1_kernel: scalar threshold, or a 5-D index with a stride-0 broadcast weight; prox.py expands
  the weight itself for more than five axes.
* prox_sl1l2_kernel: one thread a group, the group's members `inner` apart.
* ball_geom: vector width, fold, cols / rows, column and row blocks, the tile cap (section 5).
* the pre / post-processing kernels of tikhonov_filter and fftconv (section 7).

Tolerances.  float64: 1e-12 (the project's figure in test_primitives.py / test_signal_device.py).
float32 where the project has a figure: solves 1e-5, proj_l2 1e-6, transforms and pipelines 1e-5, the
soft threshold exact.  float32 where it has none: the same expression is evaluated in NumPy float32 with
every sum taken sequentially (np.add.accumulate; _prims_numpy.*_f32) on the test's own seeded inputs and
compared with the float64 reference; the bound is 4 x the largest relative l2 error over the test's cases,
rounded up to one significant digit.  The factor covers the kernels' different, equally valid summation
order; no bound was measured against a kernel's output.  test_f32_bounds_are_the_measured_ones repeats
the measurement.

    test                                   cases                              measured   bound
    test_solvedbi_sm_small                 K = 128, 130, complex64            3.6e-08    2e-07
    test_solvedbi_sm_above_cap             K = 128, complex64                 3.5e-08    2e-07
    test_inner_small                       complex64, all K                   2.2e-07    9e-07
    test_inner_above_cap                   complex64, K = 16 and K = 2        8.2e-08    4e-07
    test_inner_any_axis_sixteen_lanes      complex64, K = 20                  1.1e-07    5e-07
    test_prox_sl1l2_small                  float32, all cases                 8.0e-08    4e-07
    test_prox_sl1l2_axis_none_4096         float32                            7.4e-08    3e-07
    test_prox_sl1l2_above_cap              float32                            5.1e-08    3e-07
    test_rfl2norm2_small                   complex64, all cases               2.5e-07    1e-06
    test_rfl2norm2_above_cap               complex64                          1.3e-03    6e-03

(The last figure is what a sequential float32 sum of four million squares gives; the kernel accumulates
in double, so for complex64 that case only shows that nothing gross happens above the cap -- its
complex128 twin, at 1e-12, is the one that checks the indexing.)

Conditions on the inputs: wherever an output depends on a comparison with a threshold, the seeded
inputs keep clear of it (asserted in the test: no |v| within 1e-3 alpha of alpha, no group norm within
1e-3 beta of beta, no plane norm within 1e-3 gamma of gamma); the on-threshold cases are separate and use
exactly representable numbers.  Scalar parameters that reach a float32 kernel are exactly representable in
float32 (except rho = 1e-2, whose rounding, 2e-8, is far inside the bound).
"""

import math

import numpy as np
import pytest

from conftest import load_golden, rel_l2

import _prims_numpy as pn

CAP = 4096 * 256        # kMaxPartialBlocks workgroups x kThreads


def bound_of(measured):
    """4 x measured, rounded up to one significant digit."""
    x = 4.0 * measured
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


# Largest relative l2 error of the float32 NumPy evaluation against the float64 reference over each
# test's cases (test_f32_bounds_are_the_measured_ones repeats it).
F32_MEASURED = {
    'sm_small': 3.6e-08,
    'sm_above_cap': 3.5e-08,
    'inner_small': 2.2e-07,
    'inner_above_cap': 8.2e-08,
    'inner_axis': 1.1e-07,
    'sl1l2_small': 8.0e-08,
    'sl1l2_none_4096': 7.4e-08,
    'sl1l2_above_cap': 5.1e-08,
    'rfl2_small': 2.5e-07,
    'rfl2_above_cap': 1.3e-03,
}
F32_BOUND = {
    'sm_small': 2e-07,
    'sm_above_cap': 2e-07,
    'inner_small': 9e-07,
    'inner_above_cap': 4e-07,
    'inner_axis': 5e-07,
    'sl1l2_small': 4e-07,
    'sl1l2_none_4096': 3e-07,
    'sl1l2_above_cap': 3e-07,
    'rfl2_small': 1e-06,
    'rfl2_above_cap': 6e-03,
}

CDTS = [pytest.param(np.complex128, id='c128'), pytest.param(np.complex64, id='c64')]
RDTS = [pytest.param(np.float64, id='f64'), pytest.param(np.float32, id='f32')]


def is_f32(dt):
    return np.dtype(dt) in (np.float32, np.complex64)


def crandn(rng, shape, cdt):
    return (rng.randn(*shape) + 1j * rng.randn(*shape)).astype(cdt)


# ---- 0. the NumPy expressions against the reference's recorded outputs ----------------------------------
def test_numpy_references_pinned_to_the_recorded_outputs():
    """tests/_prims_numpy.py reproduces what the reference computed (primitives.npz, signal_prims.npz):
    this fixes every convention -- no conjugation in inner, the sign of fftconv's origin, the symmetric
    padding and the gradient spectrum of tikhonov_filter, the half-spectrum weights."""
    g = load_golden('primitives')
    rho = float(g['sm_rho'])
    assert rel_l2(pn.solvedbi_sm(g['sm_ah'], rho, g['sm_b']), g['sm_x']) < 1e-14
    assert rel_l2(pn.solvedbi_sm_c(g['sm_ah'], np.conj(g['sm_ah']), rho), g['sm_c']) < 1e-14
    assert rel_l2(pn.inner(g['sm_ah'], g['sm_b']), g['inner_ab']) < 1e-14
    v, a = g['prox_v'], float(g['prox_alpha'])
    assert np.array_equal(pn.prox_l1(v, a), g['prox_l1'])
    assert np.array_equal(pn.prox_l1(v, a * g['prox_w']), g['prox_l1w'])
    assert rel_l2(pn.prox_sl1l2(v, a, 0.9, axis=2), g['prox_sl1l2']) < 1e-14
    assert rel_l2(pn.prox_sl1l2(v, 0.0, 0.9, axis=2), g['prox_l2']) < 1e-14
    assert rel_l2(pn.prox_sl1l2(g['prox_vz'], a, 0.9, axis=2), g['prox_sl1l2_z']) < 1e-14
    assert abs(pn.rfl2norm2(g['fft_af'], g['fft_a'].shape[:2]) - float(g['nrm_odd'])) < 1e-13 * float(g['nrm_odd'])
    s = load_golden('signal_prims')
    for sig, lm, npd, rl, rh in ((s['s2'], 5.0, 16, s['sl2'], s['sh2']), (s['s3'], 2.0, 4, s['sl3'], s['sh3'])):
        tol = 1e-5 if sig.dtype == np.float32 else 1e-12
        lo, hi = pn.tikhonov_filter(sig, lm, npd)
        assert rel_l2(lo, rl) < tol and rel_l2(hi, rh) < tol
    assert rel_l2(pn.fftconv(s['d'], s['x'], origin=(2, 2)), s['cv']) < 1e-12
    assert rel_l2(pn.fftconv(s['k3'], s['s2']), s['cv1']) < 1e-12


# ---- 1. solvedbi_sm / solvedbi_sm_c ---------------------------------------------------------------------
WAVE_K = (2, 4, 8, 16, 32, 64, 128)
GENERIC_K = (1, 3, 6, 12, 17, 24, 130)
SM_FORMS = [pytest.param('wave', K, id='wave-K%d' % K) for K in WAVE_K] + \
           [pytest.param('generic', K, id='generic-K%d' % K) for K in GENERIC_K]
# (37, ., .): npix C N K/2 is no multiple of 64 for small K, so the padded tail wave runs; (1, 1, 1): a
# single system, G = K/2 lanes of one wave
SM_SHAPES = [pytest.param(s, id='npix%d-C%d-N%d' % s) for s in ((37, 1, 1), (37, 3, 2), (1, 1, 1))]
SM_ABOVE_CAP = [
    # wave form, G = 64: 16 421 waves, the grid (4096 x 4 waves) walks them in two passes
    pytest.param('wave', 128, 16384 + 37, 1, 1, id='wave-K128-G64-16421-systems'),
    # wave form, G = 1: CAP + 2*256 + 37 lanes = 8393 * 25 * 5, two passes and a padded tail wave
    pytest.param('wave', 2, 8393, 25, 5, id='wave-K2-G1-cap+549-systems'),
    # generic form: CAP + 257 threads = 116 537 * 3 * 3
    pytest.param('generic', 3, 116537, 3, 3, id='generic-K3-cap+257-systems'),
]
assert 8393 * 25 * 5 == CAP + 2 * 256 + 37 and 116537 * 9 == CAP + 257 and (16384 + 37) * 64 > CAP


def sm_form(K):
    """launch_sm_solve's rule (ck_admm.hip): the wave form iff K is even and K/2 a power of two <= 64."""
    G = K // 2
    return 'wave' if K % 2 == 0 and G >= 1 and G & (G - 1) == 0 and G <= 64 else 'generic'


def sm_operands(K, npix, C, N, cdt):
    rng = np.random.RandomState([11, K, npix, C, N])
    return crandn(rng, (npix, 1, 1, K), cdt), crandn(rng, (npix, C, N, K), cdt)


def check_solve(ah, rho, b, tol, last=None):
    from sporco_amd import linalg
    x = linalg.solvedbi_sm(ah, rho, b, axis=-1)
    assert x.dtype == b.dtype and x.shape == b.shape
    want = pn.solvedbi_sm(ah, rho, b)
    err = rel_l2(x, want)
    # the defining property (rho I + a a^H) x = b; an error of the solution is magnified by at most the
    # condition number 1 + |a|^2 / rho of the worst system
    cond = 1.0 + float(np.max(np.sum(np.abs(ah.astype(np.complex128)) ** 2, axis=-1))) / rho
    res = rel_l2(pn.sm_residual(ah, rho, x), b)
    print('solvedbi_sm: rel l2 %.3e (bound %.1e), residual %.3e (bound %.1e)' % (err, tol, res, cond * tol))
    assert err < tol
    assert res < cond * tol
    if last:
        K = b.shape[-1]
        tail = rel_l2(x.reshape(-1, K)[-last:], want.reshape(-1, K)[-last:])
        print('  last %d systems: rel l2 %.3e' % (last, tail))
        assert tail < tol
    return x


def sm_tol(cdt, K, key):
    if not is_f32(cdt):
        return 1e-12
    return F32_BOUND[key] if K >= 128 else 1e-5


@pytest.mark.parametrize('cdt', CDTS)
@pytest.mark.parametrize('shape', SM_SHAPES)
@pytest.mark.parametrize('form,K', SM_FORMS)
def test_solvedbi_sm_small(backend, form, K, shape, cdt):
    from sporco_amd import linalg
    assert sm_form(K) == form
    ah, b = sm_operands(K, *shape, cdt=cdt)
    rho = 1.0
    tol = sm_tol(cdt, K, 'sm_small')
    check_solve(ah, rho, b, tol)
    c = linalg.solvedbi_sm_c(ah, np.conj(ah), rho, axis=-1)
    assert c.dtype == cdt and c.shape == ah.shape
    assert rel_l2(c, pn.solvedbi_sm_c(ah, np.conj(ah), rho)) < tol


@pytest.mark.parametrize('cdt', CDTS)
@pytest.mark.parametrize('rho', [1e-2, 1.0, 1e2])
@pytest.mark.parametrize('form,K', [pytest.param('wave', 8, id='wave-K8'), pytest.param('generic', 6, id='generic-K6')])
def test_solvedbi_sm_rho_decades(backend, form, K, rho, cdt):
    assert sm_form(K) == form
    ah, b = sm_operands(K, 37, 3, 2, cdt)
    check_solve(ah, rho, b, sm_tol(cdt, K, None))


@pytest.mark.parametrize('rdt', RDTS)
@pytest.mark.parametrize('form,K', [pytest.param('wave', 8, id='wave-K8'), pytest.param('generic', 6, id='generic-K6')])
def test_solvedbi_sm_real_operands(backend, form, K, rdt):
    """Real operands: the solution is real, of the real dtype."""
    from sporco_amd import linalg
    assert sm_form(K) == form
    rng = np.random.RandomState(12)
    ah, b = rng.randn(37, 1, 1, K).astype(rdt), rng.randn(37, 3, 2, K).astype(rdt)
    x = linalg.solvedbi_sm(ah, 0.5, b, axis=-1)
    assert x.dtype == rdt and not np.iscomplexobj(x) and x.shape == b.shape
    want = pn.solvedbi_sm(ah, 0.5, b)
    assert np.all(want.imag == 0.0)
    assert rel_l2(x, want.real) < (1e-5 if is_f32(rdt) else 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize('cdt', CDTS)
@pytest.mark.parametrize('form,K,npix,C,N', SM_ABOVE_CAP)
def test_solvedbi_sm_above_cap(backend, form, K, npix, C, N, cdt):
    """More work items than the capped grid has threads: every element, and the last 300 systems on
    their own (the ones a wrong stride or bound of the grid-stride loop drops)."""
    assert sm_form(K) == form
    assert npix * C * N * (K // 2 if form == 'wave' else 1) > CAP
    ah, b = sm_operands(K, npix, C, N, cdt)
    check_solve(ah, 1.0, b, sm_tol(cdt, K, 'sm_above_cap'), last=300)


# ---- 2. inner -------------------------------------------------------------------------------------------
INNER_FORMS = [pytest.param('thread', K, id='thread-K%d' % K) for K in (1, 7, 15)] + \
              [pytest.param('lanes16', K, id='lanes16-K%d%s' % (K, '-tail' if K % 16 else ''))
               for K in (16, 17, 31, 64, 100)]
INNER_SHAPES = [pytest.param(s, id='npix%d-CN%d' % s) for s in ((37, 1), (37, 6), (1, 1))]
INNER_ABOVE_CAP = [
    # sixteen lanes: (65 536 + 37) * 16 lanes = 2851 * 23 outputs, whole workgroups iterate together
    pytest.param('lanes16', 16, 2851, 23, id='lanes16-K16-65573-outputs'),
    # one thread an output: CAP + 257 = 116 537 * 9
    pytest.param('thread', 2, 116537, 9, id='thread-K2-cap+257-outputs'),
]
assert 2851 * 23 == 65536 + 37 and 65573 * 16 > CAP


def inner_form(K):
    """launch_inner's rule (ck_admm.hip)."""
    return 'lanes16' if K >= 16 else 'thread'


def inner_operands(K, npix, CN, cdt):
    rng = np.random.RandomState([21, K, npix, CN])
    C = 3 if CN % 3 == 0 else 1
    return crandn(rng, (npix, 1, 1, K), cdt), crandn(rng, (npix, C, CN // C, K), cdt)


def inner_any_axis_operands(cdt):
    rng = np.random.RandomState(22)
    return crandn(rng, (5, 20, 3), cdt), crandn(rng, (5, 20, 3), cdt)


def check_inner(x, y, axis, tol, last=None):
    from sporco_amd import linalg
    r = linalg.inner(x, y, axis=axis)
    want = pn.inner(x, y, axis=axis)
    assert r.dtype == y.dtype and r.shape == want.shape
    err = rel_l2(r, want)
    print('inner: rel l2 %.3e (bound %.1e)' % (err, tol))
    assert err < tol
    if last:
        assert rel_l2(r.ravel()[-last:], want.ravel()[-last:]) < tol


@pytest.mark.parametrize('cdt', CDTS)
@pytest.mark.parametrize('shape', INNER_SHAPES)
@pytest.mark.parametrize('form,K', INNER_FORMS)
def test_inner_small(backend, form, K, shape, cdt):
    assert inner_form(K) == form
    x, y = inner_operands(K, *shape, cdt=cdt)
    check_inner(x, y, -1, F32_BOUND['inner_small'] if is_f32(cdt) else 1e-12)


@pytest.mark.parametrize('cdt', CDTS)
def test_inner_any_axis_sixteen_lanes(backend, cdt):
    """An axis other than the last (linalg._moved_last), K = 20: the sixteen-lane form with a tail."""
    assert inner_form(20) == 'lanes16'
    x, y = inner_any_axis_operands(cdt)
    check_inner(x, y, 1, F32_BOUND['inner_axis'] if is_f32(cdt) else 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize('cdt', CDTS)
@pytest.mark.parametrize('form,K,npix,CN', INNER_ABOVE_CAP)
def test_inner_above_cap(backend, form, K, npix, CN, cdt):
    assert inner_form(K) == form and npix * CN * (16 if form == 'lanes16' else 1) > CAP
    x, y = inner_operands(K, npix, CN, cdt)
    check_inner(x, y, -1, F32_BOUND['inner_above_cap'] if is_f32(cdt) else 1e-12, last=300)


# ---- 3. prox_l1 -----------------------------------------------------------------------------------------
def clear_of_threshold(v, alpha):
    """Move every element within 1 % of its threshold to 1.5 x the threshold (the seeded inputs stay
    unambiguous whatever the seed)."""
    v, alpha = np.asarray(v), np.broadcast_to(alpha, np.shape(v))
    near = (np.abs(np.abs(v) - alpha) < 1e-2 * alpha) & (alpha > 0)
    return np.where(near, np.where(v < 0, -1.5, 1.5) * alpha, v)


def assert_clear_of_threshold(v, alpha):
    v64, a64 = np.asarray(v, dtype=np.float64), np.asarray(alpha, dtype=np.float64)
    assert np.all((np.abs(np.abs(v64) - a64) > 1e-3 * a64) | (a64 == 0))


def l1_case(shape, ashape, rdt, seed):
    rng = np.random.RandomState([31, seed])
    alpha = (0.1 + 0.5 * np.abs(rng.randn(*ashape))).astype(rdt)
    v = clear_of_threshold(rng.randn(*shape), np.broadcast_to(alpha.astype(np.float64), shape)).astype(rdt)
    assert_clear_of_threshold(v, np.broadcast_to(alpha, shape))
    return v, alpha


def check_prox_l1(v, alpha, what=None):
    from sporco_amd import prox
    got = prox.prox_l1(v, alpha)
    assert got.dtype == v.dtype and got.shape == v.shape, what
    want = pn.prox_l1(v, alpha)
    assert np.array_equal(got, want), (what, int(np.sum(got != want)), np.flatnonzero(got != want)[:8])
    return got


@pytest.mark.parametrize('rdt', RDTS)
def test_prox_l1_every_broadcast_pattern_5d(backend, rdt):
    """alpha with the full extent on each of the 32 subsets of the five axes and 1 elsewhere: the
    stride-0 weight of prox_l1_kernel's general path on every axis, alone and together."""
    shape = (5, 6, 2, 3, 4)
    for mask in range(32):
        ashape = tuple(n if mask >> i & 1 else 1 for i, n in enumerate(shape))
        v, alpha = l1_case(shape, ashape, rdt, mask)
        got = check_prox_l1(v, alpha, ashape)
        assert np.any(got == 0) and np.any(got != 0)


@pytest.mark.parametrize('rdt', RDTS)
def test_prox_l1_fewer_leading_axes_3d(backend, rdt):
    """A 3-D v (two leading unit axes in the kernel's 5-D view) and the 8 subsets of its axes, alpha
    given without its leading unit axes."""
    shape = (4, 5, 6)
    for mask in range(8):
        ashape = tuple(n if mask >> i & 1 else 1 for i, n in enumerate(shape))
        while len(ashape) > 1 and ashape[0] == 1:
            ashape = ashape[1:]
        v, alpha = l1_case(shape, ashape, rdt, 100 + mask)
        check_prox_l1(v, alpha, ashape)


@pytest.mark.parametrize('rdt', RDTS)
def test_prox_l1_more_than_five_axes(backend, rdt):
    """Six axes: prox.py expands alpha itself (no compact 5-D form in general)."""
    v, alpha = l1_case((2, 3, 2, 3, 2, 3), (3, 1, 3, 1, 3), rdt, 200)
    check_prox_l1(v, alpha)
    v, alpha = l1_case((2, 3, 2, 3, 2, 3), (2, 1, 1, 1, 1, 1), rdt, 201)
    check_prox_l1(v, alpha)
    check_prox_l1(v, 0.25)


@pytest.mark.parametrize('rdt', RDTS)
def test_prox_l1_values_on_the_threshold(backend, rdt):
    """alpha = 0 returns v; an element exactly at +-alpha gives zero; a weight of zero passes its element
    through -- scalar and array thresholds, exactly representable numbers."""
    rng = np.random.RandomState(32)
    v = rng.randn(7, 9).astype(rdt)
    assert np.array_equal(check_prox_l1(v, 0.0), v)
    assert np.array_equal(check_prox_l1(v, np.zeros((1, 9), dtype=rdt)), v)
    e = np.array([0.5, -0.5, 1.0, -1.0, 0.0, 0.25, -0.25, 0.5], dtype=rdt)
    assert np.array_equal(check_prox_l1(e, 0.5), np.array([0, 0, 0.5, -0.5, 0, 0, 0, 0], dtype=rdt))
    w = np.array([0.5, 0.5, 0.25, 1.0, 0.0, 0.0, 0.25, 0.125], dtype=rdt)
    assert np.array_equal(check_prox_l1(e, w), np.array([0, 0, 0.75, 0, 0, 0.25, 0, 0.375], dtype=rdt))
    e2 = np.tile(e, (3, 1))
    assert np.array_equal(check_prox_l1(e2, w), np.tile(np.array([0, 0, 0.75, 0, 0, 0.25, 0, 0.375], dtype=rdt), (3, 1)))
    # a weight array with zeros among random values
    wz = np.where(rng.rand(1, 9) < 0.4, 0.0, 0.5).astype(rdt)
    got = check_prox_l1(v, wz)
    zero_w = np.broadcast_to(wz == 0, v.shape)
    assert np.any(zero_w) and np.array_equal(got[zero_w], v[zero_w])


def test_prox_l1_float64_weights_against_float32_values(backend):
    """A float32 v with a float64 alpha array: the weights are rounded to float32 first and the result
    is float32 (documented in prox.prox_l1), so the reference is evaluated the same way."""
    from sporco_amd import prox
    v, alpha = l1_case((6, 5, 4), (5, 1), np.float32, 300)
    alpha64 = alpha.astype(np.float64) * (1.0 + 2.0 ** -30)      # not representable in float32
    assert not np.array_equal(alpha64.astype(np.float32).astype(np.float64), alpha64)
    assert_clear_of_threshold(v, np.broadcast_to(alpha64, (6, 5, 4)))
    got = prox.prox_l1(v, alpha64)
    assert got.dtype == np.float32
    assert np.array_equal(got, pn.prox_l1(v, alpha64.astype(np.float32)))


@pytest.mark.gpu
@pytest.mark.parametrize('rdt', RDTS)
@pytest.mark.parametrize('shape,ashape', [pytest.param((CAP + 257,), None, id='scalar-cap+257'),
                                          pytest.param((1, 1, 1, 4099, 257), (257,), id='weight-last-axis-4099x257')])
def test_prox_l1_above_cap(backend, shape, ashape, rdt):
    assert int(np.prod(shape)) > CAP
    if ashape is None:
        rng = np.random.RandomState(33)
        v = clear_of_threshold(rng.randn(*shape), 0.5).astype(rdt)
        assert_clear_of_threshold(v, 0.5)
        got = check_prox_l1(v, 0.5)
    else:
        v, alpha = l1_case(shape, ashape, rdt, 400)
        got = check_prox_l1(v, alpha)
    assert np.array_equal(got.ravel()[-300:], pn.prox_l1(v, 0.5 if ashape is None else alpha).ravel()[-300:])


# ---- 4. prox_sl1l2 / prox_l2 ----------------------------------------------------------------------------
# id, shape, axis, alpha, beta (alpha and beta exactly representable in float32)
SL_CASES = [
    ('axis0-outer1-inner35', (6, 5, 7), 0, 0.25, 0.875),
    ('axis1-outer6-inner7', (6, 5, 7), 1, 0.25, 0.875),
    ('axis2-outer30-inner1', (6, 5, 7), 2, 0.25, 0.875),
    ('axis-1', (6, 5, 7), -1, 0.25, 0.875),
    ('axis-tuple', (6, 5, 7), (1,), 0.25, 0.875),
    ('axisNone-one-thread', (6, 5, 7), None, 0.25, 4.0),
    ('C1', (4, 1, 3), 1, 0.25, 0.5),
    ('alpha0-prox_l2', (6, 5, 7), 1, 0.0, 1.5),
    ('alpha-large-groups-vanish', (6, 5, 7), 1, 2.0, 0.25),
    ('zero-groups-beside-others', (6, 5, 7), 1, 0.25, 0.875),
]


def clear_of_beta(v, alpha, beta, axis):
    """Give every group whose norm lies within 1 % of beta members of size alpha + 2 beta (norm >= 2 beta)."""
    n = pn.group_norm(v, alpha, axis)
    near = np.broadcast_to(np.abs(n - beta) < 1e-2 * beta, v.shape)
    return np.where(near, np.where(v < 0, -1.0, 1.0) * (alpha + 2.0 * beta), v)


def sl_operands(name, shape, axis, alpha, beta, rdt, seed):
    rng = np.random.RandomState([41, seed])
    v = clear_of_beta(clear_of_threshold(rng.randn(*shape), alpha), alpha, beta, axis)
    if name.startswith('zero-groups'):
        v[0] = 0.0
        v[2, :, 3] = 0.0
        v[5, :, 6] = 0.0
    return v.astype(rdt)


def check_sl1l2(v, alpha, beta, axis, tol, expect_vanished=False):
    from sporco_amd import prox
    assert_clear_of_threshold(v, alpha)
    n = pn.group_norm(v, alpha, axis)
    assert np.all(np.abs(n - beta) > 1e-3 * beta)
    got = prox.prox_l2(v, beta, axis=axis) if alpha == 0.0 else prox.prox_sl1l2(v, alpha, beta, axis=axis)
    assert got.dtype == v.dtype and got.shape == v.shape and np.all(np.isfinite(got))
    want = pn.prox_sl1l2(v, alpha, beta, axis)
    err = rel_l2(got, want)
    print('prox_sl1l2: rel l2 %.3e (bound %.1e); groups kept %d of %d' % (err, tol, int(np.sum(n > beta)), n.size))
    assert err < tol
    assert np.array_equal(got == 0, want == 0)        # (what vanishes in the reference vanishes exactly)
    if n.size > 1:
        assert np.any(n > beta)
    if expect_vanished:
        assert np.any(n == 0) and np.any(n > 0)


@pytest.mark.parametrize('rdt', RDTS)
@pytest.mark.parametrize('name,shape,axis,alpha,beta', [pytest.param(*c, id=c[0]) for c in SL_CASES])
def test_prox_sl1l2_small(backend, name, shape, axis, alpha, beta, rdt):
    v = sl_operands(name, shape, axis, alpha, beta, rdt, [c[0] for c in SL_CASES].index(name))
    check_sl1l2(v, alpha, beta, axis, F32_BOUND['sl1l2_small'] if is_f32(rdt) else 1e-12,
                expect_vanished=name.startswith(('zero-groups', 'alpha-large')))


@pytest.mark.parametrize('rdt', RDTS)
def test_prox_sl1l2_norm_exactly_beta(backend, rdt):
    """A group of norm exactly beta vanishes, beside a zero group and one that is halved: (3, 4) and
    (6, 8) against beta = 5 with alpha = 0, and (4, 5) and (7, 9) with alpha = 1."""
    from sporco_amd import prox
    v = np.array([[3, 4], [0, 0], [6, 8], [-3, 4]], dtype=rdt)
    want = np.array([[0, 0], [0, 0], [3, 4], [0, 0]], dtype=rdt)
    assert np.array_equal(prox.prox_l2(v, 5.0, axis=1), want)
    assert np.array_equal(prox.prox_sl1l2(v, 0.0, 5.0, axis=-1), want)
    assert np.array_equal(prox.prox_sl1l2(v.T.copy(), 0.0, 5.0, axis=0), want.T)
    v1 = np.array([[4, -5], [0.5, -1], [7, 9]], dtype=rdt)
    assert np.array_equal(prox.prox_sl1l2(v1, 1.0, 5.0, axis=1), np.array([[0, 0], [0, 0], [3, 4]], dtype=rdt))


def sl_none_operands(rdt):
    rng = np.random.RandomState(42)
    return clear_of_beta(clear_of_threshold(rng.randn(64, 64), 0.25), 0.25, 16.0, None).astype(rdt)


@pytest.mark.parametrize('rdt', RDTS)
def test_prox_sl1l2_axis_none_4096(backend, rdt):
    """axis=None on 4096 elements: one thread sums the whole array in the array's own precision."""
    v = sl_none_operands(rdt)
    check_sl1l2(v, 0.25, 16.0, None, F32_BOUND['sl1l2_none_4096'] if is_f32(rdt) else 1e-12)


def sl_above_cap_operands(rdt):
    rng = np.random.RandomState(43)
    return clear_of_beta(clear_of_threshold(rng.randn(1030, 2, 1021), 0.25), 0.25, 0.75, 1).astype(rdt)


@pytest.mark.gpu
@pytest.mark.parametrize('rdt', RDTS)
def test_prox_sl1l2_above_cap(backend, rdt):
    """(1030, 2, 1021) along axis 1: outer * inner > CAP groups, C = 2, members 1021 apart."""
    assert 1030 * 1021 > CAP
    v = sl_above_cap_operands(rdt)
    check_sl1l2(v, 0.25, 0.75, 1, F32_BOUND['sl1l2_above_cap'] if is_f32(rdt) else 1e-12)


# ---- 5. proj_l2: every branch of ball_geom --------------------------------------------------------------
# ball_geom (csc_ball.hip), with vmax = 16 / element size:
#   V = the largest of vmax, vmax/2, ..., 1 dividing inner;  Cv = C;  G = inner / V
#   fold (inner == 1 and C % vmax == 0): V = vmax, Cv = C / vmax, G = 1
#   cols = min(G, 256);  rows = 256 / cols;  CB = ceil(G / cols)
#   rb = min(max(1, ceil(Cv / (4 rows))), max(1, 1024 / (outer CB)));  RT = ceil(ceil(Cv / rb) / rows) rows
#   RB = ceil(Cv / RT)
# (outer, C, inner) -> what it selects, worked out from the above by hand:
BALL_CASES = [
    # f32: V=4 G=75 cols=75 rows=3 (225 of 256 threads work) CB=1 RB=2;  f64: V=2 G=150 cols=150 rows=1 RB=6
    ('V4-cols75-rows3-idle-threads', (1, 24, 300), False),
    # f32, f64: V=1 G=301 cols=256 rows=1 CB=2 (the second column block has 45 of 256 columns) RB=6
    ('V1-G301-CB2', (1, 24, 301), False),
    # f32, f64: V=2 G=151 cols=151 rows=1 CB=1 RB=6 (float32: the middle vector width)
    ('V2-G151', (1, 24, 302), False),
    # f32: V=4 G=1 cols=1 rows=256 RT=1024 RB=9;  f64: V=2 G=2 cols=2 rows=128 RT=512 RB=18
    ('G1-rows256-RB9', (1, 9000, 4), False),
    # f32: fold V=4 Cv=1024 rows=256 RB=1;  f64: fold V=2 Cv=2048 RT=1024 RB=2
    ('fold-outer3-Cv1024', (3, 4096, 1), False),
    # f32: fold V=4 Cv=2050 RT=768 RB=3 (last tile 514 of 768);  f64: fold V=2 Cv=4100 RT=1024 RB=5 (last 4)
    ('fold-outer3-RB3-partial-last-tile', (3, 8200, 1), False),
    # f32, f64: inner=1 but 4097 is odd: no fold, V=1 G=1 cols=1 rows=256 RT=1024 RB=5 (last tile 1 of 1024)
    ('inner1-no-fold-RB5', (3, 4097, 1), False),
    # f32, f64: V=1 G=3 cols=3 rows=85 (255 threads), 1024 / (outer CB) = 0: the cap clamps to 1, RB=1
    ('outer1100-tile-cap-clamps-to-1', (1100, 8, 3), False),
    # f32: V=4 G=257 cols=256 rows=1 CB=2 (second block: 1 column) cap=256 RT=12 RB=250
    # f64: V=2 G=514 cols=256 CB=3 (third block: 2 columns) cap=170 RT=18 RB=167
    ('CB2-and-RB250-together', (2, 3000, 1028), True),
]


def ball_operands(shape, rdt, gamma):
    rng = np.random.RandomState([51] + list(shape))
    v = rng.randn(*shape)
    d = np.sqrt(np.sum(v ** 2, axis=1, keepdims=True))
    f = np.linspace(0.2, 1.8, d.size)
    f[np.abs(f - 1.0) < 1e-2] = 0.9           # (a plane of norm gamma is test_ball.py's edge case)
    return (v * (gamma * f.reshape(d.shape) / d)).astype(rdt)


@pytest.mark.parametrize('rdt,tol', [pytest.param(np.float64, 1e-12, id='f64'), pytest.param(np.float32, 1e-6, id='f32')])
@pytest.mark.parametrize('name,shape', [pytest.param(c[0], c[1], id=c[0], marks=[pytest.mark.gpu] if c[2] else [])
                                        for c in BALL_CASES])
def test_proj_l2_geometry(backend, name, shape, rdt, tol):
    """One case per branch of ball_geom; the planes' norms straddle gamma (0.2 ... 1.8 of it), and a
    plane inside the ball comes back bit for bit."""
    from sporco_amd import prox
    gamma = 2.5
    v = ball_operands(shape, rdt, gamma)
    d = np.sqrt(np.sum(v.astype(np.float64) ** 2, axis=1, keepdims=True))
    assert np.all(np.abs(d - gamma) > 1e-3 * gamma) and np.any(d < gamma) and np.any(d > gamma)
    got = prox.proj_l2(v, gamma, axis=1)
    assert got.dtype == rdt and got.shape == v.shape
    want = pn.proj_l2(v, gamma, axis=1)
    err = rel_l2(got, want)
    print('proj_l2 %s: rel l2 %.3e (bound %.0e)' % (name, err, tol))
    assert err < tol
    inside = np.broadcast_to(d <= gamma, v.shape)
    assert np.array_equal(got[inside], v[inside])
    # every plane on its own: its norm is now min(d, gamma).  (Each element carries the rounding of sigma
    # and of one product, a few units in the last place; tol is above ten of them in either precision.)
    dn = np.sqrt(np.sum(got.astype(np.float64) ** 2, axis=1, keepdims=True))
    assert np.all(np.abs(dn - np.minimum(d, gamma)) <= tol * gamma)


# ---- 6. rfl2norm2 ---------------------------------------------------------------------------------------
RFL_SIZES = [(1, 1), (1, 2), (5, 2), (12, 9), (12, 10), (1, 33)]
RFL_ABOVE_CAP = (259, 510, 16)


def rfl_operands(H, W, P, cdt):
    """The half spectrum of a seeded real array, by NumPy, rounded to the test dtype."""
    rng = np.random.RandomState([61, H, W, P])
    x = rng.randn(H, W) if P == 1 else rng.randn(H, W, P)
    return np.fft.rfftn(x, axes=(0, 1)).astype(cdt)


def check_rfl2norm2(H, W, P, cdt, tol):
    from sporco_amd import fft
    xf = rfl_operands(H, W, P, cdt)
    assert xf.shape[:2] == (H, W // 2 + 1)
    got = fft.rfl2norm2(xf, (H, W), axis=(0, 1))
    want = pn.rfl2norm2(xf, (H, W))
    print('rfl2norm2 (%d, %d, %d): %.17g against %.17g, relative %.3e (bound %.1e)'
          % (H, W, P, got, want, abs(got - want) / want, tol))
    assert abs(got - want) < tol * want


@pytest.mark.parametrize('cdt', CDTS)
@pytest.mark.parametrize('P', [1, 3])
@pytest.mark.parametrize('H,W', RFL_SIZES, ids=['%dx%d' % s for s in RFL_SIZES])
def test_rfl2norm2_small(backend, H, W, P, cdt):
    check_rfl2norm2(H, W, P, cdt, F32_BOUND['rfl2_small'] if is_f32(cdt) else 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize('cdt', CDTS)
def test_rfl2norm2_above_cap(backend, cdt):
    H, W, P = RFL_ABOVE_CAP
    assert H * (W // 2 + 1) * P > CAP
    check_rfl2norm2(H, W, P, cdt, F32_BOUND['rfl2_above_cap'] if is_f32(cdt) else 1e-12)


# ---- 7. the device pipelines ----------------------------------------------------------------------------
TIK_CASES = [
    pytest.param((5, 4), 0, id='5x4-npd0'),
    pytest.param((5, 4, 3), 0, id='5x4-P3-npd0'),
    pytest.param((5, 4), 3, id='5x4-npd3-padded-11x10-odd-and-even'),
    pytest.param((5, 4, 3), 3, id='5x4-P3-npd3'),
    pytest.param((3, 5), 7, id='3x5-npd7-pad-wider-than-image'),
    pytest.param((3, 5, 3), 7, id='3x5-P3-npd7-pad-wider-than-image'),
]


@pytest.mark.parametrize('rdt', RDTS)
@pytest.mark.parametrize('shape,npd', TIK_CASES)
def test_tikhonov_filter_edges(backend, shape, npd, rdt):
    from sporco_amd import signal
    from sporco_amd.device import DeviceArray
    tol = 1e-5 if is_f32(rdt) else 1e-12
    s = np.random.RandomState([71] + list(shape) + [npd]).randn(*shape).astype(rdt)
    lo, hi = pn.tikhonov_filter(s, 0.5, npd)
    sl, sh = signal.tikhonov_filter(s, 0.5, npd)
    assert sl.dtype == rdt and sh.dtype == rdt and sl.shape == shape and sh.shape == shape
    print('tikhonov_filter: low %.3e high %.3e (bound %.0e)' % (rel_l2(sl, lo), rel_l2(sh, hi), tol))
    assert rel_l2(sl, lo) < tol and rel_l2(sh, hi) < tol
    dl, dh = signal.tikhonov_filter(DeviceArray.from_host(s), 0.5, npd)
    assert isinstance(dl, DeviceArray) and isinstance(dh, DeviceArray) and dl.dtype == rdt and dl.shape == shape
    assert np.array_equal(dl.get(), sl) and np.array_equal(dh.get(), sh)


FFTCONV_ORIGINS = [None, (0, 0), (2, 1), (-1, -2), (11, 10), (-13, -10)]


@pytest.mark.parametrize('rdt', RDTS)
@pytest.mark.parametrize('origin', FFTCONV_ORIGINS, ids=['origin-%s' % (o,) for o in FFTCONV_ORIGINS])
@pytest.mark.parametrize('mirror', [False, True], ids=['small-x-large', 'large-x-small'])
def test_fftconv_edges(backend, mirror, origin, rdt):
    """(3, 3, 2, 1, 4) against (10, 9, 1, 3, 1): P > 1 and a broadcast on each of the three trailing
    axes, either operand first; origins inside, negative and beyond the image on
    either side."""
    from sporco_amd import fft
    from sporco_amd.device import DeviceArray
    tol = 1e-5 if is_f32(rdt) else 1e-12
    rng = np.random.RandomState(72)
    a, b = rng.randn(3, 3, 2, 1, 4).astype(rdt), rng.randn(10, 9, 1, 3, 1).astype(rdt)
    if mirror:
        a, b = b, a
    want = pn.fftconv(a, b, origin)
    out = fft.fftconv(a, b, origin=origin)
    assert out.dtype == rdt and out.shape == (10, 9, 2, 3, 4)
    print('fftconv: rel l2 %.3e (bound %.0e)' % (rel_l2(out, want), tol))
    assert rel_l2(out, want) < tol
    outd = fft.fftconv(DeviceArray.from_host(a), DeviceArray.from_host(b), origin=origin)
    assert isinstance(outd, DeviceArray) and outd.dtype == rdt and np.array_equal(outd.get(), out)
    if origin is None:
        assert np.array_equal(fft.fftconv(a, b, origin=(0, 0)), out)


# ---- the float32 bounds ---------------------------------------------------------------------------------
def measure_f32():
    """The float32 NumPy evaluation (sequential sums) against the float64 reference, on the very inputs
    of the tests above: the largest relative l2 error per test."""
    c64, f32 = np.complex64, np.float32
    m = {}

    def sm(K, npix, C, N):
        ah, b = sm_operands(K, npix, C, N, c64)
        return rel_l2(pn.solvedbi_sm_f32(ah, 1.0, b), pn.solvedbi_sm(ah, 1.0, b))

    def inn(K, npix, CN):
        x, y = inner_operands(K, npix, CN, c64)
        return rel_l2(pn.inner_f32(x, y), pn.inner(x, y))

    def sl(v, alpha, beta, axis):
        return rel_l2(pn.prox_sl1l2_f32(v, alpha, beta, axis), pn.prox_sl1l2(v, alpha, beta, axis))

    def rfl(H, W, P):
        xf = rfl_operands(H, W, P, c64)
        want = pn.rfl2norm2(xf, (H, W))
        return abs(pn.rfl2norm2_f32(xf, (H, W)) - want) / want

    shapes = [p.values[0] for p in SM_SHAPES]
    m['sm_small'] = max(sm(K, *s) for K in (128, 130) for s in shapes)
    m['sm_above_cap'] = max(sm(p.values[1], *p.values[2:]) for p in SM_ABOVE_CAP if p.values[1] >= 128)
    m['inner_small'] = max(inn(p.values[1], *s.values[0]) for p in INNER_FORMS for s in INNER_SHAPES)
    m['inner_above_cap'] = max(inn(*p.values[1:]) for p in INNER_ABOVE_CAP)
    x, y = inner_any_axis_operands(c64)
    m['inner_axis'] = rel_l2(pn.inner_f32(x, y, 1), pn.inner(x, y, 1))
    m['sl1l2_small'] = max(sl(sl_operands(c[0], c[1], c[2], c[3], c[4], f32, i), c[3], c[4], c[2])
                           for i, c in enumerate(SL_CASES))
    m['sl1l2_none_4096'] = sl(sl_none_operands(f32), 0.25, 16.0, None)
    v = sl_above_cap_operands(f32)
    m['sl1l2_above_cap'] = sl(v, 0.25, 0.75, 1)
    m['rfl2_small'] = max(rfl(H, W, P) for H, W in RFL_SIZES for P in (1, 3))
    m['rfl2_above_cap'] = rfl(*RFL_ABOVE_CAP)
    return m


def test_f32_bounds_are_the_measured_ones():
    """F32_MEASURED is what NumPy gives in float32 (to the two digits recorded), and every bound is four
    times that, rounded up to one significant digit."""
    m = measure_f32()
    for k in sorted(m):
        print('%-18s measured %.3e   recorded %.1e   bound %.0e' % (k, m[k], F32_MEASURED[k], F32_BOUND[k]))
    assert set(m) == set(F32_MEASURED)
    for k, e in m.items():
        assert 0.5 * F32_MEASURED[k] < e < 1.5 * F32_MEASURED[k], k      # (the window of test_ball.py)
        assert abs(F32_BOUND[k] - bound_of(F32_MEASURED[k])) < 1e-9 * F32_BOUND[k], k
