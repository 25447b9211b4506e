"""The generic line FFTs (fft.hip: fft_lines_kernel in its c2c / r2c / c2r, packed / unpacked forms,
pick_cfg, launch_lines) through the public sporco_amd.fft.rfftn / irfftn / rfl2norm2, against
numpy.fft on the input cast to float64: every radix pass (8, 4, 2, 3, 5, 7 and the direct pass of the
primes from 11), every tile width pick_cfg chooses, the refusal beyond the LDS budget, the batch
edges (packed and unpacked columns, tail workgroups, batches below the tile width), the c2r rule for
the DC / Nyquist bins, degenerate lengths, and inputs whose exact spectra are known.

Every comparison reports two figures: rel_l2, and the largest absolute element error over the
largest reference magnitude ("smax") -- one wrong bin out of thousands moves the norm by little and
smax by its full size.

Bounds
------
Lengths whose prime factors are all <= 7 keep the bars of test_primitives.py on both figures:
1e-14 (float64) / 2e-6 (float32) for lengths <= 96, 1e-12 / 1e-5 beyond.  The same bar serves smax:
the rounding error of a transform of noise is itself noise-like over the elements, so max|err| and
max|ref| sit the same few standard deviations above their root mean squares and smax ~ rel_l2; a
single wrong bin of relative size d gives smax ~ d / 4.

Two groups had no bar and were measured against the float64 NumPy reference on an MI355X, at
commit c5e651b with this file added (the line kernels are those of c5e651b).  Each figure is the
maximum over every case of its group, forward and inverse; each bound is 4 x that maximum, to allow
for the spread over seeds and compilers, and lies below the caps 1e-10 (float64) / 1e-4 (float32)
of BASELINE.md and test_cols_sm.py:

    group                                       measured rel_l2 / smax     bound (4 x) rel_l2 / smax
    direct pass (a prime factor >= 11), float64  6.536e-16 / 8.842e-16      2.614e-15 / 3.537e-15
    direct pass, float32                         1.292e-07 / 2.162e-07      5.168e-07 / 8.648e-07
    lines of the tile-shape sweep, float64       5.962e-16 / 9.319e-16      2.385e-15 / 3.728e-15
    lines of the tile-shape sweep, float32       1.624e-07 / 2.086e-07      6.496e-07 / 8.344e-07

(the direct-pass group: the lengths 11, 13, 17, 22, 26, 44, 88, 104, 121, 143, 169 of the sweep and
the 35 x 17 batch cases; the CPU simulator, which runs its lengths <= 64, measured no more: 4.921e-16 /
8.337e-16 and 1.275e-07 / 1.897e-07.  The one length of the tile-shape sweep with a factor 11, 616,
takes the larger of the two bounds.)

rfl2norm2 keeps the bars test_primitives.py puts on it (1e-11 float64, 1e-5 float32: the sum itself is
accumulated in double).  The structured inputs of float64 have exact unit-magnitude answers and the
absolute bound 1e-13.
"""

import numpy as np
import pytest

F32, F64 = np.float32, np.float64
DTYPES = [pytest.param(F64, id='f64'), pytest.param(F32, id='f32')]

# measured groups: (rel_l2, smax) bounds, see the table above
MEASURED_DIRECT = {F64: (6.536e-16, 8.842e-16), F32: (1.292e-07, 2.162e-07)}
MEASURED_LONG = {F64: (5.962e-16, 9.319e-16), F32: (1.624e-07, 2.086e-07)}
BOUND_DIRECT = {dt: tuple(4 * v for v in m) for dt, m in MEASURED_DIRECT.items()}
BOUND_LONG = {dt: tuple(4 * v for v in m) for dt, m in MEASURED_LONG.items()}
CAP = {F64: 1e-10, F32: 1e-4}
assert all(max(b[dt]) < CAP[dt] for b in (BOUND_DIRECT, BOUND_LONG) for dt in CAP)


def largest_prime(n):
    p, big = 2, 1
    while n > 1:
        while n % p == 0:
            big, n = p, n // p
        p += 1
    return big


def bounds(lengths, dt):
    """(rel_l2, smax) bars of a transform over the given line lengths."""
    if max(largest_prime(n) for n in lengths) >= 11:
        return BOUND_DIRECT[dt]
    if max(lengths) <= 96:
        return (1e-14, 1e-14) if dt == F64 else (2e-6, 2e-6)
    return (1e-12, 1e-12) if dt == F64 else (1e-5, 1e-5)


def errors(a, ref):
    a = np.asarray(a, dtype=np.complex128 if np.iscomplexobj(ref) else np.float64)
    assert a.shape == ref.shape
    d = np.abs(a - ref)
    return float(np.linalg.norm(d.ravel()) / np.linalg.norm(ref.ravel())), float(d.max() / np.abs(ref).max())


def cdtype(dt):
    return np.complex64 if dt == F32 else np.complex128


def check_pair(tag, shape, dt, seed, bnd):
    """Forward transform of noise of the given shape, and the inverse transform of NumPy's spectrum
    of it, each against NumPy on the very input (cast to float64) the device got."""
    from sporco_amd import fft
    x = np.random.RandomState(seed).randn(*shape).astype(dt)
    ref = np.fft.rfftn(x.astype(F64), axes=(0, 1))
    X = fft.rfftn(x, axes=(0, 1))
    assert X.dtype == cdtype(dt)
    ef = errors(X, ref)
    xf = ref.astype(cdtype(dt))
    xr = fft.irfftn(xf, shape[:2], axes=(0, 1))
    assert xr.dtype == dt
    ei = errors(xr, np.fft.irfftn(xf.astype(np.complex128), shape[:2], axes=(0, 1)))
    print('fft_lines %s %s %s fwd rel_l2 %.3e smax %.3e  inv rel_l2 %.3e smax %.3e'
          % (tag, shape, np.dtype(dt).name, ef[0], ef[1], ei[0], ei[1]))
    assert ef[0] < bnd[0] and ef[1] < bnd[1], ('forward', ef, bnd)
    assert ei[0] < bnd[0] and ei[1] < bnd[1], ('inverse', ei, bnd)
    return ef, ei


# ---------------------------------------------------------------------------------------------
# a. length sweep on each axis
# ---------------------------------------------------------------------------------------------
LENGTHS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13, 16, 17, 22, 25, 26, 27, 32, 44, 49, 64, 88, 104, 121, 125,
           128, 143, 169, 243, 343]


def _len_param(n):      # (the CPU simulator stays at n <= 64)
    return pytest.param(n, marks=pytest.mark.gpu) if n > 64 else n


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('n', [_len_param(n) for n in LENGTHS])
@pytest.mark.parametrize('axis', [0, 1])
def test_length_sweep(backend, axis, n, dt):
    """(n, 6, P): the c2c column kernel at length n; (6, n, P): the r2c / c2r row kernels; P = 2
    (packed pair) and P = 3 (one real column per complex line)."""
    for P in (2, 3):
        shape = (n, 6, P) if axis == 0 else (6, n, P)
        check_pair('sweep', shape, dt, 1000 * axis + n + P, bounds((n, 6), dt))


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('shape', [(1, 12), (12, 1), (1, 1), (2, 1), (1, 2)])
def test_unit_axes(backend, shape, dt):
    for P in (2, 3):
        check_pair('unit', shape + (P,), dt, 7 + P, bounds(shape, dt))
    # (no batch axis at all)
    check_pair('unit', shape, dt, 5, bounds(shape, dt))


# ---------------------------------------------------------------------------------------------
# b. tile-shape sweep: a length on each side of every breakpoint of pick_cfg
# ---------------------------------------------------------------------------------------------
LDS_BUDGET = 160 * 1024
# columns per workgroup -> lengths (all with prime factors <= 7, so the direct pass stays out,
# except 616 = 8 * 7 * 11: the last 16-column length below the 620 / 621 breakpoint that is a
# multiple of 8; 600 stands next to it as the smooth one)
TILE_LENGTHS = {
    F32: {16: [180, 512, 600, 616], 8: [192, 500, 625, 1200], 4: [1215, 2268], 2: [2304, 4096],
          1: [4116, 6804]},
    F64: {8: [600], 4: [625, 1134], 2: [1152, 2048], 1: [2058, 3402]},
}


def pick_cols(n, ncols, dt):
    """The columns per workgroup pick_cfg (fft.hip) gives n-point lines of a batch of ncols
    (complex) columns; None where it refuses."""
    esz = 8 if dt == F32 else 16

    def lds(c):
        return (2 * n * c + n) * esz
    cols = 128 // esz
    while cols > 1 and lds(cols) > LDS_BUDGET:
        cols >>= 1
    if lds(cols) > LDS_BUDGET:
        return None
    while cols > 1 and cols // 2 >= ncols:
        cols >>= 1
    if dt == F32 and n < 512 and cols == 16 and lds(cols) > 48 * 1024:
        cols = 8
    return cols


def test_tile_lengths_cover_every_width():
    """The table lists, for both dtypes, every width pick_cfg can choose, each length under the
    width the rule gives it, and the lengths sit on both sides of every breakpoint."""
    for dt, widths in ((F32, (16, 8, 4, 2, 1)), (F64, (8, 4, 2, 1))):
        assert sorted(TILE_LENGTHS[dt]) == sorted(widths)
        for w, ns in TILE_LENGTHS[dt].items():
            for n in ns:
                assert pick_cols(n, 1 << 20, dt) == w, (n, w)
    # the breakpoints themselves
    for lo, w_lo, w_hi in ((186, 16, 8), (511, 8, 16), (620, 16, 8), (1204, 8, 4), (2275, 4, 2), (4096, 2, 1)):
        assert (pick_cols(lo, 1 << 20, F32), pick_cols(lo + 1, 1 << 20, F32)) == (w_lo, w_hi), lo
    for lo, w_lo, w_hi in ((602, 8, 4), (1137, 4, 2), (2048, 2, 1)):
        assert (pick_cols(lo, 1 << 20, F64), pick_cols(lo + 1, 1 << 20, F64)) == (w_lo, w_hi), lo
    assert pick_cols(6826, 4, F32) == 1 and pick_cols(6827, 4, F32) is None
    assert pick_cols(3413, 4, F64) == 1 and pick_cols(3414, 4, F64) is None
    # what the shapes of the sweep below launch: the column kernel of the (n, 4, 3) case has 9 columns
    # and runs every width in full, that of (n, 4, 2) has 6 (a 16-column tile halved for the batch);
    # the row kernels of (4, n, P) run P = 2 as one packed column and P = 3 as three of a 4-wide tile
    for dt in (F32, F64):
        seen = {pick_cols(n, 3 * 3, dt) for ns in TILE_LENGTHS[dt].values() for n in ns}
        assert seen == set(TILE_LENGTHS[dt]), seen


@pytest.mark.gpu
@pytest.mark.parametrize('axis', [0, 1])
@pytest.mark.parametrize('dt,n', [pytest.param(dt, n, id='%s-%d' % (np.dtype(dt).name, n))
                                  for dt in (F32, F64) for w in TILE_LENGTHS[dt] for n in TILE_LENGTHS[dt][w]])
def test_tile_shape_sweep(gpu_backend, dt, n, axis):
    for P in (2, 3):
        shape = (n, 4, P) if axis == 0 else (4, n, P)
        check_pair('tile', shape, dt, n + P, BOUND_LONG[dt] if largest_prime(n) < 11 else
                   tuple(max(a, b) for a, b in zip(BOUND_LONG[dt], BOUND_DIRECT[dt])))


# ---------------------------------------------------------------------------------------------
# c. refusal beyond the LDS budget: a host-side argument check, made before any launch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt,n', [pytest.param(F32, 6860, id='f32-6860'), pytest.param(F64, 3430, id='f64-3430')])
@pytest.mark.parametrize('axis', [0, 1])
def test_refusal_beyond_the_lds_budget(backend, dt, n, axis):
    from sporco_amd import fft, _lib
    assert pick_cols(n, 4, dt) is None
    shape = (n, 2, 2) if axis == 0 else (2, n, 2)
    x = np.random.RandomState(n).randn(*shape).astype(dt)
    with pytest.raises(_lib.BackendError, match='too large'):
        fft.rfftn(x, axes=(0, 1))
    xf = np.zeros((shape[0], shape[1] // 2 + 1, 2), dtype=cdtype(dt))
    with pytest.raises(_lib.BackendError, match='too large'):
        fft.irfftn(xf, shape[:2], axes=(0, 1))
    # the process is as good as before
    check_pair('after-refusal', (12, 10, 2), dt, 3, bounds((12, 10), dt))


# ---------------------------------------------------------------------------------------------
# d. batch edges
# ---------------------------------------------------------------------------------------------
BATCHES = {1: (1, 1, 1), 2: (1, 2, 1), 3: (3, 1, 1), 5: (1, 1, 5), 15: (3, 1, 5), 16: (2, 2, 4), 17: (1, 17, 1),
           31: (1, 1, 31), 33: (3, 1, 11), 34: (1, 2, 17), 66: (2, 3, 11)}


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('P', sorted(BATCHES))
@pytest.mark.parametrize('hw', [(24, 20), (35, 17)])
def test_batch_edges(backend, hw, P, dt):
    """Even batches run two columns per complex line, odd ones one; the batches leave tail workgroups
    of 1 and of cols - 1 columns, fill one workgroup or several, and fall below the tile width (the
    tile is halved until it fits).  Flat, and as (C, N, K) factors: the flattening of fft.py."""
    assert int(np.prod(BATCHES[P])) == P
    bnd = bounds(hw, dt)
    check_pair('batch', hw + (P,), dt, P, bnd)
    check_pair('batch', hw + BATCHES[P], dt, P, bnd)


# ---------------------------------------------------------------------------------------------
# e. irfftn of a spectrum that is not the spectrum of a real array
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('P', [2, 3])
@pytest.mark.parametrize('hw', [(12, 9), (12, 10), (9, 12), (1, 8)])
def test_irfftn_of_non_hermitian_input(backend, hw, P, dt):
    """The c2r load drops the imaginary parts of the DC bin and, for an even length, of the Nyquist bin
    of every row, as numpy.fft.irfft does (fft.h fft_c2r)."""
    from sporco_amd import fft
    H, W = hw
    rng = np.random.RandomState(H * W + P)
    a = (rng.randn(H, W // 2 + 1, P) + 1j * rng.randn(H, W // 2 + 1, P)).astype(cdtype(dt))
    a64 = a.astype(np.complex128)
    edges = [0] + ([W // 2] if W % 2 == 0 else [])
    assert np.abs(a64[:, edges].imag).min() > 0
    ref = np.fft.irfftn(a64, hw, axes=(0, 1))
    # NumPy's own rule, confirmed rather than assumed.  The transform along W comes last, so the
    # imaginary parts it ignores are those of the DC / Nyquist columns AFTER the transform along H
    # (for H = 1 they are the input's own): zeroing them there leaves NumPy's result as it is
    t = np.fft.ifft(a64, axis=0)
    assert np.abs(t[:, edges].imag).min() > 1e-3 * np.abs(t).max()
    t0 = t.copy()
    t0[:, edges] = t0[:, edges].real
    assert np.abs(np.fft.irfft(t0, W, axis=1) - ref).max() <= 1e-14 * np.abs(ref).max()
    if H == 1:
        a0 = a64.copy()
        a0[:, edges] = a0[:, edges].real
        assert np.abs(np.fft.irfftn(a0, hw, axes=(0, 1)) - ref).max() <= 1e-14 * np.abs(ref).max()
    r = fft.irfftn(a, hw, axes=(0, 1))
    e = errors(r, ref)
    print('fft_lines nonherm %s P=%d %s rel_l2 %.3e smax %.3e' % (hw, P, np.dtype(dt).name, e[0], e[1]))
    bnd = bounds(hw, dt)
    assert e[0] < bnd[0] and e[1] < bnd[1], (e, bnd)


# ---------------------------------------------------------------------------------------------
# f. structured inputs with exact spectra (float64)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(49, 44), (26, 27)])
def test_impulses(backend, hw):
    """A unit impulse at position p of one axis has the spectrum exp(-2 pi i k p / n) along it, constant
    along the other: every twiddle index of the direct pass (11, 13) and of the 7-, 4-, 3- and 2-point
    butterflies, one position at a time.  The batch axis carries the positions."""
    from sporco_amd import fft
    H, W = hw
    Wf = W // 2 + 1
    x = np.zeros((H, W, H))
    x[np.arange(H), 0, np.arange(H)] = 1.0
    k, p = np.arange(H)[:, None, None], np.arange(H)[None, None, :]
    e = np.exp(-2j * np.pi * ((k * p) % H) / H) * np.ones((1, Wf, 1))
    X = fft.rfftn(x, axes=(0, 1))
    print('fft_lines impulse H %s max abs err %.3e' % (hw, np.abs(X - e).max()))
    assert np.abs(X - e).max() < 1e-13
    assert np.abs(fft.irfftn(e, hw, axes=(0, 1)) - x).max() < 1e-13
    x = np.zeros((H, W, W))
    x[0, np.arange(W), np.arange(W)] = 1.0
    l, p = np.arange(Wf)[None, :, None], np.arange(W)[None, None, :]
    e = np.exp(-2j * np.pi * ((l * p) % W) / W) * np.ones((H, 1, 1))
    X = fft.rfftn(x, axes=(0, 1))
    print('fft_lines impulse W %s max abs err %.3e' % (hw, np.abs(X - e).max()))
    assert np.abs(X - e).max() < 1e-13
    assert np.abs(fft.irfftn(e, hw, axes=(0, 1)) - x).max() < 1e-13


@pytest.mark.parametrize('hw', [(49, 44), (26, 27)])
def test_single_exponentials(backend, hw):
    """One wave per batch column, scaled to a unit spectral line: cos(2 pi (k0 h / H + l0 w / W)) has
    the spectrum H W / 2 at (k0, l0) and at (-k0, -l0); swept over every k0 (at l0 = 1) and every l0 of
    the half spectrum (at k0 = 1) -- forward, and the inverse of the single line."""
    from sporco_amd import fft
    H, W = hw
    Wf = W // 2 + 1
    bins = [(k0, 1) for k0 in range(H)] + [(1, l0) for l0 in range(Wf)]
    h, w = np.arange(H)[:, None], np.arange(W)[None, :]
    x = np.zeros((H, W, len(bins)))
    E = np.zeros((H, Wf, len(bins)), dtype=np.complex128)
    for i, (k0, l0) in enumerate(bins):
        # (the phase reduced exactly in integers before it meets pi)
        ph = (k0 * h * W + l0 * w * H) % (H * W)
        x[:, :, i] = np.cos(2 * np.pi * ph / (H * W)) * (2.0 / (H * W))
        E[k0, l0, i] += 1.0
        if (-l0) % W < Wf:
            E[(-k0) % H, (-l0) % W, i] += 1.0
    X = fft.rfftn(x, axes=(0, 1))
    print('fft_lines exponential fwd %s max abs err %.3e' % (hw, np.abs(X - E).max()))
    assert np.abs(X - E).max() < 1e-13
    # inverse of ONE line at (k0, l0): cos(...) c / (H W), c = 1 on the DC / Nyquist columns (the real
    # part is what c2r keeps of them), else 2
    S = np.zeros_like(E)
    xe = np.zeros_like(x)
    for i, (k0, l0) in enumerate(bins):
        c = 1.0 if (l0 == 0 or 2 * l0 == W) else 2.0
        S[k0, l0, i] = (H * W) / c
        ph = (k0 * h * W + l0 * w * H) % (H * W)
        xe[:, :, i] = np.cos(2 * np.pi * ph / (H * W))
    xr = fft.irfftn(S, hw, axes=(0, 1))
    print('fft_lines exponential inv %s max abs err %.3e' % (hw, np.abs(xr - xe).max()))
    assert np.abs(xr - xe).max() < 1e-13


# ---------------------------------------------------------------------------------------------
# g. rfl2norm2
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('P', [1, 3, 4])
@pytest.mark.parametrize('hw', [(11, 13), (13, 22), (1, 9), (8, 1), (6, 2)])
def test_rfl2norm2(backend, hw, P, dt):
    from sporco_amd import fft
    x = np.random.RandomState(sum(hw) + P).randn(*(hw + (P,))).astype(dt)
    got = fft.rfl2norm2(fft.rfftn(x, axes=(0, 1)), x.shape, axis=(0, 1))
    ref = float(np.sum(x.astype(F64) ** 2))
    print('fft_lines rfl2norm2 %s P=%d %s rel err %.3e' % (hw, P, np.dtype(dt).name, abs(got - ref) / ref))
    assert abs(got - ref) < (1e-11 if dt == F64 else 1e-5) * ref
