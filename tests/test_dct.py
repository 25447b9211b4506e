"""sporco_amd.fft.dctii / idctii (one real transform of the same size on a permuted array, csrc/csc_spline.h)
against the float64 NumPy statement of tests/_spline_numpy.py, which a guarded test ties to scipy.fftpack.

Tolerances.  float64: 1e-12 relative l2.  float32: the larger of 1e-5 and four times what the statement run in
float32 shows at the same shape against the float64 statement; every test measures that figure again before it
compares.  Measured on the CPU, worst over the shapes below (the GPU-only ones included): forward 1.1e-7, inverse
1.7e-7, round trip 1.9e-7, so the 1e-5 applies everywhere.
"""

import numpy as np
import pytest

from conftest import rel_l2

import _spline_numpy as sn

from sporco_amd import _lib
from sporco_amd import fft as sfft
from sporco_amd.device import DeviceArray

# (shape, axes)
SHAPES = [((2, 2), None), ((2, 3), None), ((3, 2), None), ((4, 4), None), ((5, 16), None), ((16, 5), None),
          ((7, 9), None), ((13, 17), None),                  # prime lines
          ((8, 8, 2), (0, 1)), ((8, 8, 3), (0, 1)),          # 16-byte and scalar plane access
          ((33, 12, 3, 2), (0, 1)),
          ((33,), (0,)), ((6, 10), (1,)), ((6, 3, 10), (0, 2))]
GPU_SHAPES = [((60, 131, 3), (0, 1)), ((40, 520, 8), (0, 1)), ((33, 1024), None)]
F64_TOL = 1e-12

_REF = {}


def reference(shape, axes):
    """The input and its float64 transform by the statement, computed once per shape."""
    key = (shape, axes)
    if key not in _REF:
        x = np.random.RandomState(11).randn(*shape)
        _REF[key] = (x, sn.dctii(x, axes))
    return _REF[key]


def f32_tol(shape, axes):
    x, X = reference(shape, axes)
    ef = rel_l2(sn.dctii(x.astype(np.float32), axes), X)
    ei = rel_l2(sn.idctii(X.astype(np.float32), axes), x)
    er = rel_l2(sn.idctii(sn.dctii(x.astype(np.float32), axes), axes), x)
    print('float32 statement at %s: forward %.2e inverse %.2e round trip %.2e' % (shape, ef, ei, er))
    return max(1e-5, 4.0 * ef), max(1e-5, 4.0 * ei), max(1e-5, 4.0 * er)


def check(shape, axes, dtype):
    x, X = reference(shape, axes)
    tf, ti, tr = (F64_TOL, F64_TOL, F64_TOL) if dtype == np.float64 else f32_tol(shape, axes)
    Xd = sfft.dctii(x.astype(dtype), axes)
    xd = sfft.idctii(X.astype(dtype), axes)
    rt = sfft.idctii(Xd, axes)
    errs = (rel_l2(Xd, X), rel_l2(xd, x), rel_l2(rt, x))
    print(shape, axes, np.dtype(dtype).name, 'forward %.2e inverse %.2e round trip %.2e' % errs)
    assert Xd.dtype == dtype and Xd.shape == tuple(shape) and xd.dtype == dtype and xd.shape == tuple(shape)
    assert errs[0] <= tf and errs[1] <= ti and errs[2] <= tr


def test_statement_equals_scipy():
    fftpack = pytest.importorskip('scipy.fftpack')
    for shape, axes in SHAPES + [((1, 6), None), ((6, 1), None)]:
        x, X = reference(shape, axes)
        ref = x
        for ax in (range(x.ndim) if axes is None else axes):
            ref = fftpack.dct(ref, type=2, axis=ax, norm='ortho')
        assert rel_l2(X, ref) <= 1e-12, shape
        assert rel_l2(sn.idctii(ref, axes), x) <= 1e-12, shape


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('shape,axes', SHAPES)
def test_dct_against_statement(backend, shape, axes, dtype):
    check(shape, axes, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('shape,axes', GPU_SHAPES)
def test_dct_gpu_shapes_f32(gpu_backend, shape, axes):
    check(shape, axes, np.float32)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('shape', [(2, 2), (4, 4), (5, 4), (4, 5)])
def test_every_coefficient_written_once(backend, shape, dtype):
    """The self-paired rows and columns (k1 = 0, 2 k1 = H, k2 = 0, 2 k2 = W) write fewer coefficients per thread:
    none is left out.  The output is pre-filled with NaN."""
    x, X = reference(shape, None)
    xd = DeviceArray.from_host(x.astype(dtype))
    for inverse, src, want in ((False, xd, X), (True, DeviceArray.from_host(X.astype(dtype)), x)):
        out = DeviceArray.from_host(np.full(shape, np.nan, dtype))
        assert np.all(np.isnan(out.get()))
        _lib.dct2(src, out, inverse)
        got = out.get()
        assert not np.any(np.isnan(got))
        assert rel_l2(got, want) <= (F64_TOL if dtype == np.float64 else 1e-5)


def test_device_in_device_out(backend):
    x, X = reference((8, 8, 3), (0, 1))
    xd = DeviceArray.from_host(x)
    Xd = sfft.dctii(xd, (0, 1))
    assert isinstance(Xd, DeviceArray) and np.array_equal(Xd.get(), sfft.dctii(x, (0, 1)))
    back = sfft.idctii(Xd, (0, 1))
    assert isinstance(back, DeviceArray) and rel_l2(back.get(), x) <= F64_TOL
    v = DeviceArray.from_host(reference((33,), (0,))[0])
    assert rel_l2(sfft.dctii(v, (0,)).get(), reference((33,), (0,))[1]) <= F64_TOL
    # unit axes take no place in memory: what the host path serves, the device path serves
    for shape, axes in (((1, 33), None), ((33, 1), (0, 1)), ((1, 33), (1,)), ((8, 1, 8, 3), (0, 2)), ((8, 8, 3), (1, 0))):
        xs = x.reshape(shape) if len(shape) > 2 else reference((33,), (0,))[0].reshape(shape)
        got = sfft.dctii(DeviceArray.from_host(xs), axes)
        assert isinstance(got, DeviceArray) and got.shape == shape
        assert rel_l2(got.get(), sn.dctii(xs, axes)) <= F64_TOL


def test_refusals(backend):
    x = np.zeros((4, 4, 2))
    for fn in (sfft.dctii, sfft.idctii):
        with pytest.raises(NotImplementedError):
            fn(x + 0j, (0, 1))
        with pytest.raises(NotImplementedError):
            fn(x)                                   # axes=None on three axes
        with pytest.raises(NotImplementedError):
            fn(x, (0, 1, 2))
        with pytest.raises(NotImplementedError):
            fn(x, (0, 0))
        with pytest.raises(NotImplementedError):
            fn(x.astype(np.float16), (0, 1))
        with pytest.raises(NotImplementedError):
            fn(x.astype(np.int32), (0, 1))
        with pytest.raises(NotImplementedError):
            fn(DeviceArray.from_host(x), (1, 2))
