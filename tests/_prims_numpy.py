"""TEST INFRASTRUCTURE ONLY: float64 NumPy references of the stateless primitives (sporco_amd.linalg /
prox / fft / signal), written from the definitions of the operations, for tests/test_primitives_edges.py.
Nothing here comes from the library under test or from the reference project;
test_primitives_edges.py pins these expressions to the reference's recorded outputs
(tests/golden/primitives.npz, signal_prims.npz) before anything is compared with them.

The ``*_f32`` functions evaluate the same expressions in NumPy float32 with every sum taken
sequentially (``np.add.accumulate``): the measurement from which the float32 bounds of
test_primitives_edges.py are derived.  They are never compared with the library.
"""

import numpy as np


def _c128(x):
    return np.asarray(x).astype(np.complex128)


def _f64(x):
    return np.asarray(x).astype(np.float64)


def seqsum(x, axis):
    """Sum along ``axis`` (kept) in x's own dtype, strictly left to right."""
    return np.take(np.add.accumulate(x, axis=axis, dtype=x.dtype), [-1], axis=axis)


# ---- linalg ----------------------------------------------------------------------------------------------
def inner(x, y, axis=-1):
    return np.sum(_c128(x) * _c128(y), axis=axis, keepdims=True)


def inner_f32(x, y, axis=-1):
    x, y = np.broadcast_arrays(np.asarray(x, dtype=np.complex64), np.asarray(y, dtype=np.complex64))
    return seqsum(x * y, axis)


def solvedbi_sm(ah, rho, b, axis=-1):
    """x = (b - a (a^H b) / (rho + a^H a)) / rho with a = conj(ah): the solution of
    (rho I + a a^H) x = b by the Sherman-Morrison formula."""
    ah, b = _c128(ah), _c128(b)
    a = np.conj(ah)
    return (b - a * (np.sum(ah * b, axis=axis, keepdims=True) /
                     (rho + np.sum(ah * a, axis=axis, keepdims=True)))) / rho


def solvedbi_sm_f32(ah, rho, b, axis=-1):
    ah, b = np.asarray(ah, dtype=np.complex64), np.asarray(b, dtype=np.complex64)
    a, rho = np.conj(ah), np.float32(rho)
    ahb = seqsum(np.broadcast_to(ah, b.shape) * b, axis)
    x = (b - a * (ahb / (rho + seqsum(ah * a, axis)))) / rho
    assert x.dtype == np.complex64
    return x


def sm_residual(ah, rho, x, axis=-1):
    """(rho I + a a^H) x."""
    ah, x = _c128(ah), _c128(x)
    return rho * x + np.conj(ah) * np.sum(ah * x, axis=axis, keepdims=True)


def solvedbi_sm_c(ah, a, rho, axis=-1):
    ah, a = _c128(ah), _c128(a)
    return ah / (np.sum(ah * a, axis=axis, keepdims=True) + rho)


# ---- prox ------------------------------------------------------------------------------------------------
def prox_l1(v, alpha):
    """sign(v) max(|v| - alpha, 0) in v's own dtype (the operation is exact up to the one rounding of
    the subtraction, so it is compared bit for bit)."""
    v = np.asarray(v)
    alpha = np.asarray(alpha, dtype=v.dtype)
    out = np.sign(v) * np.maximum(np.abs(v) - alpha, v.dtype.type(0))
    assert out.dtype == v.dtype
    return out


def _group_axes(v, axis):
    if axis is None:
        return tuple(range(v.ndim))
    return tuple(axis) if isinstance(axis, (tuple, list)) else (axis,)


def group_norm(v, alpha, axis):
    """The l2 norm over ``axis`` of the soft-thresholded array (kept axes), float64."""
    v = _f64(v)
    s = np.sign(v) * np.maximum(np.abs(v) - alpha, 0.0)
    return np.sqrt(np.sum(s * s, axis=_group_axes(v, axis), keepdims=True))


def prox_sl1l2(v, alpha, beta, axis=None):
    """Soft threshold by alpha, then each group (the l2 norm over ``axis``) scaled by
    max(0, 1 - beta / norm); a group of norm zero stays zero."""
    v = _f64(v)
    s = np.sign(v) * np.maximum(np.abs(v) - alpha, 0.0)
    n = np.sqrt(np.sum(s * s, axis=_group_axes(v, axis), keepdims=True))
    fac = np.where(n > 0, np.maximum(0.0, 1.0 - beta / np.where(n > 0, n, 1.0)), 0.0)
    return fac * s


def prox_sl1l2_f32(v, alpha, beta, axis=None):
    v = np.asarray(v, dtype=np.float32)
    alpha, beta, one, zero = np.float32(alpha), np.float32(beta), np.float32(1), np.float32(0)
    s = np.sign(v) * np.maximum(np.abs(v) - alpha, zero)
    if axis is None:
        n = np.sqrt(seqsum((s * s).ravel(), 0)).reshape((1,) * v.ndim)
    else:
        (ax,) = _group_axes(v, axis)
        n = np.sqrt(seqsum(s * s, ax))
    fac = np.where(n > 0, np.maximum(zero, one - beta / np.where(n > 0, n, one)), zero)
    out = fac * s
    assert out.dtype == np.float32
    return out


def proj_l2(v, gamma, axis=None):
    """Projection of each group (the l2 norm over ``axis``) onto the ball of radius gamma."""
    v = _f64(v)
    d = np.sqrt(np.sum(v * v, axis=_group_axes(v, axis), keepdims=True))
    return np.where(d <= gamma, v, gamma * v / np.where(d == 0, 1.0, d))


# ---- fft / signal ---------------------------------------------------------------------------------------
def rfl2norm2(xf, s):
    """The squared l2 norm of the real array whose half spectrum over axes (0, 1) is ``xf``."""
    return float(np.sum(np.fft.irfftn(_c128(xf), s, axes=(0, 1)) ** 2))


def rfl2norm2_f32(xf, s):
    x = np.fft.irfftn(np.asarray(xf, dtype=np.complex64), s, axes=(0, 1)).astype(np.float32)
    return float(seqsum((x * x).ravel(), 0)[0])


def tikhonov_filter(s, lmbda, npd):
    """Symmetric padding by npd, division of the spectrum by 1 + lmbda (|G_h|^2 + |G_w|^2) with G the
    DFT of the two-tap difference along each axis, inverse transform, crop; returns (low, high)."""
    s = _f64(s)
    H, W = s.shape[:2]
    tail = (1,) * (s.ndim - 2)
    sp = np.pad(s, ((npd, npd), (npd, npd)) + ((0, 0),) * (s.ndim - 2), mode='symmetric')
    Hp, Wp = sp.shape[:2]
    gh = np.abs(1.0 - np.exp(-2j * np.pi * np.arange(Hp) / Hp)) ** 2
    gw = np.abs(1.0 - np.exp(-2j * np.pi * np.arange(Wp // 2 + 1) / Wp)) ** 2
    A = 1.0 + lmbda * (gh.reshape((Hp, 1) + tail) + gw.reshape((1, Wp // 2 + 1) + tail))
    lo = np.fft.irfftn(np.fft.rfftn(sp, axes=(0, 1)) / A, (Hp, Wp), axes=(0, 1))
    lo = lo[npd:npd + H, npd:npd + W]
    return lo, s - lo


def fftconv(a, b, origin=None):
    """Circular convolution over axes (0, 1) at the larger of the two sizes, the trailing axes
    broadcasting; ``origin`` is the index of the result that moves to (0, 0)."""
    a, b = _f64(a), _f64(b)
    nd = max(a.ndim, b.ndim)
    a = a.reshape(a.shape + (1,) * (nd - a.ndim))
    b = b.reshape(b.shape + (1,) * (nd - b.ndim))
    s = (max(a.shape[0], b.shape[0]), max(a.shape[1], b.shape[1]))
    ab = np.fft.irfftn(np.fft.rfftn(a, s, axes=(0, 1)) * np.fft.rfftn(b, s, axes=(0, 1)), s, axes=(0, 1))
    if origin is not None:
        ab = np.roll(ab, (-int(origin[0]), -int(origin[1])), axis=(0, 1))
    return ab
