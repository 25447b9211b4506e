"""Device proximal operators with the signatures of ``sporco.prox``.

``prox_l1`` (sporco/prox/_lp.py:144-183), ``prox_sl1l2``
(sporco/prox/_l21.py:51-88), ``proj_l2`` (sporco/prox/_lp.py:334-340) and
``proj_l1`` (sporco/prox/_l1proj.py:24-154) for real arrays and scalar parameters; inside the solvers the same arithmetic runs
fused into the ADMM / PGM epilogue kernels, where weight arrays are supported.

``prox_nuclear`` and ``norm_nuclear`` (sporco/prox/_nuclear.py) for real float32 / float64 2-D arrays whose short
side is at most 512, host arrays or :class:`sporco_amd.device.DeviceArray`: the device forms the Gram matrix of the
short side in double (csrc/csc_rpca.h), the host its eigendecomposition, the device the product.  No SVD is taken.
"""

import numpy as np

from . import _lib


def _real(v):
    v = np.asarray(v)
    if np.iscomplexobj(v):
        raise NotImplementedError("sporco_amd.prox handles real arrays only")
    if v.dtype not in (np.float32, np.float64):
        v = v.astype(np.float64)
    return np.ascontiguousarray(v)


def prox_l1(v, alpha):
    """sign(v) * max(|v| - alpha, 0); ``alpha`` a scalar or an array that broadcasts against
    ``v`` (sporco/prox/_lp.py:144-183).

    The kernel works in the precision of ``v`` and the result has ``v``'s dtype: ``alpha`` is rounded to
    that dtype first.  A float32 ``v`` with a float64 ``alpha`` array therefore gives the float32 result
    of the float32 weights, where NumPy's promotion would have returned float64."""
    v = _real(v)
    out = np.empty_like(v)
    if np.ndim(alpha) == 0:
        _lib.check(_lib.lib().sporco_amd_prox_l1(_lib.dtype_code(v.dtype), v.size, _lib._ptr(v),
                                                 float(alpha), _lib._ptr(out)))
        return out
    a = np.asarray(alpha, dtype=v.dtype)
    if a.ndim > v.ndim or np.broadcast_shapes(a.shape, v.shape) != v.shape:
        raise ValueError("alpha of shape %s does not broadcast against v of shape %s"
                         % (a.shape, v.shape))
    a = a.reshape((1,) * (v.ndim - a.ndim) + a.shape)
    if v.ndim <= 5:
        vs = [1] * (5 - v.ndim) + list(v.shape)
        as_ = [1] * (5 - v.ndim) + [na if nv > 1 else 1 for nv, na in zip(v.shape, a.shape)]
    else:           # more than five axes: expand alpha (no compact 5-D form in general)
        a = np.broadcast_to(a, v.shape)
        vs, as_ = [1, 1, 1, 1, v.size], [1, 1, 1, 1, v.size]
    i64 = _lib.ctypes.c_int64
    _lib.check(_lib.lib().sporco_amd_prox_l1w(_lib.dtype_code(v.dtype), (i64 * 5)(*vs), _lib._ptr(v),
                                              (i64 * 5)(*as_), _lib._ptr(np.ascontiguousarray(a)),
                                              _lib._ptr(out)))
    return out


def prox_sl1l2(v, alpha, beta, axis=None):
    """prox of alpha*||.||_1 + beta*||.||_2 with the l2 norm over ``axis``.

    One thread forms the sum of squares of a group, member by member, in the precision of ``v``; with
    ``axis=None`` the whole array is one group.  For float32 that is the accuracy of a sequential
    float32 sum (relative error 7e-8 on 4096 standard normal values), not that of a float64 one."""
    if np.ndim(alpha) != 0 or np.ndim(beta) != 0:
        raise NotImplementedError("array-valued parameters are handled inside the solvers only")
    v = _real(v)
    if axis is None:
        outer, C, inner = 1, v.size, 1
    else:
        if isinstance(axis, (tuple, list)):
            if len(axis) != 1:
                raise NotImplementedError("a single l2 axis is supported")
            axis = axis[0]
        axis = axis % v.ndim
        outer = int(np.prod(v.shape[:axis])) if axis > 0 else 1
        C = v.shape[axis]
        inner = int(np.prod(v.shape[axis + 1:])) if axis + 1 < v.ndim else 1
    out = np.empty_like(v)
    _lib.check(_lib.lib().sporco_amd_prox_sl1l2(_lib.dtype_code(v.dtype), outer, C, inner,
                                                _lib._ptr(v), float(alpha), float(beta),
                                                _lib._ptr(out)))
    return out


def prox_l2(v, alpha, axis=None):
    """v/||v|| * max(0, ||v|| - alpha): the alpha_1 = 0 case of :func:`prox_sl1l2`."""
    return prox_sl1l2(v, 0.0, alpha, axis)


def proj_l2(v, gamma, axis=None):
    """Projection onto the l2 ball of radius ``gamma``, the norm taken over ``axis``: None (the whole
    array), an int, or a tuple of adjacent axes (sporco/prox/_lp.py:334-340).  A vector of norm 0 is
    returned as it is."""
    if np.ndim(gamma) != 0:
        raise NotImplementedError("array-valued parameters are handled inside the solvers only")
    v = _real(v)
    if axis is None:
        outer, C, inner = 1, v.size, 1
    else:
        if isinstance(axis, (int, np.integer)):
            axes = (int(axis) % v.ndim,)
        elif isinstance(axis, (tuple, list)) and len(axis) > 0 and \
                all(isinstance(a, (int, np.integer)) for a in axis):
            axes = tuple(sorted(int(a) % v.ndim for a in axis))
        else:
            raise NotImplementedError("axis must be None, an int or a tuple of adjacent axes")
        if axes != tuple(range(axes[0], axes[0] + len(axes))):
            raise NotImplementedError("the l2 axes must be adjacent: %s" % (axis,))
        outer = int(np.prod(v.shape[:axes[0]], dtype=np.int64))
        C = int(np.prod(v.shape[axes[0]:axes[-1] + 1], dtype=np.int64))
        inner = int(np.prod(v.shape[axes[-1] + 1:], dtype=np.int64))
    out = np.empty_like(v)
    if v.size:
        _lib.check(_lib.lib().sporco_amd_proj_l2(_lib.dtype_code(v.dtype), outer, C, inner, _lib._ptr(v),
                                                 float(gamma), _lib._ptr(out)))
    return out


def proj_l1(v, gamma, axis=None):
    """Euclidean projection onto the l1 ball of radius ``gamma``, the norm taken over ``axis``: None
    (the whole array), an int, or a tuple of axes (sporco/prox/_l1proj.py:24-154, without ``method``:
    the threshold comes from streaming reductions on the device, csrc/csc_projl1.h).  A vector inside
    its ball is returned as it is.  When the axes that are NOT summed over are a single axis the array
    is projected in place of its layout; otherwise those axes are moved to the front on the host."""
    if np.ndim(gamma) != 0:
        raise NotImplementedError("array-valued parameters are handled inside the solvers only")
    if not float(gamma) >= 0.0:
        raise ValueError("gamma must not be negative")
    v = _real(v)
    if v.size == 0:
        return v
    if axis is None:
        axes = tuple(range(v.ndim))
    elif isinstance(axis, (int, np.integer)):
        axes = (int(axis) % v.ndim,)
    elif isinstance(axis, (tuple, list)) and len(axis) > 0 and \
            all(isinstance(a, (int, np.integer)) for a in axis):
        axes = tuple(sorted(set(int(a) % v.ndim for a in axis)))
    else:
        raise NotImplementedError("axis must be None, an int or a tuple of ints")
    rest = tuple(k for k in range(v.ndim) if k not in axes)
    moved = None
    if len(rest) == 0:
        outer, P, inner = 1, 1, v.size
        w = v
    elif len(rest) == 1:
        k = rest[0]
        outer = int(np.prod(v.shape[:k], dtype=np.int64))
        P = int(v.shape[k])
        inner = int(np.prod(v.shape[k + 1:], dtype=np.int64))
        w = v
    else:
        moved = rest + axes
        w = np.ascontiguousarray(np.transpose(v, moved))
        P = int(np.prod([v.shape[k] for k in rest], dtype=np.int64))
        outer, inner = 1, w.size // P
    out = np.empty_like(w)
    _lib.check(_lib.lib().sporco_amd_proj_l1(_lib.dtype_code(w.dtype), outer, P, inner, _lib._ptr(w),
                                             float(gamma), _lib._ptr(out)))
    if moved is not None:
        out = np.ascontiguousarray(np.transpose(out, np.argsort(moved)))
    return out


def norm_l1(x, axis=None):
    return np.sum(np.abs(x), axis=axis, keepdims=axis is not None)


def svt_matrix(G, alpha):
    """The host step of singular value thresholding.  ``G``: the (n, n) Gram matrix of the short side of ``V``, ``G
    = W diag(sigma^2) W^T``.  Returns ``(T, sigma, ss)`` in float64, singular values descending: ``ss = max(0, sigma
    - alpha)`` and ``T = W diag(ss / sigma) W^T``, so that ``prox_nuclear(V, alpha) = V T`` (or ``T V`` for a wide
    ``V``).  Directions with ``sigma <= alpha`` get the factor 0, and the factor is continuous there."""
    G = np.asarray(G, dtype=np.float64)
    w, W = np.linalg.eigh(0.5 * (G + G.T))
    sigma = np.sqrt(np.maximum(w, 0.0))[::-1]
    W = W[:, ::-1]
    ss = np.maximum(0.0, sigma - float(alpha))
    f = np.zeros_like(sigma)
    nz = sigma > 0.0
    f[nz] = ss[nz] / sigma[nz]
    return (W * f).dot(W.T), sigma, ss


def _nuclear_handle(v, name):
    """What is refused of the argument, then a handle with the argument as its signal."""
    from .device import is_device_array
    if not is_device_array(v):
        v = np.asarray(v)
        if np.iscomplexobj(v) or v.dtype not in (np.float32, np.float64):
            raise TypeError("%s works on real float32 or float64 arrays, not %s" % (name, v.dtype))
    if len(v.shape) != 2:
        raise ValueError("%s takes an array of two axes" % name)
    if min(v.shape) < 1:
        raise ValueError("%s: empty array" % name)
    if min(v.shape) > _lib.RPCA_MAX_DIM:
        raise ValueError("%s: an array of shape %s; the kernels serve a short side of up to %d"
                         % (name, tuple(v.shape), _lib.RPCA_MAX_DIM))
    h = _lib.RpcaHandle(v.shape[0], v.shape[1], v.dtype)
    h.set_signal(v if is_device_array(v) else np.ascontiguousarray(v))
    return h, is_device_array(v)


def norm_nuclear(x):
    """The nuclear norm of a 2-D array, the sum of its singular values (sporco/prox/_nuclear.py:21-41): the square
    roots of the eigenvalues of the Gram matrix of its short side, which the device forms in double."""
    h, _ = _nuclear_handle(x, 'norm_nuclear')
    try:
        G = h.gram(_lib.RPCA_V_S)
    finally:
        h.close()
    return float(np.sum(np.sqrt(np.maximum(np.linalg.eigvalsh(0.5 * (G + G.T)), 0.0))))


def prox_nuclear(v, alpha):
    """Singular value thresholding (sporco/prox/_nuclear.py:45-67): returns ``(X, ss)``, ``X`` of the kind and dtype
    of ``v`` (a returned :class:`sporco_amd.device.DeviceArray` keeps its short-lived handle alive) and ``ss`` the
    thresholded singular values, float64, descending, of length ``min(v.shape)``."""
    if np.ndim(alpha) != 0 or not float(alpha) >= 0.0:
        raise ValueError("alpha is a scalar that is not negative")
    h, on_device = _nuclear_handle(v, 'prox_nuclear')
    try:
        T, _, ss = svt_matrix(h.gram(_lib.RPCA_V_S), alpha)
        h.apply(T)
        if on_device:
            return h.device_view(_lib.RPCA_X), ss
        x = h.download(_lib.RPCA_X)
    except Exception:
        h.close()
        raise
    h.close()
    return x, ss
