"""What ``admm.tvl2.TVL2Denoise`` and ``admm.tvl1.TVL1Denoise`` share: the geometry checks, the option tree,
the device handle and its arrays (``Y`` and ``U`` in ``NBLK`` blocks), the Jacobi-sweep loop with ``GSTol``,
the deferred ``U /= rsf`` and the device-array input and output.  A class adds its block count, its ``Y0``
rule for ``U``, its constraint on host arrays, its residual norms and its objective.
"""

import copy

import numpy as np

from .. import _lib
from ..device import DeviceArray, is_device_array
from ..fft import real_dtype
from . import admm


def geometry(shape, caxis, name):
    shape = tuple(int(s) for s in shape)
    if len(shape) < 2 or len(shape) > 4:
        raise NotImplementedError("%s: S has shape (H, W) or (H, W, ...) with up to two trailing axes" % name)
    if caxis is not None and (caxis != 2 or len(shape) < 3):
        raise NotImplementedError("%s: caxis is None or 2 (the first axis after the two spatial ones)" % name)
    H, W = shape[:2]
    if H < 2 or W < 2:
        raise NotImplementedError("%s: H and W must be at least 2 (the gradient stencil needs a neighbour)" % name)
    P = int(np.prod(shape[2:])) if len(shape) > 2 else 1
    C = shape[2] if caxis is not None else 1
    if C > 8:
        raise NotImplementedError("%s: vector TV over at most 8 channels (a pixel's channels live in "
                                  "the registers of one thread)" % name)
    return H, W, P, C


def plan(shape, dtype=np.float32, caxis=None, l1=False):
    """The kernels' launch plan for an ``S`` of ``shape``: ``dict(V, items, strips, R, nseg, TW)``
    -- elements per item, items per row, strips per row, rows per segment, segments, and the columns
    a strip of 256 items covers."""
    H, W, P, C = geometry(shape, caxis, 'plan')
    h = _lib.TvdHandle(H, W, P, dtype, C=C, vector_tv=caxis is not None, l1=l1)
    try:
        return h.plan()
    finally:
        h.close()


def grad(X, ax):
    """The forward difference along ``ax`` with a zero last entry (sporco/signal.py:115-160)."""
    g = np.roll(X, -1, axis=ax) - X
    g[(slice(None),) * ax + (slice(-1, None),)] = 0.0
    return g


def grad_t(V, ax):
    """The transpose of :func:`grad`."""
    v = V.copy()
    v[(slice(None),) * ax + (slice(-1, None),)] = 0.0
    return np.roll(v, 1, axis=ax) - v


class TVDenoise(admm.ADMM):
    """Base of the two TV denoisers on the stencil kernels of csrc/csc_tvd.h."""

    NBLK = 2           # blocks of Y and of U
    L1_HANDLE = False

    class Options(admm.ADMM.Options):
        """Adds ``gEvalY``, ``MaxGSIter``, ``GSTol``, ``DFidWeight``, ``TVWeight`` (tvl2.py:98-141,
        tvl1.py:98-141)."""

        defaults = copy.deepcopy(admm.ADMM.Options.defaults)
        defaults.update({'gEvalY': True, 'RelaxParam': 1.8, 'DFidWeight': 1.0, 'TVWeight': 1.0,
                         'GSTol': 0.0, 'MaxGSIter': 2})
        defaults['AutoRho'].update({'Enabled': False, 'Period': 1, 'AutoScaling': True, 'Scaling': 1000.0,
                                    'RsdlRatio': 1.2})

        def __init__(self, opt=None):
            admm.ADMM.Options.__init__(self, {} if opt is None else opt)
            if self['AutoRho', 'RsdlTarget'] is None:
                self['AutoRho', 'RsdlTarget'] = 1.0

    itstat_fields_objfn = ('ObjFun', 'DFid', 'RegTV')
    itstat_fields_extra = ('GSIter', 'GSRelRes')
    hdrtxt_objfn = ('Fnc', 'DFid', 'RegTV')
    hdrval_objfun = {'Fnc': 'ObjFun', 'DFid': 'DFid', 'RegTV': 'RegTV'}

    def __init__(self, S, lmbda, opt=None, axes=(0, 1), caxis=None, **backend):
        name = type(self).__name__
        if opt is None:
            opt = type(self).Options()
        if backend.get('reducer') is not None:
            raise NotImplementedError("%s: no image sharding (reducer=): the gradient stencil crosses "
                                      "the shard borders" % name)
        if not is_device_array(S):
            S = np.asarray(S)
            if np.iscomplexobj(S):
                raise NotImplementedError("%s handles real-valued S" % name)
        if tuple(axes) != (0, 1):
            raise NotImplementedError("%s: axes == (0, 1); the stencil kernels know two spatial axes, "
                                      "the first two" % name)
        self.set_dtype(opt, S.dtype)
        if self.dtype not in (np.float32, np.float64):
            raise TypeError("sporco_amd works in float32 or float64, not %s" % self.dtype)
        H, W, P, C = geometry(S.shape, caxis, name)
        self.axes = tuple(axes)
        self.caxis = caxis
        self.saxes = (-1,) if caxis is None else (caxis, -1)
        rdt = real_dtype(self.dtype)
        self.lmbda = rdt.type(lmbda)
        self.set_attr('rho', opt['rho'], dval=(2.0 * self.lmbda + 0.1), dtype=rdt)

        # the weights (before any device work: what is refused costs nothing)
        self._dev_io = is_device_array(S)
        wdf = opt['DFidWeight']
        if is_device_array(wdf):
            if wdf.shape != tuple(S.shape) or wdf.dtype != self.dtype:
                raise ValueError("a DeviceArray DFidWeight has the shape and dtype of S")
            self.Wdf = wdf
        else:
            self.Wdf = np.asarray(wdf, dtype=self.dtype)
            if np.iscomplexobj(wdf):
                raise NotImplementedError("%s handles real-valued weights" % name)
            if self.Wdf.ndim > 0:
                np.broadcast_to(self.Wdf, S.shape)      # (raises where it does not broadcast)
        self.Wtv = np.asarray(opt['TVWeight'], dtype=rdt)
        if self.Wtv.ndim > 0 and self.Wtv.size > 1:
            if caxis is not None:
                raise NotImplementedError("%s: an array TVWeight together with caxis is not offered (the "
                                          "reference's own broadcast fails there for several images)" % name)
            if self.Wtv.ndim != len(S.shape):
                raise ValueError("an array TVWeight has as many axes as S and broadcasts to it")
            np.broadcast_to(self.Wtv, S.shape)

        if self._dev_io:
            if S.dtype != self.dtype:
                raise TypeError("a DeviceArray S has the working dtype")
            self.S = S
        else:
            self.S = np.ascontiguousarray(S, dtype=self.dtype)
        self._shape = tuple(S.shape)
        self._dev = _lib.TvdHandle(H, W, P, self.dtype, C=C, vector_tv=caxis is not None,
                                   device=backend.get('device', 0), stream=backend.get('stream'),
                                   l1=self.L1_HANDLE)
        self._u_scale = 1.0
        self._sums = [0.0] * _lib.OUT_COUNT
        self._cache = {}
        self.xs = (0, np.inf)
        # X starts at S (tvl2.py:218-219, tvl1.py:218-219)
        self._dev.upload(_lib.TVD_S, S.ptr if self._dev_io else self.S)
        if is_device_array(self.Wdf):
            self._dev.upload(_lib.TVD_WDF, self.Wdf.ptr)
        elif self.Wdf.size > 1:
            self._dev.upload(_lib.TVD_WDF, np.ascontiguousarray(np.broadcast_to(self.Wdf, self._shape)))
        if self.Wtv.size > 1:
            self._dev.upload(_lib.TVD_WTV, np.ascontiguousarray(np.broadcast_to(self.Wtv, self._shape)))

        yshape = self._shape + (self.NBLK,)
        super(TVDenoise, self).__init__(int(np.prod(self._shape)), yshape, yshape, self.dtype, opt)

    # -- device state -------------------------------------------------------------------------------
    def init_state(self, yshape, ushape):
        """Y and U start at zero on the device; ``Y0`` / ``U0`` as admm.py:262-272, ``U`` from a ``Y0``
        alone by the class's :meth:`u_from_y0`."""
        if self.opt['Y0'] is not None:
            self.Y = np.asarray(self.opt['Y0']).astype(self.dtype, copy=True)
            if self.opt['U0'] is None:
                self.U = self.u_from_y0(self.Y)
        if self.opt['U0'] is not None:
            self.U = np.asarray(self.opt['U0']).astype(self.dtype, copy=True)

    def u_from_y0(self, Y):
        raise NotImplementedError()

    def _touch(self, *variables):
        for v in variables:
            self._cache.pop(v, None)

    def _fetch(self, var):
        if var not in self._cache:
            a = self._dev.download(var)
            if var in (_lib.TVD_Y, _lib.TVD_U):
                a = np.moveaxis(a.reshape((self.NBLK,) + self._shape), 0, -1)      # components on the last axis
                if var == _lib.TVD_U and self._u_scale != 1.0:
                    a = a * a.dtype.type(self._u_scale)
                a = np.ascontiguousarray(a)
            else:
                a = a.reshape(self._shape)
            self._cache[var] = a
        return self._cache[var]

    def _store_blocks(self, var, value):
        value = np.asarray(value, dtype=self.dtype)
        shp = self._shape + (self.NBLK,)
        if value.shape != shp:
            raise ValueError("array of shape %s where %s is expected" % (value.shape, shp))
        self._dev.upload(var, np.ascontiguousarray(np.moveaxis(value, -1, 0)))
        if var == _lib.TVD_U:
            self._u_scale = 1.0
        self._touch(var)
        self._dev.adjoint()

    @property
    def X(self):
        if self._dev_io:
            out = DeviceArray(self._shape, self.dtype)
            self._dev.download(_lib.TVD_X, dst_ptr=out.ptr)
            return out
        return self._fetch(_lib.TVD_X)

    @X.setter
    def X(self, value):
        if value is not None:
            if is_device_array(value):
                if value.shape != self._shape or value.dtype != self.dtype:
                    raise ValueError("X has the shape and dtype of S")
                self._dev.upload(_lib.TVD_X, value.ptr)
            else:
                value = np.asarray(value, dtype=self.dtype)
                if value.shape != self._shape:
                    raise ValueError("X has the shape of S")
                self._dev.upload(_lib.TVD_X, value)
            self._touch(_lib.TVD_X)

    @property
    def Y(self):
        """``S.shape + (NBLK,)``: the blocks on the last axis, as the reference keeps them."""
        return self._fetch(_lib.TVD_Y)

    @Y.setter
    def Y(self, value):
        if value is not None:
            self._store_blocks(_lib.TVD_Y, value)

    @property
    def U(self):
        return self._fetch(_lib.TVD_U)

    @U.setter
    def U(self, value):
        if value is not None:
            self._store_blocks(_lib.TVD_U, value)

    def __getstate__(self):
        raise NotImplementedError("%s: pickling is not offered" % type(self).__name__)

    def cnst_B(self, Y):
        return -Y

    # -- iteration ----------------------------------------------------------------------------------
    def _params(self):
        p = _lib.TvdParams()
        p.rho = float(self.rho)
        p.lmbda = float(self.lmbda)
        p.rlx = float(self.rlx)
        p.u_scale = float(self._u_scale)
        p.wdf = 1.0 if is_device_array(self.Wdf) or self.Wdf.size != 1 else float(self.Wdf.ravel()[0])
        p.wtv = float(self.Wtv.ravel()[0]) if self.Wtv.size == 1 else 1.0
        p.geval_y = 1 if self.opt['gEvalY'] else 0
        return p

    @staticmethod
    def _rrs(s):
        nrm = max(np.sqrt(s[_lib.OUT_XRRS_AX2]), np.sqrt(s[_lib.OUT_XRRS_B2]))
        return 0.0 if nrm == 0.0 else float(np.sqrt(s[_lib.OUT_XRRS_D2]) / nrm)

    def iteration(self):
        admm.refuse_step_overrides(self)
        p = self._params()
        maxgs, gstol = int(self.opt['MaxGSIter']), float(self.opt['GSTol'])
        if maxgs < 1:
            raise ValueError("MaxGSIter must be at least 1")
        if gstol > 0.0:
            # the reference tests the residual after every sweep (tvl2.py:244-252, tvl1.py:251-258): a
            # launch and a host read per sweep
            ngs, gsrrs = 0, np.inf
            while gsrrs > gstol and ngs < maxgs:
                self._dev.sweeps(p, 1)
                gsrrs = self._rrs(self._dev.gsres(p))
                ngs += 1
        else:
            self._dev.sweeps(p, maxgs)
            ngs, gsrrs = maxgs, None
        self._sums = self._dev.ystep(p)
        self._u_scale = 1.0
        if gsrrs is None:
            gsrrs = self._rrs(self._sums)
        self.xs = (ngs, gsrrs)
        self._touch(_lib.TVD_X, _lib.TVD_Y, _lib.TVD_U)
        if not self._needs_residuals():
            return None
        self.timer.stop('solve_wo_rsdl')
        res = self.compute_residuals()
        self.timer.start('solve_wo_rsdl')
        return res

    def finish_solve(self):
        self._dev.sync()

    def rescale_u(self, rsf):
        """Defer ``U /= rsf`` (admm.py:573): the factor rides along as ``u_scale``; the sweeps and the
        y step apply it, ``self.U`` shows it."""
        self._u_scale = self._u_scale / float(rsf)
        self._touch(_lib.TVD_U)

    def itstat_extra(self):
        return (self.xs[0], self.xs[1])

    def getmin(self):
        return self.X
