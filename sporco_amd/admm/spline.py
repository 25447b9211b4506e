"""l1-spline fit on the device, with the interface of the reference's ``sporco.admm.spline``
(sporco/admm/spline.py:24-291): the reference's smoother for impulse noise (``examples/scripts/misc/spline.py``).

:class:`SplineL1` solves

    minimise || Wdf (x - s) ||_1 + (lmbda / 2) || D x ||^2

with D the second difference with reflecting ends along ``axes``, by ADMM on ``x - y = s``.  D is diagonal under
the orthonormal DCT-II, so the x step is ``X = idct(Gamma dct(Y + S - U))`` with ``Gamma = 1 / (1 + (lmbda / rho)
Alpha^2)``; the DCT is one real transform of the same size on a permuted array with a pointwise twiddle kernel on
each side of ``Gamma`` (csrc/csc_spline.h), the y and u steps one more kernel.

Served: real float32 / float64 ``S`` of shape ``(H, W)`` or ``(H, W, ...)`` with up to two trailing axes (every
trailing index is an independent plane), ``H, W >= 2``, ``axes == (0, 1)``; a 1-D ``S`` with ``axes == (0,)``;
``DFidWeight`` a scalar, an array that broadcasts to ``S`` (the reference's boolean mask included) or a
:class:`sporco_amd.device.DeviceArray`; ``S`` may be a DeviceArray, ``solve()`` and ``X`` then return one.

Refused with ``NotImplementedError``: complex ``S``, other ``axes``, pickling, ``reducer=``; other dtypes raise
``TypeError``.
"""

import copy

import numpy as np

from .. import _lib
from ..device import DeviceArray, is_device_array
from ..fft import real_dtype
from . import admm

__all__ = ['SplineL1', 'plan']


def geometry(shape, axes, name):
    """``(H, W, P)`` of the device problem: a 1-D signal is a single row."""
    shape = tuple(int(s) for s in shape)
    axes = tuple(axes)
    if len(shape) == 1:
        if axes != (0,):
            raise NotImplementedError("%s: a 1-D S is fitted along axes == (0,)" % name)
        if shape[0] < 2:
            raise NotImplementedError("%s: at least two samples" % name)
        return 1, shape[0], 1
    if axes != (0, 1):
        raise NotImplementedError("%s: axes == (0, 1); the kernels know two spatial axes, the first two" % name)
    if len(shape) > 4:
        raise NotImplementedError("%s: S has shape (H, W) or (H, W, ...) with up to two trailing axes" % name)
    H, W = shape[:2]
    if H < 2 or W < 2:
        raise NotImplementedError("%s: H and W must be at least 2" % name)
    return H, W, (int(np.prod(shape[2:])) if len(shape) > 2 else 1)


def plan(shape, dtype=np.float32, axes=(0, 1)):
    """The kernels' launch plan for an ``S`` of ``shape``: ``dict(V, pairs, sblocks, yblocks)`` -- planes per
    access, the row pairs ``{k1, H - k1}`` of ``spl_solve``, its workgroups and those of ``spl_ystep``."""
    H, W, P = geometry(shape, axes, 'plan')
    h = _lib.SplHandle(H, W, P, dtype)
    try:
        return h.plan()
    finally:
        h.close()


class SplineL1(admm.ADMM):
    r"""ADMM algorithm for the l1-spline problem; interface of sporco/admm/spline.py:24-291.

    ``IterationStats``: ``Iter, ObjFun, DFid, Reg, PrimalRsdl, DualRsdl, EpsPrimal, EpsDual, Rho, XSlvRelRes,
    Time``.
    """

    class Options(admm.ADMM.Options):
        """Adds ``gEvalY``, ``DFidWeight``, ``LinSolveCheck`` (spline.py:80-119); ``AutoRho`` is enabled."""

        defaults = copy.deepcopy(admm.ADMM.Options.defaults)
        defaults.update({'gEvalY': True, 'RelaxParam': 1.8, 'DFidWeight': 1.0, 'LinSolveCheck': False})
        defaults['AutoRho'].update({'Enabled': True, 'Period': 1, 'AutoScaling': True, 'Scaling': 1000.0,
                                    'RsdlRatio': 1.2})

        def __init__(self, opt=None):
            admm.ADMM.Options.__init__(self, {} if opt is None else opt)
            if self['AutoRho', 'RsdlTarget'] is None:
                self['AutoRho', 'RsdlTarget'] = 1.0

    itstat_fields_objfn = ('ObjFun', 'DFid', 'Reg')
    itstat_fields_extra = ('XSlvRelRes',)
    hdrtxt_objfn = ('Fnc', 'DFid', 'Reg')
    hdrval_objfun = {'Fnc': 'ObjFun', 'DFid': 'DFid', 'Reg': 'Reg'}

    def __init__(self, S, lmbda, opt=None, axes=(0, 1), **backend):
        name = type(self).__name__
        if opt is None:
            opt = SplineL1.Options()
        if backend.get('reducer') is not None:
            raise NotImplementedError("%s: no image sharding (reducer=): the transform crosses the shard borders"
                                      % name)
        if not is_device_array(S):
            S = np.asarray(S)
            if np.iscomplexobj(S):
                raise NotImplementedError("%s handles real-valued S" % name)
        self.set_dtype(opt, S.dtype)
        if self.dtype not in (np.float32, np.float64):
            raise TypeError("sporco_amd works in float32 or float64, not %s" % self.dtype)
        H, W, P = geometry(S.shape, axes, name)
        self.axes = tuple(axes)
        rdt = real_dtype(self.dtype)
        self.lmbda = rdt.type(lmbda)
        self.set_attr('rho', opt['rho'], dval=(2.0 * self.lmbda + 0.1), dtype=rdt)

        # the weight (before any device work: what is refused costs nothing)
        self._dev_io = is_device_array(S)
        wdf = opt['DFidWeight']
        if is_device_array(wdf):
            if wdf.shape != tuple(S.shape) or wdf.dtype != self.dtype:
                raise ValueError("a DeviceArray DFidWeight has the shape and dtype of S")
            self.Wdf = wdf
        else:
            if np.iscomplexobj(wdf):
                raise NotImplementedError("%s handles real-valued weights" % name)
            self.Wdf = np.asarray(wdf, dtype=self.dtype)
            if self.Wdf.ndim > 0:
                np.broadcast_to(self.Wdf, S.shape)      # (raises where it does not broadcast)

        if self._dev_io:
            if S.dtype != self.dtype:
                raise TypeError("a DeviceArray S has the working dtype")
            self.S = S
        else:
            self.S = np.ascontiguousarray(S, dtype=self.dtype)
        self._shape = tuple(S.shape)
        self._dev = _lib.SplHandle(H, W, P, self.dtype, device=backend.get('device', 0), stream=backend.get('stream'))
        self._u_scale = 1.0
        self._sums = [0.0] * _lib.OUT_COUNT
        self._cache = {}
        self.xrrs = None
        self._dev.upload(_lib.SPL_S, S.ptr if self._dev_io else self.S)
        if is_device_array(self.Wdf):
            self._dev.upload(_lib.SPL_WDF, self.Wdf.ptr)
        elif self.Wdf.size > 1:
            self._dev.upload(_lib.SPL_WDF, np.ascontiguousarray(np.broadcast_to(self.Wdf, self._shape)))

        super(SplineL1, self).__init__(int(np.prod(self._shape)), self._shape, self._shape, self.dtype, opt)

    # -- device state -------------------------------------------------------------------------------
    def init_state(self, yshape, ushape):
        """Y and U start at zero on the device; ``Y0`` / ``U0`` as admm.py:262-272, ``U`` from a ``Y0`` alone
        by :meth:`uinit`."""
        if self.opt['Y0'] is not None:
            self.Y = np.asarray(self.opt['Y0']).astype(self.dtype, copy=True)
            if self.opt['U0'] is None:
                self.U = self.uinit(ushape)
        if self.opt['U0'] is not None:
            self.U = np.asarray(self.opt['U0']).astype(self.dtype, copy=True)

    def uinit(self, ushape):
        """spline.py:176-185: zero, or at a non-zero Y the dual optimality criterion (3.10) of
        boyd-2010-distributed, ``(Wdf / rho) sign(Y)``."""
        if self.opt['Y0'] is None:
            return np.zeros(ushape, dtype=self.dtype)
        wdf = self.Wdf.get() if is_device_array(self.Wdf) else self.Wdf
        return ((wdf / self.rho) * np.sign(self.Y)).astype(self.dtype)

    def _touch(self, *variables):
        for v in variables:
            self._cache.pop(v, None)

    def _fetch(self, var):
        if var not in self._cache:
            a = self._dev.download(var).reshape(self._shape)
            if var == _lib.SPL_U and self._u_scale != 1.0:
                a = a * a.dtype.type(self._u_scale)
            self._cache[var] = a
        return self._cache[var]

    def _store(self, var, value):
        value = np.asarray(value, dtype=self.dtype)
        if value.shape != self._shape:
            raise ValueError("array of shape %s where %s is expected" % (value.shape, self._shape))
        self._dev.upload(var, np.ascontiguousarray(value))
        if var == _lib.SPL_U:
            self._u_scale = 1.0
        self._touch(var)

    @property
    def X(self):
        if self._dev_io:
            out = DeviceArray(self._shape, self.dtype)
            self._dev.download(_lib.SPL_X, dst_ptr=out.ptr)
            return out
        return self._fetch(_lib.SPL_X)

    @X.setter
    def X(self, value):
        if value is not None:
            raise NotImplementedError("%s: X is the result of the x step; set Y and U" % type(self).__name__)

    @property
    def Y(self):
        return self._fetch(_lib.SPL_Y)

    @Y.setter
    def Y(self, value):
        if value is not None:
            self._store(_lib.SPL_Y, value)

    @property
    def U(self):
        return self._fetch(_lib.SPL_U)

    @U.setter
    def U(self, value):
        if value is not None:
            self._store(_lib.SPL_U, value)

    def __getstate__(self):
        raise NotImplementedError("%s: pickling is not offered" % type(self).__name__)

    # -- host copies of the diagonal, formed on demand ------------------------------------------------
    @property
    def Alpha(self):
        """The eigenvalues of D over ``axes`` (spline.py:163-171), shaped to broadcast against ``S``."""
        nd = len(self._shape)
        al = np.zeros([self._shape[ax] if ax in self.axes else 1 for ax in range(nd)], dtype=self.dtype)
        for ax in self.axes:
            shp = [1] * nd
            shp[ax] = self._shape[ax]
            al = al + (-2.0 + 2.0 * np.cos(np.arange(shp[ax]).reshape(shp) * np.pi / float(shp[ax])))
        return al.astype(self.dtype)

    @property
    def Gamma(self):
        return (1.0 / (1.0 + (self.lmbda / self.rho) * (self.Alpha ** 2))).astype(self.dtype)

    # -- the constraint on host arrays (spline.py:258-291) ------------------------------------------------
    def cnst_A(self, X):
        return X

    def cnst_AT(self, X):
        return X

    def cnst_B(self, Y):
        return -Y

    def cnst_c(self):
        return self.S.get() if self._dev_io else self.S

    # -- iteration ----------------------------------------------------------------------------------
    def _params(self):
        p = _lib.SplParams()
        p.rho = float(self.rho)
        p.lmbda = float(self.lmbda)
        p.rlx = float(self.rlx)
        p.u_scale = float(self._u_scale)
        wdf = self.Wdf
        p.wdf = 1.0 if is_device_array(wdf) or wdf.size != 1 else float(wdf.ravel()[0])
        p.geval_y = 1 if self.opt['gEvalY'] else 0
        p.lin_solve_check = 1 if self.opt['LinSolveCheck'] else 0
        p.want_stats = 0 if self.opt['FastSolve'] else 1
        return p

    def iteration(self):
        admm.refuse_step_overrides(self)
        p = self._params()
        self._dev.xstep(p)
        self._sums = self._dev.ystep(p)
        self._u_scale = 1.0
        if p.lin_solve_check:
            s = self._sums
            nrm = max(np.sqrt(s[_lib.OUT_XRRS_AX2]), np.sqrt(s[_lib.OUT_XRRS_B2]))
            self.xrrs = 0.0 if nrm == 0.0 else float(np.sqrt(s[_lib.OUT_XRRS_D2]) / nrm)
        else:
            self.xrrs = None
        self._touch(_lib.SPL_X, _lib.SPL_Y, _lib.SPL_U)
        if not self._needs_residuals():
            return None
        self.timer.stop('solve_wo_rsdl')
        res = self.compute_residuals()
        self.timer.start('solve_wo_rsdl')
        return res

    def finish_solve(self):
        self._dev.sync()

    def rescale_u(self, rsf):
        """Defer ``U /= rsf`` (admm.py:573): the factor rides along as ``u_scale``; the x and y steps apply
        it, ``self.U`` shows it."""
        self._u_scale = self._u_scale / float(rsf)
        self._touch(_lib.SPL_U)

    def residual_norms(self):
        """admm.py:722-775 with A = I, B = -I, c = S: r = ||X - Y - S||, s = rho ||Y - Yprev||,
        rn = max(||X||, ||Y||, ||S||), sn = rho ||U||."""
        s = self._sums
        rho = float(self.rho)
        return (np.sqrt(s[_lib.OUT_R2]), rho * np.sqrt(s[_lib.OUT_S2]),
                max(np.sqrt(s[_lib.OUT_AX2]), np.sqrt(s[_lib.OUT_Y2]), np.sqrt(s[_lib.OUT_C2])),
                rho * np.sqrt(s[_lib.OUT_U2]))

    def eval_objfn(self):
        """DFid = sum |Wdf g|, g = Y or X - S; Reg = (1/2) ||Alpha dct(X)||^2 (spline.py:234-247)."""
        dfd = self._sums[_lib.OUT_DFID]
        reg = 0.5 * self._sums[_lib.OUT_RGR]
        return (dfd + float(self.lmbda) * reg, dfd, reg)

    def itstat_extra(self):
        return (self.xrrs,)

    def getmin(self):
        return self.X
