"""What ``admm.tvl2.TVL2Deconv`` and ``admm.tvl1.TVL1Deconv`` share: the checks of ``A`` and ``S``, the option
tree, the device handle and its arrays (``Y`` and ``U`` in ``NBLK`` blocks), the iteration (a spectral x step,
a stencil y step), the deferred ``U /= rsf``, the spectra as host arrays on demand and the device-array input
and output.  A class adds its block count, its ``Y0`` rule for ``U``, its constraint on host arrays, its
residual norms and its objective.

The gradient operators of these two classes are circular (sporco/signal.py:204-240), unlike those of the
Denoise classes: ``(G_k x)[n] = x[n] - x[n - 1]`` and ``(G_k^T v)[n] = v[n] - v[n + 1]`` with wrap-around.
"""

import copy

import numpy as np

from .. import _lib
from ..device import DeviceArray, is_device_array
from ..fft import real_dtype, complex_dtype
from . import admm
from ._tvd import geometry


def kernel_geometry(A, sshape, name):
    """``A`` with the trailing axes of ``S`` (sporco's ``atleast_nd``): its shape, and the planes of the kernel,
    1 (one kernel for all planes) or those of ``S``."""
    ashape = tuple(int(n) for n in A.shape)
    if len(ashape) > len(sshape):
        raise NotImplementedError("%s: A has no more axes than S" % name)
    ashape = ashape + (1,) * (len(sshape) - len(ashape))
    if ashape[0] > sshape[0] or ashape[1] > sshape[1]:
        raise NotImplementedError("%s: a kernel A of spatial size %s is larger than the image %s (the reference "
                                  "crops it)" % (name, ashape[:2], tuple(sshape[:2])))
    if all(n == 1 for n in ashape[2:]):
        return ashape, 1
    if ashape[2:] != tuple(sshape[2:]):
        raise NotImplementedError("%s: the trailing axes of A are absent, all 1 or those of S, not %s against %s"
                                  % (name, ashape[2:], tuple(sshape[2:])))
    return ashape, int(np.prod(ashape[2:]))


def plan(shape, dtype=np.float32, caxis=None, l1=False):
    """The kernels' launch plan for an ``S`` of ``shape``: ``dict(V, items, strips, R, nseg, TW, SV, sblocks)``
    -- for ``tvdc_ystep`` / ``tvdc_adjoint`` the elements per item, items per row, strips per row, rows per
    segment, segments and the columns a strip of 256 items covers; for ``tvdc_solve`` the planes per access
    and the workgroups."""
    H, W, P, C = geometry(shape, caxis, 'plan')
    h = _lib.TvdcHandle(H, W, P, dtype, C=C, vector_tv=caxis is not None, l1=l1)
    try:
        return h.plan()
    finally:
        h.close()


def pgrad(X, ax):
    """The circular difference along ``ax``: ``x[n] - x[n - 1]``."""
    return X - np.roll(X, 1, axis=ax)


def pgrad_t(V, ax):
    """The transpose of :func:`pgrad`: ``v[n] - v[n + 1]``."""
    return V - np.roll(V, -1, axis=ax)


class TVDeconv(admm.ADMM):
    """Base of the two TV deconvolution classes on the kernels of csrc/csc_tvdc.h."""

    NBLK = 2           # blocks of Y and of U
    L1_HANDLE = False

    class Options(admm.ADMM.Options):
        """Adds ``gEvalY``, ``LinSolveCheck``, ``TVWeight`` (tvl2.py:448-486)."""

        defaults = copy.deepcopy(admm.ADMM.Options.defaults)
        defaults.update({'gEvalY': True, 'RelaxParam': 1.8, 'LinSolveCheck': False, 'TVWeight': 1.0})
        defaults['AutoRho'].update({'Enabled': True, 'Period': 1, 'AutoScaling': True, 'Scaling': 1000.0,
                                    'RsdlRatio': 1.2})

        def __init__(self, opt=None):
            admm.ADMM.Options.__init__(self, {} if opt is None else opt)
            if self['AutoRho', 'RsdlTarget'] is None:
                self['AutoRho', 'RsdlTarget'] = 1.0

    itstat_fields_objfn = ('ObjFun', 'DFid', 'RegTV')
    itstat_fields_extra = ('XSlvRelRes',)
    hdrtxt_objfn = ('Fnc', 'DFid', 'RegTV')
    hdrval_objfun = {'Fnc': 'ObjFun', 'DFid': 'DFid', 'RegTV': 'RegTV'}

    def __init__(self, A, S, lmbda, opt=None, axes=(0, 1), caxis=None, **backend):
        name = type(self).__name__
        if opt is None:
            opt = type(self).Options()
        if backend.get('reducer') is not None:
            raise NotImplementedError("%s: no image sharding (reducer=): the convolution and the gradient "
                                      "stencil cross the shard borders" % name)
        if not is_device_array(S):
            S = np.asarray(S)
            if np.iscomplexobj(S):
                raise NotImplementedError("%s handles real-valued S" % name)
        if not is_device_array(A):
            A = np.asarray(A)
            if np.iscomplexobj(A):
                raise NotImplementedError("%s handles a real-valued kernel A" % name)
        if tuple(axes) != (0, 1):
            raise NotImplementedError("%s: axes == (0, 1); the kernels know two spatial axes, the first two" % name)
        self.set_dtype(opt, S.dtype)
        if self.dtype not in (np.float32, np.float64):
            raise TypeError("sporco_amd works in float32 or float64, not %s" % self.dtype)
        H, W, P, C = geometry(S.shape, caxis, name)
        ashape, PA = kernel_geometry(A, tuple(S.shape), name)
        self.axes = tuple(axes)
        self.axsz = self.axshp = (H, W)
        self.caxis = caxis
        self.saxes = (-1,) if caxis is None else (caxis, -1)
        self.real_dtype = True
        rdt = real_dtype(self.dtype)
        self.lmbda = rdt.type(lmbda)
        self.set_attr('rho', opt['rho'], dval=(2.0 * self.lmbda + 0.1), dtype=rdt)

        # the weights (before any device work: what is refused costs nothing)
        self._dev_io = is_device_array(S)
        self.Wdf = self._dfid_weight(opt, S, name)
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
        if is_device_array(A):
            if A.dtype != self.dtype:
                raise TypeError("a DeviceArray A has the working dtype")
            self._A = A
        else:
            self._A = np.ascontiguousarray(A, dtype=self.dtype).reshape(ashape)
        self._ashape = ashape
        self._shape = tuple(S.shape)
        self._dev = _lib.TvdcHandle(H, W, P, self.dtype, C=C, vector_tv=caxis is not None, PA=PA,
                                    device=backend.get('device', 0), stream=backend.get('stream'),
                                    l1=self.L1_HANDLE)
        self._u_scale = 1.0
        self._sums = [0.0] * _lib.OUT_COUNT
        self._cache = {}
        self._spec = {}
        self.xrrs = None
        self._dev.upload(_lib.TVDC_S, S.ptr if self._dev_io else self.S)
        if is_device_array(A):
            self._dev.set_kernel(A.ptr, ashape[0], ashape[1])
        else:
            self._dev.set_kernel(self._A.reshape(ashape[0], ashape[1], PA))
        if self.Wdf is not None:
            if is_device_array(self.Wdf):
                self._dev.upload(_lib.TVDC_WDF, self.Wdf.ptr)
            elif self.Wdf.size > 1:
                self._dev.upload(_lib.TVDC_WDF, np.ascontiguousarray(np.broadcast_to(self.Wdf, self._shape)))
        if self.Wtv.size > 1:
            self._dev.upload(_lib.TVDC_WTV, np.ascontiguousarray(np.broadcast_to(self.Wtv, self._shape)))

        yshape = self._shape + (self.NBLK,)
        super(TVDeconv, self).__init__(int(np.prod(self._shape)), yshape, yshape, self.dtype, opt)

    def _dfid_weight(self, opt, S, name):
        """The l2 problem has no ``DFidWeight``."""
        return None

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
            if var in (_lib.TVDC_Y, _lib.TVDC_U):
                a = np.moveaxis(a.reshape((self.NBLK,) + self._shape), 0, -1)      # components on the last axis
                if var == _lib.TVDC_U and self._u_scale != 1.0:
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
        if var == _lib.TVDC_U:
            self._u_scale = 1.0
        self._touch(var)
        self._dev.adjoint()

    @property
    def X(self):
        if self._dev_io:
            out = DeviceArray(self._shape, self.dtype)
            self._dev.download(_lib.TVDC_X, dst_ptr=out.ptr)
            return out
        return self._fetch(_lib.TVDC_X)

    @X.setter
    def X(self, value):
        if value is not None:
            raise NotImplementedError("%s: X is the result of the x step; set Y and U" % type(self).__name__)

    @property
    def Y(self):
        """``S.shape + (NBLK,)``: the blocks on the last axis, as the reference keeps them."""
        return self._fetch(_lib.TVDC_Y)

    @Y.setter
    def Y(self, value):
        if value is not None:
            self._store_blocks(_lib.TVDC_Y, value)

    @property
    def U(self):
        return self._fetch(_lib.TVDC_U)

    @U.setter
    def U(self, value):
        if value is not None:
            self._store_blocks(_lib.TVDC_U, value)

    def __getstate__(self):
        raise NotImplementedError("%s: pickling is not offered" % type(self).__name__)

    # -- host copies of the spectra, formed on demand -------------------------------------------------
    def _host(self, a):
        return a.get() if is_device_array(a) else a

    def _rfft(self, a, s=None):
        return np.fft.rfftn(a, s=s, axes=self.axes).astype(complex_dtype(self.dtype))

    def _irfft(self, af):
        return np.fft.irfftn(af, s=self.axsz, axes=self.axes).astype(self.dtype)

    def _spectrum(self, key, make):
        if key not in self._spec:
            self._spec[key] = make()
        return self._spec[key]

    @property
    def A(self):
        """The kernel with the trailing axes of ``S``."""
        return self._host(self._A).reshape(self._ashape)

    @property
    def Af(self):
        return self._spectrum('Af', lambda: self._rfft(self.A, self.axshp))

    @property
    def Sf(self):
        return self._spectrum('Sf', lambda: self._rfft(self._host(self.S)))

    @property
    def AHAf(self):
        return self._spectrum('AHAf', lambda: np.conj(self.Af) * self.Af)

    @property
    def AHSf(self):
        return self._spectrum('AHSf', lambda: np.conj(self.Af) * self.Sf)

    @property
    def Gf(self):
        """The spectra of the filters [1, -1] on each axis, stacked on a last axis (sporco/signal.py:204-240)."""
        def make():
            nd = len(self._shape)
            g = np.zeros((2, 2) + (1,) * (nd - 2) + (2,), self.dtype)
            g[:, 0, ..., 0] = np.array([1, -1], self.dtype).reshape((2,) + (1,) * (nd - 2))
            g[0, :, ..., 1] = np.array([1, -1], self.dtype).reshape((2,) + (1,) * (nd - 2))
            return self._rfft(g, self.axshp)
        return self._spectrum('Gf', make)

    @property
    def GHGf(self):
        return self._spectrum('GHGf', lambda: np.sum(np.conj(self.Gf) * self.Gf, axis=-1).real)

    @property
    def Xf(self):
        return self._rfft(self._fetch(_lib.TVDC_X))

    def cnst_B(self, Y):
        return -Y

    # -- iteration ----------------------------------------------------------------------------------
    def _params(self):
        p = _lib.TvdcParams()
        p.rho = float(self.rho)
        p.lmbda = float(self.lmbda)
        p.rlx = float(self.rlx)
        p.u_scale = float(self._u_scale)
        wdf = self.Wdf
        p.wdf = 1.0 if wdf is None or is_device_array(wdf) or wdf.size != 1 else float(wdf.ravel()[0])
        p.wtv = float(self.Wtv.ravel()[0]) if self.Wtv.size == 1 else 1.0
        p.geval_y = 1 if self.opt['gEvalY'] else 0
        p.lin_solve_check = 1 if self.opt['LinSolveCheck'] else 0
        p.want_rsdl = 1 if self._needs_residuals() else 0
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
        self._touch(_lib.TVDC_X, _lib.TVDC_HX, _lib.TVDC_Y, _lib.TVDC_U)
        if not p.want_rsdl:
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
        self._touch(_lib.TVDC_U)

    def itstat_extra(self):
        return (self.xrrs,)

    def getmin(self):
        return self.X
