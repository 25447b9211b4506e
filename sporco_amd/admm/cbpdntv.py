"""ADMM convolutional sparse coding with total-variation terms on the GPU.

Drop-in for the classes of the reference's ``sporco.admm.cbpdntv`` (ConvBPDNScalarTV
sporco/admm/cbpdntv.py:31-571, ConvBPDNVectorTV :577-727, ConvBPDNRecTV :733-1356): same
constructor signature, Options tree, IterationStats fields, attributes (``X, Y, U, D, S, rho, lmbda,
mu, Wl1, Wtv, cri, itstat``) and the ``var_y0 / var_y1 / var_yx``, ``cnst_*``, ``obfn_*`` methods.
:class:`ConvBPDNRecTV`, the total variation of the reconstruction, is described at the class.

The first two classes:

The constraint is ``(Gamma_0; Gamma_1; I) x = (y_0; y_1; y_L)``: ``Y`` and ``U`` have three blocks
(``cri.shpX + (3,)``).  The x step is the system of :class:`sporco_amd.admm.cbpdn.ConvBPDNGradReg`
with ``mu = rho`` and the per-filter weights ``Wtv^2`` and runs on that class's kernels unchanged.
The reference applies the gradient operators through six FFT round trips per iteration; its
gradient filters are the two-tap ``[1, -1]``, so ``G_i x`` is ``x`` minus its circular predecessor
along axis ``i`` and everything around the x step is two streaming HIP kernels
(csrc/csc_tv.hip): ``tv_ystep`` (relaxation, both proximal maps, the dual update and every sum of
the residuals and the objective) and ``tv_adjoint`` (``A^T Y``, ``A^T U`` for the next x step and
the dual residual).
"""

import copy

import numpy as np

from . import admm
from . import cbpdn
from .. import _lib
from .. import cnvrep as cr
from ..fft import real_dtype

__all__ = ['ConvBPDNScalarTV', 'ConvBPDNVectorTV', 'ConvBPDNRecTV']


class ConvBPDNScalarTV(admm.ADMM):
    r"""Convolutional BPDN with a scalar total-variation term on every coefficient map: minimise
    (1/2)||sum_m d_m * x_m - s||_2^2 + lambda sum_m ||x_m||_1 +
    mu sum_m || sqrt(sum_i (G_i x_m)^2) ||_1 (reference class: sporco/admm/cbpdntv.py:31-571).

    The iterations are driven from the host: per iteration the staged x step, ``tv_ystep`` and
    ``tv_adjoint``.  ``xstep`` may be overridden; the relaxation, the y step and the u step are one
    kernel, so overriding ``relax_AX`` / ``ystep`` / ``ustep`` is refused.

    In scope: ``dimN = 2``, float32 / float64, ``dimK`` 0 / 1, multi-signal and multi-channel ``S``
    with a single-channel ``D``, scalar or array ``L1Weight``, scalar or per-filter ``TVWeight``,
    ``AutoRho``, ``RelaxParam``, ``AuxVarObj`` / ``fEvalX`` / ``gEvalY``, ``LinSolveCheck``, ``Y0`` /
    ``U0``.  Refused (``NotImplementedError``): ``dimN`` 1 and 3, multi-channel dictionaries,
    complex data, ``reducer=``, resident or device inputs, wrapping in ``AddMaskSim``,
    ``NonNegCoef`` / ``NoBndryCross`` (the reference's TV y step ignores them), pickling.

    A ``TVWeight`` whose entries differ between filters is the slow path: the x step then leaves
    the register-resident and mixed-radix kernels for the generic transform chain with one extra
    kernel (one thread per frequency, strided over the K filters) that repeats the reference's
    ``solvedbi_sm`` arithmetic, which is not an exact solve for such weights (``LinSolveCheck``
    shows the residual).  A scalar, or an array of equal weights, stays on the fast x step.

    IterationStats fields: ``Iter, ObjFun, DFid, RegL1, RegTV, PrimalRsdl, DualRsdl, EpsPrimal,
    EpsDual, Rho, XSlvRelRes, Time``.
    """

    class Options(cbpdn.ConvBPDN.Options):
        """Adds ``TVWeight`` (cbpdntv.py:128-138): a scalar, or one weight per filter."""

        defaults = copy.deepcopy(cbpdn.ConvBPDN.Options.defaults)
        defaults.update({'TVWeight': 1.0})

        def __init__(self, opt=None):
            cbpdn.ConvBPDN.Options.__init__(self, {} if opt is None else opt)

    itstat_fields_objfn = ('ObjFun', 'DFid', 'RegL1', 'RegTV')
    itstat_fields_extra = ('XSlvRelRes',)
    hdrtxt_objfn = ('Fnc', 'DFid', u'Regℓ1', 'RegTV')
    hdrval_objfun = {'Fnc': 'ObjFun', 'DFid': 'DFid', u'Regℓ1': 'RegL1', 'RegTV': 'RegTV'}

    _vector_tv = False
    # everything but xstep runs inside the two kernels: an override could not take effect
    _device_only_names = tuple(n for n in admm.STEP_HOOKS if n != 'xstep')

    def __init__(self, D, S, lmbda, mu=0.0, opt=None, dimK=None, dimN=2, **backend):
        name = type(self).__name__
        if opt is None:
            opt = ConvBPDNScalarTV.Options()
        admm.refuse_backend_extras(name, D, S, dimN, backend,
                                   dim_note="dimN = 2 (images); the stencil kernels know two spatial axes",
                                   shard_note=": the gradient stencil crosses the shard borders")
        if opt['NonNegCoef'] or opt['NoBndryCross']:
            raise NotImplementedError("%s: NonNegCoef / NoBndryCross are not offered (the "
                                      "reference's TV y step ignores them)" % name)
        self.cri = cr.CSC_ConvRepIndexing(D, S, dimK=dimK, dimN=dimN)
        if self.cri.Cd > 1:
            raise NotImplementedError("%s with a multi-channel dictionary is not offered (its x "
                                      "step would need the iterated Sherman-Morrison form)" % name)
        self.set_dtype(opt, S.dtype)
        if self.dtype not in (np.float32, np.float64):
            raise TypeError("sporco_amd works in float32 or float64, not %s" % self.dtype)
        H, W = self.cri.Nv
        self._dev = _lib.Solver(H, W, self.cri.C, self.cri.K, self.cri.M, self.dtype,
                                device=backend.get('device', 0), stream=backend.get('stream'))
        self._cache = {}
        self._u_scale = 1.0
        self._sums = [0.0] * _lib.OUT_COUNT
        self._tv_ready = False
        self.xrrs = None

        Nx = int(np.prod(np.array(self.cri.shpX)))
        yshape = self._yshape()
        super(ConvBPDNScalarTV, self).__init__(Nx, yshape, yshape, S.dtype, opt)

        rdt = real_dtype(self.dtype).type
        self.lmbda = rdt(lmbda)
        self.Wl1 = np.asarray(opt['L1Weight'], dtype=self.dtype)
        self.Wl1 = self.Wl1.reshape(cr.l1Wshape(self.Wl1, self.cri))
        self.mu = rdt(mu)
        tvw = opt['TVWeight']
        if hasattr(tvw, 'ndim') and np.ndim(tvw) > 0:
            # one weight per filter, broadcast along the filter axis (cbpdntv.py:213-215)
            self.Wtv = np.asarray(np.asarray(tvw).reshape((1,) * (dimN + 2) + np.shape(tvw)),
                                  dtype=self.dtype)
            if self.Wtv.size != self.cri.M:
                raise ValueError("TVWeight must be a scalar or hold one weight per filter")
        else:
            self.Wtv = np.asarray(tvw, dtype=self.dtype)
        # (as in the reference, cbpdntv.py:221-226: without `reset` these calls do not replace what
        # admm.ADMM.__init__ has set, so the effective defaults are rho = 1 and rho_xi = 1 -- not
        # the 50 lmbda + 1 the call names; the fixtures of the unmodified reference pin this)
        self.set_attr('rho', opt['rho'], dval=(50.0 * self.lmbda + 1.0), dtype=rdt)
        self.set_attr('rho_xi', opt['AutoRho', 'RsdlTarget'], dval=1.0, dtype=rdt)

        self.D = np.asarray(D.reshape(self.cri.shpD), dtype=self.dtype)
        self.S = np.asarray(S.reshape(self.cri.shpS), dtype=self.dtype)
        self._dev.set_signal(self.S)
        self.setdict()
        self._upload_weights()
        # warm start (admm.py:262-272): the blocks, then P = A^T Y and Q = A^T U for the x step
        if opt['Y0'] is not None:
            self.Y = np.asarray(opt['Y0']).astype(self.dtype, copy=True)
        if opt['U0'] is not None:
            self.U = np.asarray(opt['U0']).astype(self.dtype, copy=True)

    def _yshape(self):
        return self.cri.shpX + (len(self.cri.axisN) + 1,)

    # -- device state -------------------------------------------------------------------------
    def init_state(self, yshape, ushape):
        """Y and U start at zero on the device; Y0 / U0 are stored once the weights exist."""

    def _upload_weights(self):
        if self.Wl1.size == 1:
            self._wl1_scalar = float(self.Wl1.ravel()[0])
            self._dev.set_l1_weight(None)
        else:
            self._wl1_scalar = 1.0
            self._dev.set_l1_weight(cbpdn._broadcastable(self.Wl1, self.cri.shpX))
        self._dev.tv_setup(np.asarray(self.Wtv, dtype=np.float64).ravel(), self._vector_tv)
        self._tv_ready = True

    def setdict(self, D=None):
        """Set the dictionary (internal layout); Df is rebuilt on the device."""
        if D is not None:
            self.D = np.asarray(D, dtype=self.dtype)
        self._dev.set_dict(self.D)
        self._touch(_lib.VAR_DF)
        self.c = None

    def _touch(self, *variables):
        for v in variables:
            self._cache.pop(v, None)

    def _fetch(self, var):
        if var not in self._cache:
            a = self._dev.download(var)
            if var in (_lib.VAR_TVY, _lib.VAR_TVU):
                a = np.ascontiguousarray(np.moveaxis(a, 0, -1))     # blocks on the last axis
            if var == _lib.VAR_TVU and self._u_scale != 1.0:
                a *= a.dtype.type(self._u_scale)
            self._cache[var] = a
        return self._cache[var]

    def _store_blocks(self, var, value):
        value = np.asarray(value, dtype=self.dtype)
        shp = self.cri.shpX + (3,)
        if value.size != int(np.prod(shp)):
            raise ValueError("array of shape %s is not a three-block array of shape %s"
                             % (value.shape, shp))
        self._dev.upload(var, np.ascontiguousarray(np.moveaxis(value.reshape(shp), -1, 0)))
        if var == _lib.VAR_TVU:
            self._u_scale = 1.0
        self._touch(var)
        if self._tv_ready:
            self._dev.tv_adjoint(self._u_scale)

    @property
    def X(self):
        return self._fetch(_lib.VAR_X)

    @X.setter
    def X(self, value):
        if value is not None:
            self._dev.upload(_lib.VAR_X, np.asarray(value, dtype=self.dtype))
            self._touch(_lib.VAR_X, _lib.VAR_XF)

    @property
    def Y(self):
        """The blocks (y_0, y_1, y_L) on the last axis, ``cri.shpX + (3,)``, as the reference keeps
        them."""
        return self._fetch(_lib.VAR_TVY)

    @Y.setter
    def Y(self, value):
        if value is not None:
            self._store_blocks(_lib.VAR_TVY, value)

    @property
    def U(self):
        return self._fetch(_lib.VAR_TVU)

    @U.setter
    def U(self, value):
        if value is not None:
            self._store_blocks(_lib.VAR_TVU, value)

    @property
    def Xf(self):
        return self._dev.download(_lib.VAR_XF)

    @property
    def Df(self):
        return self._dev.download(_lib.VAR_DF)

    @property
    def Sf(self):
        return self._dev.download(_lib.VAR_SF)

    def _set_ams(self, W):
        raise NotImplementedError("%s cannot be wrapped in AddMaskSim: the TV y step has no "
                                  "treatment of the appended impulse filter" % type(self).__name__)

    def __getstate__(self):
        raise NotImplementedError("%s: pickling is not offered" % type(self).__name__)

    # -- the blocks ---------------------------------------------------------------------------
    def var_y0(self):
        """The gradient blocks of Y (cbpdntv.py:335-339)."""
        return self.Y[..., 0:-1]

    def var_y1(self):
        """The identity block of Y (cbpdntv.py:343-347)."""
        return self.Y[..., -1:]

    def var_yx(self):
        """The block of Y constrained to equal X (cbpdntv.py:351-355)."""
        return self.Y[..., -1]

    def var_yx_idx(self):
        return np.s_[..., -1]

    def getmin(self):
        return self.X if self.opt['ReturnX'] else self.var_y1()[..., 0]

    def getcoef(self):
        return self.getmin()

    # -- the constraint on host arrays (cbpdntv.py:457-538): G_i x = x - roll(x, 1, i) ------------
    def cnst_A0(self, X, Xf=None):
        X = np.asarray(X)
        G = np.stack([X - np.roll(X, 1, axis=i) for i in self.cri.axisN], axis=-1)
        return self.Wtv[..., np.newaxis] * G

    def cnst_A0T(self, X):
        X = np.asarray(X)
        G = np.stack([X[..., i] - np.roll(X[..., i], -1, axis=ax)
                      for i, ax in enumerate(self.cri.axisN)], axis=-1)
        return self.Wtv[..., np.newaxis] * G

    def cnst_A1(self, X):
        return np.asarray(X)[..., np.newaxis]

    def cnst_A1T(self, X):
        return np.asarray(X)[..., -1]

    def cnst_A(self, X, Xf=None):
        return np.concatenate((self.cnst_A0(X, Xf), self.cnst_A1(X)), axis=-1)

    def cnst_AT(self, X):
        return np.sum(self.cnst_A0T(X), axis=-1) + self.cnst_A1T(X)

    def cnst_B(self, Y):
        return -Y

    def cnst_c(self):
        return 0.0

    @property
    def AXnr(self):
        return self.cnst_A(self.X)

    # -- parameters handed to the device ---------------------------------------------------------
    def _params(self):
        p = _lib.AdmmParams()
        p.rho = float(self.rho)
        p.lmbda = float(self.lmbda) * self._wl1_scalar
        p.mu = float(self.mu)
        p.rlx = float(self.rlx)
        p.u_scale = float(self._u_scale)
        f = _lib.FLAG_RESID
        if not self.opt['FastSolve']:
            f |= _lib.FLAG_OBJ
            if self.opt['gEvalY']:
                f |= _lib.FLAG_GEVAL_Y
            if not self.opt['fEvalX']:
                f |= _lib.FLAG_FEVAL_Y
        if self.opt['LinSolveCheck']:
            f |= _lib.FLAG_XRRS
        p.flags = f
        p.dH, p.dW = int(self.D.shape[0]), int(self.D.shape[1])
        return p

    # -- iteration ----------------------------------------------------------------------------
    def iteration(self):
        admm.refuse_step_overrides(self, self._device_only_names)
        self.xstep()
        self._yu_steps()
        if not self._needs_residuals():
            return None
        self.timer.stop('solve_wo_rsdl')
        res = self.compute_residuals()
        self.timer.start('solve_wo_rsdl')
        return res

    def finish_solve(self):
        self._dev.sync()

    def xstep(self):
        """(D^H D + rho Wtv^2 GHGf + rho) x = D^H s + rho A^T (Y - U) (cbpdntv.py:277-310): the
        gradient-regularised x step with mu = rho on P = A^T Y, Q = A^T U.  With different TVWeights
        per filter the reference's call of linalg.solvedbi_sm is not a solve of that system; the
        device then repeats the reference's arithmetic (include/sporco_amd.h, tv_xstep)."""
        out = self._dev.tv_xstep(self._params())
        for slot in (_lib.OUT_DFID, _lib.OUT_XRRS_D2, _lib.OUT_XRRS_AX2, _lib.OUT_XRRS_B2):
            self._sums[slot] = out[slot]
        self._touch(_lib.VAR_X, _lib.VAR_XF)
        if self.opt['LinSolveCheck']:
            s = self._sums
            nrm = max(np.sqrt(s[_lib.OUT_XRRS_AX2]), np.sqrt(s[_lib.OUT_XRRS_B2]))
            self.xrrs = 0.0 if nrm == 0.0 else np.sqrt(s[_lib.OUT_XRRS_D2]) / nrm
        else:
            self.xrrs = None

    def _yu_steps(self):
        """relax_AX, ystep and ustep as one kernel, then A^T of the new Y and U."""
        p = self._params()
        out = self._dev.tv_ystep(p)
        for slot in (_lib.OUT_R2, _lib.OUT_AX2, _lib.OUT_Y2, _lib.OUT_L1, _lib.OUT_L21):
            self._sums[slot] = out[slot]
        if not self.opt['fEvalX']:
            self._sums[_lib.OUT_DFID] = out[_lib.OUT_DFID]
        self._u_scale = 1.0
        out = self._dev.tv_adjoint(1.0)
        for slot in (_lib.OUT_S2, _lib.OUT_U2):
            self._sums[slot] = out[slot]
        self._touch(_lib.VAR_TVY, _lib.VAR_TVU)

    def save_yprev(self):
        """Nothing to copy: the dual residual is formed from A^T Y before and after the y step."""

    def relax_AX(self):
        """Part of ``tv_ystep`` (cbpdntv.py:542-559)."""

    def ystep(self):
        """Part of ``tv_ystep`` (cbpdntv.py:314-321)."""

    def ustep(self):
        """Part of ``tv_ystep`` (admm.py:434-437)."""

    def residual_norms(self):
        """admm.py:722-775 for the general constraint: ||AXnr - Y||, rho ||A^T (Y - Yprev)||,
        max(||AXnr||, ||Y||), rho ||A^T U||."""
        s = self._sums
        rho = float(self.rho)
        return (np.sqrt(s[_lib.OUT_R2]), rho * np.sqrt(s[_lib.OUT_S2]),
                max(np.sqrt(s[_lib.OUT_AX2]), np.sqrt(s[_lib.OUT_Y2])),
                rho * np.sqrt(s[_lib.OUT_U2]))

    def rescale_u(self, rsf):
        """Defer ``U /= rsf`` (admm.py:573): the factor rides along as ``u_scale``; the x step applies
        it to Q and ``tv_ystep`` to the blocks of U."""
        self._u_scale = self._u_scale / float(rsf)
        self._touch(_lib.VAR_TVU)

    # -- objective --------------------------------------------------------------------------
    def eval_objfn(self):
        dfd = self.obfn_dfd()
        reg = self.obfn_reg()
        return (dfd + reg[0], dfd) + reg[1:]

    def obfn_dfd(self):
        """(1/2)||sum_m Df Xf - Sf||^2 (cbpdntv.py:428-435), at rfftn(y_L) when ``fEvalX`` is off."""
        return self._sums[_lib.OUT_DFID] / 2.0

    def obfn_reg(self):
        """lmbda ||Wl1 g_L||_1 + mu sum sqrt(sum_i g_i^2) (cbpdntv.py:439-446)."""
        rl1 = abs(self._wl1_scalar) * self._sums[_lib.OUT_L1]
        rtv = self._sums[_lib.OUT_L21]
        return (self.lmbda * rl1 + self.mu * rtv, rl1, rtv)

    def itstat_extra(self):
        return (self.xrrs,)

    def reconstruct(self, X=None):
        """irfftn(sum_m Df * rfftn(X)), X defaulting to the X variable (cbpdntv.py:563-571)."""
        if X is None:
            return self._dev.reconstruct(_lib.VAR_X)[..., 0]
        self._dev.upload(_lib.VAR_AX, np.asarray(X, dtype=self.dtype))
        return self._dev.reconstruct(_lib.VAR_AX)[..., 0]

    # -- per-kernel timing ---------------------------------------------------------------------
    def profile(self, enable=True):
        self._dev.profile(enable)

    def profile_read(self):
        return self._dev.profile_read()


class ConvBPDNVectorTV(ConvBPDNScalarTV):
    r"""Convolutional BPDN with a vector total-variation term over the coefficient maps: minimise
    (1/2)||sum_m d_m * x_m - s||_2^2 + lambda sum_m ||x_m||_1 +
    mu || sqrt(sum_m sum_i (G_i x_m)^2) ||_1 (reference class: sporco/admm/cbpdntv.py:577-727).
    The l2 norm of the y step and of ``RegTV`` runs over the gradient components and the filter
    axis (per pixel, channel and signal); everything else is :class:`ConvBPDNScalarTV`."""

    _vector_tv = True


class ConvBPDNRecTV(ConvBPDNScalarTV):
    r"""Convolutional BPDN with a total-variation term on the reconstruction: minimise
    (1/2)||sum_m d_m * x_m - s||_2^2 + lambda sum_m ||x_m||_1 +
    mu || sqrt(sum_i (G_i sum_m w_m d_m * x_m)^2) ||_1 (reference class:
    sporco/admm/cbpdntv.py:733-1356); for multi-channel signals the l2 norm also runs over the
    channels.

    The constraint is ``(I; Gamma_0; Gamma_1) x = (y_0; y_1)``: ``Y`` and ``U`` have the shape of
    ``X`` with ``M + 2`` entries on the filter axis, the coefficient block first
    (``block_sep0 / block_sep1 / block_cat``).  The reference solves the x step as a rank-3 iterated
    Sherman-Morrison; its two gradient rows are collinear per frequency, so the device solves a
    rank-one system (scalar or equal ``TVWeight``) or a rank-two one (different weights per filter)
    in closed form, and applies the gradient operators as stencils on signal-shaped maps
    (csrc/csc_rtv.h).  Per iteration: ``rtv_xstep``, ``rtv_ystep``, ``rtv_dual``, driven from the host.

    In scope and refused: as :class:`ConvBPDNScalarTV`.  ``LinSolveCheck`` reports the residual of
    the system the device solves, which is the reference's system.

    IterationStats fields: ``Iter, ObjFun, DFid, RegL1, RegTV, PrimalRsdl, DualRsdl, EpsPrimal,
    EpsDual, Rho, XSlvRelRes, Time``.
    """

    class Options(ConvBPDNScalarTV.Options):
        """ConvBPDN's options plus ``TVWeight`` (cbpdntv.py:823-846): a scalar, or one weight per
        filter."""

    def _yshape(self):
        yshape = list(self.cri.shpX)
        yshape[self.cri.axisM] += len(self.cri.axisN) * self.cri.Cd
        return tuple(yshape)

    def _upload_weights(self):
        if self.Wl1.size == 1:
            self._wl1_scalar = float(self.Wl1.ravel()[0])
            self._dev.set_l1_weight(None)
        else:
            self._wl1_scalar = 1.0
            self._dev.set_l1_weight(cbpdn._broadcastable(self.Wl1, self.cri.shpX))
        self._dev.rtv_setup(np.asarray(self.Wtv, dtype=np.float64).ravel())
        self._tv_ready = True

    # -- the blocks on the device: (VAR_Y, VAR_RTVY1) and (VAR_U, VAR_RTVU1) ------------------------
    _block_vars = {'Y': (_lib.VAR_Y, _lib.VAR_RTVY1), 'U': (_lib.VAR_U, _lib.VAR_RTVU1)}

    def _fetch_blocks(self, which):
        if which not in self._cache:
            v0, v1 = self._block_vars[which]
            a = np.concatenate((self._dev.download(v0), self._dev.download(v1)), axis=self.cri.axisM)
            if which == 'U' and self._u_scale != 1.0:
                a *= a.dtype.type(self._u_scale)
            self._cache[which] = a
        return self._cache[which]

    def _store_blocks(self, which, value):
        value = np.asarray(value, dtype=self.dtype)
        shp = self._yshape()
        if value.size != int(np.prod(shp)):
            raise ValueError("array of shape %s is not a two-block array of shape %s" % (value.shape, shp))
        value = value.reshape(shp)
        v0, v1 = self._block_vars[which]
        self._dev.upload(v0, np.ascontiguousarray(value[..., :self.cri.M]))
        self._dev.upload(v1, np.ascontiguousarray(value[..., self.cri.M:]))
        if which == 'U':
            self._u_scale = 1.0
        self._touch(which)
        if self._tv_ready:
            self._dev.rtv_dual(self._params())      # the spectra the x step reads

    @property
    def Y(self):
        """The coefficient block and the gradient block on the filter axis, ``M + 2`` entries, as
        the reference keeps them."""
        return self._fetch_blocks('Y')

    @Y.setter
    def Y(self, value):
        if value is not None:
            self._store_blocks('Y', value)

    @property
    def U(self):
        return self._fetch_blocks('U')

    @U.setter
    def U(self, value):
        if value is not None:
            self._store_blocks('U', value)

    def block_sep0(self, Y):
        """The coefficient block of Y (cbpdntv.py:972-975)."""
        return Y[..., 0:self.cri.M]

    def block_sep1(self, Y):
        """The gradient block of Y, the gradient index on a new last axis (cbpdntv.py:979-995)."""
        return np.swapaxes(Y[..., self.cri.M:, np.newaxis], self.cri.axisM, -1)

    def block_cat(self, Y0, Y1):
        """(cbpdntv.py:999-1022)"""
        return np.concatenate((Y0, np.swapaxes(Y1, self.cri.axisM, -1)[..., 0]), axis=self.cri.axisM)

    def var_y0(self):
        return self.block_sep0(self.Y)

    def var_y1(self):
        return self.block_sep1(self.Y)

    def var_yx(self):
        return self.var_y0()

    def var_yx_idx(self):
        return np.s_[..., 0:self.cri.M]

    def getmin(self):
        return self.X if self.opt['ReturnX'] else self.var_y0()

    # -- the constraint on host arrays (cbpdntv.py:1237-1315) ---------------------------------------
    def _host_wdf(self):
        return self.Wtv * np.fft.rfftn(np.asarray(self.D, dtype=np.float64), self.cri.Nv, self.cri.axisN)

    def cnst_A0(self, X):
        return X

    def cnst_A0T(self, Y0):
        return Y0

    def cnst_A1(self, X, Xf=None):
        """G_i (sum_m w_m d_m * x_m), the gradient index last: (H, W, C, N, 1, 2)."""
        if Xf is None:
            Xf = np.fft.rfftn(np.asarray(X), axes=self.cri.axisN)
        R = np.fft.irfftn(np.sum(self._host_wdf() * Xf, axis=self.cri.axisM, keepdims=True), self.cri.Nv,
                          self.cri.axisN)
        return np.stack([R - np.roll(R, 1, axis=i) for i in self.cri.axisN], axis=-1)

    def cnst_A1T(self, Y1):
        """Gamma_i^T y_1i per gradient index (last axis): (H, W, C, N, M, 2)."""
        Y1 = np.asarray(Y1)
        Z = np.stack([Y1[..., i] - np.roll(Y1[..., i], -1, axis=ax) for i, ax in enumerate(self.cri.axisN)],
                     axis=-1)
        Zf = np.fft.rfftn(Z, axes=self.cri.axisN)
        return np.fft.irfftn(np.conj(self._host_wdf())[..., np.newaxis] * Zf, self.cri.Nv, self.cri.axisN)

    def cnst_A(self, X, Xf=None):
        return self.block_cat(self.cnst_A0(X), self.cnst_A1(X, Xf))

    def cnst_AT(self, Y):
        return self.cnst_A0T(self.block_sep0(Y)) + np.sum(self.cnst_A1T(self.block_sep1(Y)), axis=-1)

    # -- iteration ----------------------------------------------------------------------------
    def xstep(self):
        """The rank-one / rank-two closed form of the reference's rank-3 system
        (cbpdntv.py:1026-1094; csrc/csc_rtv.h)."""
        out = self._dev.rtv_xstep(self._params())
        for slot in (_lib.OUT_DFID, _lib.OUT_XRRS_D2, _lib.OUT_XRRS_AX2, _lib.OUT_XRRS_B2):
            self._sums[slot] = out[slot]
        self._touch(_lib.VAR_X, _lib.VAR_XF)
        if self.opt['LinSolveCheck']:
            s = self._sums
            nrm = max(np.sqrt(s[_lib.OUT_XRRS_AX2]), np.sqrt(s[_lib.OUT_XRRS_B2]))
            self.xrrs = 0.0 if nrm == 0.0 else np.sqrt(s[_lib.OUT_XRRS_D2]) / nrm
        else:
            self.xrrs = None

    def _yu_steps(self):
        """relax_AX, ystep and ustep (``rtv_ystep``), then the spectra of the new blocks and the
        dual residual norms (``rtv_dual``)."""
        p = self._params()
        out = self._dev.rtv_ystep(p)
        for slot in (_lib.OUT_R2, _lib.OUT_AX2, _lib.OUT_Y2, _lib.OUT_L1, _lib.OUT_L21):
            self._sums[slot] = out[slot]
        self._u_scale = 1.0
        out = self._dev.rtv_dual(p)
        for slot in (_lib.OUT_S2, _lib.OUT_U2):
            self._sums[slot] = out[slot]
        if not self.opt['fEvalX']:
            self._sums[_lib.OUT_DFID] = out[_lib.OUT_DFID]
        self._touch('Y', 'U')

    def relax_AX(self):
        """Part of ``rtv_ystep`` (cbpdntv.py:1319-1339)."""

    def ystep(self):
        """Part of ``rtv_ystep`` (cbpdntv.py:1098-1106)."""

    def rescale_u(self, rsf):
        """Defer ``U /= rsf`` (admm.py:573): the factor rides along as ``u_scale``; the x step applies
        it to the spectra of U and ``rtv_ystep`` to its blocks."""
        self._u_scale = self._u_scale / float(rsf)
        self._touch('U')
