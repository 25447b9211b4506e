"""ADMM convolutional sparse coding of multi-channel signals with a product dictionary on the GPU.

Drop-in for the four classes of the reference's ``sporco.admm.pdcsc`` (ConvProdDictBPDN
sporco/admm/pdcsc.py:28-192, ConvProdDictBPDNJoint :198-287, ConvProdDictL1L1Grd :293-578,
ConvProdDictL1L1GrdJoint :584-701): same constructor signatures, Options trees, IterationStats fields
and attributes (``X, Y, U, D, B, Gamma, Q, S, rho, lmbda, mu, cri, itstat``; ``W`` for the last two).

The dictionary is the product of a single-channel convolutional dictionary ``D`` and a standard
dictionary ``B`` (``Cs x Cb``) over the channel axis: the coefficient maps have ``Cb`` channels, the
signal ``Cs``.  Only the x step differs from :class:`sporco_amd.admm.cbpdn.ConvBPDN`: with
``B^T B = Q Gamma Q^T`` it is one rank-one (Sherman-Morrison) solve per eigen-channel between two
``Cb x Cb`` channel mixes, one HIP kernel (csrc/csc_pd.hip ``pd_solve``) between the generic forward
and inverse transforms.  The y step, the u step and the residuals are ConvBPDN's (ConvBPDNJoint's) on
a handle with ``Cb`` channels; the iterations are driven from the host.

The last two classes are the reference's model for impulse noise on multi-channel images: the l1 data
fidelity and gradient penalty of :class:`sporco_amd.admm.cbpdn.ConvL1L1Grd` on the two-block constraint
``y0 = D X B^T - S`` (``Cs`` channels), ``y1 = X`` (``Cb`` channels).  Their x step is a diagonal-plus-
rank-one solve per eigen-channel whose right-hand side mixes the two blocks (csrc/csc_pdl1.hip
``pdl1_solve``); it writes the block-0 constraint spectrum as a by-product.  The block steps are
ConvL1L1Grd's and ConvBPDN's (ConvBPDNJoint's), the dual residual is these classes' own
(``pdl1_dual``), and one iteration is one call, ``sporco_amd_csc_pdl1_iter``.
"""

import copy

import numpy as np

from . import admm
from . import cbpdn
from .. import _lib
from .. import cnvrep as cr

__all__ = ['ConvProdDictBPDN', 'ConvProdDictBPDNJoint', 'ConvProdDictL1L1Grd', 'ConvProdDictL1L1GrdJoint']

MAX_CB = 16      # csrc/csc_pd.h kPdMaxCb
_DIM_NOTE = "dimN = 2 (images); the channel mix of the x step is built on the two-dimensional transforms"


class ConvProdDictBPDN(cbpdn.ConvBPDN):
    r"""Minimise (1/2)||D X B^T - S||_2^2 + lambda ||X||_1 by ADMM with the constraint X = Y
    (reference class: sporco/admm/pdcsc.py:28-192).

    In scope: ``dimN = 2``, float32 / float64, ``dimK`` 0 / 1, scalar or array ``L1Weight``,
    ``NonNegCoef``, ``NoBndryCross``, ``AutoRho``, ``RelaxParam``, ``AuxVarObj`` / ``fEvalX`` /
    ``gEvalY``, ``LinSolveCheck``, ``Y0`` / ``U0``, ``setdict(D=, B=)``.  ``HighMemSolve`` is accepted
    and has no effect.  Refused: a multi-channel ``D`` (``ValueError``, as in the reference) and, with
    ``NotImplementedError``, ``dimN`` 1 / 3, complex data, ``reducer=``, resident or device-array
    inputs, wrapping in ``AddMaskSim``, pickling, more than 16 columns in ``B``.

    ``Gamma`` and ``Q`` are the eigendecomposition of ``B^T B`` (``numpy.linalg.eigh``, ``|Gamma|``),
    taken in float64 whatever the solver's dtype.  ``LinSolveCheck`` reports the reference's residual,
    evaluated in eigen-coordinates (``Q`` is orthogonal).

    IterationStats fields: ``Iter, ObjFun, DFid, RegL1, PrimalRsdl, DualRsdl, EpsPrimal, EpsDual, Rho,
    XSlvRelRes, Time``.
    """

    _dim1_ok = False
    _multichannel_dict_ok = False
    _ams_refusal = ("ConvProdDictBPDN cannot be wrapped in AddMaskSim: the appended impulse filter "
                    "would be mixed through B like every other filter")

    class Options(cbpdn.ConvBPDN.Options):
        """The options of ConvBPDN (pdcsc.py:28-56)."""

    def __init__(self, D, B, S, lmbda, opt=None, dimK=None, dimN=2, **backend):
        name = type(self).__name__
        if opt is None:
            opt = ConvProdDictBPDN.Options()
        admm.refuse_backend_extras(name, D, S, dimN, backend, dim_note=_DIM_NOTE, B=B)
        # D acts on X B^T: the coefficient maps have as many channels as B has columns
        # (pdcsc.py:83-93)
        self.cri = cr.CSC_ConvRepIndexing(D, S, dimK=dimK, dimN=dimN)
        if self.cri.Cd > 1:
            raise ValueError('Only single-channel convolutional dictionaries are supported')
        if B.ndim != 2 or B.shape[0] != self.cri.C:
            raise ValueError("B must have one row per channel of S: (%d, Cb)" % self.cri.C)
        if B.shape[1] > MAX_CB:
            raise NotImplementedError("%s: at most %d columns in B (the x step kernels hold one "
                                      "system's channels per thread)" % (name, MAX_CB))
        shpX = list(self.cri.shpX)
        shpX[self.cri.axisC] = B.shape[1]
        self.cri.shpX = tuple(shpX)
        self.set_dtype(opt, S.dtype)
        self.B = np.asarray(B, dtype=self.dtype)
        super(ConvProdDictBPDN, self).__init__(D, S, lmbda, opt, dimK, dimN, **backend)

    # -- device plumbing ------------------------------------------------------------------------
    def _new_handle(self):
        H, W = self.cri.Nv
        # (the handle's channels are those of the coefficient maps)
        self._dev = _lib.Solver(H, W, self.cri.shpX[self.cri.axisC], self.cri.K, self.cri.M, self.dtype,
                                device=self._device, stream=self._stream)
        self._cache = {}
        self._no_x = False
        self._u_scale = 1.0
        self._sums = [0.0] * _lib.OUT_COUNT
        self._wl1_scalar = 1.0
        self._wl21_scalar = 1.0

    def _upload_signal(self):
        """The handle's signal slot holds S (B Q): uploaded with the tables, by ``setdict``."""

    def setdict(self, D=None, B=None):
        """Set the convolutional dictionary ``D`` (internal layout) and / or the standard dictionary
        ``B`` (pdcsc.py:104-133)."""
        first = not hasattr(self, 'Gamma')
        if D is not None:
            self.D = np.asarray(D, dtype=self.dtype)
        if B is not None:
            B = np.asarray(B, dtype=self.dtype)
            if B.shape != self.B.shape:
                raise ValueError("B must keep its shape %s" % (self.B.shape,))
            self.B = B
        if B is not None or first:
            B64 = np.asarray(self.B, dtype=np.float64)
            self.Gamma, self.Q = np.linalg.eigh(B64.T.dot(B64))
            self.Gamma = np.abs(self.Gamma)
            S64 = np.asarray(self.S, dtype=np.float64)
            # S (B Q) along the channel axis: conj(Df) rfftn(.) is the reference's DSfBQ
            Sh = np.moveaxis(np.tensordot(S64, B64.dot(self.Q), axes=([self.cri.axisC], [0])), -1,
                             self.cri.axisC)
            self._dev.set_signal(Sh)
            self._setup_tables(B64)
        if D is not None or first:
            self._dev.set_dict(self.D)
            self._touch(_lib.VAR_DF)
        self.c = None

    def _setup_tables(self, B64):
        self._dev.pd_setup(B64, self.Q, self.Gamma, self.S)

    @property
    def Sf(self):
        """rfftn(S) of the Cs-channel signal (the handle's own signal spectrum is that of S (B Q))."""
        return np.fft.rfftn(self.S, axes=self.cri.axisN).astype(self._dev.cdtype)

    def __getstate__(self):
        raise NotImplementedError("%s: pickling is not offered" % type(self).__name__)

    def _set_ams(self, W):
        raise NotImplementedError(self._ams_refusal)

    # -- iteration: host-driven, staged ---------------------------------------------------------
    def _fused_ok(self):
        return False

    def _device_loop_ok(self):
        return False

    def _flags(self):
        # (the fidelity at Y is pd_dfid's: admm_stats must not evaluate it against S (B Q))
        return super(ConvProdDictBPDN, self)._flags() & ~_lib.FLAG_FEVAL_Y

    def xstep(self):
        """rfftn(Y - U) -> channel mix, scaled rank-one solve per eigen-channel, mix back -> irfftn
        (pdcsc.py:137-159; csrc/csc_pd.h)."""
        p = self._params(0 if self.opt['fEvalX'] else _lib.FLAG_FEVAL_Y)
        out = self._dev.pd_xstep(p)
        for slot in (_lib.OUT_DFID, _lib.OUT_XRRS_D2, _lib.OUT_XRRS_AX2, _lib.OUT_XRRS_B2):
            self._sums[slot] = out[slot]
        self._touch(_lib.VAR_X, _lib.VAR_XF)
        self._set_xrrs()

    def obfn_dfd(self):
        """(1/2)||B sum_m Df_m Xf_m - Sf||^2 by half-spectrum Parseval over the Cs signal channels
        (pdcsc.py:163-171): a by-product of the solve, or evaluated at rfftn(Y) when ``fEvalX`` is off."""
        if self.opt['fEvalX']:
            return self._sums[_lib.OUT_DFID] / 2.0
        return self._dev.pd_dfid(_lib.VAR_Y) / 2.0

    def rhochange(self):
        """Nothing is cached per rho: the denominators are formed in the kernel."""

    def reconstruct(self, X=None):
        """irfftn(B sum_m Df_m rfftn(X)_m), X defaulting to Y: (H, W, Cs, N) (pdcsc.py:184-192)."""
        if X is None:
            return self._dev.pd_reconstruct(_lib.VAR_Y)
        # (VAR_AX is the relaxation buffer of the staged loop: dead between iterations, where the
        # callers of reconstruct(X) are -- not to be called from inside an iteration)
        self._dev.upload(_lib.VAR_AX, np.asarray(X, dtype=self.dtype))
        self._touch(_lib.VAR_AX)
        return self._dev.pd_reconstruct(_lib.VAR_AX)

    def _solve_form_counts(self):
        """(wave-form, generic-form) launches of ``pd_solve`` on this object's handle so far."""
        return (self._dev.query(_lib.QUERY_PD_WAVE_LAUNCHES), self._dev.query(_lib.QUERY_PD_GENERIC_LAUNCHES))


class ConvProdDictBPDNJoint(ConvProdDictBPDN):
    r"""ConvProdDictBPDN with an additional l2,1 term over the channel axis of the coefficient maps,
    mu ||X||_{2,1} (reference class: sporco/admm/pdcsc.py:198-287); the y step is ConvBPDNJoint's.

    IterationStats fields: ``Iter, ObjFun, DFid, RegL1, RegL21, PrimalRsdl, DualRsdl, EpsPrimal,
    EpsDual, Rho, XSlvRelRes, Time``.
    """

    _ams_refusal = ConvProdDictBPDN._ams_refusal.replace('ConvProdDictBPDN', 'ConvProdDictBPDNJoint')

    # the joint term is ConvBPDNJoint's, taken from that class so that the two cannot drift apart (the
    # handle has no L21Weight array: _wl21_scalar stays 1)
    itstat_fields_objfn = cbpdn.ConvBPDNJoint.itstat_fields_objfn
    hdrtxt_objfn = cbpdn.ConvBPDNJoint.hdrtxt_objfn
    hdrval_objfun = cbpdn.ConvBPDNJoint.hdrval_objfun
    _mu_eff = cbpdn.ConvBPDNJoint._mu_eff
    _stats_flags = cbpdn.ConvBPDNJoint._stats_flags
    ystep = cbpdn.ConvBPDNJoint.ystep
    obfn_reg = cbpdn.ConvBPDNJoint.obfn_reg

    def __init__(self, D, B, S, lmbda, mu=0.0, opt=None, dimK=None, dimN=2, **backend):
        self.mu = None
        super(ConvProdDictBPDNJoint, self).__init__(D, B, S, lmbda, opt, dimK, dimN, **backend)
        self.mu = self.dtype.type(mu)

    def _flags(self):
        return super(ConvProdDictBPDNJoint, self)._flags() | _lib.FLAG_JOINT


class ConvProdDictL1L1Grd(cbpdn.ConvL1L1Grd):
    r"""Minimise ||W (D X B^T - S)||_1 + lambda ||X||_1 + (mu/2) sum_i ||G_i X||_2^2 by ADMM with the
    two-block constraint y0 = D X B^T - S, y1 = X (reference class: sporco/admm/pdcsc.py:293-578).

    In scope: ``dimN = 2``, float32 / float64, ``dimK`` 0 / 1, ``W``, scalar or array ``L1Weight``,
    scalar or per-filter ``GradWeight``, ``NonNegCoef``, ``NoBndryCross``, ``AutoRho`` (off by default),
    ``RelaxParam``, ``AuxVarObj``, ``LinSolveCheck``, ``Y0`` / ``U0`` (the composite arrays), ``ReturnVar``,
    ``setdict(D=, B=)``.  ``HighMemSolve`` is accepted and has no effect.  Refused: a multi-channel ``D``
    (``ValueError``, as in the reference) and, with ``NotImplementedError``, ``dimN`` 1 / 3, complex data,
    ``reducer=``, resident or device-array inputs, wrapping in ``AddMaskSim``, pickling, more than 16
    columns in ``B``.

    ``Y`` and ``U`` are the reference's composite arrays ``(H, W, y0I + y1I)``, block 0 first
    (``block_sep0`` / ``block_sep1`` / ``block_cat``, pdcsc.py:407-446); ``X`` is ``(H, W, Cb, N, K)``.
    ``Gamma`` and ``Q`` are taken in float64 whatever the solver's dtype.  The x step is exact for a
    per-filter ``GradWeight``; ``LinSolveCheck`` reports the reference's residual, evaluated in
    eigen-coordinates (``Q`` is orthogonal).

    IterationStats fields: ``Iter, ObjFun, DFid, RegL1, RegGrad, PrimalRsdl, DualRsdl, EpsPrimal,
    EpsDual, Rho, XSlvRelRes, Time``; ``DFid`` is the l1 sum itself (no factor 1/2).
    """

    _multichannel_dict_ok = False
    _ams_refusal = ConvProdDictBPDN._ams_refusal.replace('ConvProdDictBPDN', 'ConvProdDictL1L1Grd')

    class Options(cbpdn.ConvL1L1Grd.Options):
        """The options of ConvL1L1Grd (pdcsc.py:293-325)."""

    # the product-dictionary plumbing is ConvProdDictBPDN's, taken from that class so that the two
    # cannot drift apart
    _new_handle = ConvProdDictBPDN._new_handle
    _upload_signal = ConvProdDictBPDN._upload_signal
    setdict = ConvProdDictBPDN.setdict
    Sf = ConvProdDictBPDN.Sf
    _set_ams = ConvProdDictBPDN._set_ams

    def __init__(self, D, B, S, lmbda, mu, W=None, opt=None, dimK=0, dimN=2, **backend):
        name = type(self).__name__
        if opt is None:
            opt = type(self).Options()
        admm.refuse_backend_extras(name, D, S, dimN, backend, dim_note=_DIM_NOTE, B=B)
        # the reference hands its base class S B so that the arrays get Cb channels, then corrects the
        # shapes (pdcsc.py:363-403); here the indexing is built on S and the coefficient maps' channel
        # count is set, as in ConvProdDictBPDN
        self.cri = cr.CSC_ConvRepIndexing(D, S, dimK=dimK, dimN=dimN)
        if self.cri.Cd > 1:
            raise ValueError('Only single-channel convolutional dictionaries are supported')
        if B.ndim != 2 or B.shape[0] != self.cri.C:
            raise ValueError("B must have one row per channel of S: (%d, Cb)" % self.cri.C)
        if B.shape[1] > MAX_CB:
            raise NotImplementedError("%s: at most %d columns in B (the x step kernels hold one "
                                      "system's channels per thread)" % (name, MAX_CB))
        shpX = list(self.cri.shpX)
        shpX[self.cri.axisC] = B.shape[1]
        self.cri.shpX = tuple(shpX)
        self.set_dtype(opt, S.dtype)
        self.B = np.asarray(B, dtype=self.dtype)
        super(ConvProdDictL1L1Grd, self).__init__(D, S, lmbda, mu, W, opt, dimK=dimK, dimN=dimN, **backend)
        # (the reference's constraint count is that of its base class, which saw S B: pdcsc.py:372)
        self.Nc = int(np.prod(self.cri.shpX)) + int(np.prod(self.cri.shpX)) // self.cri.M

    # -- the composite layout of Y and U (pdcsc.py:396-446) -----------------------------------------
    @property
    def y0shp(self):
        return self.cri.shpS

    @property
    def y1shp(self):
        return self.cri.shpX

    @property
    def y0I(self):
        return int(np.prod(self.y0shp[self.cri.axisC:]))

    @property
    def y1I(self):
        return int(np.prod(self.y1shp[self.cri.axisC:]))

    @property
    def yshp(self):
        return self.cri.shpX[0:self.cri.axisC] + (self.y0I + self.y1I,)

    def block_sep0(self, Y):
        shp = Y.shape[0:self.cri.axisC] + self.y0shp[self.cri.axisC:]
        return Y[(slice(None),) * self.cri.axisC + (slice(0, self.y0I),)].reshape(shp)

    def block_sep1(self, Y):
        shp = Y.shape[0:self.cri.axisC] + self.y1shp[self.cri.axisC:]
        return Y[(slice(None),) * self.cri.axisC + (slice(self.y0I, None),)].reshape(shp)

    def block_cat(self, Y0, Y1):
        return np.concatenate((Y0.reshape(Y0.shape[0:self.cri.axisC] + (-1,)),
                               Y1.reshape(Y1.shape[0:self.cri.axisC] + (-1,))), axis=self.cri.axisC)

    def _set_blocks(self, A, var0, var1):
        """Store a composite two-block array: block 0 in the handle's Cs-channel buffers."""
        A = np.asarray(A, dtype=self.dtype)
        if A.shape != self.yshp:
            raise ValueError("array of shape %s is not a composite [block 0; block 1] array of shape %s"
                             % (A.shape, self.yshp))
        self._dev.pdl1_block0(0 if var0 == _lib.VAR_MY0 else 1, np.ascontiguousarray(self.block_sep0(A)))
        self._dev.upload(var1, np.ascontiguousarray(self.block_sep1(A)))
        self._touch(var1)

    def var_y0(self):
        return self._dev.pdl1_block0(0)

    @property
    def U(self):
        u0 = self._dev.pdl1_block0(1)
        if self._u_scale != 1.0:
            u0 *= u0.dtype.type(self._u_scale)
        return self.block_cat(u0, self._fetch(_lib.VAR_U))

    @U.setter
    def U(self, value):
        if value is not None:
            raise NotImplementedError("the blocks of U are device state")

    # -- device plumbing ------------------------------------------------------------------------
    def _mask_array(self):
        W = getattr(self, 'W', None)
        if W is None or (W.size == 1 and float(W.ravel()[0]) == 1.0):
            return None
        return W[..., 0]

    def _setup_tables(self, B64):
        """The tables, the Cs-channel signal and the mask; block 0 is created at zero by the first call
        and kept by later ones."""
        self._dev.pdl1_setup(B64, self.Q, self.Gamma, self.S, self._mask_array())

    def _upload_mask(self):
        self._setup_tables(np.asarray(self.B, dtype=np.float64))

    def _init_blocks(self):
        """Both blocks start at zero: block 1 with the handle, block 0 with ``_setup_tables``."""

    def _device_iteration(self, p):
        p.flags |= _lib.FLAG_GRADREG
        return self._dev.pdl1_iter(p)

    def residual_norms(self):
        """admm.py:1404-1437 with the dual residual of pdcsc.py:568-578: s = rho ||A^T U|| and
        sn = rho ||U||, both at the new U; the first norm is summed on the device in the frequency
        domain."""
        s = self._sums
        rho = float(self.rho)
        nr = np.sqrt(s[_lib.OUT_R2] + s[_lib.OUT_R02])
        ns = rho * np.sqrt(s[_lib.OUT_S2])
        rn = max(np.sqrt(s[_lib.OUT_AX2] + s[_lib.OUT_RGR]),
                 np.sqrt(s[_lib.OUT_Y2] + s[_lib.OUT_CNSTR]), self._nrm_c)
        sn = rho * np.sqrt(s[_lib.OUT_U2] + s[_lib.OUT_CGIT])
        return nr, ns, rn, sn

    def reconstruct(self, X=None):
        """irfftn(B sum_m Df_m rfftn(X)_m), X defaulting to the X variable: (H, W, Cs, N)
        (pdcsc.py:554-562)."""
        if X is None:
            return self._dev.pd_reconstruct(_lib.VAR_X)
        self._dev.upload(_lib.VAR_AX, np.asarray(X, dtype=self.dtype))
        self._touch(_lib.VAR_AX)
        return self._dev.pd_reconstruct(_lib.VAR_AX)

    def _solve_form_counts(self):
        """(wave-form, generic-form) launches of ``pdl1_solve`` on this object's handle so far."""
        return (self._dev.query(_lib.QUERY_PDL1_WAVE_LAUNCHES), self._dev.query(_lib.QUERY_PDL1_GENERIC_LAUNCHES))


class ConvProdDictL1L1GrdJoint(ConvProdDictL1L1Grd):
    r"""ConvProdDictL1L1Grd with the l2,1 norm over the channel axis of the coefficient maps in the l1
    norm's place, lambda ||X||_{2,1} (reference class: sporco/admm/pdcsc.py:584-701): block 1 is
    prox_sl1l2(., 0, (lambda / rho) L21Weight), ConvBPDNJoint's epilogue with a zero l1 weight.
    ``L1Weight`` is ignored, as in the reference; ``L21Weight`` must be a scalar.

    IterationStats fields: ``Iter, ObjFun, DFid, RegL21, RegGrad, PrimalRsdl, DualRsdl, EpsPrimal,
    EpsDual, Rho, XSlvRelRes, Time``.
    """

    _ams_refusal = ConvProdDictBPDN._ams_refusal.replace('ConvProdDictBPDN', 'ConvProdDictL1L1GrdJoint')

    class Options(ConvProdDictL1L1Grd.Options):
        """Adds ``L21Weight`` (pdcsc.py:618-637): a scalar here."""

        defaults = copy.deepcopy(ConvProdDictL1L1Grd.Options.defaults)
        defaults.update({'L21Weight': 1.0})

    itstat_fields_objfn = ('ObjFun', 'DFid', 'RegL21', 'RegGrad')
    hdrtxt_objfn = ('Fnc', 'DFid', u'Reg\u21132,1', u'Reg\u21132\u2207')
    hdrval_objfun = {'Fnc': 'ObjFun', 'DFid': 'DFid', u'Reg\u21132,1': 'RegL21', u'Reg\u21132\u2207': 'RegGrad'}

    def __init__(self, D, B, S, lmbda, mu=0.0, opt=None, dimK=None, dimN=2, **backend):
        # (with opt=None the reference fails on opt['L21Weight']: default options instead)
        if opt is None:
            opt = ConvProdDictL1L1GrdJoint.Options()
        w = opt['L21Weight'] if 'L21Weight' in opt else 1.0
        if np.ndim(w) > 0 and np.size(w) != 1:
            raise NotImplementedError("ConvProdDictL1L1GrdJoint: a scalar L21Weight (the handle has no "
                                      "l2,1 weight array)")
        self.wl21 = np.asarray(w, dtype=np.float64).reshape(())
        super(ConvProdDictL1L1GrdJoint, self).__init__(D, B, S, lmbda, mu, None, opt, dimK=dimK, dimN=dimN,
                                                       **backend)
        self.wl21 = np.asarray(self.wl21, dtype=self.dtype)
        self._wl21_scalar = float(self.wl21)

    def _upload_weights(self):
        # (L1Weight is ignored, pdcsc.py:681-701: the handle keeps no l1 weight array)
        self.wl1 = np.ones((1,) * 5, dtype=self.dtype)
        super(ConvProdDictL1L1GrdJoint, self)._upload_weights()
        self._wl21_scalar = float(self.wl21)

    def _lmbda_eff(self):
        # the l2,1 threshold of the device step is (lmbda / rho) L21Weight
        return float(self.lmbda) * self._wl21_scalar

    def _device_iteration(self, p):
        p.flags |= _lib.FLAG_JOINT
        return super(ConvProdDictL1L1GrdJoint, self)._device_iteration(p)

    def eval_objfn(self):
        """||W g0||_1 + lmbda ||wl21 g1||_{2,1} + (mu/2) sum_i ||Wgrd^(1/2) G_i x||^2 (pdcsc.py:696-701)."""
        g0v = self._sums[_lib.OUT_DFID]
        g1v = self._wl21_scalar * self._sums[_lib.OUT_L21]
        rgr = self._wg_scalar * self._sums[_lib.OUT_RGRX] / 2.0
        return (g0v + self.lmbda * g1v + self.mu * rgr, g0v, g1v, rgr)
