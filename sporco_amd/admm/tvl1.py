"""ADMM l1-TV denoising on the device: a drop-in for the reference's
``sporco.admm.tvl1.TVL1Denoise`` (sporco/admm/tvl1.py:27-399), the denoiser of its ``tvl1den_gry`` /
``tvl1den_clr`` examples and the natural pre-processing step for impulse noise.

    minimise || Wdf (x - s) ||_1 + lmbda || Wtv sqrt((G_0 x)^2 + (G_1 x)^2) ||_1

on the constraint (G_0; G_1; I) x - (y_0; y_1; y_d) = (0; 0; s): ``Y`` and ``U`` have shape
``S.shape + (3,)``, the last block the data block.  Like :mod:`sporco_amd.admm.tvl2` nothing here is an FFT
problem.  The x step is the same Jacobi sweep (with rho = 1 and a unit weight, tvl1.py:240-260) on the
three-block adjoint A^T (Y - U), which includes the identity block; the y step -- the l2 shrinkage of the
gradient blocks and the soft threshold ``prox_l1(AX_d + U_d - S, Wdf / rho)`` of the data block -- and the
adjoint are stencil kernels of their own (``tvl1_ystep``, ``tvl1_adjoint`` in csrc/csc_tvd.h).  The dual
residual is ``rho ||A^T U||`` and its normaliser ``rho ||U||`` (tvl1.py:362-372): no ``Y - Yprev`` is kept.
With the default ``MaxGSIter = 2`` an iteration is four launches and one read of its sums.

Served: the surface of :class:`sporco_amd.admm.tvl2.TVL2Denoise` -- float32 / float64 real ``S`` of shape
(H, W) or (H, W, ...) with up to two trailing axes, H, W >= 2, ``axes == (0, 1)``; ``caxis=None`` or
``caxis=2`` (vector TV over at most 8 channels); ``DFidWeight`` a scalar or an array that broadcasts to
``S`` (it enters linearly; a zero weight leaves ``y_d`` unshrunk); ``TVWeight`` a scalar or, with
``caxis=None``, an array of ``S.ndim`` axes that broadcasts to ``S``; ``Y0`` / ``U0`` of shape
``S.shape + (3,)``.  ``S`` and ``DFidWeight`` may be :class:`sporco_amd.device.DeviceArray`; ``solve()``
and ``getmin()`` then return one.

Refused with ``NotImplementedError``: complex ``S``, other ``axes``, other ``caxis``, H or W of 1, an array
``TVWeight`` together with ``caxis``, pickling, ``reducer=``; other dtypes with ``TypeError``.

:class:`TVL1Deconv` (sporco/admm/tvl1.py:403-758) is the deconvolution problem

    minimise || Wdf (H x - s) ||_1 + lmbda || Wtv sqrt((G_0 x)^2 + (G_1 x)^2) ||_1

on (G_0; G_1; H) x - y = (0; 0; s), with H the circular convolution by a kernel ``A`` and CIRCULAR gradients.
The x step is a pointwise solve between one forward transform of two planes per image plane and one inverse
transform that returns X and H X; the rest are periodic stencil kernels (csrc/csc_tvdc.h).  The dual residual
``rho ||A^T U||`` needs ``H^T U_d`` and is formed over spectra.  The surface is that of
:class:`sporco_amd.admm.tvl2.TVL2Deconv` plus ``DFidWeight``.
"""

import copy

import numpy as np

from .. import _lib
from ..device import is_device_array
from . import _tvd
from . import _tvdc

__all__ = ['TVL1Denoise', 'TVL1Deconv', 'plan', 'plan_deconv']


def plan(shape, dtype=np.float32, caxis=None):
    """The kernels' launch plan for an ``S`` of ``shape``, as :func:`sporco_amd.admm.tvl2.plan`."""
    return _tvd.plan(shape, dtype, caxis, l1=True)


class TVL1Denoise(_tvd.TVDenoise):
    r"""ADMM algorithm for the l1-TV denoising problem; interface of sporco/admm/tvl1.py:27-399.

    ``IterationStats``: ``Iter, ObjFun, DFid, RegTV, PrimalRsdl, DualRsdl, EpsPrimal, EpsDual, Rho,
    GSIter, GSRelRes, Time``.
    """

    NBLK = 3
    L1_HANDLE = True

    class Options(_tvd.TVDenoise.Options):
        """Adds ``gEvalY``, ``MaxGSIter``, ``GSTol``, ``DFidWeight``, ``TVWeight`` (tvl1.py:98-141)."""

    def u_from_y0(self, Y):
        """tvl1.py:223-236: the dual optimality criterion (3.10) of boyd-2010-distributed at a non-zero Y."""
        Yg = Y[..., 0:-1]
        Yss = np.sqrt(np.sum(Yg ** 2, axis=len(self._shape), keepdims=True))
        U0 = (self.lmbda / self.rho) * np.divide(Yg, Yss, out=np.zeros_like(Yg), where=(Yss != 0))
        U1 = (1.0 / self.rho) * np.sign(Y[..., -1:])
        return np.concatenate((U0, U1), axis=len(self._shape))

    # -- the constraint on host arrays (tvl1.py:317-358) ------------------------------------------------
    def cnst_A(self, X):
        X = np.asarray(X)
        return np.stack([_tvd.grad(X, ax) for ax in self.axes] + [X], axis=X.ndim)

    def cnst_AT(self, Y):
        Y = np.asarray(Y)
        out = Y[..., -1].copy()
        for i, ax in enumerate(self.axes):
            out += _tvd.grad_t(Y[..., i], ax)
        return out

    def cnst_c(self):
        c = np.zeros(self._shape + (self.NBLK,), self.dtype)
        c[..., -1] = self.S.get() if self._dev_io else self.S
        return c

    def residual_norms(self):
        """r = ||A X - Y - c||, rn = max(||A X||, ||Y||, ||c||) (admm.py:722-775), and the class's own
        s = rho ||A^T U||, sn = rho ||U|| (tvl1.py:362-372)."""
        s = self._sums
        rho = float(self.rho)
        return (np.sqrt(s[_lib.OUT_R2]), rho * np.sqrt(s[_lib.OUT_S2]),
                max(np.sqrt(s[_lib.OUT_AX2]), np.sqrt(s[_lib.OUT_Y2]), np.sqrt(s[_lib.OUT_C2])),
                rho * np.sqrt(s[_lib.OUT_U2]))

    def eval_objfn(self):
        """DFid = sum |Wdf g_d|, RegTV = sum Wtv sqrt(sum g_g^2) (tvl1.py:290-306)."""
        dfd = self._sums[_lib.OUT_DFID]
        reg = self._sums[_lib.OUT_L21]
        return (dfd + float(self.lmbda) * reg, dfd, reg)


def plan_deconv(shape, dtype=np.float32, caxis=None):
    """The launch plan of :class:`TVL1Deconv`, as :func:`sporco_amd.admm.tvl2.plan_deconv`."""
    return _tvdc.plan(shape, dtype, caxis, l1=True)


class TVL1Deconv(_tvdc.TVDeconv):
    r"""ADMM algorithm for the l1-TV deconvolution problem; interface of sporco/admm/tvl1.py:403-758.

    ``IterationStats``: ``Iter, ObjFun, DFid, RegTV, PrimalRsdl, DualRsdl, EpsPrimal, EpsDual, Rho,
    XSlvRelRes, Time``.
    """

    NBLK = 3
    L1_HANDLE = True

    class Options(_tvdc.TVDeconv.Options):
        """Adds ``gEvalY``, ``LinSolveCheck``, ``DFidWeight``, ``TVWeight`` (tvl1.py:475-516); ``AutoRho`` is
        disabled."""

        defaults = copy.deepcopy(_tvdc.TVDeconv.Options.defaults)
        defaults.update({'DFidWeight': 1.0})
        defaults['AutoRho'].update({'Enabled': False})

    def _dfid_weight(self, opt, S, name):
        wdf = opt['DFidWeight']
        if is_device_array(wdf):
            if wdf.shape != tuple(S.shape) or wdf.dtype != self.dtype:
                raise ValueError("a DeviceArray DFidWeight has the shape and dtype of S")
            return wdf
        if np.iscomplexobj(wdf):
            raise NotImplementedError("%s handles real-valued weights" % name)
        w = np.asarray(wdf, dtype=self.dtype)
        if w.ndim > 0:
            np.broadcast_to(w, S.shape)      # (raises where it does not broadcast)
        return w

    def u_from_y0(self, Y):
        """tvl1.py:612-625: the dual optimality criterion (3.10) of boyd-2010-distributed at a non-zero Y."""
        Yg = Y[..., 0:-1]
        Yss = np.sqrt(np.sum(Yg ** 2, axis=len(self._shape), keepdims=True))
        U0 = (self.lmbda / self.rho) * np.divide(Yg, Yss, out=np.zeros_like(Yg), where=(Yss != 0))
        U1 = (1.0 / self.rho) * np.sign(Y[..., -1:])
        return np.concatenate((U0, U1), axis=len(self._shape))

    @property
    def GAf(self):
        def make():
            # (Gf has singleton trailing axes; a kernel per plane broadcasts it)
            shp = np.broadcast_shapes(self.Gf.shape[:-1], self.Af.shape)
            return np.concatenate((np.broadcast_to(self.Gf, shp + (2,)),
                                   np.broadcast_to(self.Af, shp)[..., np.newaxis]), axis=-1)
        return self._spectrum('GAf', make)

    # -- the constraint on host arrays (tvl1.py:701-743) ------------------------------------------------
    def cnst_A(self, X, Xf=None):
        if Xf is None:
            X = np.asarray(X)
            Xf = np.fft.rfftn(X, axes=self.axes)
        else:
            X = self._irfft(Xf)
        HX = np.fft.irfftn(self.Af * Xf, s=self.axsz, axes=self.axes).astype(X.dtype)
        return np.stack([_tvdc.pgrad(X, ax) for ax in self.axes] + [HX], axis=X.ndim)

    def cnst_AT(self, Y):
        Y = np.asarray(Y)
        out = np.fft.irfftn(np.conj(self.Af) * np.fft.rfftn(Y[..., -1], axes=self.axes), s=self.axsz,
                            axes=self.axes).astype(Y.dtype)
        for i, ax in enumerate(self.axes):
            out += _tvdc.pgrad_t(Y[..., i], ax)
        return out

    def cnst_c(self):
        c = np.zeros(self._shape + (self.NBLK,), self.dtype)
        c[..., -1] = self._host(self.S)
        return c

    def residual_norms(self):
        """r = ||A X - Y - c||, rn = max(||A X||, ||Y||, ||c||) (admm.py:722-775), and the class's own
        s = rho ||A^T U||, sn = rho ||U|| (tvl1.py:747-757)."""
        s = self._sums
        rho = float(self.rho)
        return (np.sqrt(s[_lib.OUT_R2]), rho * np.sqrt(s[_lib.OUT_S2]),
                max(np.sqrt(s[_lib.OUT_AX2]), np.sqrt(s[_lib.OUT_Y2]), np.sqrt(s[_lib.OUT_C2])),
                rho * np.sqrt(s[_lib.OUT_U2]))

    def eval_objfn(self):
        """DFid = sum |Wdf g_d|, RegTV = sum Wtv sqrt(sum g_g^2) (tvl1.py:674-690)."""
        dfd = self._sums[_lib.OUT_DFID]
        reg = self._sums[_lib.OUT_L21]
        return (dfd + float(self.lmbda) * reg, dfd, reg)
