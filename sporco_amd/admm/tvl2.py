"""ADMM l2-TV denoising on the device: a drop-in for the reference's
``sporco.admm.tvl2.TVL2Denoise`` (sporco/admm/tvl2.py:27-372), the pre-processing step of its masked
examples (``sl = TVL2Denoise(imgwp, lmbda, opt).solve(); sh = mskp * (imgwp - sl)``).

    minimise (1/2) || Wdf (x - s) ||^2 + lmbda || Wtv sqrt((G_0 x)^2 + (G_1 x)^2) ||_1

on the constraint (G_0; G_1) x = (y_0; y_1).  Nothing here is an FFT problem: G_i is the forward
difference along axis i with a zero last row, and the x step (Jacobi sweeps), the y / u steps and the
constraint adjoint are nearest-neighbour stencil kernels (csrc/csc_tvd.h): with the default
``MaxGSIter = 2`` an iteration is four launches and one read of its sums.  The loop is host-driven,
``admm.ADMM`` keeps the residual, ``AutoRho`` and stopping logic.

Served: float32 / float64 real ``S`` of shape (H, W) or (H, W, ...) with up to two trailing axes,
H, W >= 2, ``axes == (0, 1)``; ``caxis=None`` (planes independent) or ``caxis=2`` (vector TV over at
most 8 channels); ``DFidWeight`` a scalar or an array that broadcasts to ``S``; ``TVWeight`` a scalar
or, with ``caxis=None``, an array of ``S.ndim`` axes that broadcasts to ``S``.  ``S`` and ``DFidWeight``
may be :class:`sporco_amd.device.DeviceArray`; ``solve()`` and ``getmin()`` then return one.

Refused with ``NotImplementedError``: complex ``S``, other ``axes`` (the reference's three-axis volumes
included), other ``caxis``, H or W of 1, an array ``TVWeight`` together with ``caxis`` (the reference's
own broadcast fails there for several images), pickling, ``reducer=``.  The l1-fidelity denoiser is
:mod:`sporco_amd.admm.tvl1`.

:class:`TVL2Deconv` (sporco/admm/tvl2.py:377-702) is the deconvolution problem

    minimise (1/2) || H x - s ||^2 + lmbda || Wtv sqrt((G_0 x)^2 + (G_1 x)^2) ||_1

with H the circular convolution by a kernel ``A`` and CIRCULAR gradients.  Its x step is a pointwise solve
between one forward and one inverse transform; the gradients, their adjoint and the y / u steps are periodic
stencil kernels (csrc/csc_tvdc.h).  It serves the same ``S``, ``caxis`` and ``TVWeight`` as the denoiser, a
real ``A`` no larger than the image whose trailing axes are absent, all 1 or those of ``S``, and
``LinSolveCheck``; ``S`` and ``A`` may be device arrays.
"""

import numpy as np

from .. import _lib
from . import _tvd
from . import _tvdc

__all__ = ['TVL2Denoise', 'TVL2Deconv', 'plan', 'plan_deconv']


def plan(shape, dtype=np.float32, caxis=None):
    """The kernels' launch plan for an ``S`` of ``shape``: ``dict(V, items, strips, R, nseg, TW)``
    -- elements per item, items per row, strips per row, rows per segment, segments, and the columns
    a strip of 256 items covers."""
    return _tvd.plan(shape, dtype, caxis)


class TVL2Denoise(_tvd.TVDenoise):
    r"""ADMM algorithm for the l2-TV denoising problem; interface of sporco/admm/tvl2.py:27-372.

    ``IterationStats``: ``Iter, ObjFun, DFid, RegTV, PrimalRsdl, DualRsdl, EpsPrimal, EpsDual, Rho,
    GSIter, GSRelRes, Time``.
    """

    NBLK = 2

    class Options(_tvd.TVDenoise.Options):
        """Adds ``gEvalY``, ``MaxGSIter``, ``GSTol``, ``DFidWeight``, ``TVWeight`` (tvl2.py:98-141)."""

    def u_from_y0(self, Y):
        """tvl2.py:223-233: the dual optimality criterion (3.10) of boyd-2010-distributed at a non-zero Y."""
        Yss = np.sqrt(np.sum(Y ** 2, axis=len(self._shape), keepdims=True))
        q = np.divide(Y, Yss, out=np.zeros_like(Y), where=(Yss != 0))
        return (self.lmbda / self.rho) * q

    # -- the constraint on host arrays (tvl2.py:307-345) ------------------------------------------------
    def cnst_A(self, X):
        X = np.asarray(X)
        return np.stack([_tvd.grad(X, ax) for ax in self.axes], axis=X.ndim)

    def cnst_AT(self, Y):
        Y = np.asarray(Y)
        out = np.zeros(Y.shape[:-1], dtype=Y.dtype)
        for i, ax in enumerate(self.axes):
            out += _tvd.grad_t(Y[..., i], ax)
        return out

    def cnst_c(self):
        return np.zeros(self._shape + (len(self.axes),), self.dtype)

    def residual_norms(self):
        """admm.py:722-775 for the general constraint with c = 0."""
        s = self._sums
        rho = float(self.rho)
        return (np.sqrt(s[_lib.OUT_R2]), rho * np.sqrt(s[_lib.OUT_S2]),
                max(np.sqrt(s[_lib.OUT_AX2]), np.sqrt(s[_lib.OUT_Y2])), rho * np.sqrt(s[_lib.OUT_U2]))

    def eval_objfn(self):
        """DFid = (1/2) ||Wdf (X - S)||^2, RegTV = sum Wtv sqrt(sum g^2) (tvl2.py:281-296)."""
        dfd = 0.5 * self._sums[_lib.OUT_DFID]
        reg = self._sums[_lib.OUT_L21]
        return (dfd + float(self.lmbda) * reg, dfd, reg)


def plan_deconv(shape, dtype=np.float32, caxis=None):
    """The launch plan of :class:`TVL2Deconv` for an ``S`` of ``shape``: ``dict(V, items, strips, R, nseg, TW,
    SV, sblocks)`` -- as :func:`plan` for the stencil kernels, then the planes per access and the
    workgroups of the pointwise solve."""
    return _tvdc.plan(shape, dtype, caxis)


class TVL2Deconv(_tvdc.TVDeconv):
    r"""ADMM algorithm for the l2-TV deconvolution problem; interface of sporco/admm/tvl2.py:377-702.

    ``IterationStats``: ``Iter, ObjFun, DFid, RegTV, PrimalRsdl, DualRsdl, EpsPrimal, EpsDual, Rho,
    XSlvRelRes, Time``.
    """

    NBLK = 2

    class Options(_tvdc.TVDeconv.Options):
        """Adds ``gEvalY``, ``LinSolveCheck``, ``TVWeight`` (tvl2.py:448-486); ``AutoRho`` is enabled."""

    def u_from_y0(self, Y):
        """tvl2.py:580-590: the dual optimality criterion (3.10) of boyd-2010-distributed at a non-zero Y."""
        Yss = np.sqrt(np.sum(Y ** 2, axis=len(self._shape), keepdims=True))
        q = np.divide(Y, Yss, out=np.zeros_like(Y), where=(Yss != 0))
        return (self.lmbda / self.rho) * q

    # -- the constraint on host arrays (tvl2.py:662-701) ------------------------------------------------
    def cnst_A(self, X, Xf=None):
        X = self._irfft(Xf) if X is None else np.asarray(X)
        return np.stack([_tvdc.pgrad(X, ax) for ax in self.axes], axis=X.ndim)

    def cnst_AT(self, Y):
        Y = np.asarray(Y)
        out = np.zeros(Y.shape[:-1], dtype=Y.dtype)
        for i, ax in enumerate(self.axes):
            out += _tvdc.pgrad_t(Y[..., i], ax)
        return out

    def cnst_c(self):
        return np.zeros(self._shape + (len(self.axes),), self.dtype)

    def residual_norms(self):
        """admm.py:722-775 for the general constraint with c = 0: s = rho ||A^T (Y - Yprev)||,
        sn = rho ||A^T U||."""
        s = self._sums
        rho = float(self.rho)
        return (np.sqrt(s[_lib.OUT_R2]), rho * np.sqrt(s[_lib.OUT_S2]),
                max(np.sqrt(s[_lib.OUT_AX2]), np.sqrt(s[_lib.OUT_Y2])), rho * np.sqrt(s[_lib.OUT_U2]))

    def eval_objfn(self):
        """DFid = (1/2) ||H X - S||^2 over spectra, RegTV = sum Wtv sqrt(sum g^2) (tvl2.py:635-651)."""
        dfd = 0.5 * self._sums[_lib.OUT_DFID]
        reg = self._sums[_lib.OUT_L21]
        return (dfd + float(self.lmbda) * reg, dfd, reg)
