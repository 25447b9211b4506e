"""Robust PCA on the device, with the interface of the reference's ``sporco.admm.rpca`` (sporco/admm/rpca.py:23-262):
:class:`RobustPCA`.

``S``, ``X``, ``Y``, ``U`` are ``(R, C)``.  The x step is singular value thresholding of ``V = S - Y - U`` at
``1 / rho``.  No SVD is taken: the device forms the Gram matrix of the short side of ``V`` in double
(csrc/csc_rpca.h ``rpca_gram``), the host its eigendecomposition ``W diag(sigma^2) W^T`` and ``T = W diag(max(0, 1 -
(1 / rho) / sigma)) W^T`` in float64 (:func:`sporco_amd.prox.svt_matrix`), and one launch does the rest of the
iteration: ``X = V T`` (``T V`` for a wide ``S``), relaxation, the shrinkage of ``Y``, the update of ``U`` and every
sum the loop needs.  ``self.ss`` holds the thresholded singular values, float64, descending, of length
``min(R, C)``.  Under ``fEvalX = False`` ``NrmNuc`` is the sum of the square roots of the eigenvalues of the Gram
matrix of ``S - Y``: a singular value near zero then carries an absolute error of about ``sqrt(eps) sigma_max``.

Served: real float32 / float64, ``S`` a host array or a :class:`sporco_amd.device.DeviceArray` (read in place, not
copied; ``solve()`` then returns device arrays, views of the solver's buffers), ``min(R, C)`` up to 512, any long
side with fewer than 2^31 elements in all, ``fEvalX``, ``gEvalY``, ``Y0`` / ``U0``, ``AutoRho``, ``Callback``,
restart.

Refused: complex, float16 and other dtypes (``TypeError``; the reference's own float16 test, tests/admm/test_rpca.py
``test_03``, is the one test of its file that this class refuses), ``S.ndim != 2``, empty arrays and ``min(S.shape) >
512`` (``ValueError``), ``reducer=`` and pickling (``NotImplementedError``).  There is no CPU path.
"""

import copy
import warnings

import numpy as np

from .. import _lib
from ..device import is_device_array
from ..prox import svt_matrix
from . import admm

__all__ = ['RobustPCA']


class RobustPCA(admm.ADMM):
    r"""ADMM algorithm for  minimise ||X||_* + lambda ||Y||_1  such that  X + Y = S  (rpca.py:23-262).

    ``IterationStats``: ``Iter, ObjFun, NrmNuc, NrmL1, Cnstr, PrimalRsdl, DualRsdl, EpsPrimal, EpsDual, Rho, Time``.
    """

    class Options(admm.ADMM.Options):
        """Options of rpca.py:68-104: ``fEvalX``, ``gEvalY``; ``RelaxParam`` 1.8, ``AutoRho`` enabled with ``Period``
        1, ``AutoScaling``, ``Scaling`` 1000, ``RsdlRatio`` 1.2 and ``RsdlTarget`` 1.0 when unset."""

        defaults = copy.deepcopy(admm.ADMM.Options.defaults)
        defaults.update({'gEvalY': True, 'fEvalX': True, 'RelaxParam': 1.8})
        defaults['AutoRho'].update({'Enabled': True, 'Period': 1, 'AutoScaling': True, 'Scaling': 1000.0,
                                    'RsdlRatio': 1.2})

        def __init__(self, opt=None):
            admm.ADMM.Options.__init__(self, {} if opt is None else opt)
            if self['AutoRho', 'RsdlTarget'] is None:
                self['AutoRho', 'RsdlTarget'] = 1.0

    itstat_fields_objfn = ('ObjFun', 'NrmNuc', 'NrmL1', 'Cnstr')
    hdrtxt_objfn = ('Fnc', 'NrmNuc', u'Nrmℓ1', 'Cnstr')
    hdrval_objfun = {'Fnc': 'ObjFun', 'NrmNuc': 'NrmNuc', u'Nrmℓ1': 'NrmL1', 'Cnstr': 'Cnstr'}

    def __init__(self, S, lmbda=None, opt=None, **backend):
        if opt is None:
            opt = RobustPCA.Options()
        if backend.get('reducer') is not None:
            raise NotImplementedError("rpca: no sharding over processes (reducer=)")
        if not is_device_array(S):
            S = np.asarray(S)
            if np.iscomplexobj(S):
                raise TypeError("rpca handles a real-valued S")
        if len(S.shape) != 2:
            raise ValueError("S has two axes")
        if min(S.shape) < 1:
            raise ValueError("empty S")
        if min(S.shape) > _lib.RPCA_MAX_DIM:
            raise ValueError("an S of shape %s: the kernels serve a short side of up to %d"
                             % (tuple(S.shape), _lib.RPCA_MAX_DIM))
        self.set_dtype(opt, S.dtype)
        if self.dtype not in (np.float32, np.float64):
            raise TypeError("sporco_amd works in float32 or float64, not %s" % self.dtype)
        if is_device_array(S) and S.dtype != self.dtype:
            raise TypeError("a device array S has the working precision, %s" % self.dtype)
        if lmbda is None:
            lmbda = S.shape[0] ** -0.5
        self.lmbda = self.dtype.type(lmbda)
        self.set_attr('rho', opt['rho'], dval=(2.0 * self.lmbda + 0.1), dtype=self.dtype)
        self._shape = tuple(int(v) for v in S.shape)
        self._on_device = is_device_array(S)
        self._dev = _lib.RpcaHandle(self._shape[0], self._shape[1], self.dtype, device=backend.get('device', 0),
                                    stream=backend.get('stream'))
        self._u_scale = 1.0
        self._sums = [0.0] * _lib.OUT_COUNT
        self._cache = {}
        self._have_x = False
        self._nrmnuc_y = None
        self.ss = None
        self.S = S if self._on_device else np.ascontiguousarray(S, dtype=self.dtype)
        self._dev.set_signal(self.S)
        super(RobustPCA, self).__init__(int(np.prod(self._shape)), self._shape, self._shape, self.dtype, opt)

    # -- device state ------------------------------------------------------------------------------------
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
        """rpca.py:149-158: zero, or ``(lambda / rho) sign(Y)`` at a given ``Y0`` (the dual optimality criterion)."""
        if self.opt['Y0'] is None:
            return np.zeros(ushape, dtype=self.dtype)
        return (self.lmbda / self.rho) * np.sign(self.Y)

    def _touch(self, *variables):
        for v in variables:
            self._cache.pop(v, None)

    def _fetch(self, var):
        if var not in self._cache:
            a = self._dev.download(var)
            if var == _lib.RPCA_U and self._u_scale != 1.0:
                a = a * a.dtype.type(self._u_scale)
            self._cache[var] = a
        return self._cache[var]

    def _store(self, var, value):
        value = np.asarray(value, dtype=self.dtype)
        if value.shape != self._shape:
            raise ValueError("array of shape %s where %s is expected" % (value.shape, self._shape))
        self._dev.upload(var, np.ascontiguousarray(value))
        if var == _lib.RPCA_U:
            self._u_scale = 1.0
        self._touch(var)

    @property
    def X(self):
        """The result of the last x step (None before the first iteration)."""
        return self._fetch(_lib.RPCA_X) if self._have_x else None

    @X.setter
    def X(self, value):
        if value is not None:
            raise NotImplementedError("%s: X is the result of the x step; set Y and U" % type(self).__name__)

    @property
    def Y(self):
        return self._fetch(_lib.RPCA_Y)

    @Y.setter
    def Y(self, value):
        if value is not None:
            self._store(_lib.RPCA_Y, value)

    @property
    def U(self):
        return self._fetch(_lib.RPCA_U)

    @U.setter
    def U(self, value):
        if value is not None:
            self._store(_lib.RPCA_U, value)

    def __getstate__(self):
        raise NotImplementedError("%s: pickling is not offered" % type(self).__name__)

    @property
    def runtime(self):
        """The reference's transitional attribute (admm.py:393-403): init plus solve time of :attr:`timer`."""
        warnings.warn("admm.ADMM.runtime attribute has been replaced by an upgraded timer class: please see the "
                      "documentation for admm.ADMM.solve method and util.Timer class", PendingDeprecationWarning)
        return self.timer.elapsed('init') + self.timer.elapsed('solve')

    # -- iteration -----------------------------------------------------------------------------------------
    def solve(self):
        """Start (or re-start) optimisation; returns ``(X, Y)`` (rpca.py:162-166), device arrays where ``S`` is
        one: views of the solver's buffers, which show whatever a later ``solve()`` leaves there."""
        super(RobustPCA, self).solve()
        if self._on_device:
            if self._u_scale != 1.0:      # (the views show U as it is stored; X and Y carry no pending factor)
                self.U = self.U
            return self._dev.device_view(_lib.RPCA_X), self._dev.device_view(_lib.RPCA_Y)
        return self.X, self.Y

    def getmin(self):
        return None

    def iteration(self):
        admm.refuse_step_overrides(self)
        rho = float(self.rho)
        T, _, self.ss = svt_matrix(self._dev.gram(_lib.RPCA_V_SYU, self._u_scale), 1.0 / rho)
        p = _lib.RpcaParams()
        p.rho = rho
        p.lmbda = float(self.lmbda)
        p.rlx = float(self.rlx)
        p.u_scale = float(self._u_scale)
        self._sums = self._dev.iter(p, T)
        self._u_scale = 1.0
        self._have_x = True
        self._touch(_lib.RPCA_X, _lib.RPCA_Y, _lib.RPCA_U)
        self._nrmnuc_y = None
        if not self.opt['fEvalX'] and not self.opt['FastSolve']:
            G = self._dev.gram(_lib.RPCA_V_SY)
            self._nrmnuc_y = float(np.sum(np.sqrt(np.maximum(np.linalg.eigvalsh(0.5 * (G + G.T)), 0.0))))
        if not self._needs_residuals():
            return None
        self.timer.stop('solve_wo_rsdl')
        res = self.compute_residuals()
        self.timer.start('solve_wo_rsdl')
        return res

    def finish_solve(self):
        self._dev.sync()

    def rescale_u(self, rsf):
        """Defer ``U /= rsf`` (admm.py:573): the factor rides along as ``u_scale``; the next Gram matrix and
        iteration apply it, ``self.U`` shows it."""
        self._u_scale = self._u_scale / float(rsf)
        self._touch(_lib.RPCA_U)

    def residual_norms(self):
        """admm.py:462-486 with A = I, B = I, c = S, on the unrelaxed X as the reference's ``AXnr``."""
        s = self._sums
        rho = float(self.rho)
        return (np.sqrt(s[_lib.OUT_R2]), rho * np.sqrt(s[_lib.OUT_S2]),
                max(np.sqrt(s[_lib.OUT_AX2]), np.sqrt(s[_lib.OUT_Y2]), np.sqrt(s[_lib.OUT_C2])),
                rho * np.sqrt(s[_lib.OUT_U2]))

    def eval_objfn(self):
        """rpca.py:214-226: the nuclear norm from the thresholded singular values of the x step (``fEvalX``) or of
        ``S - Y``; the l1 norm of ``Y`` (``gEvalY``) or of ``S - X``; ``||X + Y - S||``."""
        rnn = float(np.sum(self.ss)) if self.opt['fEvalX'] else self._nrmnuc_y
        rl1 = self._sums[_lib.OUT_L1] if self.opt['gEvalY'] else self._sums[_lib.OUT_L21]
        cns = float(np.sqrt(self._sums[_lib.OUT_R2]))
        return (rnn + float(self.lmbda) * rl1, rnn, rl1, cns)

    # -- the constraint's operators on host arrays (rpca.py:230-262) ---------------------------------------------
    def cnst_A(self, X):
        return X

    def cnst_AT(self, X):
        return X

    def cnst_B(self, Y):
        return Y

    def cnst_c(self):
        return self.S
