"""The dictionary update of the dense (patch-based) family on the device, with the interface of the reference's
``sporco.admm.cmod`` (sporco/admm/cmod.py:21-342): :class:`CnstrMOD`, :func:`getPcn`, :func:`zeromean`,
:func:`normalise`.

The coefficients ``Z`` are ``(M, K)``, the signals ``S`` ``(N, K)``, the dictionary variables ``(N, M)``.  The x
step is ``X = (S Z^T + rho (Y - U)) Q`` with ``Q = (Z Z^T + rho I)^-1``.  ``setcoef`` forms ``Z Z^T`` and ``S Z^T``
on the device, two reductions over ``K`` (csrc/csc_cmod.h ``cmod_gram``); the host forms ``Q`` in float64 from a
Cholesky factor and hands it to the device in the working precision, again whenever ``rho`` changes (from the kept
Gram matrix: no launch).  The reference's ``K < M`` branch (matrix inversion lemma) is the same matrix; the
``M x M`` one is always formed.  The device does the rest of an iteration in two launches and a reduction.

Served: real float32 / float64, ``Z`` and ``S`` host arrays or :class:`sporco_amd.device.DeviceArray` (read in
place, not copied), ``M`` and ``N`` up to 512, ``ZeroMean``, ``AuxVarObj``, ``ReturnX``, ``Y0`` / ``U0``,
``AutoRho``.

Refused: complex or non-floating inputs and float16 (``TypeError``), wrong shapes, empty arrays and ``M`` or ``N``
above 512 (``ValueError``), ``reducer=`` and pickling (``NotImplementedError``).  The reference's attributes
``lu`` and ``piv`` do not exist.  There is no CPU path.

``rho``: the reference's constructor names ``K / 500`` as the default, after its base class has already set the
attribute to 1.0, and ``set_attr`` keeps a value that is set (cmod.py:182-186, common.py:177-230): its default is
1.0 in effect, and so is the default here.
"""

import copy
import warnings

import numpy as np

from .. import _lib
from ..device import is_device_array
from . import admm

__all__ = ['CnstrMOD', 'getPcn', 'zeromean', 'normalise']


def solve_matrix(G, rho):
    """``(G + rho I)^-1`` in float64 from a Cholesky factor; ``G`` is ``Z Z^T``."""
    G = np.asarray(G, dtype=np.float64)
    M = G.shape[0]
    L = np.linalg.cholesky(0.5 * (G + G.T) + float(rho) * np.identity(M))
    Li = np.linalg.solve(L, np.identity(M))
    return Li.T.dot(Li)


def plan(N, M, K, dtype=np.float32):
    """The kernels' launch plan of an ``(N, M, K)`` problem (``_lib.CmodHandle.plan``)."""
    h = _lib.CmodHandle(N, M, K, dtype)
    try:
        return h.plan()
    finally:
        h.close()


class CnstrMOD(admm.ADMMEqual):
    r"""ADMM algorithm for  minimise ||D Z - S||^2  such that  ||d_m|| = 1  (cmod.py:21-282).

    ``IterationStats``: ``Iter, DFid, Cnstr, PrimalRsdl, DualRsdl, EpsPrimal, EpsDual, Rho, Time``.
    """

    class Options(admm.ADMMEqual.Options):
        """Options of cmod.py:77-137: ``AuxVarObj`` (couples ``fEvalX`` / ``gEvalY``), ``ZeroMean``; ``RelaxParam``
        1.8, ``ReturnX`` False, ``AutoRho`` enabled with ``RsdlTarget`` 1.0 when unset."""

        defaults = copy.deepcopy(admm.ADMMEqual.Options.defaults)
        defaults.update({'AuxVarObj': True, 'fEvalX': False, 'gEvalY': True, 'ReturnX': False,
                         'RelaxParam': 1.8, 'ZeroMean': False})
        defaults['AutoRho'].update({'Enabled': True})

        def __init__(self, opt=None):
            admm.ADMMEqual.Options.__init__(self, {} if opt is None else opt)
            if self['AutoRho', 'RsdlTarget'] is None:
                self['AutoRho', 'RsdlTarget'] = 1.0

        def __setitem__(self, key, value):
            admm.ADMMEqual.Options.__setitem__(self, key, value)
            if key == 'AuxVarObj':
                self['fEvalX'] = value is not True
                self['gEvalY'] = value is True

    itstat_fields_objfn = ('DFid', 'Cnstr')
    hdrtxt_objfn = ('DFid', 'Cnstr')
    hdrval_objfun = {'DFid': 'DFid', 'Cnstr': 'Cnstr'}

    def __init__(self, Z, S, dsz=None, opt=None, **backend):
        if opt is None:
            opt = CnstrMOD.Options()
        if backend.get('reducer') is not None:
            raise NotImplementedError("cmod: no sharding over processes (reducer=)")
        S = self._check_array(S, 'S')
        N, K = S.shape
        if Z is None:
            if dsz is None:
                raise ValueError("without Z, dsz gives the dictionary size: dsz[0] is M")
            M = int(dsz[0])
        else:
            if not is_device_array(Z):
                Z = np.asarray(Z)
            if len(Z.shape) != 2:
                raise ValueError("Z has shape (M, K)")
            M = int(Z.shape[0])
        if M < 1:
            raise ValueError("empty Z or S")
        if max(M, N) > _lib.CMOD_MAX_DIM:
            raise ValueError("a dictionary of shape %s: the kernels serve dictionaries of up to %d rows and %d columns"
                             % ((N, M), _lib.CMOD_MAX_DIM, _lib.CMOD_MAX_DIM))
        self.set_dtype(opt, S.dtype)
        if self.dtype not in (np.float32, np.float64):
            raise TypeError("sporco_amd works in float32 or float64, not %s" % self.dtype)
        self._dims = (N, M, K)
        self._dev = _lib.CmodHandle(N, M, K, self.dtype, device=backend.get('device', 0), stream=backend.get('stream'))
        self._u_scale = 1.0
        self._sums = [0.0] * _lib.OUT_COUNT
        self._cache = {}
        self._have_x = False
        self._G = None
        self.Z = None
        self.S = S if is_device_array(S) else np.ascontiguousarray(S, dtype=self.dtype)
        if is_device_array(S) and S.dtype != self.dtype:
            raise TypeError("a device array S has the working precision, %s" % self.dtype)
        self._dev.set_signal(self.S)
        super(CnstrMOD, self).__init__((N, M), self.dtype, opt)
        # (a no-op where the base class has set rho, as in the reference: see the module's text)
        self.set_attr('rho', opt['rho'], dval=K / 500.0, dtype=self.dtype)
        self.Pcn = getPcn(opt['ZeroMean'])
        if Z is not None:
            self.setcoef(Z)

    @staticmethod
    def _check_array(a, nm):
        """What is refused of Z or S, before any device work."""
        if not is_device_array(a):
            a = np.asarray(a)
            if np.iscomplexobj(a):
                raise TypeError("cmod handles real-valued Z and S")
            if a.dtype not in (np.float32, np.float64):
                raise TypeError("sporco_amd works in float32 or float64, not %s (%s)" % (a.dtype, nm))
        if len(a.shape) != 2:
            raise ValueError("%s has two axes, the K signals last" % nm)
        if a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError("empty Z or S")
        return a

    # -- coefficients and solve matrix ---------------------------------------------------------------------
    def _set_solve(self):
        self._dev.set_solve(solve_matrix(self._G, self.rho).astype(self.dtype))

    def setcoef(self, Z):
        """Set the coefficient array (cmod.py:211-218): ``S Z^T`` and ``Z Z^T`` are formed on the device, the solve
        matrix on the host; Y and U stay.  A :class:`sporco_amd.device.DeviceArray` is read in place: it stays
        unchanged until the next ``setcoef``."""
        Z = self._check_array(Z, 'Z')
        if tuple(Z.shape) != (self._dims[1], self._dims[2]):
            raise ValueError("Z of shape %s where %s is expected" % (tuple(Z.shape), (self._dims[1], self._dims[2])))
        if Z.dtype != self.dtype:
            if is_device_array(Z):
                raise TypeError("a device array Z has the working precision, %s" % self.dtype)
            Z = Z.astype(self.dtype)
        self.Z = Z if is_device_array(Z) else np.ascontiguousarray(Z)
        self._dev.set_coef(self.Z)
        self._G = self._dev.download(_lib.CMOD_G)
        self._cache.pop(_lib.CMOD_SZT, None)
        self._set_solve()

    def rhochange(self):
        """The solve matrix of the new rho (cmod.py:278-282), from the kept Gram matrix."""
        self._set_solve()

    @property
    def SZT(self):
        return self._fetch(_lib.CMOD_SZT)

    def getdict(self):
        """The final dictionary (cmod.py:222-225)."""
        return self.Y

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
        """cmod.py:198-207: zero, or ``Y`` at a given ``Y0``."""
        if self.opt['Y0'] is None:
            return np.zeros(ushape, dtype=self.dtype)
        return self.Y

    def _touch(self, *variables):
        for v in variables:
            self._cache.pop(v, None)

    def _fetch(self, var):
        if var not in self._cache:
            a = self._dev.download(var)
            if var == _lib.CMOD_U and self._u_scale != 1.0:
                a = a * a.dtype.type(self._u_scale)
            self._cache[var] = a
        return self._cache[var]

    def _store(self, var, value):
        value = np.asarray(value, dtype=self.dtype)
        if value.shape != self._dims[:2]:
            raise ValueError("array of shape %s where %s is expected" % (value.shape, self._dims[:2]))
        self._dev.upload(var, np.ascontiguousarray(value))
        if var == _lib.CMOD_U:
            self._u_scale = 1.0
        self._touch(var)

    @property
    def X(self):
        """The result of the last x step (None before the first iteration)."""
        return self._fetch(_lib.CMOD_X) if self._have_x else None

    @X.setter
    def X(self, value):
        if value is not None:
            raise NotImplementedError("%s: X is the result of the x step; set Y and U" % type(self).__name__)

    @property
    def Y(self):
        return self._fetch(_lib.CMOD_Y)

    @Y.setter
    def Y(self, value):
        if value is not None:
            self._store(_lib.CMOD_Y, value)

    @property
    def U(self):
        return self._fetch(_lib.CMOD_U)

    @U.setter
    def U(self, value):
        if value is not None:
            self._store(_lib.CMOD_U, value)

    def __getstate__(self):
        raise NotImplementedError("%s: pickling is not offered" % type(self).__name__)

    @property
    def runtime(self):
        """The reference's transitional attribute (admm.py:393-403): init plus solve time of :attr:`timer`."""
        warnings.warn("admm.ADMM.runtime attribute has been replaced by an upgraded timer class: please see the "
                      "documentation for admm.ADMM.solve method and util.Timer class", PendingDeprecationWarning)
        return self.timer.elapsed('init') + self.timer.elapsed('solve')

    # -- iteration -----------------------------------------------------------------------------------------
    def _params(self):
        p = _lib.CmodParams()
        p.rho = float(self.rho)
        p.rlx = float(self.rlx)
        p.u_scale = float(self._u_scale)
        p.zero_mean = 1 if self.opt['ZeroMean'] else 0
        p.feval_x = 1 if self.opt['fEvalX'] else 0
        p.geval_y = 1 if self.opt['gEvalY'] else 0
        p.want_dfid = 0 if self.opt['FastSolve'] else 1
        return p

    def iteration(self):
        admm.refuse_step_overrides(self)
        if self.Z is None:
            raise ValueError("%s: setcoef comes before solve" % type(self).__name__)
        self._sums = self._dev.iter(self._params())
        self._u_scale = 1.0
        self._have_x = True
        self._touch(_lib.CMOD_X, _lib.CMOD_Y, _lib.CMOD_U)
        if not self._needs_residuals():
            return None
        self.timer.stop('solve_wo_rsdl')
        res = self.compute_residuals()
        self.timer.start('solve_wo_rsdl')
        return res

    def finish_solve(self):
        self._dev.sync()

    def rescale_u(self, rsf):
        """Defer ``U /= rsf`` (admm.py:573): the factor rides along as ``u_scale``; the iteration applies it,
        ``self.U`` shows it."""
        self._u_scale = self._u_scale / float(rsf)
        self._touch(_lib.CMOD_U)

    def residual_norms(self):
        """admm.py:462-486 with A = I, B = -I, c = 0, on the unrelaxed X as the reference's ``AXnr``."""
        s = self._sums
        rho = float(self.rho)
        return (np.sqrt(s[_lib.OUT_R2]), rho * np.sqrt(s[_lib.OUT_S2]),
                max(np.sqrt(s[_lib.OUT_AX2]), np.sqrt(s[_lib.OUT_Y2])), rho * np.sqrt(s[_lib.OUT_U2]))

    def obfn_dfd(self):
        """(1/2) ||f Z - S||^2, f = Y, or X under ``fEvalX`` (cmod.py:260-265)."""
        return 0.5 * self._sums[_lib.OUT_DFID]

    def obfn_cns(self):
        """||Pcn(g) - g||, g = Y, or X without ``gEvalY`` (cmod.py:269-274)."""
        return float(np.sqrt(self._sums[_lib.OUT_CNSTR]))

    def eval_objfn(self):
        return (self.obfn_dfd(), self.obfn_cns())

    def dfid_device(self):
        """(1/2) ||Y Z - S||^2 with the ``Z`` in use, by a device call of its own (``BPDNDictLearn.evaluate``)."""
        return 0.5 * self._dev.dfid(_lib.CMOD_Y)


def getPcn(zm):
    """The constraint-set projection (cmod.py:286-304): :func:`normalise`, after :func:`zeromean` if ``zm``."""
    if zm:
        return lambda x: normalise(zeromean(x))
    return normalise


def zeromean(v):
    """Subtract the mean of each column (cmod.py:308-322)."""
    return v - np.mean(v, 0)


def normalise(v):
    """Normalise the columns; a column of norm 0 is divided by 1 (cmod.py:326-342)."""
    vn = np.sqrt(np.sum(v ** 2, 0))
    vn[vn == 0] = 1.0
    return np.asarray(v / vn, dtype=v.dtype)
