"""Dense (patch-based) sparse coding on the device, with the interface of the reference's ``sporco.admm.bpdn``
(sporco/admm/bpdn.py:24-914): :class:`BPDN`, :class:`BPDNJoint`, :class:`ElasticNet` and :class:`BPDNProjL1`, the
classes of :class:`GenericBPDN` that share one x step.  :class:`BPDNProjL1` replaces the l1 penalty by the constraint
``||x||_1 <= gamma`` per signal: its y step projects every column onto the l1 ball inside the same launch.

The dictionary ``D`` is ``(N, M)``, the signals ``S`` are ``(N, K)``, the coefficients ``(M, K)``.  The x step is
``X = P (D^T S + rho (Y - U))`` with ``P = (D^T D + c I)^-1``, ``c = rho`` (``ElasticNet``: ``mu + rho``).  The host
forms ``P`` in float64 from a Cholesky factor of the smaller Gram matrix and hands it to the device in the
working precision, again after ``setdict`` and whenever ``rho`` changes; the device does everything else, one
launch per iteration for ``BPDN`` and ``ElasticNet`` (csrc/csc_bpdn.h), with the products on the float32 matrix
instruction.

Served: real float32 / float64, ``S`` of shape ``(N, K)`` with ``K >= 1``, any ``N``, ``M`` up to 512, ``L1Weight``
a scalar or an array that broadcasts to ``(M, K)``, ``NonNegCoef``, ``AuxVarObj``, ``LinSolveCheck``, ``ReturnX``,
``Y0`` / ``U0``, ``AutoRho``, ``setdict``.

Refused: complex or non-floating ``D`` / ``S`` and :class:`sporco_amd.device.DeviceArray` inputs (``TypeError``),
``M`` or ``N`` above 512, shape mismatches and a negative ``gamma`` (``ValueError``), ``reducer=`` and pickling
(``NotImplementedError``).  The reference's attributes ``lu`` and ``piv`` do not exist.  There is no CPU path.
"""

import copy
import warnings

import numpy as np

from .. import _lib
from ..device import is_device_array
from . import admm

__all__ = ['GenericBPDN', 'BPDN', 'BPDNJoint', 'ElasticNet', 'BPDNProjL1']


def solve_matrix(D, c):
    """``(D^T D + c I)^-1`` in float64 from a Cholesky factor of the smaller Gram matrix (``N < M``: by the
    matrix inversion lemma, as linalg.py:724-773 solves it)."""
    D = np.asarray(D, dtype=np.float64)
    N, M = D.shape
    c = float(c)
    if N >= M:
        L = np.linalg.cholesky(D.T.dot(D) + c * np.identity(M))
        Li = np.linalg.solve(L, np.identity(M))
        return Li.T.dot(Li)
    L = np.linalg.cholesky(D.dot(D.T) + c * np.identity(N))
    W = np.linalg.solve(L, D)                  # L^-1 D:  D^T (D D^T + c I)^-1 D = W^T W
    return (np.identity(M) - W.T.dot(W)) / c


def plan(N, M, K, dtype=np.float32):
    """The kernels' launch plan of an ``(N, M, K)`` problem: ``dict(KB, blocks, mfma, lds)`` -- the columns of a
    workgroup's block, the workgroups, whether the products use the matrix instruction, the LDS bytes."""
    h = _lib.BpdnHandle(N, M, K, dtype)
    try:
        return h.plan()
    finally:
        h.close()


class GenericBPDN(admm.ADMMEqual):
    r"""Base class: data fidelity (1/2) ||D x - s||^2 plus the regulariser of the derived class
    (bpdn.py:24-266).  The whole iteration is one device call; the derived classes differ in its parameters."""

    class Options(admm.ADMMEqual.Options):
        """Options of bpdn.py:79-140: ``AuxVarObj`` (couples ``fEvalX`` / ``gEvalY``), ``LinSolveCheck``,
        ``NonNegCoef``; ``RelaxParam`` 1.8, ``ReturnX`` False, ``AutoRho`` enabled with ``Period`` 10."""

        defaults = copy.deepcopy(admm.ADMMEqual.Options.defaults)
        defaults.update({'AuxVarObj': True, 'fEvalX': False, 'gEvalY': True, 'ReturnX': False,
                         'LinSolveCheck': False, 'RelaxParam': 1.8, 'NonNegCoef': False})
        defaults['AutoRho'].update({'Enabled': True, 'Period': 10, 'AutoScaling': True, 'Scaling': 1000.0,
                                    'RsdlRatio': 1.2})

        def __init__(self, opt=None):
            admm.ADMMEqual.Options.__init__(self, {} if opt is None else opt)

        def __setitem__(self, key, value):
            admm.ADMMEqual.Options.__setitem__(self, key, value)
            if key == 'AuxVarObj':
                self['fEvalX'] = value is not True
                self['gEvalY'] = value is True

    itstat_fields_objfn = ('ObjFun', 'DFid', 'Reg')
    itstat_fields_extra = ('XSlvRelRes',)
    hdrtxt_objfn = ('Fnc', 'DFid', 'Reg')
    hdrval_objfun = {'Fnc': 'ObjFun', 'DFid': 'DFid', 'Reg': 'Reg'}

    _joint = False

    def __init__(self, D, S, opt=None, **backend):
        if opt is None:
            opt = GenericBPDN.Options()
        D, S = self._check_inputs(D, S, backend)
        self.set_dtype(opt, S.dtype)
        if self.dtype not in (np.float32, np.float64):
            raise TypeError("sporco_amd works in float32 or float64, not %s" % self.dtype)
        N, K = S.shape
        M = D.shape[1]
        self.S = np.ascontiguousarray(S, dtype=self.dtype)
        self._dims = (N, M, K)
        self._dev = _lib.BpdnHandle(N, M, K, self.dtype, device=backend.get('device', 0),
                                    stream=backend.get('stream'))
        self._u_scale = 1.0
        self._sums = [0.0] * _lib.OUT_COUNT
        self._cache = {}
        self._have_x = False
        self._last_k = None
        self.xrrs = None
        self._dev.upload(_lib.BPDN_S, self.S)
        if not hasattr(self, 'wl1'):
            self.wl1 = np.asarray(1.0, dtype=self.dtype)
        if self.wl1.size > 1:
            self._dev.upload(_lib.BPDN_WL1, np.ascontiguousarray(np.broadcast_to(self.wl1, (M, K))))
        super(GenericBPDN, self).__init__((M, K), self.dtype, opt)
        self.setdict(D)

    @staticmethod
    def _check_inputs(D, S, backend):
        """What is refused, before any device work."""
        if backend.get('reducer') is not None:
            raise NotImplementedError("bpdn: no sharding over processes (reducer=)")
        if is_device_array(D) or is_device_array(S):
            raise TypeError("bpdn takes host arrays for D and S, not DeviceArrays")
        D, S = np.asarray(D), np.asarray(S)
        if np.iscomplexobj(D) or np.iscomplexobj(S):
            raise TypeError("bpdn handles real-valued D and S")
        for nm, a in (('D', D), ('S', S)):
            if a.dtype not in (np.float32, np.float64):
                raise TypeError("sporco_amd works in float32 or float64, not %s (%s)" % (a.dtype, nm))
        if S.ndim != 2:
            raise ValueError("S has shape (N, K); a single signal is a column, shape (N, 1)")
        if D.ndim != 2:
            raise ValueError("D has shape (N, M)")
        if D.shape[0] != S.shape[0]:
            raise ValueError("D has %d rows and S %d" % (D.shape[0], S.shape[0]))
        if S.shape[1] < 1 or D.shape[1] < 1 or D.shape[0] < 1:
            raise ValueError("empty D or S")
        if max(D.shape) > _lib.BPDN_MAX_DIM:
            raise ValueError("D of shape %s: the kernels serve dictionaries of up to %d rows and %d columns"
                             % (D.shape, _lib.BPDN_MAX_DIM, _lib.BPDN_MAX_DIM))
        return D, S

    # -- dictionary and solve matrix -------------------------------------------------------------------
    def _solve_c(self):
        """The c of ``(D^T D + c I)`` (bpdn.py:180)."""
        return float(self.rho)

    def _set_solve(self):
        self._c = self._solve_c()
        self._dev.set_solve(solve_matrix(self.D, self._c).astype(self.dtype))

    def setdict(self, D):
        """Set the dictionary (bpdn.py:174-181): ``D^T S`` and the solve matrix are formed again, Y and U stay."""
        if is_device_array(D):
            raise TypeError("bpdn takes host arrays for D and S, not DeviceArrays")
        D = np.asarray(D)
        if D.ndim != 2 or D.shape != self._dims[:2]:
            raise ValueError("D of shape %s where %s is expected" % (getattr(D, 'shape', None), self._dims[:2]))
        if np.iscomplexobj(D):
            raise TypeError("bpdn handles real-valued D and S")
        self.D = np.array(D, dtype=self.dtype, order='C')
        self._dev.set_dict(self.D)
        self._cache.pop(_lib.BPDN_DTS, None)
        self._set_solve()

    def rhochange(self):
        """The solve matrix of the new rho (bpdn.py:261-265)."""
        self._set_solve()

    @property
    def DTS(self):
        return self._fetch(_lib.BPDN_DTS)

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

    def _touch(self, *variables):
        for v in variables:
            self._cache.pop(v, None)

    def _fetch(self, var):
        if var not in self._cache:
            a = self._dev.download(var)
            if var == _lib.BPDN_U and self._u_scale != 1.0:
                a = a * a.dtype.type(self._u_scale)
            self._cache[var] = a
        return self._cache[var]

    def _store(self, var, value):
        value = np.asarray(value, dtype=self.dtype)
        if value.shape != self._dims[1:]:
            raise ValueError("array of shape %s where %s is expected" % (value.shape, self._dims[1:]))
        self._dev.upload(var, np.ascontiguousarray(value))
        if var == _lib.BPDN_U:
            self._u_scale = 1.0
        self._touch(var)

    @property
    def X(self):
        """The result of the last x step (None before the first iteration)."""
        return self._fetch(_lib.BPDN_X) if self._have_x else None

    @X.setter
    def X(self, value):
        if value is not None:
            raise NotImplementedError("%s: X is the result of the x step; set Y and U" % type(self).__name__)

    @property
    def Y(self):
        return self._fetch(_lib.BPDN_Y)

    @Y.setter
    def Y(self, value):
        if value is not None:
            self._store(_lib.BPDN_Y, value)

    @property
    def U(self):
        return self._fetch(_lib.BPDN_U)

    @U.setter
    def U(self, value):
        if value is not None:
            self._store(_lib.BPDN_U, value)

    def __getstate__(self):
        raise NotImplementedError("%s: pickling is not offered" % type(self).__name__)

    @property
    def runtime(self):
        """The reference's transitional attribute (admm.py:393-403): init plus solve time of :attr:`timer`."""
        warnings.warn("admm.ADMM.runtime attribute has been replaced by an upgraded timer class: please see the "
                      "documentation for admm.ADMM.solve method and util.Timer class", PendingDeprecationWarning)
        return self.timer.elapsed('init') + self.timer.elapsed('solve')

    def getcoef(self):
        """The final coefficient array (bpdn.py:185-188)."""
        return self.Y

    def getcoef_device(self):
        """``Y`` as a :class:`sporco_amd.device.DeviceArray` over the handle's own buffer: no copy; the view keeps
        the handle alive and shows what later iterations leave there."""
        return self._dev.device_view(_lib.BPDN_Y)

    def getmin(self):
        return self.X if self.opt['ReturnX'] else self.Y

    # -- iteration -----------------------------------------------------------------------------------------
    def _wants_x(self):
        """Whether this iteration stores X: something reads it (``ReturnX``, a callback), or it may be the
        last one -- by count, or because the stopping test runs with a non-zero tolerance."""
        if self.opt['ReturnX'] or self.opt['Callback'] is not None:
            return True
        if self._needs_residuals() and (self.opt['RelStopTol'] > 0.0 or self.opt['AbsStopTol'] > 0.0):
            return True
        return self._last_k is None or self.k >= self._last_k

    def _params(self):
        p = _lib.BpdnParams()
        p.rho = float(self.rho)
        p.lmbda = float(getattr(self, 'lmbda', 0.0))
        p.mu = float(getattr(self, 'mu', 0.0))
        p.rlx = float(self.rlx)
        p.u_scale = float(self._u_scale)
        p.wl1 = float(self.wl1.ravel()[0]) if self.wl1.size == 1 else 1.0
        p.c = float(self._c)
        p.nonneg = 1 if self.opt['NonNegCoef'] else 0
        p.feval_x = 1 if self.opt['fEvalX'] else 0
        p.geval_y = 1 if self.opt['gEvalY'] else 0
        p.want_x = 1 if self._wants_x() else 0
        p.joint = 1 if self._joint else 0
        p.lin_solve_check = 1 if self.opt['LinSolveCheck'] else 0
        return p

    def solve(self):
        self._last_k = self.k + self.opt['MaxMainIter'] - 1
        try:
            return super(GenericBPDN, self).solve()
        finally:
            self._last_k = None

    def iteration(self):
        admm.refuse_step_overrides(self)
        p = self._params()
        self._sums = self._dev.iter(p)
        self._u_scale = 1.0
        self._have_x = bool(p.want_x or p.joint or p.lin_solve_check)
        if p.lin_solve_check:
            s = self._sums
            nrm = max(np.sqrt(s[_lib.OUT_XRRS_AX2]), np.sqrt(s[_lib.OUT_XRRS_B2]))
            self.xrrs = 0.0 if nrm == 0.0 else float(np.sqrt(s[_lib.OUT_XRRS_D2]) / nrm)
        else:
            self.xrrs = None
        self._touch(_lib.BPDN_X, _lib.BPDN_Y, _lib.BPDN_U)
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
        self._touch(_lib.BPDN_U)

    def residual_norms(self):
        """admm.py:462-486 with A = I, B = -I, c = 0, on the unrelaxed X as the reference's ``AXnr``:
        r = ||X - Y||, s = rho ||Y - Yprev||, rn = max(||X||, ||Y||), sn = rho ||U||."""
        s = self._sums
        rho = float(self.rho)
        return (np.sqrt(s[_lib.OUT_R2]), rho * np.sqrt(s[_lib.OUT_S2]),
                max(np.sqrt(s[_lib.OUT_AX2]), np.sqrt(s[_lib.OUT_Y2])), rho * np.sqrt(s[_lib.OUT_U2]))

    def obfn_dfd(self):
        """(1/2) ||D g - S||^2, g = Y, or X under ``fEvalX`` (bpdn.py:236-241)."""
        return 0.5 * self._sums[_lib.OUT_DFID]

    def _gvar_norm2(self):
        return self._sums[_lib.OUT_Y2 if self.opt['gEvalY'] else _lib.OUT_AX2]

    def obfn_reg(self):
        raise NotImplementedError()

    def eval_objfn(self):
        dfd = self.obfn_dfd()
        reg = self.obfn_reg()
        return (dfd + reg[0], dfd) + reg[1:]

    def itstat_extra(self):
        return (self.xrrs,)


class BPDN(GenericBPDN):
    r"""ADMM algorithm for  minimise (1/2) ||D x - s||^2 + lmbda ||wl1 x||_1  (bpdn.py:271-465).

    ``IterationStats``: ``Iter, ObjFun, DFid, RegL1, PrimalRsdl, DualRsdl, EpsPrimal, EpsDual, Rho, XSlvRelRes,
    Time``.
    """

    class Options(GenericBPDN.Options):
        """Adds ``L1Weight`` (bpdn.py:338-371): a scalar, or an array that broadcasts to ``(M, K)``."""

        defaults = copy.deepcopy(GenericBPDN.Options.defaults)
        defaults.update({'L1Weight': 1.0})

        def __init__(self, opt=None):
            GenericBPDN.Options.__init__(self, {} if opt is None else opt)

    itstat_fields_objfn = ('ObjFun', 'DFid', 'RegL1')
    hdrtxt_objfn = ('Fnc', 'DFid', u'Regℓ1')
    hdrval_objfun = {'Fnc': 'ObjFun', 'DFid': 'DFid', u'Regℓ1': 'RegL1'}

    def __init__(self, D, S, lmbda=None, opt=None, **backend):
        if opt is None:
            opt = BPDN.Options()
        D, S = self._check_inputs(D, S, backend)
        self.set_dtype(opt, S.dtype)
        if self.dtype not in (np.float32, np.float64):
            raise TypeError("sporco_amd works in float32 or float64, not %s" % self.dtype)
        if lmbda is None:
            lmbda = 0.1 * abs(D.T.dot(S)).max()
        self.lmbda = self.dtype.type(lmbda)
        wl1 = np.asarray(opt['L1Weight'])
        if np.iscomplexobj(wl1):
            raise TypeError("bpdn handles real-valued weights")
        self.wl1 = np.asarray(wl1, dtype=self.dtype)
        if self.wl1.ndim > 0:
            np.broadcast_to(self.wl1, (D.shape[1], S.shape[1]))      # (raises where it does not broadcast)
        self.set_attr('rho', opt['rho'], dval=(50.0 * self.lmbda + 1.0), dtype=self.dtype)
        # (Sec. VI.C of wohlberg-2015-adaptive, bpdn.py:417-422)
        if self.lmbda != 0.0:
            rho_xi = float((1.0 + (18.3) ** (np.log10(self.lmbda) + 1.0)))
        else:
            rho_xi = 1.0
        self.set_attr('rho_xi', opt['AutoRho', 'RsdlTarget'], dval=rho_xi, dtype=self.dtype)
        super(BPDN, self).__init__(D, S, opt, **backend)

    def uinit(self, ushape):
        """bpdn.py:434-443: zero, or at a non-zero Y the dual optimality criterion (3.10) of
        boyd-2010-distributed, ``(lmbda / rho) sign(Y)``."""
        if self.opt['Y0'] is None:
            return np.zeros(ushape, dtype=self.dtype)
        return ((self.lmbda / self.rho) * np.sign(self.Y)).astype(self.dtype)

    def obfn_reg(self):
        rl1 = self._sums[_lib.OUT_L1]
        return (float(self.lmbda) * rl1, rl1)


class BPDNJoint(BPDN):
    r"""ADMM algorithm for BPDN with an additional l2,1 term over the K signals of each coefficient row,
    minimise (1/2) ||D X - S||^2 + lmbda ||wl1 X||_1 + mu ||X||_{2,1}  (bpdn.py:469-588).

    ``IterationStats``: ``Iter, ObjFun, DFid, RegL1, RegL21, PrimalRsdl, DualRsdl, EpsPrimal, EpsDual, Rho,
    XSlvRelRes, Time``.
    """

    itstat_fields_objfn = ('ObjFun', 'DFid', 'RegL1', 'RegL21')
    hdrtxt_objfn = ('Fnc', 'DFid', u'Regℓ1', u'Regℓ2,1')
    hdrval_objfun = {'Fnc': 'ObjFun', 'DFid': 'DFid', u'Regℓ1': 'RegL1', u'Regℓ2,1': 'RegL21'}

    _joint = True

    def __init__(self, D, S, lmbda=None, mu=0.0, opt=None, **backend):
        if opt is None:
            opt = BPDN.Options()
        D, S = self._check_inputs(D, S, backend)
        self.set_dtype(opt, S.dtype)
        if self.dtype in (np.float32, np.float64):
            self.mu = self.dtype.type(mu)
        super(BPDNJoint, self).__init__(D, S, lmbda, opt, **backend)

    def obfn_reg(self):
        rl1 = self._sums[_lib.OUT_L1]
        rl21 = self._sums[_lib.OUT_L21]
        return (float(self.lmbda) * rl1 + float(self.mu) * rl21, rl1, rl21)


class ElasticNet(BPDN):
    r"""ADMM algorithm for the elastic net,
    minimise (1/2) ||D x - s||^2 + lmbda ||wl1 x||_1 + (mu / 2) ||x||^2  (bpdn.py:592-746).

    ``IterationStats``: ``Iter, ObjFun, DFid, RegL1, RegL2, PrimalRsdl, DualRsdl, EpsPrimal, EpsDual, Rho,
    XSlvRelRes, Time``.
    """

    itstat_fields_objfn = ('ObjFun', 'DFid', 'RegL1', 'RegL2')
    hdrtxt_objfn = ('Fnc', 'DFid', u'Regℓ1', u'Regℓ2')
    hdrval_objfun = {'Fnc': 'ObjFun', 'DFid': 'DFid', u'Regℓ1': 'RegL1', u'Regℓ2': 'RegL2'}

    def __init__(self, D, S, lmbda=None, mu=0.0, opt=None, **backend):
        if opt is None:
            opt = BPDN.Options()
        D, S = self._check_inputs(D, S, backend)
        self.set_dtype(opt, S.dtype)
        if self.dtype in (np.float32, np.float64):
            self.mu = self.dtype.type(mu)
        super(ElasticNet, self).__init__(D, S, lmbda, opt, **backend)

    def _solve_c(self):
        """bpdn.py:706: the l2 term joins the diagonal."""
        return float(self.mu) + float(self.rho)

    def obfn_reg(self):
        rl1 = self._sums[_lib.OUT_L1]
        rl2 = 0.5 * self._gvar_norm2()
        return (float(self.lmbda) * rl1 + float(self.mu) * rl2, rl1, rl2)


class BPDNProjL1(GenericBPDN):
    r"""ADMM algorithm for  minimise (1/2) ||D x - s||^2  such that  ||x||_1 <= gamma  per signal (bpdn.py:750-914).
    The y step is ``proj_l1(AX + U, gamma, axis=0)``, found per column inside the iteration's launch
    (csrc/csc_bpdn.h, projection mode).

    ``IterationStats``: ``Iter, ObjFun, Cnstr, PrimalRsdl, DualRsdl, EpsPrimal, EpsDual, Rho, XSlvRelRes, Time``;
    ``ObjFun`` is the data fidelity alone, ``Cnstr`` is ``||proj_l1(g, gamma) - g||`` with ``g = Y`` (``AuxVarObj``
    off: ``X``).
    """

    class Options(GenericBPDN.Options):
        """The options of :class:`GenericBPDN.Options` with ``AutoRho.RsdlTarget`` 1.0 (bpdn.py:816-837)."""

        defaults = copy.deepcopy(GenericBPDN.Options.defaults)
        defaults['AutoRho'].update({'RsdlTarget': 1.0})

        def __init__(self, opt=None):
            GenericBPDN.Options.__init__(self, {} if opt is None else opt)

    itstat_fields_objfn = ('ObjFun', 'Cnstr')
    hdrtxt_objfn = ('Fnc', 'Cnstr')
    hdrval_objfun = {'Fnc': 'ObjFun', 'Cnstr': 'Cnstr'}

    def __init__(self, D, S, gamma, opt=None, **backend):
        if opt is None:
            opt = BPDNProjL1.Options()
        D, S = self._check_inputs(D, S, backend)
        self.set_dtype(opt, S.dtype)
        if self.dtype not in (np.float32, np.float64):
            raise TypeError("sporco_amd works in float32 or float64, not %s" % self.dtype)
        if not float(gamma) >= 0.0:
            raise ValueError("gamma must not be negative")
        self.gamma = self.dtype.type(gamma)
        super(BPDNProjL1, self).__init__(D, S, opt, **backend)

    def uinit(self, ushape):
        """bpdn.py:881-891: zero, with a ``Y0`` too."""
        return np.zeros(ushape, dtype=self.dtype)

    def _params(self):
        p = super(BPDNProjL1, self)._params()
        p.lmbda = float(self.gamma)      # (the radius travels in the lmbda field)
        p.proj_l1 = 1
        return p

    def eval_objfn(self):
        """bpdn.py:906-914: the data fidelity and the distance of the g variable from the l1 balls."""
        return (self.obfn_dfd(), float(np.sqrt(self._sums[_lib.OUT_BPDN_CNSTR])))
