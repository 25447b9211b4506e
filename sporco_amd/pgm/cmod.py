"""The dictionary update of the dense (patch-based) family by proximal gradient (FISTA) steps on the device, with the
interface of the reference's ``sporco.pgm.cmod`` (sporco/pgm/cmod.py:24-407): :class:`CnstrMOD`,
:class:`WeightedCnstrMOD`, :func:`getPcn`, :func:`zeromean`, :func:`normalise`,

    minimise (1/2) ||D Z - S||^2_W  such that  ||d_m|| = 1 [, mean(d_m) = 0 | d_m >= 0] .

The coefficients ``Z`` are ``(M, K)``, the signals ``S`` and the weight ``W`` ``(N, K)``, the dictionary iterates
``(N, M)``.  The iterates live on the device.  The gradient ``(W (Y Z - S)) Z^T`` streams ``Z``, ``S`` and ``W`` once
(csrc/csc_pgm_cmod.h ``cmod_pgm_grad``, ``cmod_pgm_reduce``); ``cmod_pgm_prox`` forms ``X' = Pcn(Y - G / L)``, the
next ``Y`` and the sums of ``Q_L``, ``Rsdl`` and ``Cnstr``; ``cmod_dfid`` with the weight forms ``F(X')``.  A step
with a fixed ``L`` is those launches, one reduction and one small read; under ``FastSolve`` there is no ``cmod_dfid``,
no reduction and no read.  Both classes take this path, the plain one with the scalar weight 1.

The rules of ``pgm.momentum``, ``pgm.stepsize`` and ``pgm.backtrack`` are served by :meth:`CnstrMOD.fused_iteration`,
which reads the parameters off the objects in the options and keeps the state a rule carries with the solver.  A trial
of ``BacktrackStandard`` after the first is ``cmod_pgm_prox`` and ``cmod_dfid`` on the stored gradient;
``StepSizePolicyCauchy`` and ``StepSizePolicyBB`` launch the gradient, read their sums, fix ``L`` and launch the rest;
``Monotone`` reverts ``X`` by a prox launch that copies the previous iterate and sums for it (with ``cmod_dfid`` again
only under a backtracking rule, which reads ``F`` of the reverted iterate).  Where the Barzilai-Borwein quotient is
not a positive finite number (``<dx, dg>`` is zero after a revert, or after equal iterates) ``L`` stays as it is; the
reference would go on with an infinite ``L``.  The rule's sums are taken against the iterate and gradient of the step
before, whatever an ``X`` setter or a ``setcoef`` between two solves left of them.

Served: real float32 / float64, ``Z``, ``S`` and an ``(N, K)`` ``W`` host arrays or
:class:`sporco_amd.device.DeviceArray` (read in place, not copied), ``M`` and ``N`` up to 512, ``W`` a scalar or of
shape ``(N,)``, ``(N, 1)``, ``(1, K)`` or ``(N, K)``, every option of ``PGM.Options``, ``ZeroMean``, ``NonNegCoef``,
``setcoef``, restart of ``solve``.

Refused: complex, float16 and non-floating inputs (``TypeError``), ``M`` or ``N`` above 512, wrong shapes, a ``W``
that does not broadcast to ``S``, ``ZeroMean`` with ``NonNegCoef`` (``ValueError``), rule objects of other classes
than those of ``sporco_amd.pgm``, ``reducer=`` and pickling (``NotImplementedError``).  There is no CPU path.

The reference's ``reconstruct`` names an attribute ``D`` that its class never sets; the method is left out.
"""

import copy

import numpy as np

from .. import _lib
from ..device import is_device_array
from . import pgm
from .backtrack import BacktrackRobust, BacktrackStandard
from .momentum import MomentumGenLinear, MomentumLinear, MomentumNesterov
from .stepsize import StepSizePolicyBB, StepSizePolicyCauchy

__all__ = ['CnstrMOD', 'WeightedCnstrMOD', 'getPcn', 'zeromean', 'normalise']


def plan(N, M, K, dtype=np.float32):
    """The kernels' launch plan of an ``(N, M, K)`` problem (``_lib.PgmCmodHandle.plan``)."""
    h = _lib.PgmCmodHandle(N, M, K, dtype)
    try:
        return h.plan()
    finally:
        h.close()


def _host(a):
    return a.get() if is_device_array(a) else a


class CnstrMOD(pgm.PGM):
    r"""PGM algorithm for  minimise (1/2) ||D Z - S||^2  such that  ||d_m|| = 1  (pgm/cmod.py:24-232).

    ``IterationStats``: ``Iter, DFid, Cnstr, Rsdl, F_Btrack, Q_Btrack, IterBTrack, L, Time``.
    """

    class Options(pgm.PGM.Options):
        """``PGM.Options`` with ``ZeroMean`` False, ``NonNegCoef`` False (not both True) and ``L`` 500.0
        (pgm/cmod.py:64-101)."""

        defaults = copy.deepcopy(pgm.PGM.Options.defaults)
        defaults.update({'ZeroMean': False, 'NonNegCoef': False, 'L': 500.0})

        def __init__(self, opt=None):
            pgm.PGM.Options.__init__(self, {} if opt is None else opt)

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
        for rule, classes in ((opt['Momentum'], (MomentumNesterov, MomentumLinear, MomentumGenLinear)),
                              (opt['StepSizePolicy'], (type(None), StepSizePolicyCauchy, StepSizePolicyBB)),
                              (opt['Backtrack'], (type(None), BacktrackStandard, BacktrackRobust))):
            if type(rule) not in classes:
                raise NotImplementedError("pgm.cmod serves the rules of sporco_amd.pgm, not %s" % type(rule).__name__)
        if opt['Backtrack'] is not None and int(opt['Backtrack'].maxiter) < 1:
            raise ValueError("Backtrack.maxiter must be at least 1")
        self.Pcn = getPcn(opt['ZeroMean'], opt['NonNegCoef'])      # (raises where both are set)
        self._dims = (N, M, K)
        if is_device_array(S) and S.dtype != self.dtype:
            raise TypeError("a device array S has the working precision, %s" % self.dtype)
        self.S = S if is_device_array(S) else np.ascontiguousarray(S, dtype=self.dtype)
        if not hasattr(self, 'W'):
            self.W = np.asarray(1.0, dtype=self.dtype)
        self._dev = _lib.PgmCmodHandle(N, M, K, self.dtype, device=backend.get('device', 0),
                                       stream=backend.get('stream'))
        self._dev.set_signal(self.S)
        self._cache = {}
        self._sums = None
        self._rs2 = None
        self._ynext = False
        self._started = False
        self._Tk = 0.0
        self._zc = None
        self._have_z = False
        self._beta = self._gamma = 0.0
        self.Z = None
        super(CnstrMOD, self).__init__((N, M), self.dtype, opt)
        if Z is not None:
            self.setcoef(Z)

    @staticmethod
    def _check_array(a, nm):
        """What is refused of Z, S or W, before any device work."""
        if not is_device_array(a):
            a = np.asarray(a)
            if np.iscomplexobj(a):
                raise TypeError("cmod handles real-valued Z, S and W")
            if a.dtype not in (np.float32, np.float64):
                raise TypeError("sporco_amd works in float32 or float64, not %s (%s)" % (a.dtype, nm))
        if len(a.shape) != 2:
            raise ValueError("%s has two axes, the K signals last" % nm)
        if a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError("empty Z or S")
        return a

    # -- state ---------------------------------------------------------------------------------------------
    def init_state(self, xshape):
        """X = ``X0`` or zero, Y = X (pgm.py:257-261, pgm/cmod.py:147-148)."""
        if self.opt['X0'] is not None:
            self.X = np.asarray(self.opt['X0']).astype(self.dtype, copy=True)
            self.Y = self.X

    def _fetch(self, var):
        if var not in self._cache:
            self._cache[var] = self._dev.download(var)
        return self._cache[var]

    def _store(self, var, value):
        value = np.asarray(value, dtype=self.dtype)
        if value.shape != self._dims[:2]:
            raise ValueError("array of shape %s where %s is expected" % (value.shape, self._dims[:2]))
        self._dev.upload(var, np.ascontiguousarray(value))
        self._cache.clear()
        self._sums = None

    @property
    def X(self):
        return self._fetch(_lib.CMOD_X)

    @X.setter
    def X(self, value):
        self._store(_lib.CMOD_X, value)

    @property
    def Xprv(self):
        return self._fetch(_lib.CMOD_XPRV)

    @property
    def Y(self):
        """The auxiliary iterate: what the next gradient is taken at."""
        return self._fetch(_lib.CMOD_YALT if self._ynext else _lib.CMOD_Y)

    @Y.setter
    def Y(self, value):
        if value is not None:
            self._store(_lib.CMOD_YALT if self._ynext else _lib.CMOD_Y, value)

    @property
    def Yprv(self):
        """The Y the last iteration started from (before the first one: the reference's Y + 1e3)."""
        if not self._started:
            return self._fetch(_lib.CMOD_Y) + self.dtype.type(1e3)
        return self._fetch(_lib.CMOD_YALT if isinstance(self.backtrack, BacktrackRobust) else _lib.CMOD_Y)

    def __getstate__(self):
        raise NotImplementedError("%s: pickling is not offered" % type(self).__name__)

    def setcoef(self, Z):
        """Set the coefficient array (pgm/cmod.py:155-158); the iterates stay.  A
        :class:`sporco_amd.device.DeviceArray` is read in place by every later step: it stays valid until the next
        ``setcoef``."""
        Z = self._check_array(Z, 'Z')
        if tuple(Z.shape) != (self._dims[1], self._dims[2]):
            raise ValueError("Z of shape %s where %s is expected" % (tuple(Z.shape), (self._dims[1], self._dims[2])))
        if Z.dtype != self.dtype:
            if is_device_array(Z):
                raise TypeError("a device array Z has the working precision, %s" % self.dtype)
            Z = Z.astype(self.dtype)
        self.Z = Z if is_device_array(Z) else np.ascontiguousarray(Z)
        self._dev.set_coef(self.Z)
        self._sums = None

    def getdict(self):
        """The final dictionary (pgm/cmod.py:162-165)."""
        return self.X

    def getmin(self):
        return self.X

    def finish_solve(self):
        self._dev.sync()

    # -- the reference's methods on host arrays ----------------------------------------------------------
    def grad_f(self, V=None):
        """(W (V Z - S)) Z^T for a host array ``V`` (default: Y)."""
        if V is None:
            V = self.Y
        Z = _host(self.Z)
        return (_host(self.W) * (V.dot(Z) - _host(self.S))).dot(Z.T)

    def prox_g(self, V):
        return self.Pcn(np.asarray(V))

    def hessian_f(self, V):
        """V Z Z^T (pgm/cmod.py:187-192; the reference's weighted class does not weight it either)."""
        Z = _host(self.Z)
        return V.dot(Z).dot(Z.T)

    def obfn_f(self, X=None):
        if X is None:
            X = self.X
        return 0.5 * np.linalg.norm((np.sqrt(_host(self.W)) * (X.dot(_host(self.Z)) - _host(self.S))).ravel()) ** 2

    def obfn_cns(self):
        X = self.X
        return np.linalg.norm(self.Pcn(X) - X)

    def eval_objfn(self):
        """(DFid, Cnstr) of X: from the sums of the step that left X; else the data fidelity by a device call and
        the constraint measure on the host."""
        if self._sums is not None:
            return (self._sums[_lib.PGMC_FX], float(np.sqrt(self._sums[_lib.PGMC_CNSTR])))
        if self.Z is None:
            raise ValueError("%s: setcoef comes first" % type(self).__name__)
        return (self.dfid_device(), float(self.obfn_cns()))

    def dfid_device(self):
        """(1/2) ||X Z - S||^2_W with the ``Z`` in use, by a device call of its own."""
        return 0.5 * self._scalar_w() * self._dev.dfid()

    def rsdl(self):
        return float(np.sqrt(self._rs2))

    # -- iteration ---------------------------------------------------------------------------------------
    def _scalar_w(self):
        """The weight where it is a scalar, else 1: the handle holds the array."""
        if is_device_array(self.W) or self.W.size > 1:
            return 1.0
        return float(self.W.ravel()[0])

    def _params(self, phase, read=True, **kw):
        p = _lib.CmodPgmParams()
        p.L = float(self.L)
        p.w = self._scalar_w()
        p.zero_mean = 1 if self.opt['ZeroMean'] else 0
        p.nonneg = 1 if self.opt['NonNegCoef'] else 0
        p.phase = phase
        p.finalize = 1 if read else 0
        p.beta, p.gamma = self._beta, self._gamma
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def _first(self):
        """What the first launch of an iteration adds: X becomes Xprv, the Y the last prox phase wrote the Y in use."""
        adv_y, self._ynext = int(self._ynext), False
        return dict(advance=1, advance_y=adv_y)

    def _momentum(self):
        """The coefficients of ystep (pgm.py:426-441), fixed before the prox launch that forms the next Y."""
        tprv = self.t
        self.t = self.momentum.update(self.var_momentum())
        self._beta, self._gamma = (tprv - 1.) / self.t, tprv / self.t

    def _prox(self, read, extra=0, **kw):
        """The prox launch (with ``extra`` phases before it), F(X') where something reads it, Monotone's revert."""
        mono = bool(self.opt['Monotone'] and self.k > 0)
        rd = read or mono
        ph = extra | _lib.PGMC_PHASE_PROX | (_lib.PGMC_PHASE_DFID if rd else 0)
        kw['rs_ynext'] = int(mono and bool(kw.get('write_y')))
        s = self._dev.step(self._params(ph, rd, keep_zz=int(mono), **kw), read=rd)
        if mono:
            self.objfn = (s[_lib.PGMC_FX], float(np.sqrt(s[_lib.PGMC_CNSTR])))
            if self.objfn_prev[0] < self.objfn[0]:
                kw.pop('advance', None), kw.pop('advance_y', None)
                # (F of the reverted X is read by a backtracking trial alone: elsewhere no second pass over K)
                ph = _lib.PGMC_PHASE_PROX | (_lib.PGMC_PHASE_DFID if self.backtrack is not None else 0)
                s = self._dev.step(self._params(ph, True, revert=1, **kw))
                if self.backtrack is None:
                    s[_lib.PGMC_FX] = self.objfn_prev[0]
                self.objfn = self.objfn_prev
        return s

    def _step_plain(self, read):
        pol = self.stepsizepolicy
        first = self._first()
        self._momentum()
        if pol is None:
            s = self._prox(read, _lib.PGMC_PHASE_GRAD, write_y=1, **first)
        else:
            bb = isinstance(pol, StepSizePolicyBB)
            rule = self.k > 1
            ph = _lib.PGMC_PHASE_GRAD | (_lib.PGMC_PHASE_GZ2 if (rule and not bb) else 0)
            s1 = self._dev.step(self._params(ph, rule, bb=int(rule and bb), **first), read=rule)
            if rule and bb:
                # (NumPy's division, as the reference: a zero <dx, dg> -- X reverted, or equal iterates -- gives inf or
                # nan, which the rule's test lets through; refused here, where it would reach the kernel as L)
                with np.errstate(divide='ignore', invalid='ignore'):
                    L = float(np.float64(s1[_lib.PGMC_BBG2]) / np.float64(s1[_lib.PGMC_BBXG]))
                if L < 0. or not np.isfinite(L) or L == 0.:
                    L = self.L
                self.L = L
            elif rule:
                self.L = s1[_lib.PGMC_GZ2] / s1[_lib.PGMC_G2]
            s = self._prox(read, write_y=1)
        self._ynext = True
        return s, (None if s is None else s[_lib.PGMC_RS2])

    def _trial(self, s, fy):
        """F <= Q of backtrack.py:99-110 on the sums of a trial."""
        f = s[_lib.PGMC_FX]
        Q = fy + s[_lib.PGMC_DXG] + (float(self.L) / 2.) * s[_lib.PGMC_DXY2]
        return f, Q

    def _step_standard(self, read):
        bt = self.backtrack
        first = self._first()
        self._momentum()
        it, linesearch = 0, True
        while linesearch and it < bt.maxiter:
            if it == 0:
                s = self._prox(True, _lib.PGMC_PHASE_GRAD, write_y=1, **first)
                fy = s[_lib.PGMC_FY]
            else:
                s = self._prox(True, write_y=1)
            f, Q = self._trial(s, fy)
            if f <= Q:
                linesearch = False
            else:
                self.L = self.dtype.type(self.L * bt.gamma_u)
            it += 1
        self.F, self.Q, self.iterBTrack = f, Q, it
        self._ynext = True
        return s, s[_lib.PGMC_RS2]

    def _step_robust(self, read):
        bt = self.backtrack
        if not self._have_z:
            self._dev.upload(_lib.CMOD_PZ, self.X)
            self._have_z = True
        self._ynext = False
        self._beta = self._gamma = 0.0
        self.L = self.dtype.type(self.L * bt.gamma_d)
        it, linesearch = 0, True
        while linesearch and it < bt.maxiter:
            L = float(self.L)
            t = float(1. + np.sqrt(1. + 4. * L * self._Tk)) / (2. * L)
            T = self._Tk + t
            first = it == 0
            upd = first and self._zc is not None
            s = self._prox(True, _lib.PGMC_PHASE_YROBUST | _lib.PGMC_PHASE_GRAD, tk=self._Tk, t=t, advance=int(first),
                           advance_y=int(first), z_update=int(upd), zc=self._zc if upd else 0.0, yprv_alt=1)
            f, Q = self._trial(s, s[_lib.PGMC_FY])
            if f <= Q:
                linesearch = False
            else:
                self.L = self.dtype.type(self.L * bt.gamma_u)
            it += 1
        self._Tk = T
        self._zc = t * float(self.L)       # Z += t L (X - Y): applied on the way into the next step
        self.F, self.Q, self.iterBTrack = f, Q, it
        return s, s[_lib.PGMC_RS2]

    def fused_iteration(self):
        """on_iteration_start, the backtracking or step-size rule, xstep and ystep on the device."""
        for name in ('xstep', 'ystep', 'on_iteration_start'):
            if getattr(type(self), name) is not getattr(pgm.PGM, name):
                raise NotImplementedError("%s: the steps run on the device; %s cannot be overridden"
                                          % (type(self).__name__, name))
        if self.Z is None:
            raise ValueError("%s: setcoef comes before solve" % type(self).__name__)
        read = not self.opt['FastSolve']
        if self.opt['Monotone']:
            if self.k == 0:
                self.objfn = tuple(float(v) for v in self.eval_objfn())
            self.objfn_prev = self.objfn
        self._cache.clear()
        if isinstance(self.backtrack, BacktrackRobust):
            s, rs2 = self._step_robust(read)
        elif isinstance(self.backtrack, BacktrackStandard):
            s, rs2 = self._step_standard(read)
        else:
            s, rs2 = self._step_plain(read)
        self._started = True
        self._sums, self._rs2 = s, rs2
        return True


class WeightedCnstrMOD(CnstrMOD):
    r"""PGM algorithm for  minimise (1/2) ||D Z - S||^2_W  such that  ||d_m|| = 1  with a weight for every element
    of ``D Z - S`` (pgm/cmod.py:238-336).  ``W``: a scalar or of shape (N,), (N, 1), (1, K), (N, K); an ``(N, K)``
    :class:`sporco_amd.device.DeviceArray` is read in place.
    """

    def __init__(self, Z, S, W=None, dsz=None, opt=None, **backend):
        if opt is None:
            opt = CnstrMOD.Options()
        shape = tuple(getattr(S, 'shape', np.shape(S)))
        full = None
        if W is None:
            W = np.array([1.0])
        if is_device_array(W):
            if tuple(W.shape) != shape:
                raise ValueError("a device array W has the shape of S, %s" % (shape,))
            self.W = full = W
        else:
            W = np.asarray(W)
            if np.iscomplexobj(W) or W.dtype.kind not in 'fiub':
                raise TypeError("cmod handles real-valued weights")
            if W.ndim == 1:
                W = W.reshape(-1, 1)
            if W.ndim > 2 or len(shape) != 2:
                raise ValueError("W of shape %s does not broadcast to S %s" % (W.shape, shape))
            sdt = opt['DataType'] if opt['DataType'] is not None else getattr(S, 'dtype', np.asarray(S).dtype)
            self.W = np.asarray(W, dtype=sdt)
            if self.W.size > 1:
                full = np.ascontiguousarray(np.broadcast_to(self.W, shape))      # (raises where it does not)
        super(WeightedCnstrMOD, self).__init__(Z, S, dsz, opt, **backend)
        if full is not None:
            if is_device_array(full) and full.dtype != self.dtype:
                raise TypeError("a device array W has the working precision, %s" % self.dtype)
            self._dev.set_weight(full if is_device_array(full) else full.astype(self.dtype, copy=False))


def getPcn(zm, nnc=False):
    """The constraint-set projection (pgm/cmod.py:342-369): :func:`normalise`, after :func:`zeromean` if ``zm`` or
    after a clip at zero if ``nnc``; both set raise ``ValueError``."""
    if zm:
        if nnc:
            raise ValueError('Parameters zm and nnc may not both be True')
        return lambda x: normalise(zeromean(x))
    if nnc:
        return lambda x: normalise(np.clip(x, 0, None))
    return normalise


def zeromean(v):
    """Subtract the mean of each column (pgm/cmod.py:373-387)."""
    return v - np.mean(v, 0)


def normalise(v):
    """Normalise the columns; a column of norm 0 is divided by 1 (pgm/cmod.py:391-407)."""
    vn = np.sqrt(np.sum(v ** 2, 0))
    vn[vn == 0] = 1.0
    return np.asarray(v / vn, dtype=v.dtype)
