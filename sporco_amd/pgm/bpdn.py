"""Dense (patch-based) sparse coding by proximal gradient (FISTA) steps on the device, with the interface of the
reference's ``sporco.pgm.bpdn`` (sporco/pgm/bpdn.py:26-375): :class:`BPDN` and :class:`WeightedBPDN`,

    minimise (1/2) ||D x - s||^2_W + lmbda ||wl1 x||_1 .

The dictionary ``D`` is ``(N, M)``, the signals ``S`` are ``(N, K)``, the iterates ``X`` and ``Y`` ``(M, K)``.  The
iterates live on the device; one launch of ``bpdn_pgm_step`` (csrc/csc_pgm_bpdn.h) forms ``Y`` from the two last
iterates, the gradient, the proximal step and every scalar of ``F``, ``Q_L``, ``Rsdl``, ``DFid`` and ``RegL1``, so a
step with a fixed ``L`` is that launch, the fixed-order reduction and one small read (none under ``FastSolve``).

The rules of ``pgm.momentum``, ``pgm.stepsize`` and ``pgm.backtrack`` are served by :meth:`BPDN.fused_iteration`,
which reads the parameters (``gamma_u``, ``gamma_d``, ``maxiter``, ``b``, ``a``) off the objects in the options
and keeps the state a rule carries (``Tk`` and ``Z`` of the robust rule; the Barzilai-Borwein rule's previous
iterate and gradient are the device arrays the last step left) with the solver.  A trial of
``BacktrackStandard`` after the first is a prox phase alone on the stored gradient; ``StepSizePolicyCauchy`` and
``StepSizePolicyBB`` launch the gradient phase, read their sums, fix ``L`` and launch the prox phase; ``Monotone``
forms ``Y`` by a launch of its own and reverts ``X`` by a prox phase that copies the previous iterate and sums for it.

Served: real float32 / float64, ``S`` of shape ``(N, K)`` with ``K >= 1``, ``M`` and ``N`` up to 512, ``L1Weight`` a
scalar or an array that broadcasts to ``(M, K)``, ``W`` a scalar or of shape ``(N,)``, ``(N, 1)``, ``(1, K)`` or
``(N, K)``, every option of ``PGM.Options``, ``setdict``, restart of ``solve``.

Refused: complex, float16 and non-floating inputs (``TypeError``), ``M`` or ``N`` above 512, ``S.ndim != 2``, a row
mismatch, a ``W`` that does not broadcast to ``S`` (``ValueError``), rule objects of other classes than those of
``sporco_amd.pgm``, ``reducer=`` and pickling (``NotImplementedError``).  There is no CPU path.
"""

import copy

import numpy as np

from .. import _lib
from ..admm.bpdn import GenericBPDN as _AdmmBPDN
from ..device import is_device_array
from . import pgm
from .backtrack import BacktrackRobust, BacktrackStandard
from .momentum import MomentumGenLinear, MomentumLinear, MomentumNesterov
from .stepsize import StepSizePolicyBB, StepSizePolicyCauchy

__all__ = ['BPDN', 'WeightedBPDN']


def plan(N, M, K, dtype=np.float32):
    """The launch plan of an ``(N, M, K)`` problem: ``dict(KB, blocks, mfma, lds)`` -- the columns of a
    workgroup's block, the workgroups, whether the products use the matrix instruction, the LDS bytes."""
    h = _lib.PgmBpdnHandle(N, M, K, dtype)
    try:
        return h.plan()
    finally:
        h.close()


class BPDN(pgm.PGM):
    r"""PGM algorithm for  minimise (1/2) ||D x - s||^2 + lmbda ||wl1 x||_1  (pgm/bpdn.py:26-243).

    ``IterationStats``: ``Iter, ObjFun, DFid, RegL1, Rsdl, F_Btrack, Q_Btrack, IterBTrack, L, Time``.
    """

    class Options(pgm.PGM.Options):
        """``PGM.Options`` with ``NonNegCoef`` False, ``L1Weight`` 1.0 (a scalar, or an array that broadcasts to
        ``(M, K)``) and ``L`` 500.0 (pgm/bpdn.py:69-107)."""

        defaults = copy.deepcopy(pgm.PGM.Options.defaults)
        defaults.update({'NonNegCoef': False, 'L1Weight': 1.0, 'L': 500.0})

        def __init__(self, opt=None):
            pgm.PGM.Options.__init__(self, {} if opt is None else opt)

    itstat_fields_objfn = ('ObjFun', 'DFid', 'RegL1')
    hdrtxt_objfn = ('Fnc', 'DFid', u'Regℓ1')
    hdrval_objfun = {'Fnc': 'ObjFun', 'DFid': 'DFid', u'Regℓ1': 'RegL1'}

    # (tests) False: Y is formed by a launch of its own after every step instead of on the way into the next
    _fold_momentum = True

    def __init__(self, D, S, lmbda=None, opt=None, **backend):
        if opt is None:
            opt = BPDN.Options()
        D, S = _AdmmBPDN._check_inputs(D, S, backend)
        self.set_dtype(opt, S.dtype)
        if self.dtype not in (np.float32, np.float64):
            raise TypeError("sporco_amd works in float32 or float64, not %s" % self.dtype)
        for rule, classes in ((opt['Momentum'], (MomentumNesterov, MomentumLinear, MomentumGenLinear)),
                              (opt['StepSizePolicy'], (type(None), StepSizePolicyCauchy, StepSizePolicyBB)),
                              (opt['Backtrack'], (type(None), BacktrackStandard, BacktrackRobust))):
            if type(rule) not in classes:
                raise NotImplementedError("pgm.bpdn serves the rules of sporco_amd.pgm, not %s" % type(rule).__name__)
        if opt['Backtrack'] is not None and int(opt['Backtrack'].maxiter) < 1:
            raise ValueError("Backtrack.maxiter must be at least 1")
        N, K = S.shape
        M = D.shape[1]
        self._dims = (N, M, K)
        self.S = np.ascontiguousarray(S, dtype=self.dtype)
        wl1 = np.asarray(opt['L1Weight'])
        if np.iscomplexobj(wl1):
            raise TypeError("bpdn handles real-valued weights")
        self.wl1 = np.asarray(wl1, dtype=self.dtype)
        if self.wl1.ndim > 0:
            np.broadcast_to(self.wl1, (M, K))      # (raises where it does not broadcast)
        self._dev = _lib.PgmBpdnHandle(N, M, K, self.dtype, device=backend.get('device', 0),
                                       stream=backend.get('stream'))
        self._dev.upload(_lib.BPDN_S, self.S)
        if self.wl1.size > 1:
            self._dev.upload(_lib.BPDN_WL1, np.ascontiguousarray(np.broadcast_to(self.wl1, (M, K))))
        self._cache = {}
        self._sums = None
        self._rs2 = None
        self._pending_beta = None
        self._y_swapped = False
        self._started = False
        self._Tk = 0.0
        self._zc = None
        self._have_z = False
        if not hasattr(self, 'W'):
            self.W = np.asarray(1.0, dtype=self.dtype)
        self.setdict(D)
        if lmbda is None:
            lmbda = 0.1 * float(np.abs(self._dev.download(_lib.BPDN_DTS)).max())
        self.lmbda = self.dtype.type(lmbda)
        super(BPDN, self).__init__((M, K), self.dtype, opt)

    # -- state ---------------------------------------------------------------------------------------------
    def init_state(self, xshape):
        """X = ``X0`` or zero, Y = X (pgm.py:257-261, pgm/bpdn.py:155-156)."""
        if self.opt['X0'] is not None:
            self.X = np.asarray(self.opt['X0']).astype(self.dtype, copy=True)
        self._dev.copy(_lib.BPDN_Y, _lib.BPDN_X)

    def _fetch(self, var):
        if var not in self._cache:
            self._cache[var] = self._dev.download(var)
        return self._cache[var]

    def _store(self, var, value):
        value = np.asarray(value, dtype=self.dtype)
        if value.shape != self._dims[1:]:
            raise ValueError("array of shape %s where %s is expected" % (value.shape, self._dims[1:]))
        self._dev.upload(var, np.ascontiguousarray(value))
        self._cache.clear()
        self._sums = None

    @property
    def X(self):
        return self._fetch(_lib.BPDN_X)

    @X.setter
    def X(self, value):
        self._store(_lib.BPDN_X, value)

    @property
    def Xprv(self):
        return self._fetch(_lib.BPDN_XPRV)

    @property
    def Y(self):
        """The auxiliary iterate.  Where the momentum step is folded into the next launch it is formed here, by
        the kernel's own operations in the working precision."""
        if self._pending_beta is None:
            return self._fetch(_lib.BPDN_Y)
        X, Xp = self.X, self.Xprv
        return X + self.dtype.type(self._pending_beta) * (X - Xp)

    @Y.setter
    def Y(self, value):
        if value is not None:
            self._store(_lib.BPDN_Y, value)
            self._pending_beta = None

    @property
    def Yprv(self):
        """The Y the last iteration started from (before the first one: the reference's Y + 1e3)."""
        if not self._started:
            return self._fetch(_lib.BPDN_Y) + self.dtype.type(1e3)
        return self._fetch(_lib.BPDN_YPRV if self._y_swapped else _lib.BPDN_Y)

    def __getstate__(self):
        raise NotImplementedError("%s: pickling is not offered" % type(self).__name__)

    def setdict(self, D):
        """Set the dictionary (pgm/bpdn.py:162-165); the iterates stay."""
        if is_device_array(D):
            raise TypeError("bpdn takes host arrays for D and S, not DeviceArrays")
        D = np.asarray(D)
        if D.ndim != 2 or D.shape != self._dims[:2]:
            raise ValueError("D of shape %s where %s is expected" % (getattr(D, 'shape', None), self._dims[:2]))
        if np.iscomplexobj(D):
            raise TypeError("bpdn handles real-valued D and S")
        self.D = np.array(D, dtype=self.dtype, order='C')
        self._dev.set_dict(self.D)
        self._sums = None

    def getcoef(self):
        return self.X

    def getmin(self):
        return self.X

    def getcoef_device(self):
        """The current ``X`` as a :class:`sporco_amd.device.DeviceArray` over the handle's own buffer: no copy.  The
        two X arrays change roles with every step, so the view is taken again after each ``solve``."""
        return self._dev.device_view(_lib.BPDN_X)

    def finish_solve(self):
        self._dev.sync()

    # -- the reference's methods on host arrays ----------------------------------------------------------
    def grad_f(self, V=None):
        """D^T (W (D V - S)) for a host array ``V`` (default: Y)."""
        if V is None:
            V = self.Y
        return self.D.T.dot(self.W * (self.D.dot(V) - self.S))

    def prox_g(self, V):
        """prox_l1(V, (lmbda / L) wl1) with ``NonNegCoef`` (pgm/bpdn.py:186-193)."""
        V = np.asarray(V)
        alpha = (self.lmbda / self.L) * self.wl1
        U = np.asarray(np.sign(V) * np.maximum(0, np.abs(V) - alpha), dtype=self.dtype)
        if self.opt['NonNegCoef']:
            U[U < 0.0] = 0.0
        return U

    def hessian_f(self, V):
        """D^T D V (pgm/bpdn.py:197-201; the reference's weighted class does not weight it either)."""
        return self.D.T.dot(self.D.dot(V))

    def obfn_f(self, X=None):
        if X is None:
            X = self.X
        return 0.5 * np.linalg.norm((np.sqrt(self.W) * (self.D.dot(X) - self.S)).ravel()) ** 2

    def obfn_reg(self):
        if self._sums is not None:
            rl1 = self._sums[_lib.PGMB_L1]
        else:
            rl1 = np.linalg.norm((self.wl1 * self.X).ravel(), 1)
        return (self.lmbda * rl1, rl1)

    def eval_objfn(self):
        """(ObjFun, DFid, RegL1) of X: from the sums of the step that left X, else on the host."""
        dfd = self._sums[_lib.PGMB_FX] if self._sums is not None else self.obfn_f()
        reg = self.obfn_reg()
        return (dfd + reg[0], dfd) + reg[1:]

    def reconstruct(self, X=None):
        """``D . self.X`` whatever is passed, as the reference (pgm/bpdn.py:237-242)."""
        return self.D.dot(self.X)

    def rsdl(self):
        return float(np.sqrt(self._rs2))

    # -- iteration ---------------------------------------------------------------------------------------
    def _params(self, **kw):
        p = _lib.BpdnPgmParams()
        p.L = float(self.L)
        p.lmbda = float(self.lmbda)
        p.wl1 = float(self.wl1.ravel()[0]) if self.wl1.size == 1 else 1.0
        p.w = float(self.W.ravel()[0]) if self.W.size == 1 else 1.0
        p.nonneg = 1 if self.opt['NonNegCoef'] else 0
        p.phase = _lib.PGMB_PHASE_GRAD | _lib.PGMB_PHASE_PROX
        p.keep_zz = 1 if (self.opt['Monotone'] and self.k > 0) else 0
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def _monotone(self, s):
        """The Monotone block of xstep (pgm.py:413-420) on the sums of the step that left X; the sums of the X
        it leaves."""
        if not (self.opt['Monotone'] and self.k > 0):
            return s
        self.objfn = (s[_lib.PGMB_FX] + float(self.lmbda) * s[_lib.PGMB_L1], s[_lib.PGMB_FX], s[_lib.PGMB_L1])
        if self.objfn_prev[0] < self.objfn[0]:
            s = self._dev.step(self._params(phase=_lib.PGMB_PHASE_PROX, revert=1, keep_zz=0))
            self.objfn = self.objfn_prev
        return s

    def _take_momentum(self):
        """(ymode, beta) of the next gradient phase."""
        beta, self._pending_beta = self._pending_beta, None
        if beta is None:
            return {'ymode': _lib.PGMB_Y_LOAD}
        return {'ymode': _lib.PGMB_Y_MOMENTUM, 'beta': float(beta)}

    def _ystep(self, s, read):
        """ystep of pgm.py:426-441: folded into the next launch, or (Monotone) a launch of its own."""
        tprv = self.t
        self.t = self.momentum.update(self.var_momentum())
        beta = (tprv - 1.) / self.t
        mono = self.opt['Monotone']
        if mono and self.k > 0:
            sy = self._dev.ystep(beta, tprv / self.t, use_zz=True, advance_y=True, read=read)
            self._y_swapped = True
            return None if sy is None else sy[_lib.PGMB_RS2]
        if mono or not self._fold_momentum:
            self._dev.ystep(beta, advance_y=True, read=False)
            self._y_swapped = True
        else:
            self._pending_beta = beta
            self._y_swapped = False
        return None if s is None else s[_lib.PGMB_RS2]

    def _step_plain(self, read):
        mono = self.opt['Monotone'] and self.k > 0
        pol = self.stepsizepolicy
        first = dict(advance=1, **self._take_momentum())
        if pol is None:
            s = self._dev.step(self._params(**first), read=read or mono)
        else:
            bb = isinstance(pol, StepSizePolicyBB)
            rule = self.k > 1
            s1 = self._dev.step(self._params(phase=_lib.PGMB_PHASE_GRAD, cauchy=int(rule and not bb),
                                             bb=int(rule and bb), **first), read=rule)
            if rule and bb:
                L = s1[_lib.PGMB_BBG2] / s1[_lib.PGMB_BBXG]
                if L < 0.:
                    L = self.L
                self.L = L
            elif rule:
                self.L = s1[_lib.PGMB_DG2] / s1[_lib.PGMB_G2]
            s = self._dev.step(self._params(phase=_lib.PGMB_PHASE_PROX), read=read or mono)
        if s is not None:
            s = self._monotone(s)
        return s, self._ystep(s, read)

    def _trial(self, s, fy):
        """F <= Q of backtrack.py:99-110 on the sums of a trial."""
        f = s[_lib.PGMB_FX]
        Q = fy + s[_lib.PGMB_DXG] + (float(self.L) / 2.) * s[_lib.PGMB_DXY2]
        return f, Q

    def _step_standard(self, read):
        bt = self.backtrack
        it, linesearch = 0, True
        while linesearch and it < bt.maxiter:
            if it == 0:
                s = self._dev.step(self._params(advance=1, **self._take_momentum()))
                fy = s[_lib.PGMB_FY]
            else:
                s = self._dev.step(self._params(phase=_lib.PGMB_PHASE_PROX))
            s = self._monotone(s)
            f, Q = self._trial(s, fy)
            if f <= Q:
                linesearch = False
            else:
                self.L = self.dtype.type(self.L * bt.gamma_u)
            it += 1
        self.F, self.Q, self.iterBTrack = f, Q, it
        return s, self._ystep(s, read)

    def _step_robust(self, read):
        bt = self.backtrack
        if not self._have_z:
            self._dev.copy(_lib.BPDN_Z, _lib.BPDN_X)
            self._have_z = True
        self.L = self.dtype.type(self.L * bt.gamma_d)
        it, linesearch = 0, True
        while linesearch and it < bt.maxiter:
            L = float(self.L)
            t = float(1. + np.sqrt(1. + 4. * L * self._Tk)) / (2. * L)
            T = self._Tk + t
            first = it == 0
            upd = first and self._zc is not None
            s = self._dev.step(self._params(ymode=_lib.PGMB_Y_ROBUST, tk=self._Tk, t=t, advance=int(first),
                                            advance_y=int(first), z_update=int(upd), zc=self._zc if upd else 0.0))
            s = self._monotone(s)
            f, Q = self._trial(s, s[_lib.PGMB_FY])
            if f <= Q:
                linesearch = False
            else:
                self.L = self.dtype.type(self.L * bt.gamma_u)
            it += 1
        self._Tk = T
        self._zc = t * float(self.L)       # Z += t L (X - Y): applied on the way into the next step
        self._y_swapped = True
        self._pending_beta = None
        self.F, self.Q, self.iterBTrack = f, Q, it
        mono = self.opt['Monotone'] and self.k > 0
        return s, s[_lib.PGMB_DXY2 if mono else _lib.PGMB_RS2]

    def fused_iteration(self):
        """on_iteration_start, the backtracking or step-size rule, xstep and ystep on the device."""
        for name in ('xstep', 'ystep', 'on_iteration_start'):
            if getattr(type(self), name) is not getattr(pgm.PGM, name):
                raise NotImplementedError("%s: the steps run on the device; %s cannot be overridden"
                                          % (type(self).__name__, name))
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


class WeightedBPDN(BPDN):
    r"""PGM algorithm for  minimise (1/2) ||D x - s||^2_W + lmbda ||wl1 x||_1  with W = diag(w), a weight for
    every element of ``D x - s`` (pgm/bpdn.py:248-369).  ``W``: a scalar or of shape (N,), (N, 1), (1, K), (N, K).
    """

    def __init__(self, D, S, lmbda=None, W=None, opt=None, **backend):
        if opt is None:
            opt = BPDN.Options()
        D, S = _AdmmBPDN._check_inputs(D, S, backend)
        self.set_dtype(opt, S.dtype)
        if self.dtype not in (np.float32, np.float64):
            raise TypeError("sporco_amd works in float32 or float64, not %s" % self.dtype)
        if W is None:
            W = np.array([1.0])
        if is_device_array(W):
            raise TypeError("bpdn takes a host array for W, not a DeviceArray")
        W = np.asarray(W)
        if np.iscomplexobj(W) or W.dtype.kind not in 'fiub':
            raise TypeError("bpdn handles real-valued weights")
        if W.ndim == 1:
            W = W.reshape(-1, 1)
        if W.ndim > 2:
            raise ValueError("W of shape %s does not broadcast to S %s" % (W.shape, S.shape))
        self.W = np.asarray(W, dtype=self.dtype)
        full = np.broadcast_to(self.W, S.shape) if self.W.ndim > 0 else None      # (raises where it does not)
        super(WeightedBPDN, self).__init__(D, S, lmbda, opt, **backend)
        if self.W.size > 1:
            self._dev.upload(_lib.BPDN_W, np.ascontiguousarray(full))
