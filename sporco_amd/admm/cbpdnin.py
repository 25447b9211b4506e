"""ADMM convolutional sparse coding with lateral and self inhibition on the GPU.

Drop-in for the reference's ``sporco.admm.cbpdnin.ConvBPDNInhib`` (sporco/admm/cbpdnin.py:28-352):
same constructor signature, Options tree, IterationStats fields and attributes (``wml``, ``wms``,
``Wg``, ``mu``, ``gamma``, ``smooth``).

The iteration is the one of :class:`sporco_amd.admm.cbpdn.ConvBPDN` with an array l1 weight that
changes between iterations.  The thresholds ``lmbda wl1 + mu wml + gamma wms`` live in the handle's
L1-weight array; after every iteration one HIP kernel (``sporco_amd_csc_inhib_update``,
csrc/csc_inhib.hip) recomputes ``wml`` and ``wms`` from the X of that iteration -- the windowed
convolution of ``|X|`` as two short tap sums in LDS instead of the reference's two FFT round
trips --, rewrites the thresholds and returns the three regulariser sums.
"""

import copy

import numpy as np

from . import cbpdn
from .. import _lib
from ..fft import real_dtype

__all__ = ['ConvBPDNInhib']


class ConvBPDNInhib(cbpdn.ConvBPDN):
    r"""Convolutional BPDN with inhibition: minimise (1/2)||sum_m d_m * x_m - s||_2^2 +
    lambda sum_m ||x_m||_1 + mu sum_m omega_m^T |x_m| + gamma sum_m z_m^T |x_m|, the weights omega
    (lateral: the windowed activity of the other members of a filter's groups) and z (self: the
    filter's own windowed activity away from the origin) recomputed from X in every iteration and
    smoothed over the iterations (reference class: sporco/admm/cbpdnin.py:28-352).

    Inhibition is active when ``(Wg is not None and mu != 0) or gamma != 0``; otherwise the class is
    :class:`ConvBPDN` (its fused iteration, under the per-iteration host loop) and reports
    ``RegLat = RegSelf = 0``.
    While it is active the iterations are driven from the host, one ``admm_iter`` (fused when no
    step is overridden, the staged calls otherwise) and one ``inhib_update`` each.

    In scope: ``dimN`` 1 and 2, float32 / float64, scalar or array ``L1Weight``, ``NonNegCoef``,
    ``NoBndryCross``, ``AutoRho``, ``RelaxParam``, ``gEvalY`` / ``fEvalX``, ``dimK``, multi-signal
    and multi-channel ``S`` with a single-channel ``D``.  Refused (``NotImplementedError``):
    ``dimN = 3``, ``reducer=`` (image sharding), complex data, wrapping in ``AddMaskSim``,
    multi-channel dictionaries, pickling while inhibition is active.  The update is not part of
    the device-driven loop (``sporco_amd_csc_admm_run``).

    IterationStats fields: ``Iter, ObjFun, DFid, RegL1, RegLat, RegSelf, PrimalRsdl, DualRsdl,
    EpsPrimal, EpsDual, Rho, XSlvRelRes, Time``.
    """

    _multichannel_dict_ok = False

    class Options(cbpdn.ConvBPDN.Options):
        """Adds ``SmoothWeight`` (cbpdnin.py:115-121): the share of the previous inhibition
        weights kept by an update."""

        defaults = copy.deepcopy(cbpdn.ConvBPDN.Options.defaults)
        defaults.update({'SmoothWeight': 0.9})

        def __init__(self, opt=None):
            cbpdn.ConvBPDN.Options.__init__(self, {} if opt is None else opt)

    itstat_fields_objfn = ('ObjFun', 'DFid', 'RegL1', 'RegLat', 'RegSelf')
    hdrtxt_objfn = ('Fnc', 'DFid', u'Regℓ1', 'RegLat', 'RegSelf')
    hdrval_objfun = {'Fnc': 'ObjFun', 'DFid': 'DFid', u'Regℓ1': 'RegL1', 'RegLat': 'RegLat',
                     'RegSelf': 'RegSelf'}

    _inhib_dev = False     # the handle holds inhibition state (set at the end of __init__)

    def __init__(self, D, S, Wg=None, Whn=None, win_args=None, lmbda=None, mu=None, gamma=None,
                 opt=None, dimK=None, dimN=2, **backend):
        if opt is None:
            opt = ConvBPDNInhib.Options()
        if dimN not in (1, 2):
            raise NotImplementedError("ConvBPDNInhib: dimN = 1 (signals) and 2 (images); the "
                                      "inhibition window of volumes is not offered")
        if backend.get('reducer') is not None:
            raise NotImplementedError("ConvBPDNInhib: no image sharding (reducer=): the inhibition "
                                      "window crosses the shard borders")
        if backend.get('resident') or not isinstance(S, np.ndarray):
            raise NotImplementedError("ConvBPDNInhib takes host arrays and returns host arrays")
        super(ConvBPDNInhib, self).__init__(D, S, lmbda, opt, dimK=dimK, dimN=dimN, **backend)
        rdt = real_dtype(self.dtype).type
        self.Wg = Wg
        self.mu = rdt(10 * self.lmbda if mu is None else mu)
        self.gamma = rdt(0.0 if gamma is None else gamma)
        self.smooth = self.opt['SmoothWeight']
        self._inh_sums = (0.0, 0.0, 0.0)
        self._inhib_lat = self._inhib_self = False
        if not ((self.Wg is not None and self.mu != 0) or self.gamma):
            return
        if self.Wg is not None:
            self.Wg = np.asarray(self.Wg).astype(self.dtype)
            if self.Wg.ndim != 2 or self.Wg.shape[1] != self.cri.M:
                raise ValueError("Wg must be a (groups, filters) matrix with %d columns" % self.cri.M)
            self.cri.Ng = self.Wg.shape[0]
            self.cri.Mgs = np.sum((self.Wg != 0), axis=1)
        if Whn is None:
            Whn = np.asarray(D).shape[0]      # filter extent along the first spatial axis
        if win_args is None:
            win_args = ('tukey', 0.5)
        Whn = int(Whn)
        Whn += not Whn % 2                    # (odd: the origin is the window's centre tap)
        if Whn > min(self.cri.Nv[2 - dimN:]):
            raise ValueError("inhibition window of %d samples does not fit the signal %s"
                             % (Whn, tuple(self.cri.Nv[2 - dimN:])))
        # The reference's window (cbpdnin.py:253-274) is (w[i] w[j])^(1/dimN) with w the periodic
        # scipy window, rolled so that tap Whn // 2 sits at the origin: separable, taps
        # w^(1/dimN) along every spatial axis.
        from scipy import signal
        taps = np.power(np.asarray(signal.get_window(win_args, Whn), dtype=np.float64), 1.0 / dimN)
        self._taps = (np.ones(1) if dimN == 1 else taps, taps)
        self.Whn = Whn
        self._inhib_lat = bool(self.Wg is not None and self.mu > 0)
        self._inhib_self = bool(self.gamma > 0)
        # (a negative mu / gamma leaves the weights at zero in the reference too: plain ConvBPDN)
        self._inhib_dev = self._inhib_lat or self._inhib_self
        self._upload_weights()

    # -- device state -------------------------------------------------------------------------
    def _upload_weights(self):
        super(ConvBPDNInhib, self)._upload_weights()     # (ends any inhibition state of the handle)
        if self._inhib_dev:
            self._dev.inhib_setup(self.Wg if self._inhib_lat else None, self._taps[0], self._taps[1],
                                  self._inhib_self, float(self.lmbda) * self._wl1_scalar)
            self._touch(_lib.VAR_WML, _lib.VAR_WMS)

    @property
    def wml(self):
        """Lateral inhibition weights, ``cri.shpX`` (0 while there is no lateral term)."""
        return self._fetch(_lib.VAR_WML) if self._inhib_lat else 0

    @property
    def wms(self):
        """Self inhibition weights, ``cri.shpX`` (0 while there is no self term)."""
        return self._fetch(_lib.VAR_WMS) if self._inhib_self else 0

    def _set_ams(self, W):
        raise NotImplementedError("ConvBPDNInhib cannot be wrapped in AddMaskSim: the inhibition "
                                  "weights of the appended impulse filter are not defined here")

    def __getstate__(self):
        if self._inhib_dev:
            raise NotImplementedError("ConvBPDNInhib: pickling with inhibition active is not offered")
        return super(ConvBPDNInhib, self).__getstate__()

    # -- parameters: the thresholds are the L1-weight array, so lambda is 1 on the device ---------
    def _lmbda_eff(self):
        return 1.0 if self._inhib_dev else super(ConvBPDNInhib, self)._lmbda_eff()

    def _flags(self):
        f = super(ConvBPDNInhib, self)._flags()
        if self._inhib_dev:
            if f & _lib.FLAG_NO_X:
                raise NotImplementedError("ConvBPDNInhib needs X in every iteration (no FLAG_NO_X)")
            f |= _lib.FLAG_KEEP_X
        return f

    def _device_loop_ok(self):
        return not self._inhib_dev and super(ConvBPDNInhib, self)._device_loop_ok()

    # -- iteration ----------------------------------------------------------------------------
    def iteration(self):
        """The ConvBPDN iteration (the y step uses the weights of the previous iteration,
        cbpdnin.py:303-306), then the weight update from this iteration's X (:308-334)."""
        res = super(ConvBPDNInhib, self).iteration()
        if self._inhib_dev:
            self.inhib_update()
        return res

    def inhib_update(self):
        flags = _lib.FLAG_GEVAL_Y if self.opt['gEvalY'] else 0
        out = self._dev.inhib_update(float(self.lmbda) * self._wl1_scalar,
                                     float(self.mu) if self._inhib_lat else 0.0,
                                     float(self.gamma) if self._inhib_self else 0.0,
                                     float(self.smooth), flags)
        self._inh_sums = (abs(self._wl1_scalar) * out[_lib.OUT_L1], out[_lib.OUT_L21],
                          out[_lib.OUT_RGR])
        self._touch(_lib.VAR_WML, _lib.VAR_WMS)

    def obfn_reg(self):
        """lmbda ||wl1 G||_1 + mu ||wml G||_1 + gamma ||wms G||_1 with the updated weights
        (cbpdnin.py:341-352)."""
        if not self._inhib_dev:
            reg = super(ConvBPDNInhib, self).obfn_reg()
            return reg + (0.0, 0.0)
        rl, rm, rg = self._inh_sums
        return (self.lmbda * rl + self.mu * rm + self.gamma * rg, rl, rm, rg)


ConvBPDNInhib._fused_base = ConvBPDNInhib
