"""Dictionary learning for the dense (patch-based) problem with a weighted data fidelity term on the device, with the
interface of the reference's ``sporco.dictlrn.wbpdndl`` (sporco/dictlrn/wbpdndl.py:24-210):
:class:`WeightedBPDNDictLearn` alternates one proximal gradient step of :class:`sporco_amd.pgm.bpdn.WeightedBPDN` with
one of :class:`sporco_amd.pgm.cmod.WeightedCnstrMOD`.  ``W`` weights (or, with zeros, masks) the samples of ``S``.

The two handles share the device arrays: the dictionary update reads the signals and an ``(N, K)`` weight from the
sparse coding handle's ``S`` and ``W`` buffers and, after every x step, the coefficients from its current ``X``
buffer, in place (the x step's two X arrays change roles with every step, so the current one is handed over each
time).  During :meth:`solve` no ``(M, K)`` or ``(N, K)`` array crosses to the host; what does is the ``(N, M)``
dictionary and the sums of an iteration.
"""

import copy

import numpy as np

from .. import _lib
from ..pgm import bpdn
from ..pgm import cmod
from . import dictlrn

__all__ = ['WeightedBPDNDictLearn']


class WeightedBPDNDictLearn(dictlrn.DictLearn):
    r"""Dictionary learning based on weighted BPDN and CnstrMOD (wbpdndl.py:24-210),
    minimise (1/2) ||D X - S||_W^2 + lmbda ||X||_1  such that  ||d_m|| = 1.

    ``IterationStats``: ``Iter, ObjFun, DFid, RegL1, Cnstr, XRsdl, XL, DRsdl, DL, Time``.
    """

    class Options(dictlrn.DictLearn.Options):
        """Options of wbpdndl.py:86-127: ``AccurateDFid``, ``BPDN`` (:class:`bpdn.BPDN.Options`), ``CMOD``
        (:class:`cmod.CnstrMOD.Options`), both with ``MaxMainIter`` 1."""

        defaults = copy.deepcopy(dictlrn.DictLearn.Options.defaults)
        defaults.update({'AccurateDFid': False, 'BPDN': copy.deepcopy(bpdn.WeightedBPDN.Options.defaults),
                         'CMOD': copy.deepcopy(cmod.WeightedCnstrMOD.Options.defaults)})

        def __init__(self, opt=None):
            dictlrn.DictLearn.Options.__init__(
                self, {'BPDN': bpdn.WeightedBPDN.Options({'MaxMainIter': 1}),
                       'CMOD': cmod.WeightedCnstrMOD.Options({'MaxMainIter': 1})})
            self.update({} if opt is None else opt)

    def __init__(self, D0, S, lmbda=None, W=None, opt=None, **backend):
        if opt is None:
            opt = WeightedBPDNDictLearn.Options()
        self.opt = opt
        D0 = np.asarray(D0)
        S = np.asarray(S)
        # (the dictionary is normalised as the D update will keep it, and starts that update: wbpdndl.py:151-157)
        D0 = cmod.getPcn(opt['CMOD', 'ZeroMean'], opt['CMOD', 'NonNegCoef'])(D0)
        Nc = D0.shape[1]
        opt['CMOD'].update({'X0': D0})
        xstep = bpdn.WeightedBPDN(D0, S, lmbda, W, opt['BPDN'], **backend)
        self.W = xstep.W
        # the D update reads S, an (N, K) W and, from post_xstep on, the coefficients in the x step's own device arrays
        Wd = xstep._dev.device_view(_lib.BPDN_W) if xstep.W.size > 1 else xstep.W
        dstep = cmod.WeightedCnstrMOD(xstep.getcoef_device(), xstep._dev.device_view(_lib.BPDN_S), Wd,
                                      (Nc, S.shape[1]), opt['CMOD'], **backend)
        xstep._return_min = False
        dstep._return_min = False
        if self.opt['AccurateDFid']:
            isxmap = {'XRsdl': 'Rsdl', 'XL': 'L'}
            evlmap = {'ObjFun': 'ObjFun', 'DFid': 'DFid', 'RegL1': 'RegL1'}
        else:
            isxmap = {'ObjFun': 'ObjFun', 'DFid': 'DFid', 'RegL1': 'RegL1', 'XRsdl': 'Rsdl', 'XL': 'L'}
            evlmap = {}
        isc = dictlrn.IterStatsConfig(
            isfld=['Iter', 'ObjFun', 'DFid', 'RegL1', 'Cnstr', 'XRsdl', 'XL', 'DRsdl', 'DL', 'Time'],
            isxmap=isxmap,
            isdmap={'Cnstr': 'Cnstr', 'DRsdl': 'Rsdl', 'DL': 'L'},
            evlmap=evlmap,
            hdrtxt=['Itn', 'Fnc', 'DFid', u'ℓ1', 'Cnstr', 'X_Rsdl', 'X_L', 'D_Rsdl', 'D_L'],
            hdrmap={'Itn': 'Iter', 'Fnc': 'ObjFun', 'DFid': 'DFid', u'ℓ1': 'RegL1', 'Cnstr': 'Cnstr',
                    'X_Rsdl': 'XRsdl', 'X_L': 'XL', 'D_Rsdl': 'DRsdl', 'D_L': 'DL'})
        super(WeightedBPDNDictLearn, self).__init__(xstep, dstep, opt, isc)

    def post_xstep(self):
        """The coefficients go to the D update on the device: it reads the x step's current ``X`` in place."""
        self.dstep.setcoef(self.xstep.getcoef_device())
        # (setdict, after the D step, drops the x step's sums: keep the one evaluate wants)
        s = self.xstep._sums
        self._rl1 = None if s is None else float(s[_lib.PGMB_L1])

    def evaluate(self):
        """Under ``AccurateDFid`` the functional at the (D, X) pair the outer iteration ends with
        (wbpdndl.py:199-210): the weighted data fidelity by ``cmod_dfid``, the l1 term from the x step's own sum
        where that sum is ``||X||_1``."""
        if not self.opt['AccurateDFid']:
            return None
        x = self.xstep
        dfd = self.dstep.dfid_device()
        if getattr(self, '_rl1', None) is not None and x.wl1.size == 1 and float(x.wl1.ravel()[0]) == 1.0:
            rl1 = self._rl1
        else:
            # (the x step's sum is that of a weighted array, or there is none: this rare setting pays a download)
            rl1 = float(np.sum(np.abs(x.X)))
        return dict(DFid=dfd, RegL1=rl1, ObjFun=dfd + float(x.lmbda) * rl1)
