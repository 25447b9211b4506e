"""Dictionary learning for the dense (patch-based) problem on the device, with the interface of the reference's
``sporco.dictlrn.bpdndl`` (sporco/dictlrn/bpdndl.py:23-206): :class:`BPDNDictLearn` alternates one iteration of
:class:`sporco_amd.admm.bpdn.BPDN` with one of :class:`sporco_amd.admm.cmod.CnstrMOD`.

The two handles share the device arrays: the dictionary update reads the signals from the sparse coding handle's
``S`` buffer and, after every x step, the coefficients from its ``Y`` buffer, in place.  During :meth:`solve` no
``(M, K)`` or ``(N, K)`` array crosses to the host; what does is the ``(N, M)`` dictionary, the ``(M, M)`` Gram
and solve matrices and the sums of an iteration.
"""

import copy

import numpy as np

from .. import _lib
from ..admm import bpdn
from ..admm import cmod
from . import dictlrn

__all__ = ['BPDNDictLearn']


class BPDNDictLearn(dictlrn.DictLearn):
    r"""Dictionary learning based on BPDN and CnstrMOD (bpdndl.py:23-206),
    minimise (1/2) ||D X - S||_F^2 + lmbda ||X||_1  such that  ||d_m|| = 1.

    ``IterationStats``: ``Iter, ObjFun, DFid, RegL1, Cnstr, XPrRsdl, XDlRsdl, XRho, DPrRsdl, DDlRsdl, DRho, Time``.
    """

    class Options(dictlrn.DictLearn.Options):
        """Options of bpdndl.py:73-117: ``AccurateDFid``, ``BPDN`` (:class:`bpdn.BPDN.Options`), ``CMOD``
        (:class:`cmod.CnstrMOD.Options`), with the reference's inner defaults."""

        defaults = copy.deepcopy(dictlrn.DictLearn.Options.defaults)
        defaults.update({'AccurateDFid': False, 'BPDN': copy.deepcopy(bpdn.BPDN.Options.defaults),
                         'CMOD': copy.deepcopy(cmod.CnstrMOD.Options.defaults)})

        def __init__(self, opt=None):
            dictlrn.DictLearn.Options.__init__(
                self, {'BPDN': bpdn.BPDN.Options(
                    {'MaxMainIter': 1, 'AutoRho': {'Period': 10, 'AutoScaling': False, 'RsdlRatio': 10.0,
                                                   'Scaling': 2.0, 'RsdlTarget': 1.0}}),
                       'CMOD': cmod.CnstrMOD.Options({'MaxMainIter': 1, 'AutoRho': {'Period': 10},
                                                      'AuxVarObj': False})})
            self.update({} if opt is None else opt)

    def __init__(self, D0, S, lmbda=None, opt=None, **backend):
        if opt is None:
            opt = BPDNDictLearn.Options()
        self.opt = opt
        D0 = np.asarray(D0)
        S = np.asarray(S)
        # (the dictionary is normalised as the D update will keep it, and starts that update: bpdndl.py:151-156)
        D0 = cmod.getPcn(opt['CMOD', 'ZeroMean'])(D0)
        Nc = D0.shape[1]
        opt['CMOD'].update({'Y0': D0, 'U0': np.zeros((S.shape[0], Nc))})
        xstep = bpdn.BPDN(D0, S, lmbda, opt['BPDN'], **backend)
        # the D update reads S and, from post_xstep on, the coefficients in the x step's own device arrays
        dstep = cmod.CnstrMOD(xstep.getcoef_device(), xstep._dev.device_view(_lib.BPDN_S), (Nc, S.shape[1]),
                              opt['CMOD'], **backend)
        xstep._return_min = False
        dstep._return_min = False
        if self.opt['AccurateDFid']:
            isxmap = {'XPrRsdl': 'PrimalRsdl', 'XDlRsdl': 'DualRsdl', 'XRho': 'Rho'}
            evlmap = {'ObjFun': 'ObjFun', 'DFid': 'DFid', 'RegL1': 'RegL1'}
        else:
            isxmap = {'ObjFun': 'ObjFun', 'DFid': 'DFid', 'RegL1': 'RegL1', 'XPrRsdl': 'PrimalRsdl',
                      'XDlRsdl': 'DualRsdl', 'XRho': 'Rho'}
            evlmap = {}
        isc = dictlrn.IterStatsConfig(
            isfld=['Iter', 'ObjFun', 'DFid', 'RegL1', 'Cnstr', 'XPrRsdl', 'XDlRsdl', 'XRho', 'DPrRsdl',
                   'DDlRsdl', 'DRho', 'Time'],
            isxmap=isxmap,
            isdmap={'Cnstr': 'Cnstr', 'DPrRsdl': 'PrimalRsdl', 'DDlRsdl': 'DualRsdl', 'DRho': 'Rho'},
            evlmap=evlmap,
            hdrtxt=['Itn', 'Fnc', 'DFid', u'\u21131', 'Cnstr', 'r_X', 's_X', u'\u03c1_X', 'r_D', 's_D', u'\u03c1_D'],
            hdrmap={'Itn': 'Iter', 'Fnc': 'ObjFun', 'DFid': 'DFid', u'\u21131': 'RegL1', 'Cnstr': 'Cnstr',
                    'r_X': 'XPrRsdl', 's_X': 'XDlRsdl', u'\u03c1_X': 'XRho', 'r_D': 'DPrRsdl', 's_D': 'DDlRsdl',
                    u'\u03c1_D': 'DRho'})
        super(BPDNDictLearn, self).__init__(xstep, dstep, opt, isc)

    def post_xstep(self):
        """The coefficients go to the D update on the device: it reads the x step's ``Y`` in place."""
        self.dstep.setcoef(self.xstep.getcoef_device())

    def evaluate(self):
        """Under ``AccurateDFid`` the functional at the (D, X) pair the outer iteration ends with
        (bpdndl.py:195-206): the data fidelity by ``cmod_dfid``, the l1 term from the x step's own sum."""
        if not self.opt['AccurateDFid']:
            return None
        x = self.xstep
        dfd = self.dstep.dfid_device()
        if x.opt['gEvalY'] and x.wl1.size == 1 and float(x.wl1.ravel()[0]) == 1.0 and x.itstat:
            rl1 = float(x._sums[_lib.OUT_L1])
        else:
            # (the x step's sum is that of a weighted array, or of X: this rare setting pays a download)
            rl1 = float(np.sum(np.abs(x.Y)))
        return dict(DFid=dfd, RegL1=rl1, ObjFun=dfd + float(x.lmbda) * rl1)
