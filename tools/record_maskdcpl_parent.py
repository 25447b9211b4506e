#!/usr/bin/env python3
"""Record what ConvBPDNMaskDcpl computes on the existing mask-decoupling fixtures with a given build
of the CPU simulator library, bit for bit: tests/golden/l1l1_parent_mdcpl.npz.

TEST INFRASTRUCTURE ONLY.  Written once, with the simulator library built from the commit BEFORE
ConvL1L1Grd (which gave the ADMM epilogue its optional ``dy_out`` output and the class its
``_device_iteration`` hook): tests/test_l1l1.py compares the current build's arrays with these by
``==``, so a change that alters anything the parent class computes shows.

    python tools/record_maskdcpl_parent.py /path/to/libsporco_amd_hostsim.so [OUT.npz]

Run it from a checkout of that commit (this file copied into its tools/): the Python package and
the library then agree on the entry points.

The cases and their options are those of tests/test_maskdcpl.py.  Stored per case: X, Y, U, the final
rho and every IterationStats trace but Time.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

TRACES = ('ObjFun', 'DFid', 'RegL1', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho')


def run_case(name, optd, golden):
    """The arrays of one case as a dict (also what tests/test_l1l1.py runs)."""
    from sporco_amd.admm import cbpdn
    g = golden(name)
    optd = dict(optd)
    if 'wl1' in g:
        optd['L1Weight'] = g['wl1']
    b = cbpdn.ConvBPDNMaskDcpl(g['D'], g['S'], float(g['lmbda']), g['W'], cbpdn.ConvBPDNMaskDcpl.Options(optd))
    b.solve()
    out = {'X': b.X, 'Y': b.Y, 'U': b.U, 'rho': np.asarray(b.rho)}
    its = b.getitstat()
    for f in TRACES:
        out['it_' + f] = np.asarray(getattr(its, f), dtype=np.float64)
    if optd.get('LinSolveCheck'):
        out['it_XSlvRelRes'] = np.asarray(its.XSlvRelRes, dtype=np.float64)
    return out


def main():
    import sporco_amd
    from conftest import load_golden
    from test_maskdcpl import CASES
    path = os.path.abspath(sys.argv[1])
    os.environ['SPORCO_AMD_RCCL_LIB'] = path
    sporco_amd.load_library(path)
    arrs = {}
    for name in sorted(CASES):
        for k, v in run_case(name, CASES[name], load_golden).items():
            arrs[name + '.' + k] = v
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(REPO, 'tests', 'golden', 'l1l1_parent_mdcpl.npz')
    np.savez_compressed(out, **arrs)
    print('%s: %d arrays, %.1f KB' % (out, len(arrs), os.path.getsize(out) / 1024.0))


if __name__ == '__main__':
    main()
