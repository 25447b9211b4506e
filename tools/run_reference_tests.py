#!/usr/bin/env python3
"""AUTHORING-CONTAINER TOOL (reads /root/reference; nothing under tests/ or on the GPU box uses
it): run the unmodified reference's OWN test files for the hot-path modules with
``sporco.admm.cbpdn`` etc. replaced by the modules of this package, on the CPU simulator build,
and report per test whether it passes.  A failure inside a class that SURVEY.md section 8 puts in
scope is a gap to close; classes outside it (ConvElasticNet, ConvTwoBlockCnstrnt, ...) are
expected to be missing.  A test that ends in this package's NotImplementedError is a refusal, not a gap:
in admm/test_tvl1.py and admm/test_tvl2.py those are the complex-valued cases, the three-axis volumes and (a
TypeError) the float16 case: 10 of 32; every other Denoise and Deconv test there passes against this package.

    python tools/run_reference_tests.py [pytest args]
"""
import importlib
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get('SPORCO_REFERENCE', '/root/reference')
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(REPO, 'oracle', '_stubs'))

ALIASES = {
    'sporco.admm.cbpdn': 'sporco_amd.admm.cbpdn',
    'sporco.admm.ccmod': 'sporco_amd.admm.ccmod',
    'sporco.admm.ccmodmd': 'sporco_amd.admm.ccmodmd',
    'sporco.pgm.cbpdn': 'sporco_amd.pgm.cbpdn',
    'sporco.pgm.ccmod': 'sporco_amd.pgm.ccmod',
    'sporco.dictlrn.cbpdndl': 'sporco_amd.dictlrn.cbpdndl',
    'sporco.dictlrn.cbpdndlmd': 'sporco_amd.dictlrn.cbpdndlmd',
    'sporco.dictlrn.onlinecdl': 'sporco_amd.dictlrn.onlinecdl',
    'sporco.pgm.backtrack': 'sporco_amd.pgm.backtrack',
    'sporco.pgm.stepsize': 'sporco_amd.pgm.stepsize',
    'sporco.pgm.momentum': 'sporco_amd.pgm.momentum',
    'sporco.admm.tvl1': 'sporco_amd.admm.tvl1',
    'sporco.admm.tvl2': 'sporco_amd.admm.tvl2',
    'sporco.admm.bpdn': 'sporco_amd.admm.bpdn',
    'sporco.admm.cmod': 'sporco_amd.admm.cmod',
    'sporco.dictlrn.bpdndl': 'sporco_amd.dictlrn.bpdndl',
    'sporco.pgm.bpdn': 'sporco_amd.pgm.bpdn',
}
FILES = ['admm/test_cbpdn.py', 'admm/test_ccmod.py', 'admm/test_ccmodmd.py', 'pgm/test_cbpdn.py',
         'pgm/test_ccmod.py', 'dictlrn/test_cbpdndl.py', 'dictlrn/test_cbpdndlmd.py',
         'dictlrn/test_onlinecdl.py', 'admm/test_tvl1.py', 'admm/test_tvl2.py', 'admm/test_bpdn.py',
         'admm/test_cmod.py', 'dictlrn/test_bpdndl.py', 'pgm/test_bpdn.py']


def main():
    import warnings
    warnings.filterwarnings('ignore')
    from conftest import use_backend
    use_backend('hostsim')
    import sporco  # noqa: F401  (the reference package: everything not aliased comes from it)
    try:
        import past.utils  # noqa: F401  (the reference's test_tvl1.py / test_tvl2.py import old_div from it)
    except ImportError:
        import numbers
        import types
        past, utils = types.ModuleType('past'), types.ModuleType('past.utils')
        utils.old_div = lambda a, b: a // b if isinstance(a, numbers.Integral) and isinstance(b, numbers.Integral) else a / b
        past.utils = utils
        sys.modules['past'], sys.modules['past.utils'] = past, utils
    if any(a.endswith('test_prox.py') for a in sys.argv[1:]):
        # (the reference's tests/test_prox.py against this package's prox module: what it lacks fails)
        ALIASES['sporco.prox'] = 'sporco_amd.prox'
    for ref_name, our_name in ALIASES.items():
        mod = importlib.import_module(our_name)
        importlib.import_module(ref_name.rsplit('.', 1)[0])
        sys.modules[ref_name] = mod
        setattr(sys.modules[ref_name.rsplit('.', 1)[0]], ref_name.rsplit('.', 1)[1], mod)
    import pytest
    args = [os.path.join(REF, 'tests', f) for f in FILES] if not any(a.endswith('.py') or '::' in a for a in sys.argv[1:]) else []
    return pytest.main(['-q', '-p', 'no:cacheprovider', '--rootdir', '/tmp/reftests',
                        '-o', 'python_files=test_*.py', '--tb=line', '-n', '0', '--timeout', '300'] + args +
                       list(sys.argv[1:]))


if __name__ == '__main__':
    sys.exit(main())
