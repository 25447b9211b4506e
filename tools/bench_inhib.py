#!/usr/bin/env python3
"""Cost of the inhibition update at the flagship size: ConvBPDNInhib beside plain ConvBPDN with an
array L1Weight, both through the per-iteration host loop (512x512, K = 64, N = 32, float32, paired
groups, Whn = 9, 20 warm-up + 100 timed iterations).  Prints one JSON line per solver.

    python tools/bench_inhib.py                      # both solvers, each in a child process
    python tools/bench_inhib.py --only inhib         # one solver in this process (for a profiler)

Each child runs under its own time limit and a failure ends the script.
"""

import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (SPORCO_AMD_TREE: a checkout of another commit whose package is measured instead -- the plain
# ConvBPDN baseline of the parent commit)
sys.path.insert(0, os.environ.get('SPORCO_AMD_TREE', REPO))


def run(which, size, K, N, warmup, steps):
    import numpy as np
    os.environ['SPORCO_AMD_HOST_LOOP'] = '1'
    from sporco_amd.admm import cbpdn
    rng = np.random.RandomState(1)
    D = rng.randn(8, 8, K).astype(np.float32)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(size, size, N).astype(np.float32)
    base = {'Verbose': False, 'RelStopTol': 0.0, 'MaxMainIter': warmup}
    if which == 'inhib':
        from sporco_amd.admm import cbpdnin
        Wg = np.append(np.eye(K // 2), np.eye(K // 2), axis=-1)
        b = cbpdnin.ConvBPDNInhib(D, S, Wg=Wg, Whn=9, lmbda=0.05, mu=0.5, gamma=0.02,
                                  opt=cbpdnin.ConvBPDNInhib.Options(base), dimK=1)
    else:
        base['L1Weight'] = (0.5 + rng.rand(size, size, 1, N, K)).astype(np.float32)
        b = cbpdn.ConvBPDN(D, S, 0.05, cbpdn.ConvBPDN.Options(base), dimK=1)
    b._return_min = False
    b.solve()
    b._dev.sync()
    b.opt['MaxMainIter'] = steps
    b.profile(True)
    t0 = time.perf_counter()
    b.solve()
    b._dev.sync()
    dt = time.perf_counter() - t0
    prof = {k: [round(v[0], 3), v[1]] for k, v in b.profile_read().items() if v[1]}
    elems = size * size * N * K
    res = {'solver': which, 'size': size, 'K': K, 'N': N, 'steps': steps, 'it_per_s': steps / dt,
           'ms_per_it': 1e3 * dt / steps, 'kernel_ms_total': prof}
    if 'inhib_update' in prof:
        ms = prof['inhib_update'][0] / prof['inhib_update'][1]
        nbytes = 7 * 4 * elems      # reads X, Y, wml, wms; writes wml, wms, T
        res.update(inhib_update_ms=ms, inhib_bytes_by_construction=nbytes,
                   inhib_tb_per_s=nbytes / (ms * 1e-3) / 1e12)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['inhib', 'plain'])
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--K', type=int, default=64)
    ap.add_argument('--N', type=int, default=32)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--timeout', type=int, default=240)
    a = ap.parse_args()
    if a.only:
        run(a.only, a.size, a.K, a.N, a.warmup, a.steps)
        return
    for which in ('plain', 'inhib'):
        cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--only', which,
               '--size', str(a.size), '--K', str(a.K), '--N', str(a.N), '--warmup', str(a.warmup),
               '--steps', str(a.steps)]
        rc = subprocess.call(cmd)
        if rc != 0:
            sys.exit('bench_inhib: %s ended with status %d; stopping' % (which, rc))


if __name__ == '__main__':
    main()
