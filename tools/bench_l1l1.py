#!/usr/bin/env python3
"""Cost of ConvL1L1Grd beside ConvBPDNMaskDcpl, both on the generic transforms and through the same
per-iteration host loop (512x512, K = 64, N = 8, float32, 5 warm-up + 30 timed iterations), with
residuals (the default) and without (FastSolve, AutoRho off).  ConvBPDNMaskDcpl is forced onto its
generic path by the handle's switch SPORCO_AMD_MD_GENERIC, so the two differ by what this class adds:
the gradient diagonal in the solve, the block-0 soft threshold, the Yprev - Y outputs and the dual
residual of two X-sized transforms more.  Prints one JSON line per run with it/s, the per-kernel
milliseconds of the library's event profile, the bytes l1l1_dual reads by construction -- two X-sized
spectra, Df and the two signal-sized spectra -- and the resulting TB/s (DESIGN.md 4.7 gives 6.3 TB/s
for a copy).

    python tools/bench_l1l1.py --out profiles/l1l1_bench.jsonl
    python tools/bench_l1l1.py --only l1l1 --steps 10            # e.g. under a kernel trace

(`_return_min = False` makes solve() return None instead of downloading the minimiser.)
"""

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ['SPORCO_AMD_MD_GENERIC'] = '1'       # read when a handle is made


def run(which, resid, size, K, N, warmup, steps, out=None):
    import numpy as np
    from sporco_amd.admm import cbpdn
    rng = np.random.RandomState(1)
    D = rng.randn(8, 8, K).astype(np.float32)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = (0.3 * rng.randn(size, size, N)).astype(np.float32)
    hit = rng.rand(size, size, N) < 0.25
    S[hit] = 4.0 * np.sign(rng.randn(int(hit.sum()))).astype(np.float32)
    base = {'Verbose': False, 'RelStopTol': 0.0, 'MaxMainIter': warmup, 'FastSolve': not resid}
    if which == 'l1l1':
        b = cbpdn.ConvL1L1Grd(D, S, 0.6, 0.05, None, cbpdn.ConvL1L1Grd.Options(base), dimK=1)
    else:
        b = cbpdn.ConvBPDNMaskDcpl(D, S, 0.6, None, cbpdn.ConvBPDNMaskDcpl.Options(base), dimK=1)
    assert b._needs_residuals() == resid
    b._return_min = False
    b.solve()
    b._dev.sync()
    b.opt['MaxMainIter'] = steps
    b._dev.profile(True)
    t0 = time.perf_counter()
    b.solve()
    b._dev.sync()
    dt = time.perf_counter() - t0
    prof = {k: [round(v[0], 3), v[1]] for k, v in b._dev.profile_read().items() if v[1]}
    res = {'solver': which, 'residuals': bool(resid), 'size': size, 'K': K, 'N': N, 'steps': steps,
           'it_per_s': steps / dt, 'ms_per_it': 1e3 * dt / steps, 'kernel_ms_total': prof}
    if 'l1l1_dual' in prof:
        npix = size * (size // 2 + 1)
        nbytes = 8 * (2 * npix * N * K + npix * K + 2 * npix * N)
        ms = prof['l1l1_dual'][0] / prof['l1l1_dual'][1]
        res.update(l1l1_dual_ms=ms, l1l1_dual_bytes=nbytes, l1l1_dual_tb_per_s=nbytes / (ms * 1e-3) / 1e12,
                   copy_tb_per_s=6.3, l1l1_dual_ms_at_copy_rate=nbytes / 6.3e12 * 1e3)
    print(json.dumps(res), flush=True)
    if out:
        with open(out, 'a') as f:
            f.write(json.dumps(res) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['l1l1', 'mdcpl'])
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--K', type=int, default=64)
    ap.add_argument('--N', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--out', help='append the JSON rows to this file as well')
    a = ap.parse_args()
    for which in ([a.only] if a.only else ['mdcpl', 'l1l1']):
        for resid in (True, False):
            run(which, resid, a.size, a.K, a.N, a.warmup, a.steps, a.out)


if __name__ == '__main__':
    main()
