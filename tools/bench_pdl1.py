#!/usr/bin/env python3
"""Cost of ConvProdDictL1L1Grd beside ConvL1L1Grd on a signal with as many channels as the product
dictionary's coefficient maps, both through the same per-iteration host loop on the generic transforms
(256x256, K = 64, Cs = 3, Cb = 6, N = 8, float32, 10 warm-up + 50 timed iterations), with residuals
(the default) and without (FastSolve, AutoRho off).  The two move the same X-sized arrays.  Prints one
JSON line per run with it/s, the per-kernel milliseconds of the library's event profile, the bytes
pdl1_solve and pdl1_dual move by construction -- one X-sized complex read and one write, Df and the two
signal-sized spectra for the solve; one X-sized read, Df and one signal-sized spectrum for the dual
pass -- and the resulting TB/s (DESIGN.md 4.7 gives 6.3 TB/s for a copy).

    python tools/bench_pdl1.py --out profiles/pdl1_bench.jsonl
    python tools/bench_pdl1.py --only pdl1 --steps 20            # e.g. under a kernel trace

(`_return_min = False` makes solve() return None instead of downloading the minimiser.)
"""

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def run(which, resid, size, K, Cs, Cb, N, warmup, steps, out=None):
    import numpy as np
    from sporco_amd.admm import cbpdn, pdcsc
    rng = np.random.RandomState(1)
    D = rng.randn(8, 8, K).astype(np.float32)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    B = rng.randn(Cs, Cb).astype(np.float32)
    B /= np.sqrt(np.sum(B ** 2, axis=0, keepdims=True))
    base = {'Verbose': False, 'RelStopTol': 0.0, 'MaxMainIter': warmup, 'FastSolve': not resid}
    C = Cb if which == 'l1l1' else Cs
    S = (0.3 * rng.randn(size, size, C, N)).astype(np.float32)
    hit = rng.rand(size, size, C, N) < 0.25
    S[hit] = 4.0 * np.sign(rng.randn(int(hit.sum()))).astype(np.float32)
    if which == 'l1l1':
        b = cbpdn.ConvL1L1Grd(D, S, 0.6, 0.05, None, cbpdn.ConvL1L1Grd.Options(base), dimK=1)
    else:
        b = pdcsc.ConvProdDictL1L1Grd(D, B, S, 0.6, 0.05, None, pdcsc.ConvProdDictL1L1Grd.Options(base), dimK=1)
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
    res = {'solver': which, 'residuals': bool(resid), 'size': size, 'K': K, 'Cs': Cs, 'Cb': Cb, 'N': N, 'steps': steps,
           'it_per_s': steps / dt, 'ms_per_it': 1e3 * dt / steps, 'kernel_ms_total': prof}
    npix = size * (size // 2 + 1)
    if 'pdl1_solve' in prof:
        nbytes = 8 * (2 * npix * Cb * N * K + npix * K + 2 * npix * Cs * N)
        ms = prof['pdl1_solve'][0] / prof['pdl1_solve'][1]
        res.update(pdl1_solve_ms=ms, pdl1_solve_bytes=nbytes, pdl1_solve_tb_per_s=nbytes / (ms * 1e-3) / 1e12,
                   pdl1_solve_share_of_copy_rate=nbytes / (ms * 1e-3) / 6.3e12, copy_tb_per_s=6.3,
                   pdl1_solve_forms=list(b._solve_form_counts()))
    if 'pdl1_dual' in prof:
        nbytes = 8 * (npix * Cb * N * K + npix * K + npix * Cs * N)
        ms = prof['pdl1_dual'][0] / prof['pdl1_dual'][1]
        res.update(pdl1_dual_ms=ms, pdl1_dual_bytes=nbytes, pdl1_dual_tb_per_s=nbytes / (ms * 1e-3) / 1e12,
                   pdl1_dual_share_of_copy_rate=nbytes / (ms * 1e-3) / 6.3e12)
    print(json.dumps(res), flush=True)
    if out:
        with open(out, 'a') as f:
            f.write(json.dumps(res) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['l1l1', 'pdl1'])
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--K', type=int, default=64)
    ap.add_argument('--Cs', type=int, default=3)
    ap.add_argument('--Cb', type=int, default=6)
    ap.add_argument('--N', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--out', help='append the JSON rows to this file as well')
    a = ap.parse_args()
    for which in ([a.only] if a.only else ['l1l1', 'pdl1']):
        for resid in (True, False):
            run(which, resid, a.size, a.K, a.Cs, a.Cb, a.N, a.warmup, a.steps, a.out)


if __name__ == '__main__':
    main()
