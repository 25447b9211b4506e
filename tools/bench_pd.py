#!/usr/bin/env python3
"""Cost of ConvProdDictBPDN beside ConvBPDN on a signal with as many channels as the product
dictionary's coefficient maps, both through the per-iteration host loop (256x256, K = 64, Cs = 3,
Cb = 6, N = 8, float32, default options, 10 warm-up + 50 timed iterations).  The two move the same
X-sized arrays.  Prints one JSON line per solver with it/s, the per-kernel milliseconds of the
library's event profile, the bytes pd_solve moves by construction -- one X-sized complex read and one
write -- and the resulting TB/s (DESIGN.md 4.7 gives 6.3 TB/s for a copy).

    python tools/bench_pd.py --out profiles/pd_bench.jsonl     # bpdn, pd
    python tools/bench_pd.py --only pd --steps 20               # e.g. under a kernel trace

(`_return_min = False` makes solve() return None instead of downloading the minimiser,
admm/admm.py, so the timed region holds no device-to-host copy of X.)
"""

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def run(which, size, K, Cs, Cb, N, warmup, steps, out=None, tag=None):
    import numpy as np
    os.environ['SPORCO_AMD_HOST_LOOP'] = '1'
    from sporco_amd.admm import cbpdn, pdcsc
    rng = np.random.RandomState(1)
    D = rng.randn(8, 8, K).astype(np.float32)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    B = rng.randn(Cs, Cb).astype(np.float32)
    B /= np.sqrt(np.sum(B ** 2, axis=0, keepdims=True))
    base = {'Verbose': False, 'RelStopTol': 0.0, 'MaxMainIter': warmup}
    if which == 'bpdn':
        S = rng.randn(size, size, Cb, N).astype(np.float32)
        b = cbpdn.ConvBPDN(D, S, 0.05, cbpdn.ConvBPDN.Options(base), dimK=1)
        # (the same staged host-driven loop as the product-dictionary class)
        b.xstep = lambda: type(b).xstep(b)
    else:
        S = rng.randn(size, size, Cs, N).astype(np.float32)
        b = pdcsc.ConvProdDictBPDN(D, B, S, 0.05, pdcsc.ConvProdDictBPDN.Options(base), dimK=1)
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
    res = {'solver': which, 'build': tag or 'this tree', 'size': size, 'K': K, 'Cs': Cs, 'Cb': Cb, 'N': N,
           'steps': steps, 'it_per_s': steps / dt, 'ms_per_it': 1e3 * dt / steps, 'kernel_ms_total': prof}
    if 'pd_solve' in prof:
        felems = size * (size // 2 + 1) * Cb * N * K
        sb = 2 * 8 * felems
        sm = prof['pd_solve'][0] / prof['pd_solve'][1]
        res.update(pd_solve_ms=sm, pd_solve_bytes=sb, pd_solve_tb_per_s=sb / (sm * 1e-3) / 1e12,
                   copy_tb_per_s=6.3, pd_solve_forms=list(b._solve_form_counts()))
    print(json.dumps(res), flush=True)
    if out:
        with open(out, 'a') as f:
            f.write(json.dumps(res) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['bpdn', 'pd'])
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--K', type=int, default=64)
    ap.add_argument('--Cs', type=int, default=3)
    ap.add_argument('--Cb', type=int, default=6)
    ap.add_argument('--N', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--out', help='append the JSON rows to this file as well')
    ap.add_argument('--lib', help='load this build of libsporco_amd.so instead of the in-tree one')
    ap.add_argument('--tag', help='name of the build in the rows')
    a = ap.parse_args()
    if a.lib:
        import sporco_amd
        sporco_amd.load_library(os.path.abspath(a.lib))
    for which in ([a.only] if a.only else ['bpdn', 'pd']):
        run(which, a.size, a.K, a.Cs, a.Cb, a.N, a.warmup, a.steps, a.out, a.tag)


if __name__ == '__main__':
    main()
