#!/usr/bin/env python3
"""Cost of ConvBPDNRecTV at the flagship size beside ConvBPDN, both through the per-iteration host
loop (512x512, K = 64, N = 32, float32, scalar TVWeight, default options, 10 warm-up + 50 timed
iterations).  Prints one JSON line per solver with it/s, the per-kernel milliseconds of the
library's event profile, the bytes rtv_solve and rtv_ystep move by construction and the resulting
TB/s (DESIGN.md 4.7 gives 6.3 TB/s for a copy).

    python tools/bench_rtv.py --out profiles/rtv_bench.jsonl     # bpdn, rectv
    python tools/bench_rtv.py --only bpdn --lib /path/to/libsporco_amd.so --tag parent

--lib loads another build of the library (the yardstick row of ConvBPDN is measured with the
parent commit's build); --tag names the build in the row.

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


def run(which, size, K, N, warmup, steps, out=None, tag=None):
    import numpy as np
    os.environ['SPORCO_AMD_HOST_LOOP'] = '1'
    from sporco_amd.admm import cbpdn, cbpdntv
    rng = np.random.RandomState(1)
    D = rng.randn(8, 8, K).astype(np.float32)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(size, size, N).astype(np.float32)
    base = {'Verbose': False, 'RelStopTol': 0.0, 'MaxMainIter': warmup}
    if which == 'bpdn':
        b = cbpdn.ConvBPDN(D, S, 0.05, cbpdn.ConvBPDN.Options(base), dimK=1)
    else:
        b = cbpdntv.ConvBPDNRecTV(D, S, 0.05, 0.02, cbpdntv.ConvBPDNRecTV.Options(base), dimK=1)
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
    res = {'solver': which, 'build': tag or 'this tree', 'size': size, 'K': K, 'N': N, 'steps': steps,
           'it_per_s': steps / dt, 'ms_per_it': 1e3 * dt / steps, 'kernel_ms_total': prof}
    if 'rtv_ystep' in prof:
        # rtv_ystep: reads X, y0 (RelaxParam != 1), u0, writes y0, u0 = 5 passes over a K-map array,
        # plus the signal-shaped ones (rw three times, y1 / u1 read twice and written once: 9 maps of
        # 1 / K the size).  rtv_solve: reads rfftn(y0), rfftn(u0), writes Xf = 3 passes over a K-map
        # half spectrum, plus Df and five signal-shaped spectra.
        elems = size * size * N * K
        felems = size * (size // 2 + 1) * N * K
        yb = 5 * 4 * elems + 9 * 4 * elems // K
        sb = 3 * 8 * felems + 8 * felems // N + 5 * 8 * felems // K
        ym = prof['rtv_ystep'][0] / prof['rtv_ystep'][1]
        sm = prof['rtv_solve'][0] / prof['rtv_solve'][1]
        res.update(rtv_ystep_ms=ym, rtv_solve_ms=sm, rtv_ystep_bytes=yb, rtv_solve_bytes=sb,
                   rtv_ystep_tb_per_s=yb / (ym * 1e-3) / 1e12, rtv_solve_tb_per_s=sb / (sm * 1e-3) / 1e12,
                   copy_tb_per_s=6.3)
    print(json.dumps(res), flush=True)
    if out:
        with open(out, 'a') as f:
            f.write(json.dumps(res) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['bpdn', 'rectv'])
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--K', type=int, default=64)
    ap.add_argument('--N', type=int, default=32)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--out', help='append the JSON rows to this file as well')
    ap.add_argument('--lib', help='load this build of libsporco_amd.so instead of the in-tree one')
    ap.add_argument('--tag', help='name of the build in the rows')
    a = ap.parse_args()
    if a.lib:
        import sporco_amd
        sporco_amd.load_library(os.path.abspath(a.lib))
    for which in ([a.only] if a.only else ['bpdn', 'rectv']):
        run(which, a.size, a.K, a.N, a.warmup, a.steps, a.out, a.tag)


if __name__ == '__main__':
    main()
