#!/usr/bin/env python3
"""Cost of ConvMinL1InL2Ball beside ConvBPDNMaskDcpl, both through the same per-iteration host loop
(512x512, K = 64, N = 8, float32, 5 warm-up + 30 timed iterations, residuals on, AutoRho off so that
the two run the same launches every iteration), on the register-resident kernels and forced onto the
generic chain (SPORCO_AMD_MD_GENERIC, read when a handle is made).  ConvBPDNMaskDcpl is unchanged code:
the yardstick.  The two differ by block 0: md_y0step (one pass, five arrays moved) against ball_norms +
ball_totals + ball_y0step (two passes).  Prints one JSON line per run with it/s, the per-kernel
milliseconds of the library's event profile, the bytes the two new kernels move by construction and
the resulting TB/s (DESIGN.md 4.7 gives 6.3 TB/s for a copy).

    python tools/bench_ball.py --out profiles/ball_bench.jsonl

(`_return_min = False` makes solve() return None instead of downloading the minimiser.)
"""

import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def commit():
    try:
        return subprocess.check_output(['git', '-C', REPO, 'rev-parse', '--short', 'HEAD'], text=True,
                                       stderr=subprocess.DEVNULL).strip()
    except Exception:
        return None


def run(which, generic, size, K, N, warmup, steps, out=None):
    import numpy as np
    from sporco_amd.admm import cbpdn
    if generic:
        os.environ['SPORCO_AMD_MD_GENERIC'] = '1'
    else:
        os.environ.pop('SPORCO_AMD_MD_GENERIC', None)
    rng = np.random.RandomState(1)
    D = rng.randn(8, 8, K).astype(np.float32)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    # images scaled alternately 0.2 / 1.0, the radius between their norms: both branches of the projection
    S = (rng.randn(size, size, N) * np.where(np.arange(N) % 2 == 0, 0.2, 1.0)).astype(np.float32)
    eps = 0.25 * size
    base = {'Verbose': False, 'RelStopTol': 0.0, 'MaxMainIter': warmup, 'AutoRho': {'Enabled': False}}
    if which == 'ball':
        b = cbpdn.ConvMinL1InL2Ball(D, S, eps, cbpdn.ConvMinL1InL2Ball.Options(base), dimK=1)
    else:
        b = cbpdn.ConvBPDNMaskDcpl(D, S, 0.1, None, cbpdn.ConvBPDNMaskDcpl.Options(base), dimK=1)
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
    res = {'solver': which, 'path': 'generic' if generic else 'fused', 'size': size, 'K': K, 'N': N, 'steps': steps,
           'it_per_s': steps / dt, 'ms_per_it': 1e3 * dt / steps, 'kernel_ms_total': prof, 'commit': commit()}
    ns = 4 * size * size * N                       # bytes of one signal-sized float32 array
    relaxed = float(b.rlx) != 1.0
    for name, arrays in (('ball_norms', 3 + relaxed), ('ball_y0step', 3 + relaxed + 2)):
        if name in prof:
            ms = prof[name][0] / prof[name][1]
            res.update({name + '_ms': ms, name + '_bytes': arrays * ns,
                        name + '_tb_per_s': arrays * ns / (ms * 1e-3) / 1e12})
    if 'ball_norms' in prof:
        res['copy_tb_per_s'] = 6.3
    print(json.dumps(res), flush=True)
    if out:
        with open(out, 'a') as f:
            f.write(json.dumps(res) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['ball', 'mdcpl'])
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--K', type=int, default=64)
    ap.add_argument('--N', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--out', help='append the JSON rows to this file as well')
    a = ap.parse_args()
    for generic in (False, True):
        for which in ([a.only] if a.only else ['mdcpl', 'ball']):
            run(which, generic, a.size, a.K, a.N, a.warmup, a.steps, a.out)


if __name__ == '__main__':
    main()
