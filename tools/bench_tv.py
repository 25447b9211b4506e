#!/usr/bin/env python3
"""Cost of the two TV kernels at the flagship size: ConvBPDNScalarTV and ConvBPDNVectorTV beside
ConvBPDNGradReg, all three through the per-iteration host loop in one process (512x512, K = 64,
N = 32, float32, 10 warm-up + 50 timed iterations).  Prints one JSON line per solver with it/s, the
per-kernel milliseconds of the library's event profile, the bytes the two kernels move by
construction and the resulting TB/s (DESIGN.md 4.7 gives 6.3 TB/s for a copy).

    python tools/bench_tv.py --out profiles/tv_bench.jsonl       # gradreg, scalar, vector
    python tools/bench_tv.py --only vector                       # one solver
    python tools/bench_tv.py --rocprof profiles/tv_rocprofv3_kernel_stats.csv

--rocprof measures nothing in this process: it starts `rocprofv3 --kernel-trace --stats` around a
fresh `bench_tv.py --only scalar` and `--only vector` child each (a run of their own, 20 timed
iterations) and writes the two kernel-stats tables, one after the other, to the given file.

(`_return_min = False` makes solve() return None instead of downloading the minimiser,
admm/admm.py, so the timed region holds no device-to-host copy of X.)
"""

import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def run(which, size, K, N, warmup, steps, out=None):
    import numpy as np
    os.environ['SPORCO_AMD_HOST_LOOP'] = '1'
    from sporco_amd.admm import cbpdn, cbpdntv
    rng = np.random.RandomState(1)
    D = rng.randn(8, 8, K).astype(np.float32)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(size, size, N).astype(np.float32)
    base = {'Verbose': False, 'RelStopTol': 0.0, 'MaxMainIter': warmup}
    if which == 'gradreg':
        b = cbpdn.ConvBPDNGradReg(D, S, 0.05, 0.02, cbpdn.ConvBPDNGradReg.Options(base), dimK=1)
        b._return_min = False
    else:
        cls = cbpdntv.ConvBPDNVectorTV if which == 'vector' else cbpdntv.ConvBPDNScalarTV
        base['ReturnX'] = False
        b = cls(D, S, 0.05, 0.02, cls.Options(base), dimK=1)
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
    if 'tv_ystep' in prof:
        # tv_ystep: reads X, 3 Y (RelaxParam != 1), 3 U, writes 3 Y, 3 U = 13 passes; the scalar
        # class's norm launch before it reads X, 3 Y, 3 U again = 7 more.  tv_adjoint: reads 3 Y,
        # 3 U, P, writes P, Q = 9 passes.
        yp = 13 + (7 if which == 'scalar' else 0)
        ym = prof['tv_ystep'][0] / prof['tv_ystep'][1]
        am = prof['tv_adjoint'][0] / prof['tv_adjoint'][1]
        res.update(tv_ystep_ms=ym, tv_adjoint_ms=am, tv_ystep_bytes=yp * 4 * elems,
                   tv_adjoint_bytes=9 * 4 * elems, tv_ystep_tb_per_s=yp * 4 * elems / (ym * 1e-3) / 1e12,
                   tv_adjoint_tb_per_s=9 * 4 * elems / (am * 1e-3) / 1e12, copy_tb_per_s=6.3)
    print(json.dumps(res), flush=True)
    if out:
        with open(out, 'a') as f:
            f.write(json.dumps(res) + '\n')


def rocprof(csv, size, K, N, warmup):
    """Kernel statistics of the two TV classes, each from a profiler run of its own."""
    with open(csv, 'w') as dst:
        for which in ('scalar', 'vector'):
            with tempfile.TemporaryDirectory() as d:
                subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '--',
                                sys.executable, os.path.abspath(__file__), '--only', which, '--size', str(size),
                                '--K', str(K), '--N', str(N), '--warmup', str(warmup), '--steps', '20'],
                               check=True, timeout=600)
                files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
                if len(files) != 1:
                    raise RuntimeError('expected one kernel_stats.csv from rocprofv3, found %r' % (files,))
                dst.write('# %s: %dx%d, K = %d, N = %d, float32, %d + 20 iterations\n'
                          % (which, size, size, K, N, warmup))
                dst.write(open(files[0]).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['gradreg', 'scalar', 'vector'])
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--K', type=int, default=64)
    ap.add_argument('--N', type=int, default=32)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--out', help='append the JSON rows to this file as well')
    ap.add_argument('--rocprof', metavar='CSV', help='write rocprofv3 kernel statistics here instead of timing')
    a = ap.parse_args()
    if a.rocprof:
        return rocprof(a.rocprof, a.size, a.K, a.N, a.warmup)
    for which in ([a.only] if a.only else ['gradreg', 'scalar', 'vector']):
        run(which, a.size, a.K, a.N, a.warmup, a.steps, a.out)


if __name__ == '__main__':
    main()
