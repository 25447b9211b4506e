#!/usr/bin/env python3
"""Time dictlrn.wbpdndl.WeightedBPDNDictLearn on a patch-sized problem with 30 % of the samples masked out,

    N = 64, K = 32768, M = 128 or 256, float32 or float64,

the problem of tools/bench_bpdndl.py (Gaussian D0, S = D X0 + noise, lmbda = 0.1) with W a 0 / 1 mask, inner L = 2 M
(x step) and 2 ||X0 X0^T|| (D step), 50 outer iterations.  Nothing here is a gate.

One (M, dtype) a process, one JSON row, everything in it from that process:
  outer_it_per_s        host clock around solve() and a device synchronise of both handles, after a warm-up learner of
                        the same shape; one run, not averaged (`runs`: 1)
  kernels_ms / launches milliseconds per launch of every kernel of the two handles from their event profiles in a
                        second run: cmod_pgm_grad, cmod_pgm_reduce, cmod_pgm_prox, cmod_pgm_dfid, bpdn_pgm_step, ...
  grad_over_step        cmod_pgm_grad / bpdn_pgm_step per launch, beside `multiplies_ratio` = 2 N M / 3 N M
  grad_bytes, us_at_copy_rate   of one cmod_pgm_grad BY CONSTRUCTION: Z, S and W once each (`grad_bytes_min`), Z staged
                        once a block of 32 rows (`grad_bytes_requested`), the slab partials written and read; the
                        microseconds the minimum takes at the measured copy rate of 6.3 TB/s
  bpdndl                dictlrn.bpdndl.BPDNDictLearn on the unmasked problem of tools/bench_bpdndl.py at the same
                        shape: outer_it_per_s and its kernels per launch

Each GPU step under a limit of its own, a failure ends the chain:

    timeout -k 10 300 python tools/bench_wbpdndl.py --M 128 --dtype float32 --out profiles/wbpdndl_bench.jsonl && \\
    timeout -k 10 300 python tools/bench_wbpdndl.py --M 128 --dtype float64 --out profiles/wbpdndl_bench.jsonl && \\
    timeout -k 10 300 python tools/bench_wbpdndl.py --M 256 --dtype float32 --out profiles/wbpdndl_bench.jsonl && \\
    timeout -k 10 300 python tools/bench_wbpdndl.py --M 256 --dtype float64 --out profiles/wbpdndl_bench.jsonl
"""

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_bpdndl as bb       # noqa: E402

COPY_TB_S = 6.3
N = 64


def make(D0, S, W, Lx, Ld, steps):
    from sporco_amd.dictlrn import wbpdndl
    o = {'Verbose': False, 'MaxMainIter': steps, 'BPDN': {'L': Lx}, 'CMOD': {'L': Ld}}
    return wbpdndl.WeightedBPDNDictLearn(D0, S, bb.LMBDA, W=W, opt=wbpdndl.WeightedBPDNDictLearn.Options(o))


def timed(d, steps):
    t = time.perf_counter()
    d.solve()
    bb.sync(d)
    return steps / (time.perf_counter() - t)


def run(M, K, dtype, steps, out, tag):
    import numpy as np
    D0, S = bb.problem(N, M, K, dtype)
    e = np.dtype(dtype).itemsize
    W = (np.random.RandomState(2).rand(N, K) >= 0.3).astype(dtype)
    Lx = 2.0 * M
    # five unit-variance non-zeros a column: ||X0 X0^T|| is about 5 K / M; doubled
    Ld = 2.0 * 5.0 * K / M
    make(D0, S, W, Lx, Ld, 3).solve()                     # warm-up: code objects, allocator
    d = make(D0, S, W, Lx, Ld, steps)
    pl = d.dstep._dev.plan()
    rate = timed(d, steps)
    row = {'N': N, 'M': M, 'K': K, 'dtype': np.dtype(dtype).name, 'steps': steps, 'runs': 1, 'mask_share': 0.3,
           'outer_it_per_s': rate, 'ms_per_outer_it': 1e3 / rate, 'slab': pl['slab'], 'slabs': pl['slabs'],
           'row_blocks': pl['row_blocks'], 'mfma': pl['mfma'], 'objfun': float(d.itstat[-1].ObjFun), 'commit': tag}
    prof = bb.profiled(make(D0, S, W, Lx, Ld, steps))
    row['kernels_ms'] = {k: v[0] for k, v in sorted(prof.items())}
    row['launches'] = {k: v[1] for k, v in sorted(prof.items())}
    row['device_ms_per_outer_it'] = sum(ms * n for ms, n in prof.values()) / steps
    row['grad_over_step'] = prof['cmod_pgm_grad'][0] / prof['bpdn_pgm_step'][0]
    row['multiplies_ratio'] = 2.0 / 3.0
    row['grad_bytes_min'] = (M + 2 * N) * K * e
    row['grad_bytes_requested'] = (pl['row_blocks'] * M + 2 * N) * K * e
    row['grad_bytes_partials'] = 2 * pl['slabs'] * ((M + 15) // 16 * 16) * ((N + 15) // 16 * 16) * e
    row['us_at_copy_rate'] = 1e6 * row['grad_bytes_min'] / (COPY_TB_S * 1e12)
    row['copy_tb_per_s'] = COPY_TB_S
    bb.make(D0, S, 3).solve()
    b = bb.make(D0, S, steps)
    brate = timed(b, steps)
    bprof = bb.profiled(bb.make(D0, S, steps))
    row['bpdndl'] = {'outer_it_per_s': brate, 'kernels_ms': {k: v[0] for k, v in sorted(bprof.items())}}
    print(json.dumps(row), flush=True)
    if out:
        with open(out, 'a') as fh:
            fh.write(json.dumps(row) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--M', type=int, choices=(128, 256), help='one dictionary size (default: both, one after the other)')
    ap.add_argument('--dtype', choices=('float32', 'float64'), help='one precision (default: both)')
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--K', type=int, default=32768)
    ap.add_argument('--out', help='append the JSON rows to this file as well')
    ap.add_argument('--commit', help='recorded in the rows where the tree is not a git checkout')
    a = ap.parse_args()
    import numpy as np
    import sporco_amd
    if sporco_amd.device_count() < 1:
        raise SystemExit("bench_wbpdndl needs an AMD GPU")
    tag = bb.commit(a.commit)
    for M in ((a.M,) if a.M else (128, 256)):
        for dt in ((a.dtype,) if a.dtype else ('float32', 'float64')):
            run(M, a.K, np.dtype(dt).type, a.steps, a.out, tag)


if __name__ == '__main__':
    main()
