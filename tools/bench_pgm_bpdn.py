#!/usr/bin/env python3
"""Iteration rates of pgm.bpdn.BPDN beside admm.bpdn.BPDN at the same shape, from one process, on one GPU.

    python tools/bench_pgm_bpdn.py [--iters 200] [--K 32768] [--out profiles/pgm_bpdn_bench.jsonl]

N = 64, M = 128 and 256, float32 and float64; pgm.bpdn with a fixed L, BacktrackStandard and BacktrackRobust
(FastSolve off: the per-iteration read is part of what is timed), admm.bpdn.BPDN with a fixed rho.  One run each after
a warm-up solve of 5 iterations; the per-kernel times are the handle's profile slots of a second, profiled run.
One JSON line per configuration.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sporco_amd.admm import bpdn as abpdn                                  # noqa: E402
from sporco_amd.pgm import bpdn as pbpdn                                   # noqa: E402
from sporco_amd.pgm.backtrack import BacktrackRobust, BacktrackStandard     # noqa: E402


def problem(N, M, K, dtype):
    rng = np.random.RandomState(1)
    D = rng.randn(N, M)
    D /= np.sqrt(np.sum(D ** 2, axis=0, keepdims=True))
    X = np.zeros((M, K))
    X[rng.randint(0, M, 4 * K), np.repeat(np.arange(K), 4)] = rng.randn(4 * K)
    S = D.dot(X) + 0.01 * rng.randn(N, K)
    return D.astype(dtype), S.astype(dtype)


def timed(make, iters):
    b = make(5)
    b.solve()
    b = make(iters)
    t0 = time.perf_counter()
    b.solve()
    dt = time.perf_counter() - t0
    p = make(iters)
    p._dev.profile(True)
    p.solve()
    prof = p._dev.profile_read()
    p._dev.profile(False)
    return dt, {k: {'ms_per_launch': v[0] / v[1], 'launches': v[1]} for k, v in prof.items()}, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--K', type=int, default=32768)
    ap.add_argument('--out', default=os.path.join('profiles', 'pgm_bpdn_bench.jsonl'))
    a = ap.parse_args()
    lines = []
    for dtype in (np.float32, np.float64):
        for M in (128, 256):
            N, K = 64, a.K
            D, S = problem(N, M, K, dtype)
            L = float(np.linalg.norm(D.astype(np.float64), 2) ** 2)
            lmbda = 0.05

            def admm(n):
                return abpdn.BPDN(D, S, lmbda, abpdn.BPDN.Options(
                    {'Verbose': False, 'MaxMainIter': n, 'RelStopTol': 0.0, 'AutoRho': {'Enabled': False}, 'rho': 1.0}))
            dt_a, prof_a, _ = timed(admm, a.iters)
            t_iter = prof_a.get('bpdn_iter', {}).get('ms_per_launch')
            for rule, bt, L0 in (('fixed_L', lambda: None, L), ('BacktrackStandard', BacktrackStandard, 0.5 * L),
                                 ('BacktrackRobust', BacktrackRobust, 0.5 * L)):
                def pgm(n):
                    return pbpdn.BPDN(D, S, lmbda, pbpdn.BPDN.Options(
                        {'Verbose': False, 'MaxMainIter': n, 'RelStopTol': 0.0, 'L': L0, 'Backtrack': bt()}))
                dt, prof, b = timed(pgm, a.iters)
                t_step = prof.get('bpdn_pgm_step', {}).get('ms_per_launch')
                its = b.getitstat()
                rec = {'N': N, 'M': M, 'K': K, 'dtype': np.dtype(dtype).name, 'rule': rule, 'iters': a.iters, 'runs': 1,
                       'pgm_it_per_s': a.iters / dt, 'admm_fixed_rho_it_per_s': a.iters / dt_a,
                       'pgm_kernels': prof, 'admm_kernels': prof_a,
                       'step_over_bpdn_iter': (t_step / t_iter) if t_step and t_iter else None,
                       'trials_per_iter': float(np.mean(its.IterBTrack)) if its.IterBTrack[0] is not None else 1.0,
                       'ObjFun_last': float(its.ObjFun[-1])}
                print(json.dumps(rec))
                lines.append(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
