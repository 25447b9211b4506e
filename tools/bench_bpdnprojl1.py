#!/usr/bin/env python3
"""Time admm.bpdn.BPDNProjL1 beside BPDN, and _lib.proj_l1_cols beside prox.proj_l1, float32 and float64, at

    N = 64, M = 128, K = 32768        and        N = 64, M = 256, K = 32768,

on the problem of tools/bench_bpdn.py (unit-norm Gaussian D, S = D X0 + noise with five non-zeros a column), 200
iterations, RelStopTol 0, AutoRho off (a fixed rho: the launches are compared, not the paths of rho), gamma = 1.0:
the l1 norm of a column of X0 is about 4, so almost every column lies outside its ball (`outside_share`: the share
of columns of the final Y on the ball).  Nothing here is a gate.

Per (shape, dtype) one JSON row `kind: solver`, from ONE process:
  proj_it_per_s / bpdn_it_per_s     host clock around solve() and a device synchronise, after a warm-up solve; one run
  proj_iter_ms / bpdn_iter_ms       milliseconds per `bpdn_iter` launch from the library's event profile in a second run
                                    of each class (projection mode, and BPDN's l1 shrinkage with lmbda = 0.1)
and per dtype one row `kind: routine` on a (256, 32768) array of normal deviates, gamma a tenth of the mean l1 norm of
a column:
  cols_ms / proj_l1_ms              host clock around one call of _lib.proj_l1_cols and of prox.proj_l1(v, gamma, axis=0)
                                    on the same array, after one warm-up call each; both include the copies of the host
                                    array in and out
  passes_mean / passes_max          passes over a column of the search, counted by the same iteration in NumPy float64
  max_abs_diff                      between the two results

    python tools/bench_bpdnprojl1.py --out profiles/bpdnprojl1_bench.jsonl
"""

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_bpdn as bb      # noqa: E402

GAMMA = 1.0


def make(cname, D, S, steps):
    from sporco_amd.admm import bpdn
    cls = getattr(bpdn, cname)
    opt = cls.Options(bb.options(steps, False))
    return cls(D, S, GAMMA if cname == 'BPDNProjL1' else bb.LMBDA, opt)


def passes(v, gamma):
    """Passes over each column of the shrinking-active-set search (the first sum included), in NumPy float64."""
    import numpy as np
    av = np.abs(np.asarray(v, dtype=np.float64))
    M, K = av.shape
    s = av.sum(axis=0)
    n = np.full(K, M)
    live = s > gamma
    tau = np.where(live, (s - gamma) / n, 0.0)
    count = np.ones(K, dtype=np.int64)
    while np.any(live):
        act = av > tau
        n2, s2 = act.sum(axis=0), (av * act).sum(axis=0)
        count += live
        done = (n2 == n) | (n2 == 0)
        upd = live & ~done
        tau = np.where(upd, (s2 - gamma) / np.maximum(n2, 1), tau)
        n = np.where(upd, n2, n)
        live = upd
    return count


def run_solver(N, M, K, dtype, steps, out, tag):
    import numpy as np
    D, S = bb.problem(N, M, K, dtype)
    row = {'kind': 'solver', 'N': N, 'M': M, 'K': K, 'dtype': np.dtype(dtype).name, 'steps': steps, 'runs': 1,
           'gamma': GAMMA, 'lmbda_bpdn': bb.LMBDA, 'auto_rho': False, 'commit': tag}
    for cname, key in (('BPDNProjL1', 'proj'), ('BPDN', 'bpdn')):
        make(cname, D, S, 3).solve()                        # warm-up: code objects, allocator
        b = make(cname, D, S, steps)
        secs, _, _ = bb.timed_solve(b)
        row[key + '_it_per_s'] = steps / secs
        row[key + '_objfun'] = float(b.itstat[-1].ObjFun)
        if cname == 'BPDNProjL1':
            pl = b._dev.plan()
            row.update(KB=pl['KB'], blocks=pl['blocks'], lds_bytes=pl['lds'], mfma=pl['mfma'])
            l1 = np.sum(np.abs(b.Y.astype(np.float64)), axis=0)
            row['outside_share'] = float(np.mean(l1 >= GAMMA * (1 - 1e-5)))
            row['cnstr_last'] = float(b.itstat[-1].Cnstr)
        row[key + '_iter_ms'] = bb.profiled(make(cname, D, S, steps)).get('bpdn_iter')
    row['iter_ms_ratio'] = row['proj_iter_ms'] / row['bpdn_iter_ms']
    emit(row, out)


def run_routine(M, K, dtype, out, tag):
    import numpy as np
    from sporco_amd import _lib, prox
    v = np.random.RandomState(2).randn(M, K).astype(dtype)
    gamma = float(0.1 * np.mean(np.sum(np.abs(v), axis=0)))
    res = {}
    row = {'kind': 'routine', 'M': M, 'K': K, 'dtype': np.dtype(dtype).name, 'gamma': gamma, 'runs': 1, 'commit': tag}
    for key, fn in (('cols_ms', lambda: _lib.proj_l1_cols(v, gamma)), ('proj_l1_ms', lambda: prox.proj_l1(v, gamma, axis=0))):
        fn()
        t = time.perf_counter()
        res[key] = fn()
        row[key] = 1e3 * (time.perf_counter() - t)
    row['ratio'] = row['cols_ms'] / row['proj_l1_ms']
    row['max_abs_diff'] = float(np.max(np.abs(res['cols_ms'].astype(np.float64) - res['proj_l1_ms'])))
    p = passes(v, gamma)
    row['passes_mean'], row['passes_max'] = float(np.mean(p)), int(np.max(p))
    emit(row, out)


def emit(row, out):
    print(json.dumps(row), flush=True)
    if out:
        with open(out, 'a') as fh:
            fh.write(json.dumps(row) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--K', type=int, default=32768)
    ap.add_argument('--out', help='append the JSON rows to this file as well')
    ap.add_argument('--commit', help='recorded in the rows where the tree is not a git checkout')
    a = ap.parse_args()
    import numpy as np
    import sporco_amd
    if sporco_amd.device_count() < 1:
        raise SystemExit("bench_bpdnprojl1 needs an AMD GPU")
    tag = bb.commit(a.commit)
    for M in (128, 256):
        for dtype in (np.float32, np.float64):
            run_solver(64, M, a.K, dtype, a.steps, a.out, tag)
    for dtype in (np.float32, np.float64):
        run_routine(256, a.K, dtype, a.out, tag)


if __name__ == '__main__':
    main()
