#!/usr/bin/env python3
"""Cost of ConvBPDNProjL1 beside ConvBPDN (512x512, K = 64, N = 32, float32, 5 warm-up + 30 timed
iterations, default options).  ConvBPDN is unchanged code, the yardstick; it runs twice, through the
device-driven loop it takes by default and through the per-iteration host loop (a callback that does
nothing), which is the loop ConvBPDNProjL1 uses.  Prints one JSON line per run with it/s and the
per-kernel milliseconds of the library's event profile; for ConvBPDNProjL1 also the search passes per
iteration (y step, constraint measure) and the duration of the FIRST search pass of the y step, which the
library times in a slot of its own (projl1_pass0): it runs on every image and reads x, y and u whole, a
known number of bytes.  Beside it, on the same handle and the same three arrays, the existing streaming
kernel admm_relax (AX = rlx X + (1 - rlx) Y: two arrays read, one written -- the same bytes), timed through
the profile's `other` slot.  The later passes (slot projl1_search) run on the images still searching only,
so no bandwidth is derived from them.

    python tools/bench_projl1.py --out profiles/projl1_bench.jsonl

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


COMMIT = None      # --commit: where the tree is not a git checkout


def commit():
    if COMMIT:
        return COMMIT
    try:
        return subprocess.check_output(['git', '-C', REPO, 'rev-parse', '--short', 'HEAD'], text=True,
                                       stderr=subprocess.DEVNULL).strip()
    except Exception:
        return None


def run(which, size, K, N, warmup, steps, fast, out=None):
    import numpy as np
    from sporco_amd.admm import cbpdn
    rng = np.random.RandomState(1)
    D = rng.randn(8, 8, K).astype(np.float32)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    # images scaled alternately 0.02 / 1.0: both branches of the projection
    S = (rng.randn(size, size, N) * np.where(np.arange(N) % 2 == 0, 0.02, 1.0)).astype(np.float32)
    gamma = 0.02 * size * size
    passes = []
    base = {'Verbose': False, 'RelStopTol': 0.0, 'MaxMainIter': warmup, 'FastSolve': fast}
    if which == 'projl1':
        base['Callback'] = lambda b: passes.append(b.search_passes) and False
        b = cbpdn.ConvBPDNProjL1(D, S, gamma, cbpdn.ConvBPDNProjL1.Options(base), dimK=1)
    else:
        if which == 'cbpdn_host_loop':
            base['Callback'] = lambda b: False
        b = cbpdn.ConvBPDN(D, S, 0.05, cbpdn.ConvBPDN.Options(base), dimK=1)
    b._return_min = False
    b.solve()
    b._dev.sync()
    del passes[:]
    b.opt['MaxMainIter'] = steps
    b._dev.profile(True)
    t0 = time.perf_counter()
    b.solve()
    b._dev.sync()
    dt = time.perf_counter() - t0
    prof = {k: [round(v[0], 3), v[1]] for k, v in b._dev.profile_read().items() if v[1]}
    res = {'solver': which, 'size': size, 'K': K, 'N': N, 'steps': steps, 'fast_solve': fast,
           'it_per_s': steps / dt, 'ms_per_it': 1e3 * dt / steps, 'kernel_ms_total': prof, 'commit': commit()}
    if which == 'projl1':
        py = [p[0] for p in passes]
        pc = [p[1] for p in passes]
        res.update(passes_ystep_mean=float(np.mean(py)), passes_ystep_max=int(max(py)),
                   passes_cnstr_mean=float(np.mean(pc)), passes_cnstr_max=int(max(pc)),
                   projected_images=int(np.sum(np.sum(np.abs(b.Y), axis=(0, 1, 2, 4)) > gamma * (1 - 1e-4))))
        e = 4 * size * size * N * K            # bytes of one coefficient-sized float32 array
        if 'projl1_pass0' in prof:
            ms = prof['projl1_pass0'][0] / prof['projl1_pass0'][1]
            nbytes = (3 if float(b.rlx) != 1.0 else 2) * e
            res.update(first_pass_ms=ms, first_pass_bytes=nbytes, first_pass_tb_per_s=nbytes / (ms * 1e-3) / 1e12)
        if 'projl1_apply' in prof:
            ms = prof['projl1_apply'][0] / prof['projl1_apply'][1]
            res.update(apply_pass_ms=ms, apply_pass_bytes=5 * e, apply_pass_tb_per_s=5 * e / (ms * 1e-3) / 1e12)
        # the yardstick: an existing streaming kernel on the same three arrays
        b._dev.profile_read()
        for _ in range(10):
            b._dev.admm_relax(float(b.rlx))
        b._dev.sync()
        oth = b._dev.profile_read().get('other')
        if oth and oth[1]:
            ms = oth[0] / oth[1]
            res.update(relax_ms=ms, relax_bytes=3 * e, relax_tb_per_s=3 * e / (ms * 1e-3) / 1e12)
    print(json.dumps(res), flush=True)
    if out:
        with open(out, 'a') as f:
            f.write(json.dumps(res) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', choices=['projl1', 'cbpdn', 'cbpdn_host_loop'])
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--K', type=int, default=64)
    ap.add_argument('--N', type=int, default=32)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--out', help='append the JSON rows to this file as well')
    ap.add_argument('--commit', help='recorded in the rows where the tree is not a git checkout')
    a = ap.parse_args()
    global COMMIT
    COMMIT = a.commit
    for which in ([a.only] if a.only else ['cbpdn', 'cbpdn_host_loop', 'projl1']):
        for fast in ((False, True) if which == 'projl1' else (False,)):
            run(which, a.size, a.K, a.N, a.warmup, a.steps, fast, a.out)


if __name__ == '__main__':
    main()
