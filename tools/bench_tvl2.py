#!/usr/bin/env python3
"""Time the masked examples' pre-processing call, TVL2Denoise with a DFidWeight mask, AutoRho on,
gEvalY False, 200 iterations, float32, device arrays in and out, at

    512 x 512 (P = 1),   768 x 512 x 3 (caxis=2),   512 x 512 x 8.

Per shape one JSON row: it/s of an unprofiled run (host clock around solve() and a device synchronise,
after a warm-up solve of the same shape), then -- from a second, profiled run -- the milliseconds per launch
of each kernel (the library's event profile), the bytes each launch moves BY CONSTRUCTION (every array it
reads or writes once, halo rows not counted) and the TB/s that makes, beside the 6.3 TB/s copy rate the
project measures against.  Arrays per launch, e = H W P * 4 bytes:
    tvd_sweep    reads X, PD, S, Wdf, writes X                                 5 e   (6 e in the iterations
                 after rho moved: Q is read too; counted as 5)
    tvd_ystep    reads X, PD, S, Wdf, Y (2), U (2), writes Y (2), U (2), dY (2)  14 e
    tvd_adjoint  reads Y (2), U (2), dY (2), writes PD, Q                        8 e
The launch count per iteration is 4 (+ one launch that reduces the partial sums and one 128-byte read).
The reference's own time for the largest shape is recorded with each row as `reference_cpu`: the unmodified
reference took 1.3 s per iteration at 512 x 512 x 8 in float64 on the authoring machine's CPU (one run of
10 iterations; the only timing there is).

    python tools/bench_tvl2.py --out profiles/tvl2_bench.jsonl
"""

import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COPY_TB_S = 6.3
ARRAYS = {'tvd_sweep': 5, 'tvd_ystep': 14, 'tvd_adjoint': 8}
REFERENCE_CPU = {'shape': [512, 512, 8], 'dtype': 'float64', 's_per_it': 1.3, 'iterations': 10,
                 'host': 'authoring machine CPU, unmodified reference, one run'}
COMMIT = None


def commit():
    if COMMIT:
        return COMMIT
    try:
        return subprocess.check_output(['git', '-C', REPO, 'rev-parse', '--short', 'HEAD'], text=True,
                                       stderr=subprocess.DEVNULL).strip()
    except Exception:
        return None


def run(shape, caxis, steps, out=None):
    import numpy as np
    import sporco_amd
    from sporco_amd.admm import tvl2
    from sporco_amd.device import DeviceArray
    if sporco_amd.device_count() < 1:
        raise SystemExit("bench_tvl2 needs an AMD GPU")
    rng = np.random.RandomState(1)
    H, W = shape[:2]
    img = np.ones((H, W))
    img[:, W // 2:] = -1.0
    img[H // 3:] *= 0.5
    S = (img.reshape((H, W) + (1,) * (len(shape) - 2)) + 0.1 * rng.randn(*shape)).astype(np.float32)
    msk = (rng.rand(*shape) < 0.7).astype(np.float32)
    imgwp, mskp = DeviceArray.from_host(S), DeviceArray.from_host(msk)
    lmbda = 0.3 if caxis is not None else 0.1

    def make():
        opt = tvl2.TVL2Denoise.Options({'Verbose': False, 'MaxMainIter': steps, 'DFidWeight': mskp, 'gEvalY': False,
                                        'AutoRho': {'Enabled': True}, 'RelStopTol': 0.0})
        return tvl2.TVL2Denoise(imgwp, lmbda, opt, caxis=caxis)

    make().solve()                 # warm-up: code objects, allocator
    b = make()
    b._dev.sync()
    t0 = time.perf_counter()
    sl = b.solve()
    b._dev.sync()
    dt = time.perf_counter() - t0
    sh = mskp * (imgwp - sl)
    res = {'solver': 'tvl2', 'shape': list(shape), 'caxis': caxis, 'dtype': 'float32', 'steps': steps,
           'it_per_s': steps / dt, 'ms_per_it': 1e3 * dt / steps, 'plan': b._dev.plan(),
           'ObjFun_last': float(b.itstat[-1].ObjFun), 'rho_last': float(b.rho),
           'sh_abs_mean': float(np.mean(np.abs(sh.get()))), 'launches_per_it': 4, 'copy_tb_per_s': COPY_TB_S,
           'reference_cpu': REFERENCE_CPU, 'commit': commit()}
    # per-kernel times: a run of its own, with the event profile on
    b = make()
    b._dev.profile(True)
    b.solve()
    b._dev.sync()
    e = 4 * int(np.prod(shape))
    kern = {}
    for name, (ms, cnt) in b._dev.profile_read().items():
        row = {'launches': cnt, 'ms_per_launch': ms / cnt}
        if name in ARRAYS:
            row['bytes_per_launch'] = ARRAYS[name] * e
            row['tb_per_s'] = ARRAYS[name] * e / (ms / cnt * 1e-3) / 1e12
        kern[name] = row
    res['kernels'] = kern
    print(json.dumps(res), flush=True)
    if out:
        with open(out, 'a') as f:
            f.write(json.dumps(res) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--out', help='append the JSON rows to this file as well')
    ap.add_argument('--commit', help='recorded in the rows where the tree is not a git checkout')
    a = ap.parse_args()
    global COMMIT
    COMMIT = a.commit
    for shape, caxis in (((512, 512), None), ((768, 512, 3), 2), ((512, 512, 8), None)):
        run(shape, caxis, a.steps, a.out)


if __name__ == '__main__':
    main()
