#!/usr/bin/env python3
"""Time the reference's tvl1den_clr call, TVL1Denoise on an image with impulse noise, AutoRho on, 200
iterations, float32, device arrays in and out, at the shapes of tools/bench_tvl2.py,

    512 x 512 (P = 1),   768 x 512 x 3 (caxis=2),   512 x 512 x 8,

with TVL2Denoise at the same shape, from the same process, beside it.

Per shape one JSON row: it/s of an unprofiled run (host clock around solve() and a device synchronise,
after a warm-up solve of the same shape), then -- from a second, profiled run -- the milliseconds per launch
of each kernel (the library's event profile), the bytes each launch moves BY CONSTRUCTION (every array it
reads or writes once, halo rows not counted) and the TB/s that makes, beside the 6.3 TB/s copy rate the
project measures against.  Arrays per launch, e = H W P * 4 bytes:
    tvd_sweep     reads X, PD, S, writes X                                         4 e   (5 e in the iterations
                  after rho moved: Q is read too; counted as 4.  TVL1Denoise's sweep reads no DFidWeight;
                  TVL2Denoise's does: 5 e, as tools/bench_tvl2.py counts it)
    tvl1_ystep    reads X, PD, S, Y (3), U (3), writes Y (3), U (3)                15 e
    tvl1_adjoint  reads Y (3), U (3), writes PD, Q                                  8 e
    tvd_ystep     14 e and tvd_adjoint 8 e, as tools/bench_tvl2.py counts them (its 14 includes the DFidWeight
                  mask, which this call does not set: 13 e here)
The launch count per iteration is 4 (+ one launch that reduces the partial sums and one 128-byte read).

    python tools/bench_tvl1.py --out profiles/tvl1_bench.jsonl
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
ARRAYS = {'tvl1': {'tvd_sweep': 4, 'tvl1_ystep': 15, 'tvl1_adjoint': 8},
          'tvl2': {'tvd_sweep': 4, 'tvd_ystep': 13, 'tvd_adjoint': 8}}
COMMIT = None


def commit():
    if COMMIT:
        return COMMIT
    try:
        return subprocess.check_output(['git', '-C', REPO, 'rev-parse', '--short', 'HEAD'], text=True,
                                       stderr=subprocess.DEVNULL).strip()
    except Exception:
        return None


def timed(make, steps, shape, arrays):
    """it/s of an unprofiled run after a warm-up, then the per-kernel figures of a profiled one."""
    import numpy as np
    make().solve()                 # warm-up: code objects, allocator
    b = make()
    b._dev.sync()
    t0 = time.perf_counter()
    sl = b.solve()
    b._dev.sync()
    dt = time.perf_counter() - t0
    res = {'it_per_s': steps / dt, 'ms_per_it': 1e3 * dt / steps, 'ObjFun_last': float(b.itstat[-1].ObjFun),
           'rho_last': float(b.rho), 'iterations': len(b.itstat)}
    p = make()
    p._dev.profile(True)
    p.solve()
    p._dev.sync()
    e = 4 * int(np.prod(shape))
    kern = {}
    for name, (ms, cnt) in p._dev.profile_read().items():
        row = {'launches': cnt, 'ms_per_launch': ms / cnt}
        if name in arrays:
            row['bytes_per_launch'] = arrays[name] * e
            row['tb_per_s'] = arrays[name] * e / (ms / cnt * 1e-3) / 1e12
        kern[name] = row
    res['kernels'] = kern
    return res, sl, b


def run(shape, caxis, steps, out=None):
    import numpy as np
    import sporco_amd
    from sporco_amd.admm import tvl1, tvl2
    from sporco_amd.device import DeviceArray
    if sporco_amd.device_count() < 1:
        raise SystemExit("bench_tvl1 needs an AMD GPU")
    rng = np.random.RandomState(1)
    H, W = shape[:2]
    img = np.ones((H, W))
    img[:, W // 2:] = -1.0
    img[H // 3:] *= 0.5
    S = img.reshape((H, W) + (1,) * (len(shape) - 2)) + 0.05 * rng.randn(*shape)
    S = np.where(rng.rand(*shape) < 0.2, rng.uniform(-1.5, 1.5, shape), S).astype(np.float32)
    imgn = DeviceArray.from_host(S)
    lmbda = 1.0 if caxis is not None else 0.8
    o = {'Verbose': False, 'MaxMainIter': steps, 'gEvalY': False, 'AutoRho': {'Enabled': True}, 'RelStopTol': 0.0}

    def make1():
        return tvl1.TVL1Denoise(imgn, lmbda, tvl1.TVL1Denoise.Options(o), caxis=caxis)

    def make2():
        return tvl2.TVL2Denoise(imgn, lmbda, tvl2.TVL2Denoise.Options(o), caxis=caxis)

    r1, sl, b = timed(make1, steps, shape, ARRAYS['tvl1'])
    r2, _, _ = timed(make2, steps, shape, ARRAYS['tvl2'])
    clean = img.reshape((H, W) + (1,) * (len(shape) - 2))
    res = {'solver': 'tvl1', 'shape': list(shape), 'caxis': caxis, 'dtype': 'float32', 'steps': steps,
           'lmbda': lmbda, 'plan': b._dev.plan(), 'launches_per_it': 4, 'copy_tb_per_s': COPY_TB_S,
           'mse_in': float(np.mean((S - clean) ** 2)), 'mse_out': float(np.mean((sl.get() - clean) ** 2)),
           'commit': commit()}
    res.update(r1)
    res['tvl2_same_shape'] = r2
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
