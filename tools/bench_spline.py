#!/usr/bin/env python3
"""Time SplineL1 on the call of the reference's examples/scripts/misc/spline.py: an image with 20 % impulse
noise, gEvalY off, AutoRho, 200 iterations, float32, device arrays in and out, at

    512 x 512 (P = 1),   768 x 512 x 3,   512 x 512 x 8,

with TVL2Deconv (impulse kernel, the same options) at the same shape, from the same process, beside it.

Per shape and solver one JSON row: it/s of an unprofiled run (host clock around solve() and a device
synchronise, after a warm-up solve of the same shape), then -- from a second, profiled run -- the milliseconds
per launch group of each profile slot (the library's event profile) and the bytes each moves BY CONSTRUCTION
(every array it reads or writes once, the small tables not counted), with the TB/s that makes, beside the
6.3 TB/s copy rate the project measures against.  e = H W P * 4 bytes (a real array of S's shape),
f = H (W/2+1) P * 8 bytes (a spectrum of S's planes):
    spl_rfft2     rows: RY, RU -> wf; columns in place          2 e + 3 f
    spl_solve     wf in, wf out                                 2 f
    spl_irfft2    columns in place; rows wf -> XV               3 f + e
    spl_ystep     XV, S, Y, U in; Y, U, RY, RU out              8 e   (9 e with an array DFidWeight)
Launches per iteration: 7 (2 + 1 + 2 + 1 and one that reduces the partial sums of both kernels); one
128-byte read.  One run each: the figures are not averaged.

    python tools/bench_spline.py --out profiles/spline_bench.jsonl
"""

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench_tvdcn as bt      # noqa: E402

ARRAYS = {'spl_rfft2': (2, 3), 'spl_solve': (0, 2), 'spl_irfft2': (1, 3), 'spl_ystep': (8, 0)}


def run(shape, steps, out=None):
    import numpy as np
    import sporco_amd
    from sporco_amd.admm import spline, tvl2
    from sporco_amd.device import DeviceArray
    if sporco_amd.device_count() < 1:
        raise SystemExit("bench_spline needs an AMD GPU")
    rng = np.random.RandomState(1)
    H, W = shape[:2]
    img = np.cos(np.linspace(0, np.pi, H))[:, None] * np.cos(np.linspace(0, 1.5 * np.pi, W))[None]
    clean = np.broadcast_to(img.reshape((H, W) + (1,) * (len(shape) - 2)), shape)
    S = np.where(rng.rand(*shape) < 0.2, rng.uniform(-1.5, 1.5, shape), clean).astype(np.float32)
    Sd, Ad = DeviceArray.from_host(S), DeviceArray.from_host(np.ones((1, 1), np.float32))
    o = {'Verbose': False, 'MaxMainIter': steps, 'gEvalY': False, 'AutoRho': {'Enabled': True}, 'RelStopTol': 0.0}
    rows = []
    r = bt.timed(lambda: spline.SplineL1(Sd, 1.0, spline.SplineL1.Options(o)), steps, shape, ARRAYS)
    rows.append(dict({'solver': 'spline', 'launches_per_it': 7, 'lmbda': 1.0}, **r))
    r = bt.timed(lambda: tvl2.TVL2Deconv(Ad, Sd, 0.05, tvl2.TVL2Deconv.Options(o)), steps, shape, bt.ARRAYS['l2'])
    rows.append(dict({'solver': 'tvl2dcn', 'launches_per_it': 9, 'lmbda': 0.05}, **r))
    rows[0]['it_per_s_over_tvl2dcn'] = rows[0]['it_per_s'] / rows[1]['it_per_s']
    for res in rows:
        res.update({'shape': list(shape), 'dtype': 'float32', 'steps': steps, 'copy_tb_per_s': bt.COPY_TB_S,
                    'commit': bt.commit()})
        print(json.dumps(res), flush=True)
        if out:
            with open(out, 'a') as fh:
                fh.write(json.dumps(res) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--out', help='append the JSON rows to this file as well')
    ap.add_argument('--commit', help='recorded in the rows where the tree is not a git checkout')
    a = ap.parse_args()
    bt.COMMIT = a.commit
    for shape in ((512, 512), (768, 512, 3), (512, 512, 8)):
        run(shape, a.steps, a.out)


if __name__ == '__main__':
    main()
