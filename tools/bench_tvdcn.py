#!/usr/bin/env python3
"""Time TVL2Deconv and TVL1Deconv: the reference's tvl2dcn_den call (A = ones((1, 1)), gEvalY off, 200
iterations) and a 15 x 15 blur, the same for l1 on an image with 20 % impulse noise, float32, device arrays in
and out, at

    512 x 512 (P = 1),   768 x 512 x 3 (caxis=2),   512 x 512 x 8,

with TVL2Denoise / TVL1Denoise at the same shape, from the same process, for scale.

Per shape, solver and kernel one JSON row: it/s of an unprofiled run (host clock around solve() and a device
synchronise, after a warm-up solve of the same shape), then -- from a second, profiled run -- the milliseconds
per launch group of each profile slot (the library's event profile) and the bytes each moves BY CONSTRUCTION
(every array it reads or writes once, halo rows and the small per-frequency tables not counted), with the TB/s
that makes, beside the 6.3 TB/s copy rate the project measures against.  e = H W P * 4 bytes (a real array of
S's shape), f = H (W/2+1) P * 8 bytes (a spectrum of S's planes):
    slot           l2                                            l1
    tvdc_rfft2     rows: RY, RU -> wf; columns in place          2 e + 3 f     4 e + 6 f
    tvdc_solve     wf, AHSf, Sf in, wf out (l1: no Sf, 2 wf)     4 f           5 f       (+ Af, |Af|^2 per plane)
    tvdc_irfft2    columns in place; rows wf -> XH               3 f + e       6 f + 2 e
    tvdc_ystep     XH, (S,) Y, U in; Y, U (, dY) out             11 e          15 e
    tvdc_adjoint   Y, U (, dY) in; RY, RU out                    8 e           10 e
    tvdc_dual      l1: RU -> wf, columns, read wf                --            2 e + 8 f
Launches per iteration: l2 8 (2 + 1 + 2 + 1 + 1 and one that reduces the partial sums; 9 with LinSolveCheck
or statistics: the solve's sums have a reduction of their own), l1 11 (+ 2 + 1 for the dual residual); one
128-byte read.  Plane transforms per iteration: l2 P forward + P inverse; l1 2 P + 2 P and 2 P for the dual
residual.

    python tools/bench_tvdcn.py --out profiles/tvdcn_bench.jsonl
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
# (e, f) multiples per profile slot
ARRAYS = {'l2': {'tvdc_rfft2': (2, 3), 'tvdc_solve': (0, 4), 'tvdc_irfft2': (1, 3), 'tvdc_ystep': (11, 0),
                 'tvdc_adjoint': (8, 0)},
          'l1': {'tvdc_rfft2': (4, 6), 'tvdc_solve': (0, 5), 'tvdc_irfft2': (2, 6), 'tvdc_ystep': (15, 0),
                 'tvdc_adjoint': (10, 0), 'tvdc_dual': (2, 8)}}
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
    """it/s of an unprofiled run after a warm-up, then the per-slot figures of a profiled one."""
    import numpy as np
    make().solve()                 # warm-up: code objects, allocator
    b = make()
    b._dev.sync()
    t0 = time.perf_counter()
    b.solve()
    b._dev.sync()
    dt = time.perf_counter() - t0
    res = {'it_per_s': steps / dt, 'ms_per_it': 1e3 * dt / steps, 'ObjFun_last': float(b.itstat[-1].ObjFun),
           'rho_last': float(b.rho), 'iterations': len(b.itstat)}
    p = make()
    p._dev.profile(True)
    p.solve()
    p._dev.sync()
    e = 4 * int(np.prod(shape))
    f = 8 * int(np.prod(shape)) // shape[1] * (shape[1] // 2 + 1)
    kern, total = {}, 0.0
    for name, (ms, cnt) in p._dev.profile_read().items():
        row = {'launches': cnt, 'ms_per_launch': ms / cnt, 'ms_per_it': ms / steps}
        total += ms / steps
        if arrays and name in arrays:
            nbytes = arrays[name][0] * e + arrays[name][1] * f
            row['bytes_per_launch'] = nbytes
            row['tb_per_s'] = nbytes / (ms / cnt * 1e-3) / 1e12
        kern[name] = row
    res['kernels'] = kern
    res['device_ms_per_it'] = total
    return res


def run(shape, caxis, steps, out=None):
    import numpy as np
    import sporco_amd
    from sporco_amd.admm import tvl1, tvl2
    from sporco_amd.device import DeviceArray
    if sporco_amd.device_count() < 1:
        raise SystemExit("bench_tvdcn needs an AMD GPU")
    rng = np.random.RandomState(1)
    H, W = shape[:2]
    img = np.ones((H, W))
    img[:, W // 2:] = -1.0
    img[H // 3:] *= 0.5
    clean = np.broadcast_to(img.reshape((H, W) + (1,) * (len(shape) - 2)), shape)
    blur = rng.rand(15, 15)
    blur /= blur.sum()
    kernels = {'den': np.ones((1, 1), np.float32), 'blur15': blur.astype(np.float32)}
    rows = []
    for kname, A in kernels.items():
        Ap = A.reshape(A.shape + (1,) * (len(shape) - 2))
        blurred = np.fft.irfftn(np.fft.rfftn(Ap, s=(H, W), axes=(0, 1)) * np.fft.rfftn(clean, axes=(0, 1)), s=(H, W),
                                axes=(0, 1))
        S2 = (blurred + 0.05 * rng.randn(*shape)).astype(np.float32)
        S1 = np.where(rng.rand(*shape) < 0.2, rng.uniform(-1.5, 1.5, shape), S2).astype(np.float32)
        for kind, cls, S, lmbda in (('l2', tvl2.TVL2Deconv, S2, 0.05), ('l1', tvl1.TVL1Deconv, S1, 0.8)):
            Sd, Ad = DeviceArray.from_host(S), DeviceArray.from_host(A)
            o = {'Verbose': False, 'MaxMainIter': steps, 'gEvalY': False, 'AutoRho': {'Enabled': True},
                 'RelStopTol': 0.0}
            r = timed(lambda: cls(Ad, Sd, lmbda, cls.Options(o), caxis=caxis), steps, shape, ARRAYS[kind])
            res = {'solver': 'tv%sdcn' % kind, 'kernel': kname, 'shape': list(shape), 'caxis': caxis,
                   'dtype': 'float32', 'steps': steps, 'lmbda': lmbda, 'copy_tb_per_s': COPY_TB_S,
                   'launches_per_it': 9 if kind == 'l2' else 11, 'commit': commit()}
            res.update(r)
            rows.append(res)
    # the Denoise classes at the same shape, for scale
    Sd = DeviceArray.from_host((clean + 0.05 * rng.randn(*shape)).astype(np.float32))
    for name, cls, lmbda in (('tvl2den', tvl2.TVL2Denoise, 0.05), ('tvl1den', tvl1.TVL1Denoise, 0.8)):
        o = {'Verbose': False, 'MaxMainIter': steps, 'gEvalY': False, 'AutoRho': {'Enabled': True}, 'RelStopTol': 0.0}
        r = timed(lambda: cls(Sd, lmbda, cls.Options(o), caxis=caxis), steps, shape, None)
        res = {'solver': name, 'shape': list(shape), 'caxis': caxis, 'dtype': 'float32', 'steps': steps,
               'lmbda': lmbda, 'commit': commit()}
        res.update(r)
        rows.append(res)
    for res in rows:
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
    global COMMIT
    COMMIT = a.commit
    for shape, caxis in (((512, 512), None), ((768, 512, 3), 2), ((512, 512, 8), None)):
        run(shape, caxis, a.steps, a.out)


if __name__ == '__main__':
    main()
