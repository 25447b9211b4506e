#!/usr/bin/env python3
"""Time admm.rpca.RobustPCA on device arrays, float32 and float64, at

    76800 x 128  (a 320 x 240 video of 128 frames, one frame a column)        and        512 x 512,

S a rank-5 product of Gaussian factors plus outliers at 5 % of the positions, the class's default options with
RelStopTol = 0, 100 iterations.  Nothing here is a gate, there is no earlier figure to compare with.

Per (shape, dtype) one JSON row, from ONE process:
  it_per_s              host clock around solve() (it ends with a device synchronise), after a warm-up solver of the
                        same shape; one run, not averaged (`runs`: 1)
  kernels_ms            milliseconds per launch of every kernel of the handle, from its event profile in a second
                        run (`launches`: how many), and `device_ms_per_it`, their sum over an iteration
  host_step             seconds per iteration of the second run spent in the host step (`eigh_ms`: svt_matrix, i.e.
                        numpy.linalg.eigh and the n x n product) and in the handle's calls outside kernels
                        (`copies_ms`: the wall clock of gram() and iter() minus their kernels: the G download, the T
                        upload, the 128-byte read, launch and synchronise overheads); `host_share` is their part of
                        the wall-clock iteration of that run
  bytes / flops         BY CONSTRUCTION, per iteration: rpca_gram reads S, Y, U once (3 elements), rpca_iter reads
                        them once from memory and writes X, Y, U (3 + 3; its second pass over S, Y, U is expected from
                        cache and is not counted); 2 L n^2 flops each.  `gram_tb_s`, `iter_tb_s`, `gram_tf`,
                        `iter_tf`: those counts over the measured kernel times
  reference             the UNMODIFIED reference (staged by build() into oracle/_ref) on this host's CPU at the same
                        call, float64, `--ref-steps` iterations, one run, in a subprocess; null where it is not
                        staged or --no-reference

    python tools/bench_rpca.py --out profiles/rpca_bench.jsonl
"""

import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

_REF_CODE = r"""
import sys, time, json, warnings
warnings.filterwarnings('ignore')
sys.path.insert(0, %(ref)r); sys.path.insert(0, %(stubs)r); sys.path.insert(0, %(tools)r)
import numpy as np
import bench_rpca as br
from sporco.admm import rpca
R, C, steps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
S = br.problem(R, C, np.float64)
b = rpca.RobustPCA(S, None, rpca.RobustPCA.Options(br.options(steps)))
t = time.perf_counter(); b.solve(); t = time.perf_counter() - t
print(json.dumps({'it_per_s': steps / t, 'seconds': t, 'steps': steps, 'objfun': float(b.itstat[-1].ObjFun)}))
"""


def problem(R, C, dtype):
    import numpy as np
    rng = np.random.RandomState(1)
    S = rng.randn(R, 5).dot(rng.randn(5, C)) / np.sqrt(5.0)
    idx = rng.permutation(R * C)[:(R * C) // 20]
    S.ravel()[idx] += 5.0 * rng.randn(len(idx))
    return S.astype(dtype)


def options(steps):
    return {'Verbose': False, 'MaxMainIter': steps, 'RelStopTol': 0.0}


def commit():
    try:
        return subprocess.check_output(['git', '-C', REPO, 'rev-parse', '--short', 'HEAD'],
                                       stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return None


def reference(R, C, steps):
    ref = os.path.join(REPO, 'oracle', '_ref')
    if not os.path.isfile(os.path.join(ref, 'sporco', 'admm', 'rpca.py')):
        return None
    code = _REF_CODE % {'ref': ref, 'stubs': os.path.join(REPO, 'oracle', '_stubs'),
                        'tools': os.path.join(REPO, 'tools')}
    try:
        out = subprocess.run([sys.executable, '-c', code, str(R), str(C), str(steps)],
                             capture_output=True, timeout=900, check=True).stdout.decode()
        return json.loads(out.strip().splitlines()[-1])
    except Exception as e:      # (the row says so instead of the run ending here)
        return {'error': repr(e)[:200]}


class Clock(object):
    """Wall-clock seconds spent inside a wrapped callable."""

    def __init__(self, fn):
        self.fn, self.seconds = fn, 0.0

    def __call__(self, *a, **kw):
        t = time.perf_counter()
        try:
            return self.fn(*a, **kw)
        finally:
            self.seconds += time.perf_counter() - t


def run(R, C, dtype, steps, ref_steps, out, tag):
    import numpy as np
    from sporco_amd.admm import rpca
    from sporco_amd.device import DeviceArray
    S = DeviceArray.from_host(problem(R, C, dtype))
    n, L, isz = min(R, C), max(R, C), np.dtype(dtype).itemsize
    rpca.RobustPCA(S, None, rpca.RobustPCA.Options(options(3))).solve()      # warm-up
    b = rpca.RobustPCA(S, None, rpca.RobustPCA.Options(options(steps)))
    t = time.perf_counter()
    b.solve()
    t = time.perf_counter() - t
    objfun = float(b.itstat[-1].ObjFun)
    plan = b._dev.plan()
    # second run: the kernels by their events, the host step and the handle's calls by the host clock
    b = rpca.RobustPCA(S, None, rpca.RobustPCA.Options(options(steps)))
    b._dev.profile(True)
    b._dev.profile_read()
    gram, it = Clock(b._dev.gram), Clock(b._dev.iter)
    b._dev.gram, b._dev.iter = gram, it
    svt = Clock(rpca.svt_matrix)
    rpca.svt_matrix = svt
    try:
        t2 = time.perf_counter()
        b.solve()
        t2 = time.perf_counter() - t2
    finally:
        rpca.svt_matrix = svt.fn
    prof = b._dev.profile_read()
    b._dev.profile(False)
    kernels = {k: {'ms': ms / cnt, 'launches': cnt} for k, (ms, cnt) in prof.items()}
    dev_ms = sum(ms for ms, _ in prof.values()) / steps
    kernel_s = sum(ms for ms, _ in prof.values()) * 1e-3
    copies_s = max(gram.seconds + it.seconds - kernel_s, 0.0)
    g_ms = kernels.get('rpca_gram', {}).get('ms')
    i_ms = kernels.get('rpca_iter', {}).get('ms')
    flops = 2.0 * L * n * n
    row = {'tool': 'bench_rpca', 'tag': tag, 'commit': commit(), 'shape': [R, C], 'dtype': np.dtype(dtype).name,
           'steps': steps, 'runs': 1, 'it_per_s': steps / t, 'seconds': t, 'objfun': objfun, 'plan': plan,
           'kernels_ms': kernels, 'device_ms_per_it': dev_ms,
           'host_step': {'eigh_ms': 1e3 * svt.seconds / steps, 'copies_ms': 1e3 * copies_s / steps,
                         'wall_ms_per_it': 1e3 * t2 / steps, 'host_share': (svt.seconds + copies_s) / t2,
                         'eigh_share': svt.seconds / t2},
           'bytes_by_construction': {'gram': 3 * L * n * isz, 'iter': 6 * L * n * isz},
           'flops_by_construction': {'gram': flops, 'iter': flops},
           'gram_tb_s': 3 * L * n * isz / (g_ms * 1e-3) / 1e12 if g_ms else None,
           'iter_tb_s': 6 * L * n * isz / (i_ms * 1e-3) / 1e12 if i_ms else None,
           'gram_tf': flops / (g_ms * 1e-3) / 1e12 if g_ms else None,
           'iter_tf': flops / (i_ms * 1e-3) / 1e12 if i_ms else None,
           'reference': reference(R, C, ref_steps) if ref_steps else None}
    line = json.dumps(row, sort_keys=True)
    print(line, flush=True)
    if out:
        with open(out, 'a') as f:
            f.write(line + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--ref-steps', type=int, default=10)
    ap.add_argument('--no-reference', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--tag', default='')
    a = ap.parse_args()
    import numpy as np
    if a.out and os.path.dirname(a.out):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for R, C in ((76800, 128), (512, 512)):
        for dtype in (np.float32, np.float64):
            # (the reference is float64 whatever the row's dtype: time it once a shape)
            ref_steps = 0 if (a.no_reference or dtype == np.float32) else a.ref_steps
            run(R, C, dtype, a.steps, ref_steps, a.out, a.tag)


if __name__ == '__main__':
    main()
