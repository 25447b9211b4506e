#!/usr/bin/env python3
"""Time dictlrn.bpdndl.BPDNDictLearn on a patch-sized problem, float32 and float64, at

    N = 64, M = 128, K = 32768        and        N = 64, M = 256, K = 32768,

Gaussian D0, S = D X0 + noise with five non-zeros a column through a unit-norm dictionary, lmbda = 0.1, the class's
default options (one inner iteration a step, both AutoRho periods 10), 50 outer iterations.  Nothing here is a gate.

Per (shape, dtype) one JSON row, from ONE process:
  outer_it_per_s        host clock around solve() and a device synchronise of both handles, after a warm-up learner
                        of the same shape; one run, not averaged (`runs`: 1)
  kernels_ms            milliseconds per launch of every kernel of the two handles, from their event profiles in a
                        second run (`launches`: how many), and `device_ms_per_outer_it`, their sum over an outer
                        iteration; `gram_share` is cmod_gram's part of that sum, `gram_share_wall` its part of the
                        wall-clock outer iteration of the first run
  gram_ms_mfma / _plain float32: milliseconds per `cmod_gram` launch, the second from a third run whose D-update handle
                        is made with SPORCO_AMD_CMOD_PLAIN=1 (the switch is read when a handle is made, so both come
                        from the same process); float64 has the plain form only
  bytes / flops         of one `cmod_gram` BY CONSTRUCTION: Z and S once (`gram_bytes_min`), what the workgroups
                        request with every output block staging its 128 rows (`gram_bytes_requested`), the slab
                        partials written and read (`gram_bytes_partials`); 2 (M + N) M K flops; with the microseconds
                        those take at the 6.3 TB/s copy rate and at the guide's 122 TF (matrix) / 52 TF (packed VALU)
  reference             the UNMODIFIED reference (staged by build() into oracle/_ref) on this host's CPU at the same
                        call, float64, `--ref-steps` outer iterations, one run, in a subprocess; null where it is not
                        staged or --no-reference

    python tools/bench_bpdndl.py --out profiles/bpdndl_bench.jsonl
"""

import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COPY_TB_S, MFMA_TF, VALU_TF = 6.3, 122.0, 52.0
LMBDA = 0.1

_REF_CODE = r"""
import sys, time, json, warnings
warnings.filterwarnings('ignore')
sys.path.insert(0, %(ref)r); sys.path.insert(0, %(stubs)r); sys.path.insert(0, %(tools)r)
import numpy as np
import bench_bpdndl as bb
from sporco.dictlrn import bpdndl
N, M, K, steps = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
D0, S = bb.problem(N, M, K, np.float64)
d = bpdndl.BPDNDictLearn(D0, S, bb.LMBDA, bpdndl.BPDNDictLearn.Options(bb.options(steps)))
t = time.perf_counter(); d.solve(); t = time.perf_counter() - t
print(json.dumps({'outer_it_per_s': steps / t, 'seconds': t, 'steps': steps, 'objfun': float(d.itstat[-1].ObjFun)}))
"""


def problem(N, M, K, dtype):
    import numpy as np
    rng = np.random.RandomState(1)
    D0 = rng.randn(N, M)
    Dt = rng.randn(N, M)
    Dt /= np.sqrt(np.sum(Dt ** 2, axis=0, keepdims=True))
    X0 = np.zeros((M, K))
    rows = rng.randint(0, M, size=(5, K))
    X0[rows, np.arange(K)[None, :]] = rng.randn(5, K)
    S = Dt.dot(X0) + 0.05 * rng.randn(N, K)
    return D0.astype(dtype), S.astype(dtype)


def options(steps):
    return {'Verbose': False, 'MaxMainIter': steps}


def commit(given=None):
    if given:
        return given
    try:
        return subprocess.check_output(['git', '-C', REPO, 'rev-parse', '--short', 'HEAD'],
                                       stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return None


def make(D0, S, steps, plain=False):
    from sporco_amd.dictlrn import bpdndl
    old = os.environ.pop('SPORCO_AMD_CMOD_PLAIN', None)
    if plain:
        os.environ['SPORCO_AMD_CMOD_PLAIN'] = '1'
    try:
        return bpdndl.BPDNDictLearn(D0, S, LMBDA, bpdndl.BPDNDictLearn.Options(options(steps)))
    finally:
        os.environ.pop('SPORCO_AMD_CMOD_PLAIN', None)
        if old is not None:
            os.environ['SPORCO_AMD_CMOD_PLAIN'] = old


def sync(d):
    d.xstep._dev.sync()
    d.dstep._dev.sync()


def profiled(d):
    """{kernel: (ms per launch, launches)} of one solve, both handles."""
    for h in (d.xstep._dev, d.dstep._dev):
        h.profile(True)
        h.profile_read()
    d.solve()
    sync(d)
    res = {}
    for h in (d.xstep._dev, d.dstep._dev):
        for k, (ms, n) in h.profile_read().items():
            tot, cnt = res.get(k, (0.0, 0))
            res[k] = (tot + ms, cnt + n)
        h.profile(False)
    return {k: (ms / n, n) for k, (ms, n) in res.items()}


def reference(N, M, K, steps):
    ref = os.path.join(REPO, 'oracle', '_ref')
    if not os.path.isfile(os.path.join(ref, 'sporco', 'dictlrn', 'bpdndl.py')):
        return None
    code = _REF_CODE % {'ref': ref, 'stubs': os.path.join(REPO, 'oracle', '_stubs'),
                        'tools': os.path.dirname(os.path.abspath(__file__))}
    try:
        out = subprocess.run([sys.executable, '-c', code, str(N), str(M), str(K), str(steps)],
                             capture_output=True, timeout=900, check=True).stdout.decode()
        return json.loads(out.strip().splitlines()[-1])
    except Exception as e:      # (the row says so instead of the run ending here)
        return {'error': str(e)[:200]}


def run(N, M, K, dtype, steps, ref_steps, out, tag):
    import numpy as np
    D0, S = problem(N, M, K, dtype)
    e = np.dtype(dtype).itemsize
    make(D0, S, 3).solve()                               # warm-up: code objects, allocator
    d = make(D0, S, steps)
    pl = d.dstep._dev.plan()
    t = time.perf_counter()
    d.solve()
    sync(d)
    secs = time.perf_counter() - t
    row = {'N': N, 'M': M, 'K': K, 'dtype': np.dtype(dtype).name, 'steps': steps, 'runs': 1,
           'outer_it_per_s': steps / secs, 'ms_per_outer_it': 1e3 * secs / steps, 'slab': pl['slab'], 'slabs': pl['slabs'],
           'gram_blocks': pl['row_blocks'] * pl['col_blocks'], 'gram_workgroups': pl['row_blocks'] * pl['col_blocks'] * pl['slabs'],
           'objfun': float(d.itstat[-1].ObjFun), 'commit': tag}
    prof = profiled(make(D0, S, steps))
    row['kernels_ms'] = {k: v[0] for k, v in sorted(prof.items())}
    row['launches'] = {k: v[1] for k, v in sorted(prof.items())}
    dev_ms = sum(ms * n for ms, n in prof.values()) / steps
    row['device_ms_per_outer_it'] = dev_ms
    gram = prof['cmod_gram'][0]
    row['gram_share'] = gram / dev_ms
    row['gram_share_wall'] = gram / row['ms_per_outer_it']
    row['gram_ms_mfma' if pl['mfma'] else 'gram_ms_plain'] = gram
    if pl['mfma']:
        row['gram_ms_plain'] = profiled(make(D0, S, steps, plain=True))['cmod_gram'][0]
    row['gram_bytes_min'] = (M + N) * K * e
    row['gram_bytes_requested'] = row['gram_blocks'] * 128 * K * e
    row['gram_bytes_partials'] = 2 * pl['slabs'] * pl['row_blocks'] * 64 * pl['col_blocks'] * 64 * e
    row['gram_flops'] = 2 * (M + N) * M * K
    row['gram_flops_issued'] = 2 * row['gram_blocks'] * 64 * 64 * K
    row['us_at_copy_rate'] = 1e6 * (row['gram_bytes_min'] + row['gram_bytes_partials']) / (COPY_TB_S * 1e12)
    row['us_at_mfma_rate'] = 1e6 * row['gram_flops'] / (MFMA_TF * 1e12)
    row['us_at_valu_rate'] = 1e6 * row['gram_flops'] / (VALU_TF * 1e12)
    row['copy_tb_per_s'], row['mfma_tf'], row['valu_tf'] = COPY_TB_S, MFMA_TF, VALU_TF
    for k in ('gram_ms_mfma', 'gram_ms_plain'):
        if row.get(k):
            row[k.replace('gram_ms', 'gram_tflops')] = row['gram_flops'] / (row[k] * 1e-3) / 1e12
    row['reference'] = reference(N, M, K, ref_steps) if ref_steps and dtype == np.float64 else None
    print(json.dumps(row), flush=True)
    if out:
        with open(out, 'a') as fh:
            fh.write(json.dumps(row) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--ref-steps', type=int, default=5)
    ap.add_argument('--K', type=int, default=32768)
    ap.add_argument('--out', help='append the JSON rows to this file as well')
    ap.add_argument('--commit', help='recorded in the rows where the tree is not a git checkout')
    ap.add_argument('--no-reference', action='store_true', help='skip the CPU runs of the reference')
    a = ap.parse_args()
    import numpy as np
    import sporco_amd
    if sporco_amd.device_count() < 1:
        raise SystemExit("bench_bpdndl needs an AMD GPU")
    tag = commit(a.commit)
    for M in (128, 256):
        for dtype in (np.float32, np.float64):
            run(64, M, a.K, dtype, a.steps, 0 if a.no_reference else a.ref_steps, a.out, tag)


if __name__ == '__main__':
    main()
