#!/usr/bin/env python3
"""Time admm.bpdn BPDN and BPDNJoint on a patch-sized problem, float32 and float64, at

    N = 64, M = 128, K = 32768        and        N = 64, M = 256, K = 32768,

unit-norm Gaussian D, S = D X0 + noise with five non-zeros a column, lmbda = 0.1, 200 iterations, RelStopTol 0,
with AutoRho on (the class's default, Period 10) and off.  Nothing here is a gate.

Per (shape, dtype, class, AutoRho) one JSON row, from ONE process:
  it_per_s              host clock around solve() and a device synchronise, after a warm-up solve of the same
                        handle shape; one run, not averaged (`runs`: 1)
  rho_host_share        the share of that time the host spent in rhochange (forming the solve matrix in float64
                        and uploading it), and `rho_changes`, how often
  iter_ms_mfma / _plain float32: milliseconds per `bpdn_iter` launch from the library's event profile in a second
                        and a third run, the third on a handle made with SPORCO_AMD_BPDN_PLAIN=1 (the switch is
                        read when a handle is made, so both come from the same process); float64 has the plain form
                        only.  joint rows add `joint_apply_ms`.  The plain-form time is the comparison for the claim
                        that the matrix form keeps the kernel memory bound: the row carries both, beside
  bytes / flops         of one `bpdn_iter` BY CONSTRUCTION: it reads D^T S, Y, U and writes Y, U (five M x K arrays;
                        `bytes_hbm`), reads Y and U a second time and S once (`bytes_all` counts those too), X when it
                        is stored (not in a fixed-count run); 2 M M K + 2 N M K flops; with the microseconds those
                        take at the 6.3 TB/s copy rate and at the guide's 122 TF (matrix) and 52 TF (packed VALU)
  reference             the UNMODIFIED reference (staged by build() into oracle/_ref) on this host's CPU at the same
                        call, float64, one run, in a subprocess; null where it is not staged or --no-reference

    python tools/bench_bpdn.py --out profiles/bpdn_bench.jsonl
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
LMBDA, MU = 0.1, 0.05

_REF_CODE = r"""
import sys, time, json, warnings
warnings.filterwarnings('ignore')
sys.path.insert(0, %(ref)r); sys.path.insert(0, %(stubs)r); sys.path.insert(0, %(tools)r)
import numpy as np
import bench_bpdn as bb
from sporco.admm import bpdn
cname, N, M, K, steps, auto = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
D, S = bb.problem(N, M, K, np.float64)
cls = getattr(bpdn, cname)
opt = cls.Options(bb.options(steps, bool(auto)))
b = cls(D, S, bb.LMBDA, opt) if cname == 'BPDN' else cls(D, S, bb.LMBDA, bb.MU, opt)
t = time.perf_counter(); b.solve(); t = time.perf_counter() - t
print(json.dumps({'it_per_s': steps / t, 'seconds': t, 'objfun': float(b.itstat[-1].ObjFun)}))
"""


def problem(N, M, K, dtype):
    import numpy as np
    rng = np.random.RandomState(1)
    D = rng.randn(N, M)
    D /= np.sqrt(np.sum(D ** 2, axis=0, keepdims=True))
    X0 = np.zeros((M, K))
    rows = rng.randint(0, M, size=(5, K))
    X0[rows, np.arange(K)[None, :]] = rng.randn(5, K)
    S = D.dot(X0) + 0.05 * rng.randn(N, K)
    return D.astype(dtype), S.astype(dtype)


def options(steps, auto):
    return {'Verbose': False, 'MaxMainIter': steps, 'RelStopTol': 0.0, 'AutoRho': {'Enabled': bool(auto)}}


def commit(given=None):
    if given:
        return given
    try:
        return subprocess.check_output(['git', '-C', REPO, 'rev-parse', '--short', 'HEAD'],
                                       stderr=subprocess.DEVNULL).decode().strip()
    except Exception:
        return None


def make(cname, D, S, steps, auto, plain=False):
    from sporco_amd.admm import bpdn
    cls = getattr(bpdn, cname)
    old = os.environ.pop('SPORCO_AMD_BPDN_PLAIN', None)
    if plain:
        os.environ['SPORCO_AMD_BPDN_PLAIN'] = '1'
    try:
        opt = cls.Options(options(steps, auto))
        return cls(D, S, LMBDA, opt) if cname == 'BPDN' else cls(D, S, LMBDA, MU, opt)
    finally:
        os.environ.pop('SPORCO_AMD_BPDN_PLAIN', None)
        if old is not None:
            os.environ['SPORCO_AMD_BPDN_PLAIN'] = old


def timed_solve(b):
    """(seconds of solve(), seconds inside rhochange, rho changes)."""
    spent = [0.0, 0]
    inner = b.rhochange

    def rhochange():
        t = time.perf_counter()
        inner()
        spent[0] += time.perf_counter() - t
        spent[1] += 1
    b.rhochange = rhochange
    b._return_min = False
    t = time.perf_counter()
    b.solve()
    b._dev.sync()
    return time.perf_counter() - t, spent[0], spent[1]


def profiled(b):
    """{slot: ms per launch} of one solve."""
    b._return_min = False
    b._dev.profile(True)
    b._dev.profile_read()
    b.solve()
    b._dev.sync()
    res = {k: ms / n for k, (ms, n) in b._dev.profile_read().items()}
    b._dev.profile(False)
    return res


def reference(cname, N, M, K, steps, auto):
    ref = os.path.join(REPO, 'oracle', '_ref')
    if not os.path.isdir(os.path.join(ref, 'sporco')):
        return None
    code = _REF_CODE % {'ref': ref, 'stubs': os.path.join(REPO, 'oracle', '_stubs'),
                        'tools': os.path.dirname(os.path.abspath(__file__))}
    try:
        out = subprocess.run([sys.executable, '-c', code, cname, str(N), str(M), str(K), str(steps), str(int(auto))],
                             capture_output=True, timeout=1500, check=True).stdout.decode()
        return json.loads(out.strip().splitlines()[-1])
    except Exception as e:      # (the row says so instead of the run ending here)
        return {'error': str(e)[:200]}


def run(N, M, K, dtype, cname, auto, steps, with_ref, out, tag):
    import numpy as np
    D, S = problem(N, M, K, dtype)
    e = np.dtype(dtype).itemsize
    make(cname, D, S, 3, auto).solve()                      # warm-up: code objects, allocator
    b = make(cname, D, S, steps, auto)
    pl = b._dev.plan()
    secs, rho_s, rho_n = timed_solve(b)
    row = {'N': N, 'M': M, 'K': K, 'dtype': np.dtype(dtype).name, 'solver': cname, 'auto_rho': bool(auto),
           'steps': steps, 'runs': 1, 'it_per_s': steps / secs, 'ms_per_it': 1e3 * secs / steps,
           'rho_changes': rho_n, 'rho_host_share': rho_s / secs, 'KB': pl['KB'], 'blocks': pl['blocks'],
           'lds_bytes': pl['lds'], 'launches_per_it': 2 if cname == 'BPDN' else 5,
           'objfun': float(b.itstat[-1].ObjFun), 'commit': tag}
    prof = profiled(make(cname, D, S, steps, auto))
    key = 'iter_ms_mfma' if pl['mfma'] else 'iter_ms_plain'
    row[key] = prof.get('bpdn_iter')
    if cname == 'BPDNJoint':
        row['joint_apply_ms'] = prof.get('bpdn_joint_apply')
        row['joint_rows_ms'] = prof.get('bpdn_joint_rows')
    row['finalize_ms'] = prof.get('finalize')
    if pl['mfma']:
        pp = profiled(make(cname, D, S, steps, auto, plain=True))
        row['iter_ms_plain'] = pp.get('bpdn_iter')
        if cname == 'BPDNJoint':
            row['joint_apply_ms_plain'] = pp.get('bpdn_joint_apply')
    arr = M * K * e
    row['bytes_hbm'] = 5 * arr
    row['bytes_all'] = 7 * arr + N * K * e
    row['flops'] = 2 * M * M * K + 2 * N * M * K
    row['us_at_copy_rate'] = 1e6 * row['bytes_hbm'] / (COPY_TB_S * 1e12)
    row['us_at_mfma_rate'] = 1e6 * row['flops'] / (MFMA_TF * 1e12)
    row['us_at_valu_rate'] = 1e6 * row['flops'] / (VALU_TF * 1e12)
    row['copy_tb_per_s'], row['mfma_tf'], row['valu_tf'] = COPY_TB_S, MFMA_TF, VALU_TF
    for k in ('iter_ms_mfma', 'iter_ms_plain'):
        if row.get(k):
            row[k.replace('iter_ms', 'tb_per_s')] = row['bytes_hbm'] / (row[k] * 1e-3) / 1e12
            row[k.replace('iter_ms', 'tflops')] = row['flops'] / (row[k] * 1e-3) / 1e12
    row['reference'] = reference(cname, N, M, K, steps, auto) if with_ref and dtype == np.float64 else None
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
    ap.add_argument('--no-reference', action='store_true', help='skip the CPU runs of the reference')
    a = ap.parse_args()
    import numpy as np
    import sporco_amd
    if sporco_amd.device_count() < 1:
        raise SystemExit("bench_bpdn needs an AMD GPU")
    tag = commit(a.commit)
    for M in (128, 256):
        for dtype in (np.float32, np.float64):
            for cname in ('BPDN', 'BPDNJoint'):
                for auto in (True, False):
                    # (the reference once a shape and class: its AutoRho-on call, the class's default)
                    run(64, M, a.K, dtype, cname, auto, a.steps, (not a.no_reference) and auto, a.out, tag)


if __name__ == '__main__':
    main()
