"""bench.py's plain run and `--dump-outputs`, end to end on CPU (the simulator build, a tiny
workload): a plain run prints the headline alone, `--steps` is the number of timed iterations, and
two runs with the same arguments write the same outputs."""

import json
import os
import subprocess
import sys

import numpy as np

from conftest import REPO, build_hostsim, use_backend

FULL_ONLY = ('steady_state', 'roofline', 'iteration_roofline', 'other_options', 'parity',
             'kernel_roofline', 'configs', 'next_rows', 'time_to_tol', 'cpu_baseline')


def run_bench(out_dir, steps, *extra):
    env = dict(os.environ, OMP_NUM_THREADS='1', SPORCO_AMD_LIBRARY=build_hostsim())
    for v in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(v, None)
    cmd = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', str(steps),
           '--warmup', '1', '--size', '128', '--filters', '8', '--images', '1',
           '--dump-outputs', str(out_dir)] + list(extra)
    r = subprocess.run(cmd, env=env, timeout=600, cwd=REPO, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0])


def load_dir(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith('.npy')}


def test_plain_run_headline_and_dumped_outputs(tmp_path):
    d = run_bench(tmp_path / 'a', 3)
    assert d['metric'] == 'ConvBPDN ADMM iterations/s' and d['higher_is_better'] is True
    assert d['dtype'] == 'f32' and d['unit'].startswith('iterations/s')
    assert d['steps'] == 3 and d['warmup'] == 1 and d['n_gpus'] == 1
    assert d['ms_per_step'] > 0 and abs(d['value'] * d['ms_per_step'] - 1e3) < 1e-6 * 1e3
    assert not any(k in d for k in FULL_ONLY), sorted(d)
    assert list(d)[-1] == 'summary' and d['summary']['ms_per_step'] == d['ms_per_step']

    a = load_dir(tmp_path / 'a')
    assert a['Y'].dtype == np.float32 and a['Y'].size == 128 * 128 * 8
    assert np.isfinite(a['Y']).all() and np.abs(a['Y']).max() > 0
    for f in ('ObjFun', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert a['itstat_' + f].dtype == np.float64 and a['itstat_' + f].shape == (3,)
    assert list(a['itstat_Iter']) == [1, 2, 3]          # the timed iterations, after the warm-up one
    assert 'itstat_Time' not in a
    assert sum(os.path.getsize(os.path.join(tmp_path / 'a', f + '.npy')) for f in a) <= 64 << 20

    # same arguments, same inputs: the same outputs -- with --full too, whose later figures are
    # taken from the timed solver and whose dump comes from a second run of the same steps
    run_bench(tmp_path / 'b', 3)
    f = run_bench(tmp_path / 'f', 3, '--full', '--tiny', '--steady-steps', '2', '--no-parity',
                  '--no-time-to-tol', '--no-cpu-baseline', '--configs', 'none')
    assert 'steady_state' in f and f['steps'] == 3
    for other in ('b', 'f'):
        o = load_dir(tmp_path / other)
        assert sorted(a) == sorted(o)
        for k in a:
            assert np.array_equal(a[k], o[k]), (other, k)


def test_dump_samples_large_outputs(tmp_path, monkeypatch):
    """Beyond DUMP_MAX_VALUES the coefficient map is written as a fixed seeded sample."""
    use_backend('hostsim')
    import bench
    from sporco_amd.admm import cbpdn
    D, S = bench.make_problem(32, 32, 8, 1, 0)
    b = cbpdn.ConvBPDN(D, S, 0.05, cbpdn.ConvBPDN.Options({'MaxMainIter': 2, 'RelStopTol': 0.0}))
    Y = b.solve().reshape(-1)
    monkeypatch.setattr(bench, 'DUMP_MAX_VALUES', 1000)
    bench.dump_outputs(str(tmp_path), b, 2)
    out = load_dir(tmp_path)
    assert 'Y' not in out and out['Y_sample'].shape == (1000,)
    idx = np.sort(np.random.RandomState(0).randint(0, Y.size, 1000))
    assert np.array_equal(out['Y_sample'], Y[idx])
    assert list(out['itstat_Iter']) == [0, 1]
