"""The generic X-step's column pass as one kernel (fft.h fft_cols_sm): forward transform along H
in place in LDS (decimation in frequency), Sherman-Morrison solve at the digit-reversed
positions (sporco/linalg.py:232-297), inverse transform (decimation in time) -- against the
three kernels it replaces (SPORCO_AMD_NO_COLS_SM=1: fft_c2c, launch_sm_solve, fft_c2c), which
the float64 fixtures of test_admm_cbpdn.py pin to the reference; plus the oracle directly.

The host code of fft_cols_sm picks one of four instantiations of cols_sm_kernel per dtype and one of
two workgroup sizes (fft.hip); FORMS below has the smallest shape for every combination the rule can
reach, and SPORCO_AMD_QUERY_COLS_SM_FORM says which one ran, so a case cannot silently exercise
another.  Those cases are compared with the float64 oracle (its bars: 1e-10 float64, 1e-4 float32,
10 x on the traces) and with the three-kernel chain."""

import functools

import os

import numpy as np
import pytest

from conftest import rel_l2

CASES = {
    # H, W, K, N, dtype       (lengths with radices 2, 3, 4, 5, 7, 8)
    'f32_48x40_k8': (48, 40, 8, 2, np.float32),
    'f64_30x36_k4': (30, 36, 4, 2, np.float64),
    'f64_63x56_k16': (63, 56, 16, 1, np.float64),
    'f32_32x24_k64': (32, 24, 64, 1, np.float32),
    'f64_35x20_k2': (35, 20, 2, 3, np.float64),
    'f32_96x80_k32': (96, 80, 32, 2, np.float32),
    'f64_36x30_k6': (36, 30, 6, 2, np.float64),        # filter counts that are not powers of two
    'f32_40x48_k24': (40, 48, 24, 1, np.float32),
    'f64_24x40_k50': (24, 40, 50, 1, np.float64),
    'f32_56x28_k8': (56, 28, 8, 2, np.float32),         # 7-point butterflies in both directions
    'f64_49x42_k4': (49, 42, 4, 1, np.float64),
}


def run(D, S, optd, fused, slab=None, generic=False, lmbda=0.05):
    from sporco_amd.admm import cbpdn
    if not fused:
        os.environ['SPORCO_AMD_NO_COLS_SM'] = '1'
    if slab:
        os.environ['SPORCO_AMD_COLS_SM_FORCE_SLAB'] = str(slab)
    if generic:      # (sizes the mixed-radix register kernels serve since round 6)
        os.environ['SPORCO_AMD_UNFUSED'] = '1'
    try:
        b = cbpdn.ConvBPDN(D, S, lmbda, cbpdn.ConvBPDN.Options(optd))
        b._dev.profile(True)
        b.solve()
        prof = b._dev.profile_read()
    finally:
        os.environ.pop('SPORCO_AMD_NO_COLS_SM', None)
        os.environ.pop('SPORCO_AMD_COLS_SM_FORCE_SLAB', None)
        os.environ.pop('SPORCO_AMD_UNFUSED', None)
    return b, prof


@pytest.mark.parametrize('name', sorted(CASES))
def test_fused_column_pass_equals_the_three_kernels(backend, name):
    H, W, K, N, dt = CASES[name]
    if backend == 'hostsim' and name == 'f32_96x80_k32':
        pytest.skip("kept short on the CPU simulator")
    rng = np.random.RandomState(len(name))
    D = rng.randn(5, 5, K).astype(dt)
    S = rng.randn(H, W, N).astype(dt)
    optd = {'MaxMainIter': 8, 'RelStopTol': 0.0, 'DataType': dt}
    a, pa = run(D, S, optd, False)
    b, pb = run(D, S, optd, True)
    assert pa['fft_c2c_cols_fwd'][1] == 8 and pb['fft_c2c_cols_fwd'][1] == 0
    assert pb['fft_c2c_cols_inv'][1] == 0 and pb['sm_solve'][1] == 8
    tol = 1e-11 if dt == np.float64 else 2e-5
    for v in ('Y', 'U', 'X'):
        assert rel_l2(getattr(a, v), getattr(b, v)) < tol, v
    # a reader of Xf gets the spectrum of X, not the half-transformed buffer
    assert rel_l2(np.asarray(b.Xf), np.fft.rfft2(np.asarray(b.X, np.float64), axes=(0, 1))) < 10 * tol
    ia, ib = a.getitstat(), b.getitstat()
    for f in ('ObjFun', 'DFid', 'RegL1', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert rel_l2(np.asarray(getattr(ia, f)), np.asarray(getattr(ib, f))) < tol, f


def test_fused_column_pass_against_the_oracle(backend):
    from oracle import cbpdn_oracle as orc
    H, W, K, N = 40, 48, 8, 2
    rng = np.random.RandomState(7)
    D = rng.randn(4, 4, K)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(H, W, N)
    b, prof = run(D, S, {'MaxMainIter': 10, 'RelStopTol': 0.0}, True)
    assert prof['fft_c2c_cols_fwd'][1] == 0
    ref = orc.admm_cbpdn(D.reshape(4, 4, 1, 1, K), S.reshape(H, W, 1, N, 1), 0.05, dtype=np.float64,
                         maxiter=10, rel_tol=0.0)
    assert rel_l2(b.Y, ref['Y']) < 1e-10 and rel_l2(b.U, ref['U']) < 1e-10
    st = b.getitstat()
    for f in ('ObjFun', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert rel_l2(np.asarray(getattr(st, f)), ref[f]) < 1e-10, f


@pytest.mark.gpu
@pytest.mark.parametrize('H,W,K,N,dt', [(384, 320, 32, 2, np.float32), (240, 480, 64, 2, np.float32),
                                        (256, 192, 32, 2, np.float64), (360, 300, 16, 2, np.float32),
                                        (320, 240, 48, 2, np.float32)])
def test_generic_chain_at_mid_sizes_against_the_oracle(gpu_backend, H, W, K, N, dt):
    """The whole generic chain as it runs outside the register kernels (single-array state, fused
    column pass with radices 8, 4, 2, 3, 5, 64-byte tiles for the mid-sized float32 lines) against
    the float64 oracle at sizes of a few hundred points."""
    from oracle import cbpdn_oracle as orc
    from sporco_amd import _lib
    rng = np.random.RandomState(H + K)
    D = rng.randn(8, 8, K)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(H, W, N)
    b, prof = run(D.astype(dt), S.astype(dt), {'MaxMainIter': 10, 'RelStopTol': 0.0, 'DataType': dt}, True,
                  generic=True)
    assert not b._dev.uses_fused_rows()
    assert prof['fft_c2c_cols_fwd'][1] == 0 and prof['sm_solve'][1] == 10
    ref = orc.admm_cbpdn(D.reshape(8, 8, 1, 1, K), S.reshape(H, W, 1, N, 1), 0.05, dtype=np.float64,
                         maxiter=10, rel_tol=0.0)
    tol = 1e-10 if dt == np.float64 else 1e-4
    assert rel_l2(b.Y, ref['Y']) < tol and rel_l2(b.U, ref['U']) < tol and rel_l2(b.X, ref['X']) < tol
    st = b.getitstat()
    for f in ('ObjFun', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert rel_l2(np.asarray(getattr(st, f)), ref[f]) < 10 * tol, f


@pytest.mark.parametrize('H,W,K,slab,dt', [(48, 40, 16, 8, np.float32), (30, 36, 12, 8, np.float64),
                                           (63, 24, 20, 4, np.float64), (32, 32, 64, 32, np.float32)])
def test_slab_form_of_the_fused_column_pass(backend, H, W, K, slab, dt):
    """Tiles beyond LDS go through in slabs of filters (cols_sm_slab_kernel: forward transform and
    the slab's share of the inner product, then solve and inverse transform per slab); forced here
    at small sizes (SPORCO_AMD_COLS_SM_FORCE_SLAB), incl. a last slab that is not full."""
    rng = np.random.RandomState(H + K)
    D = rng.randn(5, 5, K).astype(dt)
    S = rng.randn(H, W, 2).astype(dt)
    optd = {'MaxMainIter': 6, 'RelStopTol': 0.0, 'DataType': dt}
    a, pa = run(D, S, optd, False)
    b, pb = run(D, S, optd, True, slab=slab)
    assert pa['fft_c2c_cols_fwd'][1] == 6 and pb['fft_c2c_cols_fwd'][1] == 0 and pb['sm_solve'][1] == 6
    # (the slab kernel at 1024 threads, 4 operand rows per batch, slabs of the forced width)
    big = int(H % 2 == 0 and (H % 3 == 0 or H % 5 == 0))
    assert form_of(b) == (1024, 4, big, slab) and form_of(a) is None
    tol = 1e-11 if dt == np.float64 else 2e-5
    for v in ('Y', 'U', 'X'):
        assert rel_l2(getattr(a, v), getattr(b, v)) < tol, v
    ia, ib = a.getitstat(), b.getitstat()
    for f in ('ObjFun', 'DFid', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert rel_l2(np.asarray(getattr(ia, f)), np.asarray(getattr(ib, f))) < tol, f


@pytest.mark.gpu
@pytest.mark.parametrize('H,W,K,dt', [(384, 320, 64, np.float32), (256, 192, 64, np.float64)])
def test_slab_form_at_the_sizes_it_is_for(gpu_backend, H, W, K, dt):
    from oracle import cbpdn_oracle as orc
    rng = np.random.RandomState(H)
    D = rng.randn(8, 8, K)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))
    S = rng.randn(H, W, 2)
    b, prof = run(D.astype(dt), S.astype(dt), {'MaxMainIter': 8, 'RelStopTol': 0.0, 'DataType': dt}, True,
                  generic=True)
    assert prof['fft_c2c_cols_fwd'][1] == 0 and prof['sm_solve'][1] == 8
    ref = orc.admm_cbpdn(D.reshape(8, 8, 1, 1, K), S.reshape(H, W, 1, 2, 1), 0.05, dtype=np.float64,
                         maxiter=8, rel_tol=0.0)
    tol = 1e-10 if dt == np.float64 else 1e-4
    assert rel_l2(b.Y, ref['Y']) < tol and rel_l2(b.U, ref['U']) < tol
    for f in ('ObjFun', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert rel_l2(np.asarray(getattr(b.getitstat(), f)), ref[f]) < 10 * tol, f


# ---------------------------------------------------------------------------------------------
# every form of the one-kernel pass, pinned by SPORCO_AMD_QUERY_COLS_SM_FORM
# ---------------------------------------------------------------------------------------------
F32, F64 = np.float32, np.float64
LMBDA = 0.1


def form_of(b):
    """(threads, US, BIG, slab width) of the handle's last fft_cols_sm launch; None before any."""
    from sporco_amd import _lib
    q = b._dev.query(_lib.QUERY_COLS_SM_FORM)
    return None if q == -1 else (q & 0xfff, (q >> 12) & 0xf, (q >> 16) & 1, q >> 17)


def radix_ip(n):
    """The passes of the in-place transform (fft.hip FftPlan::init): every 3 with a 4 or a 2, every 5
    with a 2, then 8, 4, 2, 3, 5, 7 and the primes from 11."""
    e = {2: 0, 3: 0, 5: 0, 7: 0}
    for p in e:
        while n % p == 0:
            n //= p
            e[p] += 1
    a2, a3, a5, r = e[2], e[3], e[5], []
    while a3 > 0 and a2 >= 2:
        r, a3, a2 = r + [12], a3 - 1, a2 - 2
    while a3 > 0 and a2 >= 1:
        r, a3, a2 = r + [6], a3 - 1, a2 - 1
    while a5 > 0 and a2 >= 1:
        r, a5, a2 = r + [10], a5 - 1, a2 - 1
    r += [8] * (a2 // 3) + [4] * (a2 % 3 // 2) + [2] * (a2 % 3 % 2) + [3] * a3 + [5] * a5 + [7] * e[7]
    p = 11
    while n > 1:
        while n % p == 0:
            r.append(p)
            n //= p
        p += 2
    return r


def expected_form(n, K, dt):
    """What fft_cols_sm launches for n-point columns of K <= 64 filters held in LDS, by the rule of
    fft.hip: (threads, US, BIG, nit beyond UMAX); None for a height it does not serve or a tile
    beyond LDS."""
    esz = 8 if dt == F32 else 16
    r = radix_ip(n)
    if K < 2 or K > 64 or n < 2 or any(x > 12 or x in (9, 11) for x in r) or esz * (n * K + n) + 128 + 4 * n > 160 * 1024:
        return None
    Kp = 2
    while Kp < K:
        Kp *= 2
    threads = 1024 if n * K >= 4096 else 256
    nit = -(-n // (threads // Kp))
    umax = 12 if dt == F32 else 6
    big = any(x in (6, 10, 12) for x in r)
    if big or nit <= umax // 3:
        us = umax // 3
    elif nit <= 2 * umax // 3 or nit > umax:
        us = 2 * umax // 3
    else:
        us = umax
    return threads, us, int(big), (not big) and nit > umax


# name: H, W, K, N, dtype, threads, US, BIG, slab.  UMAX is 12 (float32) / 6 (float64); "fallback": a
# thread has more rows than UMAX, and the kernel with 2 UMAX / 3 serves them in batches.
FORMS = {
    # float32, 256 threads
    'f32_2x20_k2': (2, 20, 2, 2, F32, 256, 4, 0, 0),          # Kp = 2; one 2-point pass
    'f32_3x20_k3': (3, 20, 3, 2, F32, 256, 4, 0, 0),          # odd K, Kp = 4
    'f32_4x20_k4': (4, 20, 4, 2, F32, 256, 4, 0, 0),
    'f32_6x20_k4': (6, 20, 4, 2, F32, 256, 4, 1, 0),          # one 6-point pass: BIG
    'f32_21x12_k64': (21, 12, 64, 1, F32, 256, 8, 0, 0),      # nit 6
    'f32_35x20_k64': (35, 20, 64, 1, F32, 256, 12, 0, 0),     # nit 9: US = UMAX
    'f32_49x12_k64': (49, 12, 64, 1, F32, 256, 8, 0, 0),      # nit 13: fallback
    # float32, 1024 threads (n K >= 4096)
    'f32_64x10_k64': (64, 10, 64, 1, F32, 1024, 4, 0, 0),     # nit 4 (the only one <= UMAX / 3 here)
    'f32_75x10_k64': (75, 10, 64, 1, F32, 1024, 8, 0, 0),     # nit 5
    'f32_135x8_k64': (135, 8, 64, 1, F32, 1024, 12, 0, 0),    # nit 9
    'f32_147x12_k64': (147, 12, 64, 1, F32, 1024, 12, 0, 0),  # nit 10
    'f32_196x6_k64': (196, 6, 64, 1, F32, 1024, 8, 0, 0),     # nit 13: fallback
    'f32_196x10_k64': (196, 10, 64, 1, F32, 1024, 8, 0, 0),
    'f32_80x8_k64': (80, 8, 64, 1, F32, 1024, 4, 1, 0),       # 10- and 8-point passes
    # float64, 256 threads
    'f64_2x20_k3': (2, 20, 3, 2, F64, 256, 2, 0, 0),
    'f64_3x20_k2': (3, 20, 2, 2, F64, 256, 2, 0, 0),
    'f64_4x20_k3': (4, 20, 3, 2, F64, 256, 2, 0, 0),
    'f64_6x20_k2': (6, 20, 2, 2, F64, 256, 2, 1, 0),
    'f64_27x12_k32': (27, 12, 32, 1, F64, 256, 4, 0, 0),      # nit 4
    'f64_35x20_k32': (35, 20, 32, 1, F64, 256, 6, 0, 0),      # nit 5: US = UMAX
    'f64_49x12_k32': (49, 12, 32, 1, F64, 256, 4, 0, 0),      # nit 7: fallback
    # float64, 1024 threads (nit >= 4 there: US 2 is out of reach without the wide butterflies)
    'f64_64x10_k64': (64, 10, 64, 1, F64, 1024, 4, 0, 0),
    'f64_75x10_k64': (75, 10, 64, 1, F64, 1024, 6, 0, 0),     # nit 5
    'f64_98x8_k64': (98, 8, 64, 1, F64, 1024, 4, 0, 0),       # nit 7: fallback
    'f64_80x8_k64': (80, 8, 64, 1, F64, 1024, 2, 1, 0),
}
# (the CPU simulator stays below about 1e5 coefficients)
FORMS_GPU_ONLY = ('f32_147x12_k64', 'f32_196x10_k64')


def test_forms_table_reaches_every_instantiation():
    """Every entry is what the rule gives its shape, and the entries cover every (dtype, threads, US,
    BIG, fallback) the rule can reach with the tile in LDS."""
    have = set()
    for name, (H, W, K, N, dt, threads, us, big, slab) in FORMS.items():
        e = expected_form(H, K, dt)
        assert e is not None and e[:3] == (threads, us, big) and slab == 0, name
        have.add((dt,) + e)
    reach = {(dt,) + e for dt in (F32, F64) for n in range(2, 640) for K in range(2, 65)
             for e in [expected_form(n, K, dt)] if e is not None}
    assert have == reach, reach - have
    assert len(reach) == 19
    assert {FORMS[k][0] for k in FORMS} >= {2, 3, 4, 6} and {FORMS[k][2] for k in FORMS} >= {2, 3}


@functools.lru_cache(maxsize=None)
def form_problem(H, W, K, N, dt):
    """Dictionary, signal and the float64 oracle's 6 iterations on them (computed once per shape)."""
    from oracle import cbpdn_oracle as orc
    rng = np.random.RandomState(H * 1000 + W * 10 + K)
    dh, dw = min(H, 4), 4
    D = rng.randn(dh, dw, K)
    D = (D / np.sqrt(np.sum(D ** 2, axis=(0, 1), keepdims=True))).astype(dt)
    S = rng.randn(H, W, N).astype(dt)
    ref = orc.admm_cbpdn(D.astype(F64).reshape(dh, dw, 1, 1, K), S.astype(F64).reshape(H, W, 1, N, 1), LMBDA,
                         dtype=F64, maxiter=6, rel_tol=0.0)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return D, S, ref


def check_against_oracle(b, ref, dt):
    # a dead threshold (all of Y zero, or none of it) would let a wrong solve pass
    nz = float(np.mean(ref['Y'] != 0))
    assert 0.02 < nz < 0.98, nz
    tol = 1e-10 if dt == F64 else 1e-4
    for v in ('Y', 'U', 'X'):
        assert rel_l2(getattr(b, v), ref[v]) < tol, v
    st = b.getitstat()
    for f in ('ObjFun', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert rel_l2(np.asarray(getattr(st, f)), ref[f]) < 10 * tol, f


@pytest.mark.parametrize('name', [pytest.param(k, marks=pytest.mark.gpu) if k in FORMS_GPU_ONLY else k
                                  for k in FORMS])
def test_each_form_against_the_oracle_and_the_three_kernels(backend, name):
    H, W, K, N, dt, threads, us, big, slab = FORMS[name]
    D, S, ref = form_problem(H, W, K, N, dt)
    optd = {'MaxMainIter': 6, 'RelStopTol': 0.0, 'DataType': dt}
    b, pb = run(D, S, optd, True, generic=True, lmbda=LMBDA)
    assert not b._dev.uses_fused_rows()
    assert form_of(b) == (threads, us, big, slab)
    assert pb['fft_c2c_cols_fwd'][1] == 0 and pb['fft_c2c_cols_inv'][1] == 0 and pb['sm_solve'][1] == 6
    check_against_oracle(b, ref, dt)
    a, pa = run(D, S, optd, False, generic=True, lmbda=LMBDA)
    assert form_of(a) is None and pa['fft_c2c_cols_fwd'][1] == 6
    tol = 1e-11 if dt == F64 else 2e-5
    for v in ('Y', 'U', 'X'):
        assert rel_l2(getattr(a, v), getattr(b, v)) < tol, v
    ia, ib = a.getitstat(), b.getitstat()
    for f in ('ObjFun', 'DFid', 'RegL1', 'PrimalRsdl', 'DualRsdl', 'Rho'):
        assert rel_l2(np.asarray(getattr(ia, f)), np.asarray(getattr(ib, f))) < tol, f


@pytest.mark.parametrize('dt', [pytest.param(F64, id='f64'), pytest.param(F32, id='f32')])
@pytest.mark.parametrize('H', [11, 22, 26, 33])
def test_heights_the_one_kernel_pass_refuses(backend, H, dt):
    """A height with a prime factor of 11 or more has no in-place pass: the handle runs the three
    kernels (the direct pass of the line FFT serves the prime), once per iteration each."""
    assert expected_form(H, 4, dt) is None
    D, S, ref = form_problem(H, 20, 4, 2, dt)
    b, prof = run(D, S, {'MaxMainIter': 6, 'RelStopTol': 0.0, 'DataType': dt}, True, lmbda=LMBDA)
    assert form_of(b) is None
    assert prof['fft_c2c_cols_fwd'][1] == 6 and prof['fft_c2c_cols_inv'][1] == 6 and prof['sm_solve'][1] == 6
    check_against_oracle(b, ref, dt)
