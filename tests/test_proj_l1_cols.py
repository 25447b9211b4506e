"""_lib.proj_l1_cols -- the column search of the bpdn handle's projection mode (csrc/csc_bpdn.h) behind its stateless
entry -- against the sort-based NumPy projection of tests/_bpdnprojl1_numpy.py run in float64 on the same inputs.

Bounds.  float64: 1e-12 relative l2.  float32: four times the figure that the NumPy projection run in float32 shows
against its float64 self on the same (float32) inputs, measured and printed per array; four is the project's margin
for the order of summation.  Every column stays within gamma (1 + 8 eps M), signs are kept, no element is left
unwritten (the entry prefills its output with NaN), and two calls agree bit for bit.

The inputs are designed columns, cycling through KINDS along the array so that neighbouring columns of a workgroup's
block settle after different numbers of passes.  gamma = 0.75 is a float32 number, magnitudes stay within 5 gamma, so
that the rounding of the threshold to float32 (half an ulp of at most 4 gamma, over at most M entries) stays inside
the 8 eps M gamma of the norm bound.  Column 0 is a generic column outside its ball: at K = 1 the float32 figure is
that of a generic column, not of one that both precisions reproduce exactly.
"""

import numpy as np
import pytest

from conftest import rel_l2, use_backend

import _bpdnprojl1_numpy as pn

from sporco_amd import _lib
from sporco_amd.admm import bpdn

GAMMA = 0.75
KINDS = ('random', 'inside', 'on_ball', 'zero', 'one_entry', 'equal', 'ties', 'dominant', 'geometric')
BITWISE = ('inside', 'on_ball', 'zero')       # the output equals the input bit for bit


def column(kind, M, rng, j):
    sgn = np.where(rng.rand(M) < 0.5, -1.0, 1.0)
    v = np.zeros(M)
    if kind == 'random':
        v = rng.randn(M)
        v *= 3.0 * GAMMA / np.sum(np.abs(v))
    elif kind == 'inside':
        v = rng.randn(M)
        v *= 0.5 * GAMMA / np.sum(np.abs(v))
    elif kind == 'on_ball':                    # dyadic parts of gamma: the sum is exact in either precision
        parts = {1: (1.0,), 2: (0.5, 0.5)}.get(M, (0.5, 0.25, 0.25))
        v[:len(parts)] = GAMMA * np.array(parts)
        v = np.roll(v, j % M) * sgn
    elif kind == 'one_entry':
        v[j % M] = -5.0 * GAMMA
    elif kind == 'equal':
        v = 0.75 * GAMMA * sgn
    elif kind == 'ties':                       # 2 gamma and gamma everywhere else: the first threshold is gamma itself
        v = GAMMA * sgn
        v[j % M] *= 2.0
    elif kind == 'dominant':
        v = 3e-6 * GAMMA * rng.rand(M) * sgn
        v[j % M] = 3.0 * GAMMA * sgn[j % M]
    elif kind == 'geometric':                  # one entry leaves the active set per pass for many passes
        v = rng.permutation(4.0 * GAMMA * 0.7 ** np.arange(M)) * sgn
    return v


def designed(M, K, dtype, seed=0):
    rng = np.random.RandomState(seed + 31 * M + K)
    kinds = [KINDS[j % len(KINDS)] for j in range(K)]
    v = np.stack([column(k, M, rng, j) for j, k in enumerate(kinds)], axis=1)
    return np.ascontiguousarray(v.astype(dtype)), kinds


def k_values(M, dtype):
    KB = bpdn.plan(1, M, 5, dtype)['KB']
    assert KB in (16, 32)
    return sorted({1, 5, KB - 1, KB, KB + 1, 3 * KB + 1})


def bound_for(v, ref):
    """float64: 1e-12; float32: four times what the NumPy projection in float32 shows on the same inputs."""
    if v.dtype == np.float64:
        return 1e-12
    return 4.0 * rel_l2(pn.proj_l1_cols(v, np.float32(GAMMA)), ref)


def check(M, K, dtype):
    v, kinds = designed(M, K, dtype)
    ref = pn.proj_l1_cols(v.astype(np.float64), GAMMA)
    out = _lib.proj_l1_cols(v, GAMMA)
    again = _lib.proj_l1_cols(v, GAMMA)
    assert out.dtype == dtype and out.shape == (M, K)
    assert not np.any(np.isnan(out))                                       # every element was written
    assert np.array_equal(out, again)
    err, bound = rel_l2(out, ref), bound_for(v, ref)
    print('M %d K %d %s: bound %.2e, device %.2e' % (M, K, np.dtype(dtype).name, bound, err))
    assert err <= bound, (M, K, err, bound)
    eps = np.finfo(dtype).eps
    assert np.all(np.sum(np.abs(out.astype(np.float64)), axis=0) <= GAMMA * (1 + 8 * eps * M))
    assert np.all(out * v >= 0) and np.all(np.abs(out) <= np.abs(v))       # signs kept, nothing grows
    for j, kind in enumerate(kinds):
        if kind in BITWISE or (kind == 'equal' and M == 1):
            assert np.array_equal(out[:, j], v[:, j]), (kind, j)
        else:                                                              # every other kind ends on its ball
            assert abs(np.sum(np.abs(out[:, j].astype(np.float64))) - GAMMA) <= 8 * eps * M * GAMMA, (kind, j)
    zero = _lib.proj_l1_cols(v, 0.0)                                       # gamma = 0 (negative zeros allowed)
    assert zero.shape == (M, K) and not np.any(zero)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
@pytest.mark.parametrize('M', [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 132, 176] +
                         [pytest.param(m, marks=pytest.mark.gpu) for m in (255, 256, 257, 512)])
def test_designed_columns(backend, M, dtype):
    for K in k_values(M, dtype):
        check(M, K, dtype)


def test_block_columns_follow_the_plan(backend):
    """The 16-column block from M = 176 in float32 and throughout float64 above M = 85; 32 below."""
    assert bpdn.plan(1, 176, 5, np.float32)['KB'] == 16 and bpdn.plan(1, 132, 5, np.float32)['KB'] == 32
    assert bpdn.plan(1, 132, 5, np.float64)['KB'] == 16 and bpdn.plan(1, 40, 5, np.float64)['KB'] == 32


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_nan_and_inf_columns_return(dtype):
    """The CPU simulator only: a column that holds NaN, and one that holds Inf, end their search (a count of zero ends
    it), and the other columns of the same block come out right."""
    use_backend('hostsim')
    for M in (9, 40):
        K = bpdn.plan(1, M, 5, dtype)['KB'] + 3
        v, _ = designed(M, K, dtype)
        bad = v.copy()
        bad[M // 2, 2] = np.nan
        bad[M - 1, 5] = np.inf
        bad[0, K - 1] = -np.inf
        out = _lib.proj_l1_cols(bad, GAMMA)
        good = [j for j in range(K) if j not in (2, 5, K - 1)]
        clean = _lib.proj_l1_cols(v, GAMMA)
        ref = pn.proj_l1_cols(v.astype(np.float64), GAMMA)
        assert rel_l2(clean, ref) <= bound_for(v, ref)
        assert np.array_equal(out[:, good], clean[:, good])


def test_refusals(backend):
    v = np.ones((4, 3))
    with pytest.raises(_lib.BackendError):
        _lib.proj_l1_cols(v, -1.0)
    with pytest.raises(_lib.BackendError, match='512'):
        _lib.proj_l1_cols(np.ones((513, 2)), 1.0)
    with pytest.raises(ValueError):
        _lib.proj_l1_cols(np.ones(4), 1.0)
    with pytest.raises(ValueError):
        _lib.proj_l1_cols(v.astype(np.float16), 1.0)
