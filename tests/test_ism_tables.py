"""The tables of the iterated Sherman-Morrison solve (multi-channel dictionary) are cached on the
handle under the system they were built for: rho, and the gradient diagonal (mu and GradWeight).
One handle that serves different systems in turn must give, call for call, exactly what a fresh
handle gives for that call alone -- a stale table would go unnoticed otherwise: no fault, and
plausible numbers.

16 x 16 (no register-resident path), K = 4, N = 2, two-channel dictionary and signal; float32
and float64; on the simulator and, under -m gpu, on the device.
"""

import numpy as np
import pytest

from sporco_amd import _lib

H = W = 16
K, N, CD = 4, 2, 2
DH = DW = 5


def _problem(dtype):
    rng = np.random.RandomState(20240)
    D = rng.randn(DH, DW, CD, 1, K)
    D /= np.sqrt(np.sum(D ** 2, axis=(0, 1, 2), keepdims=True))
    g = {'D': D, 'S': rng.randn(H, W, CD, N), 'Y': rng.randn(H, W, 1, N, K),
         'U': 0.1 * rng.randn(H, W, 1, N, K), 'wg': 0.5 + rng.rand(K)}
    return {k: np.ascontiguousarray(v, dtype=dtype) for k, v in g.items()}


def _handle(g, dtype):
    s = _lib.Solver(H, W, CD, N, K, dtype, Cd=CD)
    s.set_dict(g['D'])
    s.set_signal(g['S'])
    s.upload(_lib.VAR_Y, g['Y'])
    s.upload(_lib.VAR_U, g['U'])
    return s


def _params(rho, mu=None):
    p = _lib.AdmmParams()
    p.rho, p.lmbda, p.mu = float(rho), 0.05, 0.0 if mu is None else float(mu)
    p.rlx, p.u_scale = 1.8, 1.0
    p.flags = _lib.FLAG_OBJ | _lib.FLAG_XRRS | (0 if mu is None else _lib.FLAG_GRADREG)
    p.dH, p.dW = DH, DW
    return p


# (rho, mu or None for the plain system, per-filter GradWeight set before the call)
STEPS = [(1.0, None, False), (1.0, 0.3, False), (1.0, None, False), (1.0, 0.7, False),
         (1.0, 0.7, True), (2.5, None, False)]


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_xstep_sequence_matches_fresh_handles(backend, dtype):
    g = _problem(dtype)
    one = _handle(g, dtype)
    for i, (rho, mu, weighted) in enumerate(STEPS):
        fresh = _handle(g, dtype)
        if weighted:
            one.set_grad_weight(g['wg'])
            fresh.set_grad_weight(g['wg'])
        sums = one.admm_xstep(_params(rho, mu))
        ref = fresh.admm_xstep(_params(rho, mu))
        assert np.array_equal(np.asarray(sums), np.asarray(ref)), (i, sums, ref)
        assert np.array_equal(one.download(_lib.VAR_X), fresh.download(_lib.VAR_X)), i
        assert np.all(np.isfinite(one.download(_lib.VAR_X))), i


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_mdcpl_iter_after_gradient_xstep_matches_fresh_handle(backend, dtype):
    """The mask-decoupled solve has rho = 1 and no gradient term: tables a gradient-regularised
    x step with rho = 1 left on the handle differ from its own in the diagonal only."""
    g = _problem(dtype)
    one, fresh = _handle(g, dtype), _handle(g, dtype)
    one.admm_xstep(_params(1.0, 0.3))
    p = _params(3.0)
    p.flags |= _lib.FLAG_RESID
    out = []
    for s in (one, fresh):
        s.mdcpl_init(g['S'])
        s.upload(_lib.VAR_Y, g['Y'])
        s.upload(_lib.VAR_U, g['U'])
        sums = s.mdcpl_iter(p)
        out.append([np.asarray(sums)] + [s.download(v) for v in (_lib.VAR_X, _lib.VAR_Y, _lib.VAR_U,
                                                                  _lib.VAR_MY0, _lib.VAR_MU0)])
    for a, b in zip(*out):
        assert np.array_equal(a, b)
        assert np.all(np.isfinite(a))
