"""What the side handles of sporco_amd._lib share (csc_impl.h SideBase, _lib._Handle): lifetime, the upload / download
pairs, the profiler's bookkeeping and the stream and device of each handle, at the smallest shapes a family accepts
that still leave a partial block.  Every comparison is bit for bit: a handle against itself, used in another order."""

import numpy as np
import pytest

from sporco_amd import _lib

DTYPES = [np.float32, np.float64]


def _rand(shape, dtype, seed):
    return np.random.RandomState(seed).randn(*shape).astype(dtype)


class Family(object):
    """One handle class at its test shape: how to make it ready for a step, its cheapest profiled call and the slots
    that call records, a full step, and the state variables with their shapes."""

    def __init__(self, name, make, setup, cheap, slots, step, variables, result):
        self.name, self.make, self.setup, self.cheap, self.slots = name, make, setup, cheap, slots
        self.step, self.variables, self.result = step, variables, result

    def ready(self, dtype):
        h = self.make(dtype)
        self.setup(h, dtype)
        return h


def _tvd_params():
    p = _lib.TvdParams()
    p.rho, p.lmbda, p.rlx, p.u_scale, p.wdf, p.wtv, p.geval_y = 0.9, 0.3, 1.6, 1.0, 1.0, 1.0, 1
    return p


def _tvd(l1):
    H = W = 4
    nb = 3 if l1 else 2

    def setup(h, dtype):
        h.upload(_lib.TVD_S, _rand((H, W, 1), dtype, 1))
        h.upload(_lib.TVD_Y, _rand((nb, H, W, 1), dtype, 2))
        h.upload(_lib.TVD_U, _rand((nb, H, W, 1), dtype, 3))

    def step(h):
        h.sweeps(_tvd_params(), 1)
        return h.ystep(_tvd_params())

    E = (H, W, 1)
    return Family('tvl1' if l1 else 'tvd', lambda dtype: _lib.TvdHandle(H, W, 1, dtype, l1=l1), setup,
                  lambda h: h.sweeps(_tvd_params(), 1), {'tvd_sweep'}, step,
                  {_lib.TVD_S: E, _lib.TVD_X: E, _lib.TVD_Y: (nb,) + E, _lib.TVD_U: (nb,) + E, _lib.TVD_WDF: E,
                   _lib.TVD_WTV: E},
                  lambda h: [h.download(v) for v in (_lib.TVD_X, _lib.TVD_Y, _lib.TVD_U)])


def _tvdc_params():
    p = _lib.TvdcParams()
    p.rho, p.lmbda, p.rlx, p.u_scale, p.wdf, p.wtv = 0.9, 0.3, 1.6, 1.0, 1.0, 1.0
    p.geval_y, p.lin_solve_check, p.want_rsdl, p.want_stats = 1, 0, 1, 1
    return p


def _tvdc(l1):
    H = W = 4
    nb = 3 if l1 else 2

    def setup(h, dtype):
        h.set_kernel(_rand((3, 3, 1), dtype, 4))
        h.upload(_lib.TVDC_S, _rand((H, W, 1), dtype, 1))
        h.upload(_lib.TVDC_Y, _rand((nb, H, W, 1), dtype, 2))
        h.upload(_lib.TVDC_U, _rand((nb, H, W, 1), dtype, 3))
        h.adjoint()

    def step(h):
        h.xstep(_tvdc_params())
        return h.ystep(_tvdc_params())

    E = (H, W, 1)
    variables = {_lib.TVDC_S: E, _lib.TVDC_Y: (nb,) + E, _lib.TVDC_U: (nb,) + E, _lib.TVDC_WTV: E}
    if l1:
        variables[_lib.TVDC_WDF] = E
    return Family('tvl1dc' if l1 else 'tvdc', lambda dtype: _lib.TvdcHandle(H, W, 1, dtype, PA=1, l1=l1), setup,
                  lambda h: h.adjoint(), {'tvdc_adjoint'}, step, variables,
                  lambda h: [h.download(v) for v in (_lib.TVDC_X, _lib.TVDC_Y, _lib.TVDC_U)])


def _spl_params():
    p = _lib.SplParams()
    p.rho, p.lmbda, p.rlx, p.u_scale, p.wdf, p.geval_y, p.lin_solve_check, p.want_stats = 0.9, 0.3, 1.6, 1.0, 1.0, 1, 0, 1
    return p


def _spl():
    E = (1, 8, 1)

    def setup(h, dtype):
        h.upload(_lib.SPL_S, _rand(E, dtype, 1))
        h.upload(_lib.SPL_Y, _rand(E, dtype, 2))
        h.upload(_lib.SPL_U, _rand(E, dtype, 3))

    def step(h):
        h.xstep(_spl_params())
        return h.ystep(_spl_params())

    return Family('spl', lambda dtype: _lib.SplHandle(1, 8, 1, dtype), setup, lambda h: h.ystep(_spl_params()),
                  {'spl_ystep', 'finalize'}, step, {v: E for v in (_lib.SPL_S, _lib.SPL_Y, _lib.SPL_U, _lib.SPL_WDF)},
                  lambda h: [h.download(v) for v in (_lib.SPL_X, _lib.SPL_Y, _lib.SPL_U)])


N, M, K = 8, 12, 5


def _bpdn_params():
    p = _lib.BpdnParams()
    p.rho, p.lmbda, p.mu, p.rlx, p.u_scale, p.wl1, p.c = 0.8, 0.2, 0.0, 1.8, 1.0, 1.0, 0.8
    p.geval_y, p.want_x = 1, 1
    return p


def _bpdn():
    def setup(h, dtype):
        D = _rand((N, M), dtype, 5)
        h.set_dict(D)
        h.set_solve(np.linalg.inv(D.T.dot(D).astype(np.float64) + 0.8 * np.eye(M)).astype(dtype))
        h.upload(_lib.BPDN_S, _rand((N, K), dtype, 1))
        h.upload(_lib.BPDN_Y, _rand((M, K), dtype, 2))
        h.upload(_lib.BPDN_U, _rand((M, K), dtype, 3))

    mk = (M, K)
    return Family('bpdn', lambda dtype: _lib.BpdnHandle(N, M, K, dtype), setup, lambda h: h.iter(_bpdn_params()),
                  {'bpdn_iter', 'finalize'}, lambda h: h.iter(_bpdn_params()),
                  {_lib.BPDN_S: (N, K), _lib.BPDN_X: mk, _lib.BPDN_Y: mk, _lib.BPDN_U: mk, _lib.BPDN_WL1: mk,
                   _lib.BPDN_DTS: mk},
                  lambda h: [h.download(v) for v in (_lib.BPDN_X, _lib.BPDN_Y, _lib.BPDN_U)])


def _pgm_bpdn():
    def setup(h, dtype):
        h.set_dict(_rand((N, M), dtype, 5))
        h.upload(_lib.BPDN_S, _rand((N, K), dtype, 1))
        h.upload(_lib.BPDN_X, _rand((M, K), dtype, 2))
        h.upload(_lib.BPDN_Y, _rand((M, K), dtype, 3))

    def step(h):
        p = _lib.BpdnPgmParams()
        p.L, p.lmbda, p.wl1, p.w = 30.0, 0.2, 1.0, 1.0
        p.phase, p.ymode = _lib.PGMB_PHASE_GRAD | _lib.PGMB_PHASE_PROX, _lib.PGMB_Y_LOAD
        return h.step(p)

    mk = (M, K)
    variables = {v: mk for v in (_lib.BPDN_X, _lib.BPDN_XPRV, _lib.BPDN_Y, _lib.BPDN_YPRV, _lib.BPDN_WL1, _lib.BPDN_DTS,
                                 _lib.BPDN_G, _lib.BPDN_Z, _lib.BPDN_ZZ)}
    variables.update({_lib.BPDN_S: (N, K), _lib.BPDN_W: (N, K)})
    return Family('pgm_bpdn', lambda dtype: _lib.PgmBpdnHandle(N, M, K, dtype), setup, lambda h: h.ystep(0.5),
                  {'bpdn_pgm_ystep', 'finalize'}, step, variables,
                  lambda h: [h.download(v) for v in (_lib.BPDN_X, _lib.BPDN_Y, _lib.BPDN_G)])


def _cmod():
    def setup(h, dtype):
        Z = _rand((M, K), dtype, 6)
        h.set_signal(_rand((N, K), dtype, 1))
        h.set_coef(Z)
        h.set_solve(np.linalg.inv(Z.dot(Z.T).astype(np.float64) + 0.8 * np.eye(M)).astype(dtype))
        h.upload(_lib.CMOD_Y, _rand((N, M), dtype, 2))
        h.upload(_lib.CMOD_U, _rand((N, M), dtype, 3))

    def step(h):
        p = _lib.CmodParams()
        p.rho, p.rlx, p.u_scale, p.zero_mean, p.feval_x, p.geval_y, p.want_dfid = 0.8, 1.8, 1.0, 0, 0, 1, 1
        return h.iter(p)

    nm = (N, M)
    return Family('cmod', lambda dtype: _lib.CmodHandle(N, M, K, dtype), setup, lambda h: h.dfid(_lib.CMOD_X),
                  {'cmod_dfid', 'finalize'}, step,
                  {_lib.CMOD_X: nm, _lib.CMOD_Y: nm, _lib.CMOD_U: nm, _lib.CMOD_SZT: nm, _lib.CMOD_G: (M, M),
                   _lib.CMOD_SZTD: nm},
                  lambda h: [h.download(v) for v in (_lib.CMOD_X, _lib.CMOD_Y, _lib.CMOD_U)])


def _pgm_cmod():
    def setup(h, dtype):
        h.set_signal(_rand((N, K), dtype, 1))
        h.set_coef(_rand((M, K), dtype, 6))
        h.upload(_lib.CMOD_X, _rand((N, M), dtype, 2))
        h.upload(_lib.CMOD_Y, _rand((N, M), dtype, 3))

    def step(h):
        p = _lib.CmodPgmParams()
        p.L, p.w, p.finalize = 30.0, 1.0, 1
        p.phase = _lib.PGMC_PHASE_GRAD | _lib.PGMC_PHASE_PROX | _lib.PGMC_PHASE_DFID
        return h.step(p)

    nm = (N, M)
    return Family('pgm_cmod', lambda dtype: _lib.PgmCmodHandle(N, M, K, dtype), setup, lambda h: h.dfid(),
                  {'cmod_pgm_dfid', 'finalize'}, step,
                  {v: nm for v in (_lib.CMOD_X, _lib.CMOD_XPRV, _lib.CMOD_Y, _lib.CMOD_YALT, _lib.CMOD_PG, _lib.CMOD_PZ,
                                   _lib.CMOD_ZZ)},
                  lambda h: [h.download(v) for v in (_lib.CMOD_X, _lib.CMOD_Y, _lib.CMOD_PG)])


def _rpca():
    R, C = 9, 7
    T = np.random.RandomState(7).randn(C, C)
    T = T.dot(T.T) / C

    def setup(h, dtype):
        h.set_signal(_rand((R, C), dtype, 1))
        h.upload(_lib.RPCA_Y, _rand((R, C), dtype, 2))
        h.upload(_lib.RPCA_U, _rand((R, C), dtype, 3))

    def step(h):
        p = _lib.RpcaParams()
        p.rho, p.lmbda, p.rlx, p.u_scale = 0.8, 0.25, 1.8, 1.0
        return h.iter(p, T)

    return Family('rpca', lambda dtype: _lib.RpcaHandle(R, C, dtype), setup, lambda h: h.apply(T), {'rpca_iter'}, step,
                  {v: (R, C) for v in (_lib.RPCA_X, _lib.RPCA_Y, _lib.RPCA_U)},
                  lambda h: [h.download(v) for v in (_lib.RPCA_X, _lib.RPCA_Y, _lib.RPCA_U)])


FAMILIES = [_tvd(False), _tvd(True), _tvdc(False), _tvdc(True), _spl(), _bpdn(), _pgm_bpdn(), _cmod(), _pgm_cmod(),
            _rpca()]
family = pytest.mark.parametrize('fam', FAMILIES, ids=[f.name for f in FAMILIES])
dtypes = pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])


@family
@dtypes
def test_close_twice_and_use_after_close(backend, fam, dtype):
    h = fam.ready(dtype)
    h.close()
    h.close()
    for call in (h.sync, h.plan, lambda: h.profile(True), h.profile_read, lambda: fam.cheap(h)):
        with pytest.raises(_lib.BackendError, match='null handle'):
            call()


@family
@dtypes
def test_upload_download_round_trip(backend, fam, dtype):
    h = fam.make(dtype)
    for i, (var, shape) in enumerate(sorted(fam.variables.items())):
        a = _rand(shape, h._dtype(var) if hasattr(h, '_dtype') else dtype, 10 + i)
        h.upload(var, a)
        got = h.download(var)
        assert got.dtype == a.dtype and got.shape == a.shape
        assert np.array_equal(got, a), (fam.name, var)
    h.close()


@family
@dtypes
def test_wrong_shape_upload(backend, fam, dtype):
    h = fam.make(dtype)
    for var, shape in fam.variables.items():
        with pytest.raises(ValueError):
            h.upload(var, np.zeros(shape[:-1] + (shape[-1] + 1,), dtype=dtype))
    h.close()


@family
@dtypes
def test_profile_bookkeeping(backend, fam, dtype):
    h = fam.ready(dtype)
    h.profile(True)
    fam.cheap(h)
    got = h.profile_read()
    assert set(got) == fam.slots
    assert all(cnt > 0 and ms >= 0.0 for ms, cnt in got.values())
    assert h.profile_read() == {}
    h.profile(False)
    fam.cheap(h)
    assert h.profile_read() == {}
    h.close()


def _run(fam, dtype, steps):
    h = fam.ready(dtype)
    sums = [fam.step(h) for _ in range(steps)]
    res = fam.result(h)
    h.close()
    return sums, res


PAIRS = [(_tvd(False), _bpdn()), (_tvdc(True), _cmod()), (_spl(), _rpca()), (_tvd(True), _pgm_bpdn()),
         (_tvdc(False), _pgm_cmod())]


@pytest.mark.parametrize('pair', PAIRS, ids=['%s+%s' % (a.name, b.name) for a, b in PAIRS])
@dtypes
def test_two_handles_alternately(backend, pair, dtype):
    """Two handles of different families, each on a stream of its own: used in turns they leave what they leave when
    one runs to its end before the other starts."""
    fa, fb = pair
    steps = 3
    want_a, want_b = _run(fa, dtype, steps), _run(fb, dtype, steps)
    ha, hb = fa.ready(dtype), fb.ready(dtype)
    sums_a, sums_b = [], []
    for _ in range(steps):
        sums_a.append(fa.step(ha))
        sums_b.append(fb.step(hb))
    got_a, got_b = (sums_a, fa.result(ha)), (sums_b, fb.result(hb))
    ha.close()
    hb.close()
    for got, want in ((got_a, want_a), (got_b, want_b)):
        assert np.array_equal(np.array(got[0]), np.array(want[0]), equal_nan=True)
        for g, w in zip(got[1], want[1]):
            assert np.array_equal(g, w)


def test_solver_profile_read_returns_every_slot(backend):
    s = _lib.Solver(8, 8, 1, 1, 2, np.float32)
    s.profile(True)
    got = s.profile_read()
    assert len(got) == _lib.lib().sporco_amd_profile_slots()
    assert all(cnt == 0 for _, cnt in got.values())
    s.profile(False)
    s.close()
    s.close()
    with pytest.raises(_lib.BackendError, match='null handle'):
        s.sync()
