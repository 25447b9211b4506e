"""NumPy statements for tests/test_projl1.py: the sort-based projection onto the l1 ball (Duchi et al.
2008, written out here, not imported from the reference) and a restatement of ConvBPDNProjL1
(sporco/admm/cbpdn.py:1220-1395 on admm.py's ADMMEqual steps, AutoRho included) on five-dimensional arrays:
the signal (H, W, C, N, 1), the dictionary (dH, dW, Cd, 1, K), the coefficient maps (H, W, Cx, N, K) with
Cx = C for a single-channel dictionary and 1 for a multi-channel one.  ``dtype`` is the precision of every
array and scalar of the iteration; the sums behind the statistics are taken in float64 either way, as on
the device.  tests/test_projl1.py pins this file to states recorded from the unmodified reference
(tests/golden/projl1_*_f64.npz) before anything is compared with it."""

import numpy as np

from _l1l1_numpy import _irfft2, _rfft2, a0, a0t, pweights, rho_factor, solve


def tau_sort(a, gamma, order=0):
    """Threshold of the projection of a vector with magnitudes ``a`` (float64) onto the l1 ball of radius
    ``gamma`` > 0, for || a ||_1 > gamma: sort, cumulative sum, the last index whose magnitude exceeds
    its running threshold.  ``order`` picks the summation order of the final sum (0: descending
    cumulative sum, 1: ascending pairwise) -- the two differ by rounding only."""
    vs = np.sort(a)[::-1]
    cs = np.cumsum(vs)
    k = np.arange(1, a.size + 1)
    K = int(np.sum(vs > (cs - gamma) / k))
    s = cs[K - 1] if order == 0 else np.sum(vs[:K][::-1])
    return (s - gamma) / K


def proj_l1_vec(v, gamma, order=0):
    a = np.abs(v.astype(np.float64)).ravel()
    if a.sum() <= gamma:
        return v.copy()
    if gamma == 0:
        return np.zeros_like(v)
    t = v.dtype.type(tau_sort(a, gamma, order))
    av = np.abs(v)
    return np.sign(v) * np.where(av > t, av - t, 0).astype(v.dtype)


def proj_l1(v, gamma, axis=None, order=0):
    """Projection of every vector along ``axis`` (None: the whole array; an int or a tuple)."""
    v = np.asarray(v)
    if axis is None:
        return proj_l1_vec(v, gamma, order)
    axes = (axis,) if isinstance(axis, (int, np.integer)) else tuple(axis)
    axes = tuple(sorted(a % v.ndim for a in axes))
    rest = tuple(k for k in range(v.ndim) if k not in axes)
    perm = rest + axes
    w = np.transpose(v, perm)
    shp = w.shape
    w = w.reshape(int(np.prod(shp[:len(rest)], dtype=np.int64)), -1).copy()
    for i in range(w.shape[0]):
        w[i] = proj_l1_vec(w[i], gamma, order)
    return np.transpose(w.reshape(shp), np.argsort(perm))


def tau_floor(v, gamma, axis=None):
    """Largest relative difference between the results of two summation orders on this input: the floor
    below which two correct evaluations of the threshold cannot be told apart."""
    a = proj_l1(v, gamma, axis, 0).astype(np.float64)
    b = proj_l1(v, gamma, axis, 1).astype(np.float64)
    n = np.linalg.norm(a)
    return 0.0 if n == 0 else np.linalg.norm(a - b) / n


AUTORHO_DEFAULT = {'Period': 1, 'Scaling': 1000.0, 'RsdlRatio': 1.2, 'AutoScaling': True, 'RsdlTarget': 1.0}
BALL_AXES = (0, 1, 2, 4)


def cnstr(g, gamma):
    return float(np.linalg.norm((proj_l1(g, float(gamma), axis=BALL_AXES) - g).astype(np.float64)))


def iterate(st, Df, Sf, gamma, rlx, auxvar, ar, k, shape, dsz, nonneg=False, nobndry=False):
    """One iteration of admm.ADMM.solve (admm.py:331-367) for ConvBPDNProjL1 on the state dict ``st`` (Y, U,
    rho); returns the IterationStats values and which images were projected."""
    dt = st['Y'].dtype
    ct = np.complex64 if dt == np.float32 else np.complex128
    f8 = lambda a: np.asarray(a, dtype=np.float64 if np.isrealobj(a) else np.complex128)
    nrm = lambda a: float(np.sqrt(np.sum(np.abs(f8(a)) ** 2)))
    rho = dt.type(st['rho'])
    rlx = dt.type(rlx)
    Yp, U = st['Y'], st['U']
    b = (a0t(Df, Sf) + rho * _rfft2(Yp - U).astype(ct)).astype(ct)
    Xf = solve(Df, rho * np.ones((1, 1, 1, 1, 1), dtype=dt), b).astype(ct)
    X = _irfft2(Xf, shape).astype(dt)
    AX = X if rlx == 1.0 else (rlx * X + (1 - rlx) * Yp).astype(dt)
    V = (AX + U).astype(dt)
    active = np.sum(np.abs(f8(V)), axis=BALL_AXES) > gamma
    Y = proj_l1(V, float(gamma), axis=BALL_AXES).astype(dt)
    if nonneg:
        Y[Y < 0] = 0
    if nobndry:
        Y[1 - dsz[0]:] = 0
        Y[:, 1 - dsz[1]:] = 0
    U = (U + AX - Y).astype(dt)
    nr, ns = nrm(X - Y), float(rho) * nrm(Y - Yp)
    rn, sn = max(nrm(X), nrm(Y)), float(rho) * nrm(U)
    r, s = nr / (rn or 1.0), ns / (sn or 1.0)
    gf = _rfft2(Y).astype(ct) if auxvar else Xf
    dfd = 0.5 * float(np.sum(pweights(shape) * np.abs(f8(a0(Df, gf) - Sf)) ** 2))
    rec = dict(ObjFun=dfd, Cnstr=cnstr(Y if auxvar else X, gamma), PrimalRsdl=r, DualRsdl=s, EpsPrimal=0.0,
               EpsDual=0.0, Rho=float(rho), active=active.ravel())
    rsf = dt.type(rho_factor(k, r, s, ar))
    st.update(X=X, Xf=Xf, Y=Y, U=(U / rsf).astype(dt), rho=rho * rsf)
    return rec


def admm_projl1(D, S, gamma, maxiter, rho=1.0, rlx=1.8, auxvar=False, ar=AUTORHO_DEFAULT, nonneg=False,
                nobndry=False, dtype=np.float64, state=None, k0=0, Y0=None):
    """The whole solve, RelStopTol = 0 (EpsPrimal = EpsDual = 0).  D (dH, dW, Cd, 1, K), S (H, W, C, N, 1);
    ``ar`` the AutoRho options or None; ``Y0`` starts Y (U stays zero, cbpdn.py:1359-1369)."""
    dt = np.dtype(dtype)
    ct = np.complex64 if dt == np.float32 else np.complex128
    D = np.asarray(D, dtype=dt)
    S = np.asarray(S, dtype=dt)
    H, Wd = S.shape[:2]
    Cd, K = D.shape[2], D.shape[4]
    shpX = (H, Wd, 1 if Cd > 1 else S.shape[2], S.shape[3], K)
    Df = _rfft2(D, (H, Wd)).astype(ct)
    Sf = _rfft2(S).astype(ct)
    st = state or dict(Y=np.zeros(shpX, dt) if Y0 is None else np.asarray(Y0, dtype=dt).reshape(shpX).copy(),
                       U=np.zeros(shpX, dt), rho=dt.type(rho))
    tr = {}
    for k in range(k0, k0 + maxiter):
        rec = iterate(st, Df, Sf, dt.type(gamma), rlx, auxvar, ar, k, (H, Wd), D.shape[:2], nonneg, nobndry)
        for key, val in rec.items():
            tr.setdefault(key, []).append(val)
    out = {key: np.array(val) for key, val in tr.items()}
    out.update(X=st['X'], Y=st['Y'], U=st['U'], rho=float(st['rho']),
               recon=_irfft2(a0(Df, _rfft2(st['Y']).astype(ct)), (H, Wd))[..., 0].astype(dt), state=st)
    return out
