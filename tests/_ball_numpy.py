"""TEST INFRASTRUCTURE ONLY: NumPy restatement of ConvMinL1InL2Ball (sporco/admm/cbpdn.py:1830-2060 on
ConvTwoBlockCnstrnt :1401-1826 and admm.ADMMTwoBlockCnstrnt) AS BUILT in sporco_amd
(csrc/csc_ball.h): the rho-free x step of the two-block constraint, the projection of block 0 onto
one l2 ball per channel and image, the soft threshold of block 1, and the parent's dual residual
rho ||A^T U|| against rho ||U||, its norm taken in the frequency domain.

Arrays are five-dimensional: the signal and block 0 (H, W, C, N, 1), the dictionary (dH, dW, Cd, 1,
K), the coefficient maps and block 1 (H, W, Cx, N, K) with Cx = C for a single-channel dictionary
and 1 for a multi-channel one.  ``dtype`` is the precision of every array and scalar of the
iteration (float64, or float32 for the measured float32 tolerances of tests/test_ball.py); the sums
behind the statistics are taken in float64 either way, as on the device.  tests/test_ball.py pins
this file to states recorded from the unmodified reference before anything is compared with it.
"""

import numpy as np

from _l1l1_numpy import _irfft2, _rfft2, a0, a0t, block_cat, pweights, rho_factor, soft, solve

AUTORHO_DEFAULT = {'Period': 10, 'Scaling': 1000.0, 'RsdlRatio': 1.2, 'AutoScaling': True, 'RsdlTarget': 1.0}


def plane_norms(v):
    """The l2 norm over the image plane, in float64: (1, 1, C, N, 1)."""
    return np.sqrt(np.sum(np.asarray(v, dtype=np.float64) ** 2, axis=(0, 1), keepdims=True))


def proj_l2(v, eps):
    """v where its plane norm is at most eps, else eps v / norm (prox/_lp.py:334-340); the factor is
    formed in float64 and applied in the precision of v."""
    d = plane_norms(v)
    sig = np.where(d <= eps, 1.0, eps / np.where(d == 0.0, 1.0, d))
    return (sig.astype(v.dtype) * v).astype(v.dtype), d > eps


def cnstr(g0, eps):
    """|| proj_l2(g0) - g0 ||: per plane the distance max(norm - eps, 0) to the ball."""
    return float(np.sqrt(np.sum(np.maximum(plane_norms(g0) - eps, 0.0) ** 2)))


def iterate(st, Df, S, wl1, eps, rlx, auxvar, ar, k, shape, dsz, nonneg=False, nobndry=False, check=False):
    """One iteration of admm.ADMM.solve (admm.py:331-367) on the state dict ``st`` (Y0, Y1, U0, U1,
    rho); returns the IterationStats values and, under ``active``, which planes were projected."""
    dt = S.dtype
    ct = np.complex64 if dt == np.float32 else np.complex128
    f8 = lambda a: np.asarray(a, dtype=np.float64 if np.isrealobj(a) else np.complex128)
    nrm = lambda a: float(np.sqrt(np.sum(np.abs(f8(a)) ** 2)))
    rho = dt.type(st['rho'])
    rlx = dt.type(rlx)
    Y0p, Y1p, U0, U1 = st['Y0'], st['Y1'], st['U0'], st['U1']
    b = (a0t(Df, _rfft2(Y0p - U0 + S).astype(ct)) + _rfft2(Y1p - U1).astype(ct)).astype(ct)
    g = np.ones((1, 1, 1, 1, 1), dtype=dt)
    Xf = solve(Df, g, b).astype(ct)
    X = _irfft2(Xf, shape).astype(dt)
    AX0nr = _irfft2(a0(Df, Xf), shape).astype(dt)
    if rlx == 1.0:
        AX0, AX1 = AX0nr, X
    else:
        AX0 = rlx * AX0nr + (1 - rlx) * (Y0p + S)
        AX1 = rlx * X + (1 - rlx) * Y1p
    Y0, active = proj_l2((AX0 + U0 - S).astype(dt), float(eps))
    Y1 = soft(AX1 + U1, (dt.type(1) / rho) * wl1).astype(dt)
    if nonneg:
        Y1[Y1 < 0] = 0
    if nobndry:
        Y1[1 - dsz[0]:] = 0
        Y1[:, 1 - dsz[1]:] = 0
    U0 = (U0 + AX0 - Y0 - S).astype(dt)
    U1 = (U1 + AX1 - Y1).astype(dt)
    nr = float(np.sqrt(nrm(AX0nr - Y0 - S) ** 2 + nrm(X - Y1) ** 2))
    rn = max(float(np.sqrt(nrm(AX0nr) ** 2 + nrm(X) ** 2)), float(np.sqrt(nrm(Y0) ** 2 + nrm(Y1) ** 2)), nrm(S))
    pw = pweights(shape)
    atu = float(np.sqrt(np.sum(pw * np.abs(f8(a0t(Df, _rfft2(U0).astype(ct)) + _rfft2(U1).astype(ct))) ** 2)))
    ns = float(rho) * atu
    sn = float(rho) * float(np.sqrt(nrm(U0) ** 2 + nrm(U1) ** 2))
    r, s = nr / (rn or 1.0), ns / (sn or 1.0)
    g0 = Y0 if auxvar else AX0nr - S
    g1 = Y1 if auxvar else X
    rec = dict(ObjFun=float(np.sum(np.abs(f8(wl1 * g1)))), Cnstr=cnstr(g0, float(eps)), PrimalRsdl=r, DualRsdl=s,
               EpsPrimal=0.0, EpsDual=0.0, Rho=float(rho), active=active.ravel())
    if check:
        ax = a0t(Df, a0(Df, Xf)) + g * Xf
        rec['XSlvRelRes'] = nrm(ax - b) / max(nrm(ax), nrm(b))
    rsf = dt.type(rho_factor(k, r, s, ar))
    st.update(X=X, Xf=Xf, Y0=Y0, Y1=Y1, U0=(U0 / rsf).astype(dt), U1=(U1 / rsf).astype(dt), rho=rho * rsf)
    return rec


def admm_ball(D, S, eps, maxiter, wl1=1.0, rho=1.0, rlx=1.8, auxvar=False, ar=AUTORHO_DEFAULT, nonneg=False,
              nobndry=False, check=False, dtype=np.float64, state=None, k0=0):
    """The whole solve, RelStopTol = 0 (EpsPrimal = EpsDual = 0).  D (dH, dW, Cd, 1, K), S (H, W, C, N,
    1); wl1 broadcastable against the coefficient maps; ``ar`` the AutoRho options or None."""
    dt = np.dtype(dtype)
    ct = np.complex64 if dt == np.float32 else np.complex128
    D = np.asarray(D, dtype=dt)
    S = np.asarray(S, dtype=dt)
    wl1 = np.asarray(wl1, dtype=dt)
    H, Wd = S.shape[:2]
    Cd, K = D.shape[2], D.shape[4]
    shpX = (H, Wd, 1 if Cd > 1 else S.shape[2], S.shape[3], K)
    Df = _rfft2(D, (H, Wd)).astype(ct)
    st = state or dict(Y0=np.zeros(S.shape, dt), Y1=np.zeros(shpX, dt), U0=np.zeros(S.shape, dt),
                       U1=np.zeros(shpX, dt), rho=dt.type(rho))
    tr = {}
    for k in range(k0, k0 + maxiter):
        rec = iterate(st, Df, S, wl1, dt.type(eps), rlx, auxvar, ar, k, (H, Wd), D.shape[:2], nonneg, nobndry, check)
        for key, val in rec.items():
            tr.setdefault(key, []).append(val)
    out = {key: np.array(val) for key, val in tr.items()}
    out.update(X=st['X'], Y0=st['Y0'], Y1=st['Y1'], U0=st['U0'], U1=st['U1'], Y=block_cat(st['Y0'], st['Y1']),
               U=block_cat(st['U0'], st['U1']), rho=float(st['rho']),
               recon=_irfft2(a0(Df, st['Xf']), (H, Wd))[..., 0], state=st)
    return out
