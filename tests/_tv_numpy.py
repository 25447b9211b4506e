"""TEST INFRASTRUCTURE ONLY: NumPy restatement of ConvBPDNScalarTV / ConvBPDNVectorTV
(sporco/admm/cbpdntv.py:31-727) with the gradient operators as np.roll stencils.

The reference's gradient filters are the two-tap [1, -1], so G_i x = x - roll(x, +1, axis i) and
G_i^T v = v - roll(v, -1, axis i).  Arrays are (H, W, C, N, K), the three blocks of Y and U on a
sixth, last axis (gradient along axis 0, gradient along axis 1, identity), float64.
tests/test_cbpdntv.py pins one iteration of this file to a state recorded from the unmodified
reference before anything is compared with it.
"""

import numpy as np


def cnst_A(X, wtv):
    """(Wtv G_0 x, Wtv G_1 x, x) (cnst_A, cbpdntv.py:502-509)."""
    return np.stack([wtv * (X - np.roll(X, 1, axis=0)), wtv * (X - np.roll(X, 1, axis=1)), X], axis=-1)


def cnst_AT(V, wtv):
    """v_L + Wtv sum_i G_i^T v_i (cnst_AT, cbpdntv.py:513-520)."""
    return V[..., 2] + wtv * ((V[..., 0] - np.roll(V[..., 0], -1, axis=0)) +
                              (V[..., 1] - np.roll(V[..., 1], -1, axis=1)))


def prox_l2(v, alpha, axis):
    a = np.sqrt(np.sum(v ** 2, axis=axis, keepdims=True))
    b = np.maximum(0.0, a - alpha)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(a == 0.0, 0.0, b / np.where(a == 0.0, 1.0, a))
    return s * v


def tv_ystep(X, Y, U, wtv, wl1, lmbda, mu, rho, rlx, vector, gevaly, u_scale=1.0):
    """relax_AX + ystep + ustep (cbpdntv.py:542-559, :314-321 / :707-715, admm.py:434-437) and the
    sums the device kernel returns."""
    AXnr = cnst_A(X, wtv)
    AX = AXnr if rlx == 1.0 else rlx * AXnr + (1.0 - rlx) * Y
    V = AX + u_scale * U
    axis = (4, 5) if vector else (5,)
    Yn = np.empty_like(V)
    # (scalar TV: the reference's call has no axis argument, cbpdntv.py:319 -- ONE norm, over the whole
    # array of gradient blocks; RegTV below is per filter and pixel all the same, :445)
    Yn[..., 0:2] = prox_l2(V[..., 0:2], mu / rho, axis if vector else None)
    Yn[..., 2] = np.sign(V[..., 2]) * np.maximum(0.0, np.abs(V[..., 2]) - (lmbda / rho) * wl1)
    Un = V - Yn
    G = Yn if gevaly else AXnr
    return dict(Y=Yn, U=Un, AXnr=AXnr, r2=np.sum((AXnr - Yn) ** 2), ax2=np.sum(AXnr ** 2),
                y2=np.sum(Yn ** 2), l1=np.sum(np.abs(wl1 * G[..., 2])),
                tv=np.sum(np.sqrt(np.sum(G[..., 0:2] ** 2, axis=axis))))


def tv_adjoint(Y, U, wtv, P_old, u_scale=1.0):
    p, q = cnst_AT(Y, wtv), u_scale * cnst_AT(U, wtv)
    return dict(P=p, Q=q, s2=np.sum((p - P_old) ** 2), u2=np.sum(q ** 2))


def _rfft2(a, s=None):
    return np.fft.rfftn(a, s=s, axes=(0, 1))


def xstep(Df, DSf, P, Q, wtv, rho, shape, exact=True):
    """(D^H D + rho Wtv^2 GHGf + rho) x = D^H s + rho rfftn(A^T (Y - U)) by Sherman-Morrison
    (cbpdntv.py:277-298); P = A^T Y, Q = A^T U.

    ``exact=False`` is the reference's own arithmetic: it hands the diagonal to linalg.solvedbi_sm
    (cbpdntv.py:290-292), whose formula x = (b - a <c, b>) / d, c = a^H / (<a^H, a> + d), solves the
    system only when d does not vary along the filter axis.  With a scalar TVWeight both forms agree
    to rounding; with different weights per filter the reference's x is not the solution of its own
    system (its LinSolveCheck shows it), and the classes under test repeat the reference's arithmetic."""
    H, W = shape
    gh = 2.0 - 2.0 * np.cos(2.0 * np.pi * np.arange(H) / H) if H > 1 else np.ones(1)
    gw = 2.0 - 2.0 * np.cos(2.0 * np.pi * np.arange(W // 2 + 1) / W) if W > 1 else np.ones(1)
    ghg = (gh[:, None] + gw[None, :]).reshape(H, W // 2 + 1, 1, 1, 1)
    d = rho * wtv ** 2 * ghg + rho
    b = DSf + rho * _rfft2(P - Q)
    if not exact:
        c = Df / (np.sum(np.abs(Df) ** 2, axis=4, keepdims=True) + d)
        Xf = (b - np.conj(Df) * np.sum(c * b, axis=4, keepdims=True)) / d
        return Xf, np.fft.irfftn(Xf, s=(H, W), axes=(0, 1))
    bd = b / d
    num = np.sum(Df * bd, axis=4, keepdims=True)
    den = 1.0 + np.sum(np.abs(Df) ** 2 / d, axis=4, keepdims=True)
    Xf = bd - (np.conj(Df) / d) * (num / den)
    return Xf, np.fft.irfftn(Xf, s=(H, W), axes=(0, 1))


def dfid(Df, Sf, Vf, shape):
    Ef = np.sum(Df * Vf, axis=4, keepdims=True) - Sf
    W = shape[1]
    w = np.full(Ef.shape[1], 2.0)
    w[0] = 1.0
    if W % 2 == 0:
        w[-1] = 1.0
    return float(np.sum(w.reshape(1, -1, 1, 1, 1) * np.abs(Ef) ** 2) / (shape[0] * shape[1])) / 2.0


def iterate(st, Df, Sf, wtv, wl1, lmbda, mu, rlx, vector, gevaly, fevalx, auto_rho, k, shape, exact=True):
    """One iteration of admm.ADMM.solve (admm.py:331-367) on the state dict ``st`` (Y, U, rho);
    returns the IterationStats values of the iteration."""
    rho = st['rho']
    Yprev = st['Y']
    Xf, X = xstep(Df, np.conj(Df) * Sf, cnst_AT(st['Y'], wtv), cnst_AT(st['U'], wtv), wtv, rho, shape, exact)
    ys = tv_ystep(X, st['Y'], st['U'], wtv, wl1, lmbda, mu, rho, rlx, vector, gevaly)
    Y, U = ys['Y'], ys['U']
    rn = max(np.sqrt(ys['ax2']), np.sqrt(ys['y2'])) or 1.0
    sn = rho * np.linalg.norm(cnst_AT(U, wtv)) or 1.0
    r = np.sqrt(ys['r2']) / rn
    s = rho * np.linalg.norm(cnst_AT(Y - Yprev, wtv)) / sn
    dfd = dfid(Df, Sf, Xf if fevalx else _rfft2(Y[..., 2]), shape)
    rec = dict(ObjFun=dfd + lmbda * ys['l1'] + mu * ys['tv'], DFid=dfd, RegL1=ys['l1'], RegTV=ys['tv'],
               PrimalRsdl=r, DualRsdl=s, EpsPrimal=0.0, EpsDual=0.0, Rho=rho)
    if auto_rho and k != 0:
        # AutoRho of ConvBPDN.Options: Period 1, AutoScaling, Scaling 1000, RsdlRatio 1.2; RsdlTarget 1
        tau, rmu, xi = 1000.0, 1.2, 1.0
        if s == 0.0 or r == 0.0:
            mlt = tau
        else:
            mlt = min(np.sqrt(r / (s * xi) if r > s * xi else (s * xi) / r), tau)
        rsf = mlt if r > xi * rmu * s else (1.0 / mlt if s > (rmu / xi) * r else 1.0)
        rho = rho * rsf
        U = U / rsf
    st.update(X=X, Y=Y, U=U, rho=rho)
    return rec


def admm_tv(D, S, lmbda, mu, maxiter, vector=False, wtv=1.0, wl1=1.0, rho=None, rlx=1.8,
            auto_rho=True, gevaly=False, fevalx=True, Y0=None, U0=None, exact=True):
    """The whole solve, RelStopTol = 0: D (dH, dW, 1, 1, K), S (H, W, C, N, 1), float64; ``wtv`` a
    scalar or (1, 1, 1, 1, K)."""
    D = np.asarray(D, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    H, W = S.shape[:2]
    shpX = (H, W, S.shape[2], S.shape[3], D.shape[-1])
    Sf, Df = _rfft2(S), _rfft2(D, (H, W))
    st = dict(Y=np.zeros(shpX + (3,)) if Y0 is None else np.array(Y0, dtype=np.float64),
              U=np.zeros(shpX + (3,)) if U0 is None else np.array(U0, dtype=np.float64),
              rho=1.0 if rho is None else float(rho))   # (the reference's effective default)
    tr = {}
    for k in range(maxiter):
        rec = iterate(st, Df, Sf, wtv, wl1, lmbda, mu, rlx, vector, gevaly, fevalx, auto_rho, k, (H, W), exact)
        for key, val in rec.items():
            tr.setdefault(key, []).append(float(val))
    out = {key: np.array(val) for key, val in tr.items()}
    out.update(X=st['X'], Y=st['Y'], U=st['U'], rho=st['rho'], Df=Df)
    return out
