"""TEST INFRASTRUCTURE ONLY: NumPy restatement of ConvProdDictL1L1Grd / ConvProdDictL1L1GrdJoint
(sporco/admm/pdcsc.py:293-701) AS BUILT in sporco_amd (csrc/csc_pdl1.h): the right-hand side that
mixes the Cs-channel block 0 through B Q and the Cb-channel block 1 through Q, the diagonal-plus-
rank-one solve per eigen-channel, the block-0 constraint spectrum (B Q)(d . xh) as a by-product of
the solve, and this class's own dual residual rho ||A^T U|| against rho ||U||, the first norm taken
in the frequency domain.

Arrays: the signal and block 0 (H, W, Cs, N, 1), the coefficient maps and block 1 (H, W, Cb, N, K),
the dictionary (dH, dW, 1, 1, K); float64.  tests/test_pdl1.py pins this file to states recorded
from the unmodified reference before anything is compared with it.
"""

import numpy as np

from _l1l1_numpy import _rfft2, _irfft2, pweights, ghg, soft, rho_factor, AUTORHO_DEFAULT   # noqa: F401
from _pd_numpy import eig, cmix, prox_sl1l2


def xstep(Df, B, gam, Q, Z0f, Z1f, G, mu_rho, shape, check=False):
    """b = conj(d) (BQ)^T z0 + Q^T z1, dd = 1 + (mu / rho) G, xh = b / dd - conj(d) / dd gamma P / (1 +
    gamma g) with P = sum_m d b / dd and g = sum_m |d|^2 / dd, x = Q xh.  Returns Xf, the block-0
    constraint spectrum (BQ)(d . xh) from d . xh = P / (1 + gamma g) and, with ``check``, the relative
    residual in eigen-coordinates (d . xh summed from xh itself)."""
    BQ = B.dot(Q)
    gm = gam.reshape(1, 1, -1, 1, 1)
    b = np.conj(Df) * cmix(BQ.T, Z0f) + cmix(Q.T, Z1f)
    dd = 1.0 + mu_rho * G
    P = np.sum(Df * b / dd, axis=4, keepdims=True)
    g = np.sum(np.abs(Df) ** 2 / dd, axis=4, keepdims=True)
    dxh = P / (1.0 + gm * g)
    xh = b / dd - np.conj(Df) / dd * (gm * dxh)
    out = [cmix(Q, xh), cmix(BQ, dxh)]
    if check:
        ax = gm * np.conj(Df) * np.sum(Df * xh, axis=4, keepdims=True) + dd * xh
        out.append(np.linalg.norm(ax - b) / max(np.linalg.norm(ax), np.linalg.norm(b)))
    return out


def at_norm(Df, B, V0, V1, shape):
    """|| A^T v || = || irfftn(B^T conj(Df) rfftn(v0)) + v1 || through the half-spectrum Parseval sum."""
    t = np.conj(Df) * cmix(B.T, _rfft2(V0)) + _rfft2(V1)
    return float(np.sqrt(np.sum(pweights(shape) * np.abs(t) ** 2)))


def iterate(st, Df, S, B, gam, Q, W, wl1, wg, lmbda, mu, rlx, auxvar, ar, k, shape, dsz, joint=False, wl21=1.0,
            nonneg=False, nobndry=False, check=False):
    """One iteration of admm.ADMM.solve (admm.py:331-367) on the state dict ``st`` (Y0, Y1, U0, U1,
    rho); returns the IterationStats values."""
    nrm = np.linalg.norm
    rho = float(st['rho'])
    Y0p, Y1p, U0, U1 = st['Y0'], st['Y1'], st['U0'], st['U1']
    G = wg * ghg(shape)
    res = xstep(Df, B, gam, Q, _rfft2(Y0p - U0 + S), _rfft2(Y1p - U1), G, mu / rho, shape, check)
    Xf, AX0f = res[:2]
    X = _irfft2(Xf, shape)
    AX0nr = _irfft2(AX0f, shape)
    if rlx == 1.0:
        AX0, AX1 = AX0nr, X
    else:
        AX0 = rlx * AX0nr + (1 - rlx) * (Y0p + S)
        AX1 = rlx * X + (1 - rlx) * Y1p
    Y0 = soft(AX0 + U0 - S, (1.0 / rho) * W)
    if joint:
        Y1 = prox_sl1l2(AX1 + U1, 0.0, (lmbda / rho) * wl21)
    else:
        Y1 = soft(AX1 + U1, (lmbda / rho) * wl1)
    if nonneg:
        Y1[Y1 < 0] = 0
    if nobndry:
        Y1[1 - dsz[0]:] = 0
        Y1[:, 1 - dsz[1]:] = 0
    U0 = U0 + AX0 - Y0 - S
    U1 = U1 + AX1 - Y1
    nr = float(np.sqrt(nrm(AX0nr - Y0 - S) ** 2 + nrm(X - Y1) ** 2))
    rn = max(float(np.sqrt(nrm(AX0nr) ** 2 + nrm(X) ** 2)), float(np.sqrt(nrm(Y0) ** 2 + nrm(Y1) ** 2)), nrm(S))
    # the dual residual of this class (pdcsc.py:568-578): both at the new U
    ns = rho * at_norm(Df, B, U0, U1, shape)
    sn = rho * float(np.sqrt(nrm(U0) ** 2 + nrm(U1) ** 2))
    r, s = nr / (rn or 1.0), ns / (sn or 1.0)
    g0 = Y0 if auxvar else AX0nr - S
    g1 = Y1 if auxvar else X
    dfd = float(np.sum(np.abs(W * g0)))
    rgr = float(np.sum(pweights(shape) * G * np.abs(Xf) ** 2)) / 2.0
    rec = dict(DFid=dfd, RegGrad=rgr, PrimalRsdl=r, DualRsdl=s, EpsPrimal=0.0, EpsDual=0.0, Rho=rho)
    if joint:
        reg = float(np.sum(wl21 * np.sqrt(np.sum(g1 ** 2, axis=2))))
        rec['RegL21'] = reg
    else:
        reg = float(np.sum(np.abs(wl1 * g1)))
        rec['RegL1'] = reg
    rec['ObjFun'] = dfd + lmbda * reg + mu * rgr
    if check:
        rec['XSlvRelRes'] = res[2]
    rsf = rho_factor(k, r, s, ar)
    st.update(X=X, Xf=Xf, Y0=Y0, Y1=Y1, U0=U0 / rsf, U1=U1 / rsf, rho=rho * rsf)
    return rec


def block_cat(V0, V1):
    """The reference's composite array (pdcsc.py:435-446): (H, W, y0I + y1I), block 0 first."""
    return np.concatenate((V0.reshape(V0.shape[:2] + (-1,)), V1.reshape(V1.shape[:2] + (-1,))), axis=2)


def block_sep(V, shp0, shp1):
    n0 = int(np.prod(shp0[2:]))
    return V[:, :, :n0].reshape(shp0), V[:, :, n0:].reshape(shp1)


def recon(Df, B, X, shape):
    """irfftn(B sum_m Df_m rfftn(X)_m): (H, W, Cs, N)."""
    return _irfft2(cmix(B, np.sum(Df * _rfft2(X), axis=4, keepdims=True)), shape)[..., 0]


def admm_pdl1(D, B, S, lmbda, mu, maxiter, W=1.0, wl1=1.0, wg=1.0, rho=1.0, rlx=1.8, auxvar=False, ar=None,
              joint=False, wl21=1.0, nonneg=False, nobndry=False, check=False, state=None, k0=0):
    """The whole solve, RelStopTol = 0 (EpsPrimal = EpsDual = 0).  D (dH, dW, 1, 1, K), B (Cs, Cb),
    S (H, W, Cs, N, 1); W broadcastable against S, wg a scalar or (K,)."""
    D = np.asarray(D, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    wg = np.asarray(wg, dtype=np.float64)
    H, Wd = S.shape[:2]
    shpX = (H, Wd, B.shape[1], S.shape[3], D.shape[4])
    Df = _rfft2(D, (H, Wd))
    gam, Q = eig(B)
    st = state or dict(Y0=np.zeros(S.shape), Y1=np.zeros(shpX), U0=np.zeros(S.shape), U1=np.zeros(shpX),
                       rho=float(rho))
    tr = {}
    for k in range(k0, k0 + maxiter):
        rec = iterate(st, Df, S, B, gam, Q, W, wl1, wg, lmbda, mu, rlx, auxvar, ar, k, (H, Wd), D.shape[:2], joint,
                      wl21, nonneg, nobndry, check)
        for key, val in rec.items():
            tr.setdefault(key, []).append(float(val))
    out = {key: np.array(val) for key, val in tr.items()}
    out.update(X=st['X'], Y0=st['Y0'], Y1=st['Y1'], U0=st['U0'], U1=st['U1'], Y=block_cat(st['Y0'], st['Y1']),
               U=block_cat(st['U0'], st['U1']), rho=float(st['rho']), recon=recon(Df, B, st['X'], (H, Wd)),
               state=st, Gamma=gam, Q=Q)
    return out
