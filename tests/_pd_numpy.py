"""TEST INFRASTRUCTURE ONLY: NumPy restatement of ConvProdDictBPDN / ConvProdDictBPDNJoint
(sporco/admm/pdcsc.py:28-287) AS BUILT in sporco_amd (csrc/csc_pd.h): the channel mix into the
eigen-coordinates of B^T B, one scaled rank-one solve per eigen-channel, the mix back, and the data
fidelity through B Q from the sums d . b the solve has anyway.

Arrays are (H, W, Cb, N, K); the signal is (H, W, Cs, N, 1); float64.  tests/test_pdcsc.py pins this
file to states recorded from the unmodified reference before anything is compared with it.
"""

import numpy as np


def _rfft2(a, s=None):
    return np.fft.rfftn(a, s=s, axes=(0, 1))


def _irfft2(a, shape):
    return np.fft.irfftn(a, s=shape, axes=(0, 1))


def pweights(shape):
    """Half-spectrum weights of fft.rfl2norm2, divided by H W."""
    H, W = shape
    w = np.full(W // 2 + 1, 2.0)
    w[0] = 1.0
    if W % 2 == 0:
        w[-1] = 1.0
    return w.reshape(1, -1, 1, 1, 1) / (H * W)


def eig(B):
    """B^T B = Q Gamma Q^T as the reference takes it (pdcsc.py:112-114)."""
    gam, Q = np.linalg.eigh(B.T.dot(B))
    return np.abs(gam), Q


def cmix(M, A):
    """sum_c M[i, c] A[:, :, c]: a matrix applied along the channel axis (axis 2)."""
    return np.moveaxis(np.tensordot(M, A, axes=([1], [2])), 0, 2)


def xstep(Df, Sf, B, gam, Q, Zf, rho, shape, check=False, want_dfid=True):
    """zh = Q^T z, b = conj(d) sh + rho zh with sh = Sf (B Q), xh = (b - conj(d) gamma (d . b) / (rho + gamma
    g)) / rho, x = Q xh.  Returns Xf, X, the data fidelity (from d . xh = (d . b) / (rho + gamma g)) and,
    with ``check``, the relative residual in eigen-coordinates."""
    BQ = B.dot(Q)
    g = np.sum(np.abs(Df) ** 2, axis=4, keepdims=True)
    gm = gam.reshape(1, 1, -1, 1, 1)
    zh = cmix(Q.T, Zf)
    sh = cmix(BQ.T, Sf)
    b = np.conj(Df) * sh + rho * zh
    p = np.sum(Df * b, axis=4, keepdims=True)
    den = rho + gm * g
    xh = (b - np.conj(Df) * (gm * p / den)) / rho
    Xf = cmix(Q, xh)
    out = [Xf, _irfft2(Xf, shape)]
    dxh = p / den
    out.append(float(np.sum(pweights(shape) * np.abs(cmix(BQ, dxh) - Sf) ** 2)) / 2.0 if want_dfid else None)
    if check:
        ax = gm * np.conj(Df) * np.sum(Df * xh, axis=4, keepdims=True) + rho * xh
        out.append(np.linalg.norm(ax - b) / max(np.linalg.norm(ax), np.linalg.norm(b)))
    return out


def recon_f(Df, B, Vf):
    """B sum_m Df_m Vf_m: (H, Wf, Cs, N, 1)."""
    return cmix(B, np.sum(Df * Vf, axis=4, keepdims=True))


def dfid(Df, Sf, B, Vf, shape):
    return float(np.sum(pweights(shape) * np.abs(recon_f(Df, B, Vf) - Sf) ** 2)) / 2.0


def prox_sl1l2(v, alpha, beta):
    """prox_l2 over the channel axis of the soft threshold (sporco/prox/_l21.py prox_sl1l2)."""
    v = np.sign(v) * np.maximum(0.0, np.abs(v) - alpha)
    if beta == 0.0:
        return v
    a = np.sqrt(np.sum(v ** 2, axis=2, keepdims=True))
    s = np.where(a == 0.0, 0.0, np.maximum(0.0, a - beta) / np.where(a == 0.0, 1.0, a))
    return s * v


def iterate(st, Df, Sf, B, gam, Q, wl1, lmbda, mu, rlx, gevaly, fevalx, auto_rho, k, shape, joint=False,
            nonneg=False, rho_xi=1.0, check=False):
    """One iteration of admm.ADMM.solve (admm.py:331-367) on the state dict ``st`` (Y, U, rho); returns the
    IterationStats values."""
    rho = st['rho']
    Yprev, U = st['Y'], st['U']
    res = xstep(Df, Sf, B, gam, Q, _rfft2(Yprev - U), rho, shape, check=check)
    Xf, X, dfd = res[:3]
    AX = X if rlx == 1.0 else rlx * X + (1.0 - rlx) * Yprev
    Y = prox_sl1l2(AX + U, (lmbda / rho) * wl1, (mu / rho) if joint else 0.0)
    if nonneg:
        Y[Y < 0.0] = 0.0
    U = U + AX - Y
    nr, ns = np.linalg.norm(X - Y), rho * np.linalg.norm(Yprev - Y)
    rn, sn = max(np.linalg.norm(X), np.linalg.norm(Y)), rho * np.linalg.norm(U)
    r, s = nr / (rn or 1.0), ns / (sn or 1.0)
    if not fevalx:
        dfd = dfid(Df, Sf, B, _rfft2(Y), shape)
    G = Y if gevaly else X
    rl1 = float(np.sum(np.abs(wl1 * G)))
    rec = dict(DFid=dfd, RegL1=rl1, PrimalRsdl=r, DualRsdl=s, EpsPrimal=0.0, EpsDual=0.0, Rho=rho)
    if joint:
        rec['RegL21'] = float(np.sum(np.sqrt(np.sum(G ** 2, axis=2))))
        rec['ObjFun'] = dfd + lmbda * rl1 + mu * rec['RegL21']
    else:
        rec['ObjFun'] = dfd + lmbda * rl1
    if check:
        rec['XSlvRelRes'] = res[3]
    if auto_rho and k != 0:
        # AutoRho of ConvBPDN.Options: Period 1, AutoScaling, Scaling 1000, RsdlRatio 1.2
        tau, rmu, xi = 1000.0, 1.2, rho_xi
        if s == 0.0 or r == 0.0:
            mlt = tau
        else:
            mlt = min(np.sqrt(r / (s * xi) if r > s * xi else (s * xi) / r), tau)
        rsf = mlt if r > xi * rmu * s else (1.0 / mlt if s > (rmu / xi) * r else 1.0)
        rho = rho * rsf
        U = U / rsf
    st.update(X=X, Y=Y, U=U, rho=rho)
    return rec


def default_rho_xi(lmbda):
    """cbpdn.py:580-588"""
    return float(1.0 + 18.3 ** (np.log10(lmbda) + 1.0)) if lmbda != 0.0 else 1.0


def admm_pd(D, B, S, lmbda, maxiter, mu=0.0, joint=False, wl1=1.0, rho=None, rlx=1.8, auto_rho=True,
            gevaly=False, fevalx=True, nonneg=False, check=False):
    """The whole solve, RelStopTol = 0 (EpsPrimal = EpsDual = 0): D (dH, dW, 1, 1, K), B (Cs, Cb),
    S (H, W, Cs, N, 1), float64."""
    D = np.asarray(D, dtype=np.float64)
    B = np.asarray(B, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    H, W = S.shape[:2]
    shpX = (H, W, B.shape[1], S.shape[3], D.shape[-1])
    Sf, Df = _rfft2(S), _rfft2(D, (H, W))
    gam, Q = eig(B)
    st = dict(Y=np.zeros(shpX), U=np.zeros(shpX), rho=(50.0 * lmbda + 1.0) if rho is None else float(rho))
    tr = {}
    for k in range(maxiter):
        rec = iterate(st, Df, Sf, B, gam, Q, wl1, lmbda, mu, rlx, gevaly, fevalx, auto_rho, k, (H, W), joint,
                      nonneg, default_rho_xi(lmbda), check)
        for key, val in rec.items():
            tr.setdefault(key, []).append(float(val))
    out = {key: np.array(val) for key, val in tr.items()}
    out.update(X=st['X'], Y=st['Y'], U=st['U'], rho=st['rho'],
               recon=_irfft2(recon_f(Df, B, _rfft2(st['Y'])), (H, W))[..., 0])
    return out
