"""TEST INFRASTRUCTURE ONLY: NumPy restatement of ConvBPDNRecTV (sporco/admm/cbpdntv.py:733-1356)
AS BUILT in sporco_amd (csrc/csc_rtv.h): the closed-form rank-one / rank-two x step, the gradient
operators as np.roll stencils on signal-shaped maps, and the residual norms of the general
constraint taken in the frequency domain.

Arrays are (H, W, C, N, K); the gradient blocks of Y and U are (H, W, C, N, 2) and follow the K
coefficient maps on the last axis of ``Y`` / ``U`` (the reference's block_cat layout), float64.
tests/test_cbpdnrtv.py pins this file to states recorded from the unmodified reference before
anything is compared with it.
"""

import numpy as np


def _rfft2(a, s=None):
    return np.fft.rfftn(a, s=s, axes=(0, 1))


def _irfft2(a, shape):
    return np.fft.irfftn(a, s=shape, axes=(0, 1))


def grad(r):
    """(G_0 r, G_1 r) on a new last axis: r minus its circular predecessor along the axis."""
    return np.stack([r - np.roll(r, 1, axis=0), r - np.roll(r, 1, axis=1)], axis=-1)


def grad_adj(v1):
    """sum_i G_i^T v1_i: each component minus its circular successor along its axis."""
    return (v1[..., 0] - np.roll(v1[..., 0], -1, axis=0)) + (v1[..., 1] - np.roll(v1[..., 1], -1, axis=1))


def ghg(shape):
    H, W = shape
    gh = 2.0 - 2.0 * np.cos(2.0 * np.pi * np.arange(H) / H)
    gw = 2.0 - 2.0 * np.cos(2.0 * np.pi * np.arange(W // 2 + 1) / W)
    return (gh[:, None] + gw[None, :]).reshape(H, W // 2 + 1, 1, 1, 1)


def pweights(shape):
    """Half-spectrum weights of fft.rfl2norm2, divided by H W."""
    H, W = shape
    w = np.full(W // 2 + 1, 2.0)
    w[0] = 1.0
    if W % 2 == 0:
        w[-1] = 1.0
    return w.reshape(1, -1, 1, 1, 1) / (H * W)


def is_uniform(wtv, K):
    w = np.broadcast_to(np.asarray(wtv, dtype=np.float64).ravel(), (K,)) if np.size(wtv) in (1, K) else None
    return bool(np.all(w == w[0])), w


def xstep(Df, Sf, Yf0, Uf0, Zyf, Zuf, wtv, rho, shape, u_scale=1.0, check=False):
    """(B^H diag(1, tau) B + rho I) x = rho yu + B^H (Sf; rho zd), B = [Df^T; (w Df)^T], tau = rho GHG.
    Zyf / Zuf (H, Wf, C, N, 1): spectra of grad_adj of the gradient blocks.  Returns Xf, X, and
    rw = irfftn(sum_m w_m Df_m Xf_m); with ``check`` also the relative residual of the system."""
    K = Df.shape[-1]
    uni, w = is_uniform(wtv, K)
    w5 = w.reshape(1, 1, 1, 1, K)
    yu = Yf0 - u_scale * Uf0
    zd = Zyf - u_scale * Zuf
    tau = rho * ghg(shape)
    g = np.sum(np.abs(Df) ** 2, axis=4, keepdims=True)
    p1 = np.sum(Df * yu, axis=4, keepdims=True)
    if uni:
        w0 = w[0]
        c = 1.0 + tau * w0 * w0
        coef = (Sf + rho * w0 * zd - c * p1) / (rho + c * g)
        Xf = yu + np.conj(Df) * coef
    else:
        p2 = np.sum(w5 * Df * yu, axis=4, keepdims=True)
        gw = np.sum(w5 * np.abs(Df) ** 2, axis=4, keepdims=True)
        gww = np.sum(w5 ** 2 * np.abs(Df) ** 2, axis=4, keepdims=True)
        r1, r2 = Sf - p1, rho * zd - tau * p2
        m11, m12, m21, m22 = g + rho, gw, tau * gw, tau * gww + rho
        det = m11 * m22 - m12 * m21
        v1, v2 = (m22 * r1 - m12 * r2) / det, (m11 * r2 - m21 * r1) / det
        Xf = yu + np.conj(Df) * (v1 + w5 * v2)
    dx = np.sum(Df * Xf, axis=4, keepdims=True)
    dxw = np.sum(w5 * Df * Xf, axis=4, keepdims=True)
    out = [Xf, _irfft2(Xf, shape), _irfft2(dxw, shape)[..., 0]]
    if check:
        ax = np.conj(Df) * (dx + tau * w5 * dxw) + rho * Xf
        b = rho * yu + np.conj(Df) * (Sf + rho * w5 * zd)
        out.append(np.linalg.norm(ax - b) / max(np.linalg.norm(ax), np.linalg.norm(b)))
    return out


def prox_l2(v, alpha, axis):
    a = np.sqrt(np.sum(v ** 2, axis=axis, keepdims=True))
    b = np.maximum(0.0, a - alpha)
    s = np.where(a == 0.0, 0.0, b / np.where(a == 0.0, 1.0, a))
    return s * v


def ystep(X, rw, Y, U, wl1, lmbda, mu, rho, rlx, gevaly, u_scale=1.0):
    """relax_AX + ystep + ustep on the block-concatenated Y, U (H, W, C, N, K + 2) and the sums the
    device returns."""
    K = X.shape[-1]
    AXnr = np.concatenate((X, grad(rw)), axis=-1)
    AX = AXnr if rlx == 1.0 else rlx * AXnr + (1.0 - rlx) * Y
    V = AX + u_scale * U
    Yn = np.empty_like(V)
    Yn[..., :K] = np.sign(V[..., :K]) * np.maximum(0.0, np.abs(V[..., :K]) - (lmbda / rho) * wl1)
    # the l2 norm runs over the channel axis and the two gradient components (cbpdntv.py:1105-1106)
    Yn[..., K:] = prox_l2(V[..., K:], mu / rho, (2, 4))
    Un = V - Yn
    Gv = Yn if gevaly else AXnr
    return dict(Y=Yn, U=Un, AXnr=AXnr, r2=np.sum((AXnr - Yn) ** 2), ax2=np.sum(AXnr ** 2), y2=np.sum(Yn ** 2),
                l1=np.sum(np.abs(wl1 * Gv[..., :K])), tv=np.sum(np.sqrt(np.sum(Gv[..., K:] ** 2, axis=(2, 4)))))


def spectra(Yb, K):
    """rfftn of the coefficient block and of the adjoint map of the gradient block."""
    return _rfft2(Yb[..., :K]), _rfft2(grad_adj(Yb[..., K:]))[..., None]


def at_norm2(Vf0, Zf, Df, wtv, shape):
    """||A^T v||^2 = ||v0 + Gamma^T v1||^2 in the frequency domain: rfftn(Gamma^T v1)_m = conj(w_m Df_m) Zf."""
    K = Df.shape[-1]
    w5 = is_uniform(wtv, K)[1].reshape(1, 1, 1, 1, K)
    return float(np.sum(pweights(shape) * np.abs(Vf0 + np.conj(w5 * Df) * Zf) ** 2))


def dfid(Df, Sf, Vf, shape):
    Ef = np.sum(Df * Vf, axis=4, keepdims=True) - Sf
    return float(np.sum(pweights(shape) * np.abs(Ef) ** 2)) / 2.0


def iterate(st, Df, Sf, wtv, wl1, lmbda, mu, rlx, gevaly, fevalx, auto_rho, k, shape, std_residuals=False,
            check=False):
    """One iteration of admm.ADMM.solve (admm.py:331-367) on the state dict ``st`` (Y, U, rho and the
    spectra Yf0, Zyf, Uf0, Zuf of the blocks); returns the IterationStats values."""
    K = Df.shape[-1]
    rho = st['rho']
    if 'Yf0' not in st:
        st['Yf0'], st['Zyf'] = spectra(st['Y'], K)
        st['Uf0'], st['Zuf'] = spectra(st['U'], K)
    res = xstep(Df, Sf, st['Yf0'], st['Uf0'], st['Zyf'], st['Zuf'], wtv, rho, shape, check=check)
    Xf, X, rw = res[:3]
    ys = ystep(X, rw, st['Y'], st['U'], wl1, lmbda, mu, rho, rlx, gevaly)
    Y, U = ys['Y'], ys['U']
    Yf0, Zyf = spectra(Y, K)
    Uf0, Zuf = spectra(U, K)
    ns = rho * np.sqrt(at_norm2(Yf0 - st['Yf0'], Zyf - st['Zyf'], Df, wtv, shape))
    sn = rho * np.sqrt(at_norm2(Uf0, Zuf, Df, wtv, shape))
    nr, rn = np.sqrt(ys['r2']), max(np.sqrt(ys['ax2']), np.sqrt(ys['y2']))
    if std_residuals:
        r, s = nr, ns
    else:
        r, s = nr / (rn or 1.0), ns / (sn or 1.0)
    dfd = dfid(Df, Sf, Xf if fevalx else Yf0, shape)
    rec = dict(ObjFun=dfd + lmbda * ys['l1'] + mu * ys['tv'], DFid=dfd, RegL1=ys['l1'], RegTV=ys['tv'],
               PrimalRsdl=r, DualRsdl=s, EpsPrimal=0.0, EpsDual=0.0, Rho=rho)
    if check:
        rec['XSlvRelRes'] = res[3]
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
        Uf0, Zuf = Uf0 / rsf, Zuf / rsf
    st.update(X=X, Y=Y, U=U, rho=rho, Yf0=Yf0, Zyf=Zyf, Uf0=Uf0, Zuf=Zuf)
    return rec


def admm_rtv(D, S, lmbda, mu, maxiter, wtv=1.0, wl1=1.0, rho=None, rlx=1.8, auto_rho=True, gevaly=False,
             fevalx=True, Y0=None, U0=None, std_residuals=False, check=False):
    """The whole solve, RelStopTol = 0 (EpsPrimal = EpsDual = 0): D (dH, dW, 1, 1, K), S (H, W, C, N, 1),
    float64; ``wtv`` a scalar or K weights."""
    D = np.asarray(D, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    H, W = S.shape[:2]
    K = D.shape[-1]
    shpY = (H, W, S.shape[2], S.shape[3], K + 2)
    Sf, Df = _rfft2(S), _rfft2(D, (H, W))
    st = dict(Y=np.zeros(shpY) if Y0 is None else np.array(Y0, dtype=np.float64),
              U=np.zeros(shpY) if U0 is None else np.array(U0, dtype=np.float64),
              rho=1.0 if rho is None else float(rho))   # (the reference's effective default)
    tr = {}
    for k in range(maxiter):
        rec = iterate(st, Df, Sf, wtv, wl1, lmbda, mu, rlx, gevaly, fevalx, auto_rho, k, (H, W), std_residuals, check)
        for key, val in rec.items():
            tr.setdefault(key, []).append(float(val))
    out = {key: np.array(val) for key, val in tr.items()}
    out.update(X=st['X'], Y=st['Y'], U=st['U'], rho=st['rho'], Df=Df,
               recon=_irfft2(np.sum(Df * _rfft2(st['X']), axis=4), (H, W)))
    return out
