"""NumPy restatement (float64, FFT-based like the reference) of the inhibition-weight update of
ConvBPDNInhib (sporco/admm/cbpdnin.py:294-352) and of the solver around it, on the 5-D arrays
(H, W, C, N, K) of this project.  TEST INFRASTRUCTURE ONLY: pinned to the reference's fixtures
by tests/test_cbpdnin.py and then used where no reference exists (C-ABI and GPU-size cases)."""

import numpy as np

from oracle import cbpdn_oracle as orc


def window_taps(Whn, dimN=2, win_args=('tukey', 0.5)):
    """(taps along H, taps along W) of the reference's window (cbpdnin.py:253-274)."""
    from scipy import signal
    Whn = int(Whn) + (not int(Whn) % 2)
    t = np.power(np.asarray(signal.get_window(win_args, Whn), dtype=np.float64), 1.0 / dimN)
    return (np.ones(1) if dimN == 1 else t), t


def window_array(H, W, taps_h, taps_w):
    """The window on the (H, W) grid: tap (t, s) at offset (t - nth // 2, s - ntw // 2), circularly."""
    h = np.zeros((H, W))
    oh, ow = len(taps_h) // 2, len(taps_w) // 2
    for t, a in enumerate(taps_h):
        for s, b in enumerate(taps_w):
            h[(t - oh) % H, (s - ow) % W] += a * b
    return h


def inhib_update(X, G, wl1, wml, wms, Wg, taps_h, taps_w, lmbda, mu, gamma, smooth):
    """One update.  Returns dict(wml, wms, T, rl, rm, rg); wml / wms pass through unchanged (0
    for None) when their term is off (mu <= 0 or Wg None; gamma <= 0)."""
    X = np.asarray(X, dtype=np.float64)
    H, W = X.shape[:2]
    h = window_array(H, W, np.asarray(taps_h, float), np.asarray(taps_w, float))
    hs = h.copy()
    hs[0, 0] = 0.0
    ax = (0, 1)
    Xaf = np.fft.rfftn(np.abs(X), axes=ax)
    shp = (H, W // 2 + 1, 1, 1, 1)
    wml = 0.0 if wml is None else wml
    wms = 0.0 if wms is None else wms
    if mu > 0 and Wg is not None:
        Wg = np.asarray(Wg, dtype=np.float64)
        c = np.fft.irfftn(np.fft.rfftn(h, axes=ax).reshape(shp) * Xaf, (H, W), axes=ax)
        lat = np.dot(np.dot(c, Wg.T), Wg) - np.sum(Wg, axis=0) * c
        wml = smooth * wml + (1 - smooth) * lat
    if gamma > 0:
        sf = np.fft.irfftn(np.fft.rfftn(hs, axes=ax).reshape(shp) * Xaf, (H, W), axes=ax)
        wms = smooth * wms + (1 - smooth) * sf
    G = np.asarray(G, dtype=np.float64)
    return dict(wml=wml, wms=wms, T=lmbda * wl1 + mu * wml + gamma * wms + 0.0 * X,
                rl=np.sum(np.abs(wl1 * G)), rm=np.sum(np.abs(wml * G)), rg=np.sum(np.abs(wms * G)))


def admm_inhib(D, S, Wg, taps_h, taps_w, lmbda, mu, gamma, maxiter, smooth=0.9, wl1=1.0, rho=None,
               rlx=1.8, auto_rho=True, nonneg=False, nobndry=False, gevaly=False, fevalx=True):
    """ConvBPDNInhib with the default AutoRho settings of ConvBPDN.Options (or a fixed rho),
    RelStopTol = 0: D (dH, dW, 1, 1, K), S (H, W, C, N, 1), float64.  The loop is
    oracle.cbpdn_oracle.admm_cbpdn's with the y step / objective of cbpdnin.py."""
    D = np.asarray(D, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    H, W = S.shape[:2]
    K = D.shape[-1]
    shpX = (H, W, S.shape[2], S.shape[3], K)
    Nx = int(np.prod(shpX))
    rho = 50.0 * lmbda + 1.0 if rho is None else float(rho)
    rho_xi, rho_tau, rho_mu = orc.default_rho_xi(lmbda), 1000.0, 1.2
    Sf, Df = orc.rfftn2(S), orc.rfftn2(D, (H, W))
    DSf = np.conj(Df) * Sf
    Y, U = np.zeros(shpX), np.zeros(shpX)
    wml = wms = 0.0
    tr = {k: [] for k in ('ObjFun', 'DFid', 'RegL1', 'RegLat', 'RegSelf', 'PrimalRsdl', 'DualRsdl',
                          'EpsPrimal', 'EpsDual', 'Rho')}
    for k in range(maxiter):
        Yprev = Y.copy()
        Xf = orc.solvedbi_sm(Df, rho, DSf + rho * orc.rfftn2(Y - U), None, orc.AX_K)
        X = orc.irfftn2(Xf, (H, W))
        AX = X if rlx == 1.0 else rlx * X + (1 - rlx) * Y
        Y = orc.prox_l1(AX + U, (lmbda * wl1 + mu * wml + gamma * wms) / rho)
        if nonneg:
            Y[Y < 0.0] = 0.0
        if nobndry:
            Y[1 - D.shape[0]:] = 0.0
            Y[:, 1 - D.shape[1]:] = 0.0
        U = U + (AX - Y)
        up = inhib_update(X, Y if gevaly else X, wl1, wml, wms, Wg, taps_h, taps_w, lmbda, mu, gamma,
                          smooth)
        wml, wms = up['wml'], up['wms']
        nAX, nY = np.linalg.norm(X), np.linalg.norm(Y)
        rn = max(nAX, nY) or 1.0
        sn = rho * np.linalg.norm(U) or 1.0
        r, s = np.linalg.norm(X - Y) / rn, np.linalg.norm(rho * (Yprev - Y)) / sn
        fvar = Xf if fevalx else orc.rfftn2(Y)
        dfd = orc.rfl2norm2(orc.inner(Df, fvar, axis=orc.AX_K) - Sf, S.shape) / 2.0
        obj = dfd + lmbda * up['rl'] + mu * up['rm'] + gamma * up['rg']
        for key, val in (('ObjFun', obj), ('DFid', dfd), ('RegL1', up['rl']), ('RegLat', up['rm']),
                         ('RegSelf', up['rg']), ('PrimalRsdl', r), ('DualRsdl', s), ('EpsPrimal', 0.0),
                         ('EpsDual', 0.0), ('Rho', rho)):
            tr[key].append(float(val))
        if auto_rho and k != 0:
            if s == 0.0 or r == 0.0:
                rhomlt = rho_tau
            else:
                rhomlt = min(np.sqrt(r / (s * rho_xi) if r > s * rho_xi else (s * rho_xi) / r), rho_tau)
            rsf = 1.0
            if r > rho_xi * rho_mu * s:
                rsf = rhomlt
            elif s > (rho_mu / rho_xi) * r:
                rsf = 1.0 / rhomlt
            rho = rho * rsf
            U = U / rsf
    out = {key: np.array(val) for key, val in tr.items()}
    out.update(X=X, Y=Y, U=U, wml=wml, wms=wms, rho=rho, Df=Df)
    return out
