"""TEST INFRASTRUCTURE ONLY: NumPy restatement of ConvL1L1Grd (sporco/admm/cbpdn.py:2488-2774 on
ConvTwoBlockCnstrnt :1401-1826 and admm.ADMMTwoBlockCnstrnt) AS BUILT in sporco_amd
(csrc/csc_l1l1.h): the gradient-regularised x step with rho = 1 and mu / rho in mu's place, the soft
threshold of both blocks, and the dual residual of this class taken in the frequency domain.

Arrays are five-dimensional: the signal and block 0 (H, W, C, N, 1), the dictionary (dH, dW, Cd, 1,
K), the coefficient maps and block 1 (H, W, Cx, N, K) with Cx = C for a single-channel dictionary
and 1 for a multi-channel one.  ``dtype`` is the precision of every array and scalar of the
iteration (float64, or float32 for the measured float32 tolerance of tests/test_l1l1.py); the sums
behind the statistics are taken in float64 either way, as on the device.  tests/test_l1l1.py pins
this file to states recorded from the unmodified reference before anything is compared with it.
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


def ghg(shape):
    """sum_i |G_i|^2 of the two-tap difference filters (signal.gradient_filters): (H, Wf, 1, 1, 1)."""
    H, W = shape
    gh = 2.0 - 2.0 * np.cos(2.0 * np.pi * np.arange(H) / H)
    gw = 2.0 - 2.0 * np.cos(2.0 * np.pi * np.arange(W // 2 + 1) / W)
    return (gh[:, None] + gw[None, :]).reshape(H, W // 2 + 1, 1, 1, 1)


def soft(v, t):
    return np.sign(v) * np.maximum(0, np.abs(v) - t)


def a0(Df, Vf):
    """D v: sum over the filters, (H, Wf, C, N, 1)."""
    return np.sum(Df * Vf, axis=4, keepdims=True)


def a0t(Df, V0f):
    """D^H v0: conj(Df) v0, summed over the channels of a multi-channel dictionary."""
    r = np.conj(Df) * V0f
    return np.sum(r, axis=2, keepdims=True) if Df.shape[2] > 1 else r


def solve(Df, g, b):
    """(D^H D + diag(g)) x = b per frequency and image, by the Woodbury identity over the Cd rows of
    D (Cd = 1: linalg.solvedbd_sm; Cd > 1: what linalg.solvemdbi_ism iterates)."""
    H, Wf, Cd, _, K = Df.shape
    A = Df[:, :, :, 0, :]
    gi = 1.0 / np.broadcast_to(g, (H, Wf, 1, 1, K))[:, :, 0, 0, :]
    b2 = b.reshape(H, Wf, -1, K)
    t = np.einsum('hwck,hwk,hwnk->hwcn', A, gi, b2)
    M = np.eye(Cd) + np.einsum('hwck,hwk,hwdk->hwcd', A, gi, np.conj(A))
    z = np.linalg.solve(M, t)
    x = gi[:, :, None, :] * (b2 - np.einsum('hwck,hwcn->hwnk', np.conj(A), z))
    return x.reshape(b.shape)


def rho_factor(k, r, s, ar):
    """admm.py:552-571.  ``ar``: the AutoRho options (Period, Scaling, RsdlRatio, AutoScaling,
    RsdlTarget), or None when disabled."""
    if ar is None or k == 0 or (k + 1) % ar['Period'] != 0:
        return 1.0
    tau, mu, xi = ar['Scaling'], ar['RsdlRatio'], ar['RsdlTarget']
    if ar['AutoScaling']:
        if s == 0.0 or r == 0.0:
            mlt = tau
        else:
            mlt = min(np.sqrt(r / (s * xi) if r > s * xi else (s * xi) / r), tau)
    else:
        mlt = tau
    if r > xi * mu * s:
        return mlt
    if s > (mu / xi) * r:
        return 1.0 / mlt
    return 1.0


AUTORHO_DEFAULT = {'Period': 10, 'Scaling': 2.0, 'RsdlRatio': 10.0, 'AutoScaling': False, 'RsdlTarget': 1.0}


def iterate(st, Df, S, W, wl1, wg, lmbda, mu, rlx, auxvar, ar, k, shape, dsz, nonneg=False, nobndry=False,
            check=False):
    """One iteration of admm.ADMM.solve (admm.py:331-367) on the state dict ``st`` (Y0, Y1, U0, U1,
    rho); returns the IterationStats values."""
    dt = S.dtype
    ct = np.complex64 if dt == np.float32 else np.complex128
    f8 = lambda a: np.asarray(a, dtype=np.float64 if np.isrealobj(a) else np.complex128)
    nrm = lambda a: float(np.sqrt(np.sum(np.abs(f8(a)) ** 2)))
    rho = dt.type(st['rho'])
    rlx = dt.type(rlx)
    Y0p, Y1p, U0, U1 = st['Y0'], st['Y1'], st['U0'], st['U1']
    G = (wg * ghg(shape)).astype(dt)
    b = (a0t(Df, _rfft2(Y0p - U0 + S).astype(ct)) + _rfft2(Y1p - U1).astype(ct)).astype(ct)
    g = (dt.type(mu) / rho) * G + dt.type(1)
    Xf = solve(Df, g, b).astype(ct)
    X = _irfft2(Xf, shape).astype(dt)
    AX0nr = _irfft2(a0(Df, Xf), shape).astype(dt)
    if rlx == 1.0:
        AX0, AX1 = AX0nr, X
    else:
        AX0 = rlx * AX0nr + (1 - rlx) * (Y0p + S)
        AX1 = rlx * X + (1 - rlx) * Y1p
    Y0 = soft(AX0 + U0 - S, (dt.type(1) / rho) * W).astype(dt)
    Y1 = soft(AX1 + U1, (dt.type(lmbda) / rho) * wl1).astype(dt)
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

    def at_norm(V0, V1):
        return float(np.sqrt(np.sum(pw * np.abs(f8(a0t(Df, _rfft2(V0).astype(ct)) + _rfft2(V1).astype(ct))) ** 2)))

    ns = float(rho) * at_norm(Y0p - Y0, Y1p - Y1)
    sn = float(rho) * at_norm(U0, U1)
    r, s = nr / (rn or 1.0), ns / (sn or 1.0)
    g0 = Y0 if auxvar else AX0nr - S
    g1 = Y1 if auxvar else X
    dfd = float(np.sum(np.abs(f8(W * g0))))
    rl1 = float(np.sum(np.abs(f8(wl1 * g1))))
    rgr = float(np.sum(pw * f8(G) * np.abs(f8(Xf)) ** 2)) / 2.0
    rec = dict(ObjFun=dfd + float(lmbda) * rl1 + float(mu) * rgr, DFid=dfd, RegL1=rl1, RegGrad=rgr, PrimalRsdl=r,
               DualRsdl=s, EpsPrimal=0.0, EpsDual=0.0, Rho=float(rho))
    if check:
        ax = a0t(Df, a0(Df, Xf)) + g * Xf
        rec['XSlvRelRes'] = nrm(ax - b) / max(nrm(ax), nrm(b))
    rsf = dt.type(rho_factor(k, r, s, ar))
    st.update(X=X, Xf=Xf, Y0=Y0, Y1=Y1, U0=(U0 / rsf).astype(dt), U1=(U1 / rsf).astype(dt), rho=rho * rsf)
    return rec


def block_cat(V0, V1):
    """[block 0; block 1] on the filter axis, block 0 swapped there when it has channels of its own
    that block 1 has not (cbpdn.py:1700-1715)."""
    if V0.shape[2] != V1.shape[2]:
        V0 = np.swapaxes(V0, 2, 4)
    return np.concatenate((V0, V1), axis=4)


def admm_l1l1(D, S, lmbda, mu, maxiter, W=1.0, wl1=1.0, wg=1.0, rho=1.0, rlx=1.8, auxvar=False, ar=None,
              nonneg=False, nobndry=False, check=False, dtype=np.float64, state=None, k0=0):
    """The whole solve, RelStopTol = 0 (EpsPrimal = EpsDual = 0).  D (dH, dW, Cd, 1, K), S (H, W, C, N,
    1); W broadcastable against S, wl1 against the coefficient maps, wg a scalar or (K,)."""
    dt = np.dtype(dtype)
    ct = np.complex64 if dt == np.float32 else np.complex128
    D = np.asarray(D, dtype=dt)
    S = np.asarray(S, dtype=dt)
    W = np.asarray(W, dtype=dt)
    wl1 = np.asarray(wl1, dtype=dt)
    wg = np.asarray(wg, dtype=dt)
    H, Wd = S.shape[:2]
    Cd, K = D.shape[2], D.shape[4]
    shpX = (H, Wd, 1 if Cd > 1 else S.shape[2], S.shape[3], K)
    Df = _rfft2(D, (H, Wd)).astype(ct)
    st = state or dict(Y0=np.zeros(S.shape, dt), Y1=np.zeros(shpX, dt), U0=np.zeros(S.shape, dt),
                       U1=np.zeros(shpX, dt), rho=dt.type(rho))
    tr = {}
    for k in range(k0, k0 + maxiter):
        rec = iterate(st, Df, S, W, wl1, wg, lmbda, mu, rlx, auxvar, ar, k, (H, Wd), D.shape[:2], nonneg, nobndry,
                      check)
        for key, val in rec.items():
            tr.setdefault(key, []).append(float(val))
    out = {key: np.array(val) for key, val in tr.items()}
    out.update(X=st['X'], Y0=st['Y0'], Y1=st['Y1'], U0=st['U0'], U1=st['U1'], Y=block_cat(st['Y0'], st['Y1']),
               U=block_cat(st['U0'], st['U1']), rho=float(st['rho']),
               recon=_irfft2(a0(Df, st['Xf']), (H, Wd))[..., 0], state=st)
    return out
