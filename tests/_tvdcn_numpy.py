"""NumPy statement of the TV deconvolution ADMM iterations (sporco_amd.admm.tvl2.TVL2Deconv and
sporco_amd.admm.tvl1.TVL1Deconv), written from the formulas with numpy.fft:

    H x     : circular convolution with the kernel A, phase of fftconv: irfft2(Af rfft2(x)), Af = rfft2(A, (H, W))
    G_k     : circular difference, (G_k x)[n] = x[n] - x[n - 1];  (G_k^T v)[n] = v[n] - v[n + 1]
    GHGf    : (2 - 2 cos(2 pi k / H)) + (2 - 2 cos(2 pi l / W))
    l2: constraint (G_0; G_1) x = y
        x step  : Xf = (conj(Af) Sf + rho F(G^T (Y - U))) / (|Af|^2 + rho GHGf)
        y step  : Y = shrink_2(AX + U, (lmbda / rho) Wtv)
        s = rho ||G^T (Y - Yprev)||, sn = rho ||G^T U||, DFid = (1/2) ||H X - S||^2 (over spectra, Parseval)
    l1: constraint (G_0; G_1; H) x - y = (0; 0; s)
        x step  : Xf = (conj(Af) Sf + F(G^T (Y_g - U_g)) + conj(Af) F(Y_d - U_d)) / (|Af|^2 + GHGf)
        y step  : Y_g as above, Y_d = soft(AX_d + U_d - S, Wdf / rho)
        s = rho ||G^T U_g + H^T U_d||, sn = rho ||U||, DFid = sum |Wdf g_d|, g = Y or A X - c
    relax   : AX = alpha A X + (1 - alpha) (Y + c);  u step: U += AX - Y - c
    r = ||A X - Y - c||, rn = max(||A X||, ||Y||, ||c||);  RegTV = sum Wtv sqrt(sum g_g^2)
    XSlvRelRes: ||den Xf - b|| / max(||den Xf||, ||b||) over the half spectrum
    U from a Y0 alone: U_g = (lmbda / rho) Y_g / ||Y_g|| (0 at norm 0), U_d = sign(Y_d) / rho.

Every array and scalar is kept in ``dtype`` (the spectra in its complex type), so that the statement can run
in float32.
"""

import numpy as np


def pgrad(x, ax):
    return x - np.roll(x, 1, axis=ax)


def pgrad_t(v, ax):
    return v - np.roll(v, -1, axis=ax)


def shrink2(v, alpha, axes):
    n = np.sqrt(np.sum(v * v, axis=axes, keepdims=True))
    f = np.divide(np.maximum(n - alpha, 0), n, out=np.zeros_like(n), where=(n != 0))
    return (f * v).astype(v.dtype)


def soft(v, alpha):
    return (np.sign(v) * np.maximum(np.abs(v) - alpha, 0)).astype(v.dtype)


def tv_deconv(kind, A, S, lmbda, iters, rho=None, rlx=1.8, wdf=1.0, wtv=1.0, caxis=None, geval_y=True, ar=None,
              std_residuals=False, lin_solve_check=False, Y0=None, U0=None, abs_tol=0.0, rel_tol=0.0,
              dtype=np.float64):
    """``kind``: 'l2' or 'l1'.  ``ar``: None, or dict(Period, Scaling, RsdlRatio, AutoScaling, RsdlTarget).
    Returns the final X, Y, U, rho and the traces."""
    t = np.dtype(dtype).type
    ct = np.complex64 if np.dtype(dtype) == np.float32 else np.complex128
    l1 = kind == 'l1'
    nb = 3 if l1 else 2
    S = np.asarray(S, dtype=dtype)
    Hh, Ww = S.shape[:2]
    A = np.asarray(A, dtype=dtype)
    A = A.reshape(A.shape + (1,) * (S.ndim - A.ndim))

    def fwd(x, s=None):
        return np.fft.rfftn(x, s=s, axes=(0, 1)).astype(ct)

    def inv(xf):
        return np.fft.irfftn(xf, s=(Hh, Ww), axes=(0, 1)).astype(dtype)

    lmbda = t(lmbda)
    rho = t(2.0 * lmbda + 0.1) if rho is None else t(rho)
    rlx = t(rlx)
    wdf = np.asarray(wdf, dtype=dtype)
    wtv = np.asarray(wtv, dtype=dtype)
    wtv_y = wtv[..., np.newaxis] if wtv.ndim == S.ndim else wtv
    naxes = (caxis, -1) if caxis is not None else (-1,)
    Af, Sf = fwd(A, (Hh, Ww)), fwd(S)
    aha = (Af.real * Af.real + Af.imag * Af.imag).astype(dtype)
    ahsf = (np.conj(Af) * Sf).astype(ct)
    kk = np.arange(Hh).reshape((Hh, 1) + (1,) * (S.ndim - 2))
    ll = np.arange(Ww // 2 + 1).reshape((1, -1) + (1,) * (S.ndim - 2))
    ghg = ((2 - 2 * np.cos(2 * np.pi * kk / Hh)) + (2 - 2 * np.cos(2 * np.pi * ll / Ww))).astype(dtype)
    pw = np.full(Ww // 2 + 1, 2.0)
    pw[0] = 1.0
    if Ww % 2 == 0:
        pw[-1] = 1.0
    pw = pw.reshape(ll.shape)

    Y = np.zeros(S.shape + (nb,), dtype) if Y0 is None else np.asarray(Y0, dtype=dtype).copy()
    if U0 is not None:
        U = np.asarray(U0, dtype=dtype).copy()
    elif Y0 is not None:
        Yg = Y[..., :2]
        n = np.sqrt(np.sum(Yg * Yg, axis=-1, keepdims=True))
        U = (lmbda / rho) * np.divide(Yg, n, out=np.zeros_like(Yg), where=(n != 0))
        if l1:
            U = np.concatenate((U, (t(1) / rho) * np.sign(Y[..., 2:])), axis=-1)
        U = U.astype(dtype)
    else:
        U = np.zeros_like(Y)
    c = np.zeros_like(Y)
    if l1:
        c[..., 2] = S
    nc = float(np.linalg.norm(S.ravel())) if l1 else 0.0
    Nx, Nc = S.size, Y.size

    def gt(v):
        return pgrad_t(v[..., 0], 0) + pgrad_t(v[..., 1], 1)

    keys = ('ObjFun', 'DFid', 'RegTV', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho', 'XSlvRelRes')
    tr = {k: [] for k in keys}
    X = np.zeros_like(S)
    for k in range(iters):
        YU = (Y - U).astype(dtype)
        if l1:
            b = (ahsf + fwd(gt(YU))) + np.conj(Af) * fwd(YU[..., 2])
            den = aha + ghg
        else:
            b = ahsf + rho * fwd(gt(YU))
            den = aha + rho * ghg
        b = b.astype(ct)
        Xf = (b / den).astype(ct)
        HXf = (Af * Xf).astype(ct)
        X = inv(Xf)
        xrrs = np.nan
        if lin_solve_check:
            ax = (den * Xf).astype(ct)
            nrm = max(np.linalg.norm(ax.ravel()), np.linalg.norm(b.ravel()))
            xrrs = 0.0 if nrm == 0 else float(np.linalg.norm((ax - b).ravel()) / nrm)
        parts = [pgrad(X, 0), pgrad(X, 1)] + ([inv(HXf)] if l1 else [])
        AXnr = np.stack(parts, axis=-1)
        AX = AXnr if rlx == 1 else (rlx * AXnr + (1 - rlx) * (Y + c)).astype(dtype)
        V = AX + U
        Yprev = Y
        Yg = shrink2(V[..., :2], (lmbda / rho) * wtv_y, naxes)
        if l1:
            Y = np.concatenate((Yg, soft(V[..., 2] - S, (t(1) / rho) * wdf)[..., np.newaxis]), axis=-1).astype(dtype)
        else:
            Y = Yg
        U = (U + ((AX - Y) - c)).astype(dtype)
        # objective
        g = Y if geval_y else AXnr - c
        if l1:
            dfid = float(np.sum(np.abs(wdf * g[..., 2])))
        else:
            e = HXf - Sf
            dfid = 0.5 * float(np.sum(pw * (e.real.astype(np.float64) ** 2 + e.imag.astype(np.float64) ** 2))) / (Hh * Ww)
        reg = float(np.sum(wtv * np.sqrt(np.sum(g[..., :2] * g[..., :2], axis=naxes))))
        # residuals
        nr = float(np.linalg.norm(((AXnr - Y) - c).ravel()))
        rn = float(max(np.linalg.norm(AXnr.ravel()), np.linalg.norm(Y.ravel()), nc))
        if l1:
            atu = gt(U) + inv(np.conj(Af) * fwd(U[..., 2]))
            ns = float(rho * np.linalg.norm(atu.ravel()))
            sn = float(rho * np.linalg.norm(U.ravel()))
        else:
            ns = float(rho * np.linalg.norm(gt(Y - Yprev).ravel()))
            sn = float(rho * np.linalg.norm(gt(U).ravel()))
        if std_residuals:
            r, s = nr, ns
            epri = np.sqrt(Nc) * abs_tol + rn * rel_tol
            edua = np.sqrt(Nx) * abs_tol + sn * rel_tol
        else:
            rn = 1.0 if rn == 0.0 else rn
            sn = 1.0 if sn == 0.0 else sn
            r, s = nr / rn, ns / sn
            epri = np.sqrt(Nc) * abs_tol / rn + rel_tol
            edua = np.sqrt(Nx) * abs_tol / sn + rel_tol
        for key, val in zip(keys, (dfid + float(lmbda) * reg, dfid, reg, r, s, epri, edua, float(rho), xrrs)):
            tr[key].append(val)
        # rho update
        if ar is not None and k != 0 and (k + 1) % ar['Period'] == 0:
            tau, mu, xi = ar['Scaling'], ar['RsdlRatio'], ar['RsdlTarget']
            if ar['AutoScaling']:
                if s == 0.0 or r == 0.0:
                    mlt = tau
                else:
                    mlt = min(np.sqrt(r / (s * xi) if r > s * xi else (s * xi) / r), tau)
            else:
                mlt = tau
            rsf = mlt if r > xi * mu * s else (1.0 / mlt if s > (mu / xi) * r else 1.0)
            rho = t(rho * t(rsf))
            U = (U / t(rsf)).astype(dtype)
        if r < epri and s < edua:
            break
    out = {k: np.asarray(v, dtype=np.float64) for k, v in tr.items()}
    out.update(X=X, Y=Y, U=U, rho=float(rho))
    return out


def from_golden(kind, g, iters=None, dtype=np.float64, **over):
    """Run the statement on the inputs and options of a fixture written by tools/make_golden_tvdcn.py."""
    ar = None
    if int(g['opt_AutoRho']):
        ar = dict(Period=int(g['opt_AutoRho_Period']), Scaling=float(g['opt_AutoRho_Scaling']),
                  RsdlRatio=float(g['opt_AutoRho_RsdlRatio']), AutoScaling=bool(g['opt_AutoRho_AutoScaling']),
                  RsdlTarget=float(g['opt_AutoRho_RsdlTarget']))
    kw = dict(rho=float(g['opt_rho']), rlx=float(g['opt_RelaxParam']), wdf=g.get('optarr_DFidWeight', 1.0),
              wtv=g.get('optarr_TVWeight', 1.0), caxis=None if int(g['caxis']) < 0 else int(g['caxis']),
              geval_y=bool(g['opt_gEvalY']), ar=ar, std_residuals=bool(g['opt_StdResiduals']),
              lin_solve_check=bool(g['opt_LinSolveCheck']), Y0=g.get('optarr_Y0'), U0=g.get('optarr_U0'), dtype=dtype)
    kw.update(over)
    return tv_deconv(kind, g['A'], g['S'], float(g['lmbda']), int(g['MaxMainIter']) if iters is None else iters, **kw)
