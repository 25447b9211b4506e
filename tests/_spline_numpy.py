"""NumPy statement of the orthonormal DCT-II through ONE real transform of the same size (Makhoul's reordering)
and of the l1-spline ADMM iteration (sporco_amd.admm.spline.SplineL1), written from the formulas with numpy.fft.

The DCT over axes (0, 1) of an (H, W, ...) array:

    permutation, along an axis of length N:  v[n] = x[2 n], n < ceil(N / 2);  v[N - 1 - n] = x[2 n + 1], n < N // 2
    forward:  Vh = rfft2(v);  w_j[k] = exp(-i pi k / (2 N_j));  a = Vh[k1, k2], b = Vh[(H - k1) mod H, k2]
        Xu[k1, k2]     = 2 Re(w1[k1] (w2[k2] a + conj(w2[k2]) conj(b)))
        Xu[k1, W - k2] = 2 Re(w1[k1] (w2[W - k2] conj(b) + conj(w2[W - k2]) a)),   0 < k2 < W - k2
        X = Xu s1[k1] s2[k2],   s_j[0] = sqrt(1 / (4 N_j)),  s_j[k > 0] = sqrt(1 / (2 N_j))
    inverse:  Xu = X / (s1 s2), Xu[H, .] = Xu[., W] = 0
        Z[k1, k2]  = (1/2) conj(w2[k2]) (Xu[k1, k2] - i Xu[k1, W - k2]),   k1 in [0, H], k2 <= W / 2
        Vh[k1, k2] = (1/2) conj(w1[k1]) (Z[k1, k2] - i Z[H - k1, k2])
        v = irfft2(Vh), then the permutation undone.

The iteration (sporco/admm/spline.py:24-291), constraint x - y = s:

    x step : X = idct(Gamma dct(Y + S - U)),  Gamma = 1 / (1 + (lmbda / rho) Alpha^2),
             Alpha[k1, k2] = (-2 + 2 cos(pi k1 / H)) + (-2 + 2 cos(pi k2 / W))
    relax  : AX = r X + (1 - r) (Y + S);   y step: Y = soft(AX - S + U, Wdf / rho);   u step: U += AX - Y - S
    DFid = sum |Wdf g|, g = Y or X - S;   Reg = (1/2) sum (Alpha Xhat)^2 (Parseval: the transform is orthonormal)
    r = ||X - Y - S||, rn = max(||X||, ||Y||, ||S||);   s = rho ||Y - Yprev||, sn = rho ||U||
    XSlvRelRes: ||(1 + (lmbda / rho) Alpha^2) Xhat - Zhat|| / max(of the two norms), Zhat = dct(Y + S - U)
    U from a Y0 alone: (Wdf / rho) sign(Y).

Every array and scalar is kept in ``dtype`` (the spectra in its complex type), so that the statement can run in
float32.
"""

import numpy as np


def perm_index(N):
    """``idx`` with v = x[idx]: the even samples in order, then the odd ones reversed."""
    return np.concatenate((np.arange(0, N, 2), np.arange(N - 1 - (N % 2), 0, -2))).astype(np.int64)


def permute(x):
    return x[perm_index(x.shape[0])][:, perm_index(x.shape[1])]


def unpermute(v):
    x = np.empty_like(v)
    i0, i1 = perm_index(v.shape[0]), perm_index(v.shape[1])
    x[np.ix_(i0, i1)] = v
    return x


def tables(N, dtype, nd, axis):
    """w[k], k <= N (complex), s[k] and alpha[k], k < N, shaped to broadcast along ``axis`` of ``nd`` axes."""
    ct = np.complex64 if np.dtype(dtype) == np.float32 else np.complex128
    k = np.arange(N + 1)
    w = np.exp(-1j * np.pi * k / (2.0 * N)).astype(ct)
    s = np.full(N, np.sqrt(1.0 / (2.0 * N)))
    s[0] = np.sqrt(1.0 / (4.0 * N))
    al = -2.0 + 2.0 * np.cos(np.pi * np.arange(N) / float(N))
    shp = [1] * nd
    shp[axis] = -1
    return w.reshape(shp), s.astype(dtype).reshape(shp), al.astype(dtype).reshape(shp)


def _ax(a, axis, sl):
    idx = [slice(None)] * a.ndim
    idx[axis] = sl
    return a[tuple(idx)]


def post_twiddle(Vh, H, W, dtype):
    """The unscaled coefficients Xu (H, W, ...) from the half spectrum of the permuted array."""
    ct = Vh.dtype
    nd = Vh.ndim
    w1, _, _ = tables(H, dtype, nd, 0)
    w2, _, _ = tables(W, dtype, nd, 1)
    Wf = W // 2 + 1
    a = Vh
    b = Vh[(-np.arange(H)) % H]
    w1k = _ax(w1, 0, slice(0, H))
    w2k = _ax(w2, 1, slice(0, Wf))
    Xu = np.zeros((H, W) + Vh.shape[2:], dtype)
    Xu[:, :Wf] = (2 * (w1k * (w2k * a + np.conj(w2k) * np.conj(b)).astype(ct)).real).astype(dtype)
    k2 = np.arange(1, (W - 1) // 2 + 1)          # 0 < k2 < W - k2
    if k2.size:
        w2m = _ax(w2, 1, W - k2)
        am, bm = a[:, k2], b[:, k2]
        Xu[:, W - k2] = (2 * (w1k * (w2m * np.conj(bm) + np.conj(w2m) * am).astype(ct)).real).astype(dtype)
    return Xu


def pre_twiddle(Xu, dtype):
    """The half spectrum (H, W // 2 + 1, ...) whose irfft2 is the permuted inverse DCT of Xu s1 s2."""
    ct = np.complex64 if np.dtype(dtype) == np.float32 else np.complex128
    H, W = Xu.shape[:2]
    nd = Xu.ndim
    w1, _, _ = tables(H, dtype, nd, 0)
    w2, _, _ = tables(W, dtype, nd, 1)
    Wf = W // 2 + 1
    P = np.zeros((H + 1, W + 1) + Xu.shape[2:], dtype)
    P[:H, :W] = Xu
    k2 = np.arange(Wf)
    half = np.dtype(dtype).type(0.5)
    Z = (half * np.conj(_ax(w2, 1, k2)) * (P[:, k2] - 1j * P[:, W - k2]).astype(ct)).astype(ct)
    k1 = np.arange(H)
    return (half * np.conj(_ax(w1, 0, k1)) * (Z[k1] - 1j * Z[H - k1]).astype(ct)).astype(ct)


def scales(shape, dtype):
    nd = len(shape)
    _, s1, a1 = tables(shape[0], dtype, nd, 0)
    _, s2, a2 = tables(shape[1], dtype, nd, 1)
    return (s1 * s2).astype(dtype), (a1 + a2).astype(dtype)


def dct2(x, dtype=None):
    """Orthonormal DCT-II over axes (0, 1)."""
    dtype = x.dtype if dtype is None else np.dtype(dtype)
    x = np.asarray(x, dtype=dtype)
    ct = np.complex64 if dtype == np.float32 else np.complex128
    H, W = x.shape[:2]
    Vh = np.fft.rfftn(permute(x), axes=(0, 1)).astype(ct)
    s, _ = scales(x.shape, dtype)
    return (post_twiddle(Vh, H, W, dtype) * s).astype(dtype)


def idct2(X, dtype=None):
    dtype = X.dtype if dtype is None else np.dtype(dtype)
    X = np.asarray(X, dtype=dtype)
    s, _ = scales(X.shape, dtype)
    Vh = pre_twiddle((X / s).astype(dtype), dtype)
    return unpermute(np.fft.irfftn(Vh, s=X.shape[:2], axes=(0, 1)).astype(dtype))


def _front(x, axes):
    """``x`` with ``axes`` (one or two) moved to the front, a single axis behind a unit one; and the way back."""
    axes = tuple(range(x.ndim)) if axes is None else tuple(axes)
    if len(axes) == 1:
        m = np.moveaxis(x, axes[0], 0)[np.newaxis]
        return m, lambda y: np.moveaxis(y[0], 0, axes[0])
    return np.moveaxis(x, axes, (0, 1)), lambda y: np.moveaxis(y, (0, 1), axes)


def dctii(x, axes=None, dtype=None):
    m, back = _front(np.asarray(x), axes)
    return np.ascontiguousarray(back(dct2(np.ascontiguousarray(m), dtype)))


def idctii(x, axes=None, dtype=None):
    m, back = _front(np.asarray(x), axes)
    return np.ascontiguousarray(back(idct2(np.ascontiguousarray(m), dtype)))


def soft(v, alpha):
    return (np.sign(v) * np.maximum(np.abs(v) - alpha, 0)).astype(v.dtype)


def spline_l1(S, lmbda, iters, rho=None, rlx=1.8, wdf=1.0, geval_y=True, ar=None, std_residuals=False,
              lin_solve_check=False, Y0=None, U0=None, abs_tol=0.0, rel_tol=0.0, dtype=np.float64):
    """``S``: (H, W, ...) with axes (0, 1), or 1-D (served as (1, N)).  ``ar``: None, or dict(Period, Scaling,
    RsdlRatio, AutoScaling, RsdlTarget).  Returns the final X, Y, U, rho and the traces."""
    t = np.dtype(dtype).type
    ct = np.complex64 if np.dtype(dtype) == np.float32 else np.complex128
    S = np.asarray(S, dtype=dtype)
    oshape = S.shape
    if S.ndim == 1:
        S = S[np.newaxis]
    Hh, Ww = S.shape[:2]

    def shaped(a):
        a = np.asarray(a, dtype=dtype)
        return a.reshape(S.shape) if a.shape == oshape and a.ndim == 1 else a

    lmbda = t(lmbda)
    rho = t(2.0 * lmbda + 0.1) if rho is None else t(rho)
    rlx = t(rlx)
    wdf = shaped(wdf)
    sc, alpha = scales(S.shape, dtype)
    al2 = (alpha * alpha).astype(dtype)
    Y = np.zeros_like(S) if Y0 is None else shaped(Y0).copy()
    if U0 is not None:
        U = shaped(U0).copy()
    elif Y0 is not None:
        U = ((wdf / rho) * np.sign(Y)).astype(dtype)
    else:
        U = np.zeros_like(S)
    ns_ = float(np.linalg.norm(S.ravel()))
    Nx = Nc = S.size

    keys = ('ObjFun', 'DFid', 'Reg', 'PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho', 'XSlvRelRes')
    tr = {k: [] for k in keys}
    X = np.zeros_like(S)
    for k in range(iters):
        lr = t(lmbda / rho)
        rhs = ((Y + S) - U).astype(dtype)
        Vh = np.fft.rfftn(permute(rhs), axes=(0, 1)).astype(ct)
        Zu = post_twiddle(Vh, Hh, Ww, dtype)
        den = (t(1) + lr * al2).astype(dtype)
        Xu = (Zu / den).astype(dtype)
        Zh, Xh = (Zu * sc).astype(dtype), (Xu * sc).astype(dtype)
        X = unpermute(np.fft.irfftn(pre_twiddle(Xu, dtype), s=(Hh, Ww), axes=(0, 1)).astype(dtype))
        xrrs = np.nan
        if lin_solve_check:
            ax = (den * Xh).astype(np.float64)
            nrm = max(np.linalg.norm(ax.ravel()), np.linalg.norm(Zh.ravel().astype(np.float64)))
            xrrs = 0.0 if nrm == 0 else float(np.linalg.norm((ax - Zh).ravel()) / nrm)
        reg = 0.5 * float(np.sum((alpha * Xh).astype(np.float64) ** 2))
        AX = X if rlx == 1 else (rlx * X + (1 - rlx) * (Y + S)).astype(dtype)
        Yprev = Y
        Y = soft((AX - S) + U, (wdf / rho).astype(dtype))
        U = (U + ((AX - Y) - S)).astype(dtype)
        g = Y if geval_y else X - S
        dfid = float(np.sum(np.abs(wdf * g).astype(np.float64)))
        nr = float(np.linalg.norm(((X - Y) - S).ravel()))
        rn = float(max(np.linalg.norm(X.ravel()), np.linalg.norm(Y.ravel()), ns_))
        ns = float(rho * np.linalg.norm((Y - Yprev).ravel()))
        sn = float(rho * np.linalg.norm(U.ravel()))
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
    out.update(X=X.reshape(oshape), Y=Y.reshape(oshape), U=U.reshape(oshape), rho=float(rho))
    return out


def from_golden(g, iters=None, dtype=np.float64, **over):
    """Run the statement on the inputs and options of a fixture written by tools/make_golden_spline.py."""
    ar = None
    if int(g['opt_AutoRho']):
        ar = dict(Period=int(g['opt_AutoRho_Period']), Scaling=float(g['opt_AutoRho_Scaling']),
                  RsdlRatio=float(g['opt_AutoRho_RsdlRatio']), AutoScaling=bool(g['opt_AutoRho_AutoScaling']),
                  RsdlTarget=float(g['opt_AutoRho_RsdlTarget']))
    kw = dict(rho=float(g['opt_rho']), rlx=float(g['opt_RelaxParam']), wdf=g.get('optarr_DFidWeight', 1.0),
              geval_y=bool(g['opt_gEvalY']), ar=ar, std_residuals=bool(g['opt_StdResiduals']),
              lin_solve_check=bool(g['opt_LinSolveCheck']), Y0=g.get('optarr_Y0'), U0=g.get('optarr_U0'), dtype=dtype)
    kw.update(over)
    return spline_l1(g['S'], float(g['lmbda']), int(g['MaxMainIter']) if iters is None else iters, **kw)
