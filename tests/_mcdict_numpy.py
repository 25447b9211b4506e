"""NumPy statements of what the multi-channel dictionary kernels (sporco_amd/csrc/ck_ism.hip) compute,
written from the definitions.  Everything marked float64 widens its inputs first and is the reference
of tests/test_mcdict_kernels.py; the `*_f32` functions evaluate the same expressions in single precision
with every sum taken sequentially, and only serve to measure what single precision costs.

Layouts (those of the library's host arrays):
    D  (dH, dW, Cd, 1, K)   Df (H, Wf, Cd, 1, K)        S  (H, W, Cd, N)   Sf (H, Wf, Cd, N)
    Y, U, X (H, W, 1, N, K) and their spectra (H, Wf, 1, N, K);  Wf = W // 2 + 1
    dictionary update: Z (H, W, 1, N, K), the dictionary variables (H, W, Cd, 1, K)

The x step (GenericConvBPDN.xstep / ConvBPDNGradReg.xstep of the reference): per frequency, with the
Cd x K matrix A = Df,
    (A^H A + diag) xf = A^H Sf + rho yuf,      yuf = rfft2(Y - u_scale U),
    diag = rho, or mu wg_k GHGf + rho with the gradient term,
solved densely (np.linalg.solve), not by the Sherman-Morrison recursion.

Scale of the sums, from include/sporco_amd.h and finalize_solve (api_transforms.inc); pw is the Parseval
weight of a half-spectrum column (1 on column 0 and on the Nyquist column of an even W, 2 elsewhere):
    OUT_DFID      sum pw |A xf - Sf|^2 / (H W)             (not halved: twice the reference's DFid)
    OUT_XRRS_D2   sum |ax - b|^2,  ax = A^H A xf + diag xf,  b = A^H Sf + rho yuf, over the half spectrum,
    OUT_XRRS_AX2  sum |ax|^2                                 unweighted and unscaled
    OUT_XRRS_B2   sum |b|^2
    OUT_RGR       sum pw wg_k GHGf |xf|^2 / (H W)          (twice the reference's RegGrad)
    PGM_F         0.5 sum |A v - Sf|^2 over the half spectrum, unweighted
    PGM_DFID      sum pw |A v - Sf|^2 / (H W)
    PGM_HESS      sum |A v|^2 over the half spectrum, unweighted
The dictionary update's check sums (api_dstep.inc) are OUT_XRRS_* of (Z^H Z + rho I) d against
b = Z^H s + rho yuf, over the half spectrum of every (channel, filter), unweighted.
"""

import contextlib
import functools

import numpy as np

try:
    from threadpoolctl import threadpool_limits
except ImportError:      # (optional: only the run time under several test workers depends on it)
    threadpool_limits = None


def one_thread(fn):
    """Run `fn` with the BLAS / LAPACK pools at one thread: the stacks of small systems here gain nothing
    from more, and several test workers with a pool each starve one another."""
    @functools.wraps(fn)
    def wrapped(*a, **kw):
        with (threadpool_limits(limits=1) if threadpool_limits else contextlib.nullcontext()):
            return fn(*a, **kw)
    return wrapped


def wide(a):
    a = np.asarray(a)
    return a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)


def zpad(D, H, W):
    out = np.zeros((H, W) + D.shape[2:], dtype=D.dtype)
    out[:D.shape[0], :D.shape[1]] = D
    return out


def rfft2(a):
    return np.fft.rfftn(a, axes=(0, 1))


def irfft2(af, H, W):
    return np.fft.irfftn(af, (H, W), axes=(0, 1))


def parseval_weight(W):
    """(1, Wf, 1, ...) broadcastable over a half spectrum (H, Wf, ...): how often a column of the half
    spectrum stands in the full one."""
    Wf = W // 2 + 1
    pw = np.full(Wf, 2.0)
    pw[0] = 1.0
    if W % 2 == 0:
        pw[-1] = 1.0
    return pw.reshape(1, Wf)


def ghg(H, W):
    """GHGf (H, Wf) of ConvBPDNGradReg (signal.gradient_filters): sum over the two axes of
    |fft([-1, 1])|^2 = 2 - 2 cos(2 pi f / n), from the definition.  A singleton axis crops the two-tap
    filter to its first tap."""
    g = np.zeros((H, W))
    g[0, 0] = -1.0
    gh, gw = g.copy(), g.copy()
    if H > 1:
        gh[1, 0] = 1.0
    if W > 1:
        gw[0, 1] = 1.0
    return np.abs(rfft2(gh)) ** 2 + np.abs(rfft2(gw)) ** 2


def cond2(M):
    """Largest 2-norm condition number of a stack of Hermitian positive definite matrices."""
    ev = np.linalg.eigvalsh(M)
    return float(np.max(ev[..., -1] / ev[..., 0]))


def spectra(D, S, Y, U, u_scale):
    """Df, Sf, yuf in float64 from host arrays of the dtype under test."""
    H, W = S.shape[:2]
    Df = rfft2(zpad(wide(D), H, W))
    Sf = rfft2(wide(S))
    yuf = rfft2(wide(Y) - float(u_scale) * wide(U))
    return Df, Sf, yuf


def diagonal(H, W, K, rho, mu=None, wg=None):
    """(H, Wf, K): rho, or mu wg GHGf + rho."""
    Wf = W // 2 + 1
    if mu is None:
        return np.full((H, Wf, K), float(rho))
    w = np.ones(K) if wg is None else wide(wg).ravel()
    return float(mu) * ghg(H, W)[:, :, None] * w[None, None, :] + float(rho)


@one_thread
def xstep(D, S, Y, U, rho, u_scale=1.0, mu=None, wg=None):
    """Dense x step.  Returns a dict: X, xf, the sums, and the largest 2-norm condition number of the
    systems solved."""
    H, W = S.shape[:2]
    N, K = Y.shape[3], Y.shape[4]
    Df, Sf, yuf = spectra(D, S, Y, U, u_scale)
    A = Df[:, :, :, 0, :]                                           # (H, Wf, Cd, K)
    dg = diagonal(H, W, K, rho, mu, wg)
    M = np.einsum('hwck,hwcm->hwkm', np.conj(A), A)                 # A^H A
    M = M + dg[:, :, :, None] * np.eye(K)
    b = np.einsum('hwck,hwcn->hwkn', np.conj(A), Sf) + float(rho) * np.swapaxes(yuf[:, :, 0], 2, 3)
    x = np.linalg.solve(M, b)                                       # (H, Wf, K, N)
    cond = cond2(M)
    xf = np.swapaxes(x, 2, 3)[:, :, None]                           # (H, Wf, 1, N, K)
    out = {'xf': xf, 'X': irfft2(xf, H, W), 'cond': cond}
    pw = parseval_weight(W)
    r = np.einsum('hwck,hwkn->hwcn', A, x) - Sf
    out['dfid'] = float(np.sum(pw[:, :, None, None] * np.abs(r) ** 2)) / (H * W)
    ax = np.einsum('hwkm,hwmn->hwkn', M, x)
    out['xrrs_d2'] = float(np.sum(np.abs(ax - b) ** 2))
    out['xrrs_ax2'] = float(np.sum(np.abs(ax) ** 2))
    out['xrrs_b2'] = float(np.sum(np.abs(b) ** 2))
    if mu is not None:
        w = np.ones(K) if wg is None else wide(wg).ravel()
        gw = ghg(H, W)[:, :, None, None] * w[None, None, :, None]
        out['rgr'] = float(np.sum(pw[:, :, None, None] * gw * np.abs(x) ** 2)) / (H * W)
    return out


@one_thread
def pgm_grad(D, S, vf):
    """gf = sum_c conj(Df_c) (sum_m Df_cm v_m - Sf_c) for a coefficient spectrum vf (H, Wf, 1, N, K), with
    PGM_F, PGM_DFID, PGM_HESS and the residual r (H, Wf, Cd, N)."""
    H, W = S.shape[:2]
    A = rfft2(zpad(wide(D), H, W))[:, :, :, 0, :]
    Sf = rfft2(wide(S))
    v = wide(vf)[:, :, 0]                                           # (H, Wf, N, K)
    av = np.einsum('hwck,hwnk->hwcn', A, v)
    r = av - Sf
    gf = np.einsum('hwck,hwcn->hwnk', np.conj(A), r)[:, :, None]
    pw = parseval_weight(W)[:, :, None, None]
    return {'gf': gf, 'r': r, 'av': av, 'f': 0.5 * float(np.sum(np.abs(r) ** 2)),
            'dfid': float(np.sum(pw * np.abs(r) ** 2)) / (H * W), 'hess': float(np.sum(np.abs(av) ** 2))}


@one_thread
def reconstruct(D, V):
    """irfft2(sum_k Df_ck rfft2(V)_nk): (H, W, Cd, N, 1)."""
    H, W = V.shape[:2]
    A = rfft2(zpad(wide(D), H, W))[:, :, :, 0, :]
    vf = rfft2(wide(V))[:, :, 0]
    return irfft2(np.einsum('hwck,hwnk->hwcn', A, vf), H, W)[..., None]


@one_thread
def conj_outer_of_residual(D, S, vf):
    """The gradient with its residual taken through the spatial domain and back (masked_grad without a
    mask): sum_c conj(Df_c) rfft2(irfft2(r_c))."""
    H, W = S.shape[:2]
    A = rfft2(zpad(wide(D), H, W))[:, :, :, 0, :]
    r = rfft2(irfft2(pgm_grad(D, S, vf)['r'], H, W))
    return np.einsum('hwck,hwcn->hwnk', np.conj(A), r)[:, :, None]


def dhs_absmax(D, S):
    """max over (frequency, channel, image, filter) of |conj(Df) Sf|."""
    H, W = S.shape[:2]
    A = rfft2(zpad(wide(D), H, W))[:, :, :, 0, :]
    Sf = rfft2(wide(S))
    return float(np.max(np.abs(np.conj(A)[:, :, :, None, :] * Sf[:, :, :, :, None])))


@one_thread
def dstep(Z, S, Y, U, rho, u_scale=1.0):
    """Dense dictionary update x step: per (frequency, channel), with the N x K matrix Zf,
    (Zf^H Zf + rho I) d = Zf^H s_c + rho yuf_c;  Y, U (H, W, Cd, 1, K).  Returns X (H, W, Cd, 1, K), the
    check sums and the largest condition number."""
    H, W = S.shape[:2]
    K = Z.shape[4]
    Zf = rfft2(wide(Z))[:, :, 0]                                    # (H, Wf, N, K)
    Sf = rfft2(wide(S))                                             # (H, Wf, Cd, N)
    yuf = rfft2(wide(Y) - float(u_scale) * wide(U))[:, :, :, 0, :]  # (H, Wf, Cd, K)
    M = np.einsum('hwnk,hwnm->hwkm', np.conj(Zf), Zf) + float(rho) * np.eye(K)
    b = np.einsum('hwnk,hwcn->hwkc', np.conj(Zf), Sf) + float(rho) * np.swapaxes(yuf, 2, 3)
    d = np.linalg.solve(M, b)                                       # (H, Wf, K, Cd)
    q = np.einsum('hwkm,hwmc->hwkc', M, d)
    xf = np.swapaxes(d, 2, 3)[:, :, :, None, :]
    return {'X': irfft2(xf, H, W), 'xf': xf, 'cond': cond2(M),
            'xrrs_d2': float(np.sum(np.abs(q - b) ** 2)), 'xrrs_ax2': float(np.sum(np.abs(q) ** 2)),
            'xrrs_b2': float(np.sum(np.abs(b) ** 2))}


# ---- single precision, sums taken sequentially -----------------------------------------------------------
C64, F32 = np.complex64, np.float32


def _c64(a):
    """A transform of a float32 array is complex64 where NumPy computes it in single precision (2.x);
    rounded to it otherwise."""
    return np.asarray(a, dtype=C64)


def seqsum(a, axis):
    """Sum along `axis` one term after the other, in the array's own precision."""
    a = np.moveaxis(np.asarray(a), axis, -1)
    return np.add.accumulate(a, axis=-1, dtype=a.dtype)[..., -1]


def inner_f32(a, b, axis):
    return seqsum(_c64(a) * _c64(b), axis)


@one_thread
def solvemdbi_ism_f32(ah, dg, b):
    """linalg.solvemdbi_ism in complex64: ah (..., Ct, K) holds the Ct rank-one terms a_c^H, dg (..., K)
    the identity term (rho, or a diagonal), b (..., R, K) the right-hand sides.  Solves
    (diag(dg) + sum_c a_c a_c^H) x = b by the recursion of the reference, term by term."""
    ah = _c64(ah)
    a = np.conj(ah)
    Ct = ah.shape[-2]
    dg = np.asarray(dg, dtype=F32)
    beta = _c64(b) / dg[..., None, :]                               # (..., R, K)
    gamma = np.zeros(a.shape, C64)
    delta = np.zeros(a.shape[:-1], C64)
    alpha = (a[..., 0, :] / dg).astype(C64)
    for k in range(Ct):
        gamma[..., k, :] = alpha
        delta[..., k] = F32(1.0) + inner_f32(ah[..., k, :], alpha, -1)
        t = inner_f32(ah[..., k:k + 1, :], beta, -1)                # (..., R)
        beta = (beta - gamma[..., k:k + 1, :] * (t / delta[..., k:k + 1])[..., None]).astype(C64)
        if k < Ct - 1:
            alpha = (a[..., k + 1, :] / dg).astype(C64)
            for l in range(k + 1):
                t = inner_f32(ah[..., l, :], alpha, -1)
                alpha = (alpha - gamma[..., l, :] * (t / delta[..., l])[..., None]).astype(C64)
    return beta


def spectra_f32(D, S, Y, U, u_scale):
    H, W = S.shape[:2]
    Df = _c64(rfft2(zpad(np.asarray(D, F32), H, W)))
    Sf = _c64(rfft2(np.asarray(S, F32)))
    yuf = _c64(rfft2(np.asarray(Y, F32) - F32(u_scale) * np.asarray(U, F32)))
    return Df, Sf, yuf


@one_thread
def xstep_f32(D, S, Y, U, rho, u_scale=1.0, mu=None, wg=None):
    """The x step in single precision by the recursion: X (the sums take its bound)."""
    H, W = S.shape[:2]
    K = Y.shape[4]
    Df, Sf, yuf = spectra_f32(D, S, Y, U, u_scale)
    A = Df[:, :, :, 0, :]                                           # (H, Wf, Cd, K)
    dg = diagonal(H, W, K, rho, mu, wg).astype(F32)
    # b = sum_c conj(Df_c) Sf_c + rho yuf, the channel sum one term after the other
    b = (F32(rho) * yuf[:, :, 0]).astype(C64)                       # (H, Wf, N, K)
    for c in range(A.shape[2]):
        b = (b + np.conj(A[:, :, c, None, :]) * Sf[:, :, c, :, None]).astype(C64)
    x = solvemdbi_ism_f32(A, dg, b)                                 # (H, Wf, N, K)
    return {'X': np.asarray(irfft2(x[:, :, None], H, W), dtype=F32)}


@one_thread
def pgm_grad_f32(D, S, vf):
    H, W = S.shape[:2]
    A = _c64(rfft2(zpad(np.asarray(D, F32), H, W)))[:, :, :, 0, :]
    Sf = _c64(rfft2(np.asarray(S, F32)))
    v = _c64(vf)[:, :, 0]
    av = np.stack([inner_f32(A[:, :, c, None, :], v, -1) for c in range(A.shape[2])], axis=2)
    r = (av - Sf).astype(C64)
    gf = np.zeros(v.shape, C64)
    for c in range(A.shape[2]):
        gf = (gf + np.conj(A[:, :, c, None, :]) * r[:, :, c, :, None]).astype(C64)
    pw = parseval_weight(W).astype(F32)[:, :, None, None]
    return {'gf': gf[:, :, None], 'r': r, 'av': av, 'f': 0.5 * float(seqsum((np.abs(r) ** 2).ravel(), 0)),
            'dfid': float(seqsum((pw * np.abs(r) ** 2).ravel(), 0)) / (H * W),
            'hess': float(seqsum((np.abs(av) ** 2).ravel(), 0))}


@one_thread
def reconstruct_f32(D, V):
    H, W = V.shape[:2]
    A = _c64(rfft2(zpad(np.asarray(D, F32), H, W)))[:, :, :, 0, :]
    vf = _c64(rfft2(np.asarray(V, F32)))[:, :, 0]
    av = np.stack([inner_f32(A[:, :, c, None, :], vf, -1) for c in range(A.shape[2])], axis=2)
    return np.asarray(irfft2(av, H, W), dtype=F32)[..., None]


@one_thread
def conj_outer_of_residual_f32(D, S, vf):
    H, W = S.shape[:2]
    A = _c64(rfft2(zpad(np.asarray(D, F32), H, W)))[:, :, :, 0, :]
    r = _c64(rfft2(np.asarray(irfft2(pgm_grad_f32(D, S, vf)['r'], H, W), dtype=F32)))
    gf = np.zeros(r.shape[:2] + (r.shape[3], A.shape[3]), C64)
    for c in range(A.shape[2]):
        gf = (gf + np.conj(A[:, :, c, None, :]) * r[:, :, c, :, None]).astype(C64)
    return gf[:, :, None]


def dhs_absmax_f32(D, S):
    H, W = S.shape[:2]
    A = _c64(rfft2(zpad(np.asarray(D, F32), H, W)))[:, :, :, 0, :]
    Sf = _c64(rfft2(np.asarray(S, F32)))
    return float(np.max(np.abs((np.conj(A)[:, :, :, None, :] * Sf[:, :, :, :, None]).astype(C64))))


@one_thread
def dstep_f32(Z, S, Y, U, rho, u_scale=1.0):
    H, W = S.shape[:2]
    K = Z.shape[4]
    Zf = _c64(rfft2(np.asarray(Z, F32)))[:, :, 0]                   # (H, Wf, N, K)
    Sf = _c64(rfft2(np.asarray(S, F32)))                            # (H, Wf, Cd, N)
    yuf = _c64(rfft2(np.asarray(Y, F32) - F32(u_scale) * np.asarray(U, F32)))[:, :, :, 0, :]
    b = (F32(rho) * yuf).astype(C64)                                # (H, Wf, Cd, K)
    for n in range(Zf.shape[2]):
        b = (b + np.conj(Zf[:, :, None, n, :]) * Sf[:, :, :, n, None]).astype(C64)
    dg = np.full(Zf.shape[:2] + (K,), rho, dtype=F32)
    d = solvemdbi_ism_f32(Zf, dg, b)                                # (H, Wf, Cd, K)
    return {'X': np.asarray(irfft2(d[:, :, :, None, :], H, W), dtype=F32)}
