"""The iteration of sporco.admm.rpca RobustPCA (sporco/admm/rpca.py:23-262 on the loop of sporco/admm/admm.py:293-389)
stated in plain NumPy, in float64 or float32, independent of the package under test.

TEST INFRASTRUCTURE ONLY.  Two forms of the x step, singular value thresholding of V = S - Y - U at 1 / rho:
    'svd'   numpy.linalg.svd in the working precision, as the reference has it;
    'gram'  the Gram matrix of the short side of V in float64 (V itself in the working precision), its
            eigendecomposition, T = W diag(max(0, 1 - alpha / sigma)) W^T in float64, X = V T (T V) in the working
            precision: what the package does, without its kernels.
In float64 both reproduce the fixtures tests/golden/rpca_*_f64.npz of the unmodified reference
(test_rpca.py::test_statement_reproduces_fixtures); in float32, against the same fixtures, the Gram form is the
yardstick from which the float32 bounds of tests/test_rpca.py are taken.
"""

import numpy as np

from _cmod_numpy import rho_update

FIELDS = ('ObjFun', 'NrmNuc', 'NrmL1', 'Cnstr')
ALG = ('PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho')

RPCA_DEFAULTS = {'fEvalX': True, 'gEvalY': True, 'RelaxParam': 1.8, 'rho': None, 'MaxMainIter': 1000,
                 'RelStopTol': 1e-3, 'AbsStopTol': 0.0, 'Y0': None, 'U0': None, 'AutoRho.Enabled': True,
                 'AutoRho.Period': 1, 'AutoRho.Scaling': 1000.0, 'AutoRho.RsdlRatio': 1.2, 'AutoRho.RsdlTarget': 1.0,
                 'AutoRho.AutoScaling': True}


def soft(v, t):
    return np.sign(v) * np.clip(np.abs(v) - t, 0, float('Inf'))


def gram(V):
    """The Gram matrix of the short side, float64."""
    V64 = V.astype(np.float64)
    return V64.T.dot(V64) if V.shape[0] >= V.shape[1] else V64.dot(V64.T)


def svt_svd(V, alpha):
    Us, s, Vs = np.linalg.svd(V, full_matrices=False)
    ss = np.maximum(0, s - alpha)
    return np.dot(Us, np.dot(np.diag(ss), Vs)), ss


def svt_gram(V, alpha):
    w, W = np.linalg.eigh(gram(V))
    sigma = np.sqrt(np.maximum(w, 0.0))[::-1]
    W = W[:, ::-1]
    ss = np.maximum(0.0, sigma - float(alpha))
    f = np.zeros_like(sigma)
    f[sigma > 0] = ss[sigma > 0] / sigma[sigma > 0]
    T = (W * f).dot(W.T).astype(V.dtype)
    return (V.dot(T) if V.shape[0] >= V.shape[1] else T.dot(V)), ss


def nrm_nuc_gram(V):
    return float(np.sum(np.sqrt(np.maximum(np.linalg.eigvalsh(gram(V)), 0.0))))


def run(S, lmbda=None, opt=None, dtype=np.float64, form='svd', iters=None):
    """``opt``: a flat dict of the option values that differ from the defaults, AutoRho keys as 'AutoRho.Key'.
    Returns dict(X, Y, U, rho, ss, <trace arrays>)."""
    o = dict(RPCA_DEFAULTS)
    o.update(opt or {})
    dt = np.dtype(dtype).type
    S = np.asarray(S, dtype=dtype)
    lmbda = dt(S.shape[0] ** -0.5 if lmbda is None else lmbda)
    rho = dt(2.0 * lmbda + 0.1 if o['rho'] is None else o['rho'])
    rlx = dt(o['RelaxParam'])
    Y = np.zeros(S.shape, dtype) if o['Y0'] is None else np.asarray(o['Y0']).astype(dtype)
    if o['U0'] is not None:
        U = np.asarray(o['U0']).astype(dtype)
    elif o['Y0'] is not None:
        U = ((lmbda / rho) * np.sign(Y)).astype(dtype)
    else:
        U = np.zeros(S.shape, dtype)
    nS = np.linalg.norm(S)
    n = np.sqrt(S.size)
    tr = {f: [] for f in FIELDS + ALG}
    X = ss = None
    svt = svt_svd if form == 'svd' else svt_gram
    for k in range(o['MaxMainIter'] if iters is None else iters):
        Yp = Y
        X, ss = svt(S - Y - U, 1 / rho)
        X = X.astype(dtype)
        AX = X if rlx == 1.0 else rlx * X - (1 - rlx) * (Y - S)
        Y = np.asarray(soft(S - AX - U, lmbda / rho), dtype=dtype)
        U = U + (AX + Y - S)
        if o['fEvalX']:
            rnn = np.sum(ss)
        else:
            rnn = np.sum(np.linalg.svd(S - Y, compute_uv=False)) if form == 'svd' else nrm_nuc_gram(S - Y)
        rl1 = np.sum(np.abs(Y if o['gEvalY'] else S - X))
        nr = np.linalg.norm(X + Y - S)
        ns = rho * np.linalg.norm(Y - Yp)
        rn = max(np.linalg.norm(X), np.linalg.norm(Y), nS)
        sn = rho * np.linalg.norm(U)
        rn = 1.0 if rn == 0.0 else rn
        sn = 1.0 if sn == 0.0 else sn
        r, s = nr / rn, ns / sn
        epri, edua = n * o['AbsStopTol'] / rn + o['RelStopTol'], n * o['AbsStopTol'] / sn + o['RelStopTol']
        for f, v in zip(FIELDS + ALG, (rnn + lmbda * rl1, rnn, rl1, nr, r, s, epri, edua, rho)):
            tr[f].append(v)
        rho, U = rho_update(o, k, r, s, rho, U, dt)
        if r < epri and s < edua:
            break
    out = {'X': X, 'Y': Y, 'U': U, 'rho': rho, 'ss': ss}
    for f, v in tr.items():
        out[f] = np.array(v, dtype=np.float64)
    return out
