"""The iteration of sporco.admm.bpdn BPDN / BPDNJoint / ElasticNet (sporco/admm/bpdn.py:24-748 on the loop of
sporco/admm/admm.py:293-389) stated in plain NumPy, in float64 or float32, independent of the package under test.

TEST INFRASTRUCTURE ONLY.  In float64 it reproduces the fixtures tests/golden/bpdn_*_f64.npz of the unmodified
reference (to 2.9e-11 on iterates, traces and the final rho: test_bpdn.py::test_statement_reproduces_fixtures); in
float32, against the same fixtures, it is the yardstick from which the float32 bounds of tests/test_bpdn.py are
taken.  The x step solves with a Cholesky factor of the Gram matrix in the working precision, as the reference does.
"""

import numpy as np

FIELDS = {
    'BPDN': ('ObjFun', 'DFid', 'RegL1'),
    'BPDNJoint': ('ObjFun', 'DFid', 'RegL1', 'RegL21'),
    'ElasticNet': ('ObjFun', 'DFid', 'RegL1', 'RegL2'),
}
ALG = ('PrimalRsdl', 'DualRsdl', 'EpsPrimal', 'EpsDual', 'Rho', 'XSlvRelRes')


def soft(v, t):
    return np.sign(v) * np.maximum(0, np.abs(v) - t)


def xsolve(D, c, b):
    """(D^T D + c I)^-1 b, linalg.py:724-773."""
    N, M = D.shape
    dt = D.dtype
    if N >= M:
        L = np.linalg.cholesky(D.T.dot(D) + c * np.identity(M, dtype=dt))
        return np.linalg.solve(L.T, np.linalg.solve(L, b)).astype(dt)
    L = np.linalg.cholesky(D.dot(D.T) + c * np.identity(N, dtype=dt))
    return ((b - D.T.dot(np.linalg.solve(L.T, np.linalg.solve(L, D.dot(b))))) / c).astype(dt)


def default_lmbda(D, S):
    return 0.1 * abs(D.T.dot(S)).max()


def run(cls, D, S, lmbda=None, mu=0.0, opt=None, dtype=np.float64, iters=None, Y=None, U=None, rho=None, k0=0):
    """``opt``: a flat dict of the option values that differ from the defaults, AutoRho keys as 'AutoRho.Key'.
    Returns dict(X, Y, U, rho, <trace arrays>).  ``Y`` / ``U`` / ``rho`` / ``k0``: continue from a state."""
    o = {'AuxVarObj': True, 'LinSolveCheck': False, 'NonNegCoef': False, 'RelaxParam': 1.8, 'L1Weight': 1.0,
         'rho': None, 'MaxMainIter': 1000, 'RelStopTol': 1e-3, 'AbsStopTol': 0.0, 'Y0': None, 'U0': None,
         'AutoRho.Enabled': True, 'AutoRho.Period': 10, 'AutoRho.Scaling': 1000.0, 'AutoRho.RsdlRatio': 1.2,
         'AutoRho.RsdlTarget': None, 'AutoRho.AutoScaling': True, 'AutoRho.StdResiduals': False}
    o.update(opt or {})
    dt = np.dtype(dtype).type
    D = np.asarray(D, dtype=dtype)
    S = np.asarray(S, dtype=dtype)
    M, K = D.shape[1], S.shape[1]
    if lmbda is None:
        lmbda = default_lmbda(D, S)
    lmbda, mu = dt(lmbda), dt(mu)
    wl1 = np.asarray(o['L1Weight'], dtype=dtype)
    if rho is None:
        rho = dt(50.0 * lmbda + 1.0) if o['rho'] is None else dt(o['rho'])
    rho = dt(rho)
    xi = o['AutoRho.RsdlTarget']
    if xi is None:
        xi = float(1.0 + 18.3 ** (np.log10(lmbda) + 1.0)) if lmbda != 0.0 else 1.0
    xi, tau, rmu, rlx = dt(xi), dt(o['AutoRho.Scaling']), dt(o['AutoRho.RsdlRatio']), dt(o['RelaxParam'])
    if Y is None:
        Y = np.zeros((M, K), dtype) if o['Y0'] is None else np.asarray(o['Y0']).astype(dtype)
        if o['U0'] is not None:
            U = np.asarray(o['U0']).astype(dtype)
        elif o['Y0'] is not None:
            U = ((lmbda / rho) * np.sign(Y)).astype(dtype)
        else:
            U = np.zeros((M, K), dtype)
    else:
        Y, U = np.asarray(Y, dtype).copy(), np.asarray(U, dtype).copy()
    DTS = D.T.dot(S)
    c_of = (lambda r: mu + r) if cls == 'ElasticNet' else (lambda r: r)
    tr = {f: [] for f in FIELDS[cls] + ALG}
    X = None
    n = o['MaxMainIter'] if iters is None else iters
    for k in range(k0, k0 + n):
        Yprev = Y
        b = DTS + rho * (Y - U)
        X = xsolve(D, c_of(rho), b)
        xrrs = None
        if o['LinSolveCheck']:
            ax = D.T.dot(D.dot(X)) + c_of(rho) * X
            nrm = max(np.linalg.norm(ax), np.linalg.norm(b))
            xrrs = 0.0 if nrm == 0.0 else np.linalg.norm(ax - b) / nrm
        AX = X if rlx == 1.0 else rlx * X + (1 - rlx) * Y
        V = AX + U
        Y = soft(V, (lmbda / rho) * wl1)
        if cls == 'BPDNJoint':
            a = np.sqrt(np.sum(Y ** 2, axis=-1, keepdims=True))
            bb = np.maximum(0, a - mu / rho)
            Y = np.where(a == 0, 0, bb / np.where(a == 0, 1, a)) * Y
        Y = np.asarray(Y, dtype)
        if o['NonNegCoef']:
            Y[Y < 0.0] = 0.0
        U = U + AX - Y
        fv = Y if o['AuxVarObj'] else X
        gv = Y if o['AuxVarObj'] else X
        dfd = 0.5 * np.linalg.norm(D.dot(fv) - S) ** 2
        rl1 = np.linalg.norm((wl1 * gv).ravel(), 1)
        if cls == 'BPDN':
            reg = (lmbda * rl1, rl1)
        elif cls == 'BPDNJoint':
            rl21 = np.sum(np.sqrt(np.sum(gv ** 2, axis=1)))
            reg = (lmbda * rl1 + mu * rl21, rl1, rl21)
        else:
            rl2 = 0.5 * np.linalg.norm(gv) ** 2
            reg = (lmbda * rl1 + mu * rl2, rl1, rl2)
        nr, ns = np.linalg.norm(X - Y), np.linalg.norm(rho * (Yprev - Y))
        rn, sn = max(np.linalg.norm(X), np.linalg.norm(Y)), rho * np.linalg.norm(U)
        if o['AutoRho.StdResiduals']:
            r, s = nr, ns
            epri = np.sqrt(M * K) * o['AbsStopTol'] + rn * o['RelStopTol']
            edua = np.sqrt(M * K) * o['AbsStopTol'] + sn * o['RelStopTol']
        else:
            rn = 1.0 if rn == 0.0 else rn
            sn = 1.0 if sn == 0.0 else sn
            r, s = nr / rn, ns / sn
            epri = np.sqrt(M * K) * o['AbsStopTol'] / rn + o['RelStopTol']
            edua = np.sqrt(M * K) * o['AbsStopTol'] / sn + o['RelStopTol']
        for f, v in zip(FIELDS[cls] + ALG, (dfd + reg[0], dfd) + reg[1:] + (r, s, epri, edua, rho, xrrs)):
            tr[f].append(v)
        if o['AutoRho.Enabled'] and k != 0 and np.mod(k + 1, o['AutoRho.Period']) == 0:
            if o['AutoRho.AutoScaling']:
                if s == 0.0 or r == 0.0:
                    mlt = tau
                else:
                    mlt = np.sqrt(r / (s * xi) if r > s * xi else (s * xi) / r)
                    if mlt > tau:
                        mlt = tau
            else:
                mlt = tau
            rsf = 1.0
            if r > xi * rmu * s:
                rsf = mlt
            elif s > (rmu / xi) * r:
                rsf = 1.0 / mlt
            rho = dt(rsf * rho)
            U = (U / rsf).astype(dtype)
        if r < epri and s < edua:
            break
    out = {'X': X, 'Y': Y, 'U': U, 'rho': rho}
    for f, v in tr.items():
        out[f] = np.array([np.nan if e is None else e for e in v], dtype=np.float64)
    return out
