"""The iteration of sporco.admm.bpdn BPDNProjL1 (sporco/admm/bpdn.py:750-914 on the loop of
sporco/admm/admm.py:293-389) stated in plain NumPy, in float64 or float32, independent of the package under test.

TEST INFRASTRUCTURE ONLY.  In float64 it reproduces the fixtures tests/golden/bpdnprojl1_*_f64.npz of the unmodified
reference (test_bpdnprojl1.py::test_statement_reproduces_fixtures); in float32, against the same fixtures, it is the
yardstick from which the float32 bounds of tests/test_bpdnprojl1.py are taken.  The projection is the sort and
cumulative sum of duchi-2008-efficient, as sporco/prox/_l1proj.py:110-154 computes it, in the working precision; the
residuals are the reference's, on the unrelaxed X; the x step and the AutoRho rule are those of tests/_bpdn_numpy.py.
"""

import numpy as np

from _bpdn_numpy import ALG, xsolve

FIELDS = ('ObjFun', 'Cnstr')


def proj_l1_cols(v, gamma):
    """The projection of every column of ``v`` (M, K) onto the l1 ball of radius ``gamma``, in ``v``'s precision."""
    v = np.asarray(v)
    dt = v.dtype.type
    gamma = dt(gamma)
    M = v.shape[0]
    av = np.abs(v)
    vs = -np.sort(-av, axis=0)                                     # descending
    inv = (dt(1.0) / np.arange(1, M + 1, dtype=v.dtype)).reshape(M, 1)
    t = inv * (np.cumsum(vs, axis=0) - gamma)
    act = vs >= t
    cnt = np.sum(act, axis=0, keepdims=True)
    t = (np.sum(vs * act, axis=0, keepdims=True) - gamma) / cnt
    t = np.maximum(0, t).astype(v.dtype)
    return np.sign(v) * np.where(av > t, av - t, 0)


def run(D, S, gamma, opt=None, dtype=np.float64, iters=None, Y=None, U=None, rho=None, k0=0):
    """``opt``: a flat dict of the option values that differ from the defaults, AutoRho keys as 'AutoRho.Key'.
    Returns dict(X, Y, U, rho, <trace arrays>).  ``Y`` / ``U`` / ``rho`` / ``k0``: continue from a state."""
    o = {'AuxVarObj': True, 'LinSolveCheck': False, 'NonNegCoef': False, 'RelaxParam': 1.8, 'rho': None,
         'MaxMainIter': 1000, 'RelStopTol': 1e-3, 'AbsStopTol': 0.0, 'Y0': None, 'U0': None,
         'AutoRho.Enabled': True, 'AutoRho.Period': 10, 'AutoRho.Scaling': 1000.0, 'AutoRho.RsdlRatio': 1.2,
         'AutoRho.RsdlTarget': 1.0, 'AutoRho.AutoScaling': True, 'AutoRho.StdResiduals': False}
    o.update(opt or {})
    dt = np.dtype(dtype).type
    D = np.asarray(D, dtype=dtype)
    S = np.asarray(S, dtype=dtype)
    M, K = D.shape[1], S.shape[1]
    gamma = dt(gamma)
    if rho is None:
        rho = dt(1.0) if o['rho'] is None else dt(o['rho'])
    rho = dt(rho)
    xi, tau, rmu, rlx = dt(o['AutoRho.RsdlTarget']), dt(o['AutoRho.Scaling']), dt(o['AutoRho.RsdlRatio']), dt(o['RelaxParam'])
    if Y is None:
        Y = np.zeros((M, K), dtype) if o['Y0'] is None else np.asarray(o['Y0']).astype(dtype)
        U = np.zeros((M, K), dtype) if o['U0'] is None else np.asarray(o['U0']).astype(dtype)      # (zero with a Y0 too)
    else:
        Y, U = np.asarray(Y, dtype).copy(), np.asarray(U, dtype).copy()
    DTS = D.T.dot(S)
    tr = {f: [] for f in FIELDS + ALG}
    X = None
    n = o['MaxMainIter'] if iters is None else iters
    for k in range(k0, k0 + n):
        Yprev = Y
        b = DTS + rho * (Y - U)
        X = xsolve(D, rho, b)
        xrrs = None
        if o['LinSolveCheck']:
            ax = D.T.dot(D.dot(X)) + rho * X
            nrm = max(np.linalg.norm(ax), np.linalg.norm(b))
            xrrs = 0.0 if nrm == 0.0 else np.linalg.norm(ax - b) / nrm
        AX = X if rlx == 1.0 else rlx * X + (1 - rlx) * Y
        Y = np.asarray(proj_l1_cols(AX + U, gamma), dtype)
        if o['NonNegCoef']:
            Y[Y < 0.0] = 0.0
        U = U + AX - Y
        gv = Y if o['AuxVarObj'] else X
        dfd = 0.5 * np.linalg.norm(D.dot(gv) - S) ** 2
        cns = np.linalg.norm(proj_l1_cols(gv, gamma) - gv)
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
        for f, v in zip(FIELDS + ALG, (dfd, cns, r, s, epri, edua, rho, xrrs)):
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
