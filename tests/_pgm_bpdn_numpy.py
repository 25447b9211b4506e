"""The NumPy statement of sporco_amd.pgm.bpdn BPDN / WeightedBPDN: the iteration of sporco/pgm/pgm.py:284-702 with the
problem of sporco/pgm/bpdn.py:26-375 and the rules of backtrack.py, stepsize.py and momentum.py, written out in one
place and runnable in float32 and float64.  TEST INFRASTRUCTURE ONLY; it imports neither the package nor the
reference.

Options are a flat dict: L, NonNegCoef, L1Weight, X0, Monotone, MaxMainIter, RelStopTol, AutoStop.Enabled,
AutoStop.Tau0, and the rules as
    Momentum        'nesterov' | 'linear' | 'genlinear'   with Momentum.a, Momentum.b
    StepSizePolicy  None | 'cauchy' | 'bb'
    Backtrack       None | 'standard' | 'robust'          with Backtrack.gamma_u, .gamma_d, .maxiter
Arrays are kept in `dtype`; scalars that the reference keeps as Python floats (t, Tk, the momentum coefficients) stay
doubles and are cast where they meet an array, L is kept in `dtype` under backtracking, every sum is taken in double.
"""

import numpy as np

FIELDS = ('ObjFun', 'DFid', 'RegL1', 'Rsdl', 'F_Btrack', 'Q_Btrack', 'IterBTrack', 'L')


def default_lmbda(D, S):
    return 0.1 * float(np.abs(np.asarray(D, np.float64).T.dot(np.asarray(S, np.float64))).max())


def soft(V, alpha):
    return np.sign(V) * np.maximum(0, np.abs(V) - alpha)


def dsum(a):
    return float(np.sum(np.asarray(a, dtype=np.float64)))


def weight(W, N, K, dtype):
    """W as the classes take it: a scalar, (N,), (N, 1), (1, K) or (N, K)."""
    W = np.asarray(1.0 if W is None else W, dtype=dtype)
    if W.ndim == 1:
        W = W.reshape(-1, 1)
    return W


class State(object):
    pass


def momentum_update(o, t, k):
    kind = o.get('Momentum', 'nesterov')
    if kind == 'nesterov':
        return 0.5 * float(1. + np.sqrt(1. + 4. * t ** 2))
    if kind == 'linear':
        b = o.get('Momentum.b', 2.)
        return (k + b) / b
    return (k + o.get('Momentum.a', 50.)) / o.get('Momentum.b', 2.)


def run(D, S, lmbda, o, W=None, dtype=np.float64, state=None, iters=None):
    """Run MaxMainIter (or `iters`) iterations, from `state` (a State a former call returned in res['state'], with
    D replaced by the D given here: `setdict`) or from the start.  Returns the traces, X, Y, L and the state."""
    dt = np.dtype(dtype).type
    D = np.asarray(D, dtype=dtype)
    S = np.asarray(S, dtype=dtype)
    N, K = S.shape
    M = D.shape[1]
    Wt = weight(W, N, K, dtype)
    wl1 = np.asarray(o.get('L1Weight', 1.0), dtype=dtype)
    nonneg = bool(o.get('NonNegCoef', False))
    mono = bool(o.get('Monotone', False))
    bt = o.get('Backtrack')
    pol = None if bt is not None else o.get('StepSizePolicy')
    if lmbda is None:
        lmbda = default_lmbda(D, S)
    lmbda = dt(lmbda)

    def f(V):
        R = D.dot(V) - S
        return 0.5 * dsum(np.asarray(Wt, np.float64) * np.asarray(R, np.float64) ** 2)

    def grad(V):
        return D.T.dot(Wt * (D.dot(V) - S))

    def prox(V, L):
        U = np.asarray(soft(V, (lmbda / dt(L)) * wl1), dtype=dtype)
        if nonneg:
            U[U < 0.0] = 0.0
        return U

    def objfn(X):
        dfd = f(X)
        rl1 = dsum(np.abs(wl1 * X))
        return (dfd + float(lmbda) * rl1, dfd, rl1)

    st = state
    if st is None:
        st = State()
        st.X = np.zeros((M, K), dtype=dtype) if o.get('X0') is None else np.asarray(o['X0']).astype(dtype, copy=True)
        st.Y = st.X.copy()
        st.L = dt(o.get('L', 500.0))
        st.k, st.t, st.Tk, st.Z = 0, 1, 0.0, None
        st.bbx, st.bbg = None, None
        st.objfn = None
        st.reverts = []
    tr = {f_: [] for f_ in FIELDS}
    n = int(o['MaxMainIter'] if iters is None else iters)
    for k in range(st.k, st.k + n):
        st.k = k
        # on_iteration_start
        Xprv, Yprv = st.X, st.Y
        if mono:
            if k == 0:
                st.objfn = objfn(st.X)
            objfn_prev = st.objfn
        F = Q = itbt = None

        def xstep(G):
            """prox step and the Monotone block at the current L; returns whether X was reverted."""
            st.X = prox(st.Y - (dt(1.) / dt(st.L)) * G, st.L)
            if mono and k > 0:
                st.ZZ = st.X
                st.objfn = objfn(st.X)
                if objfn_prev[0] < st.objfn[0]:
                    st.X = Xprv
                    st.objfn = objfn_prev
                    if k not in st.reverts:
                        st.reverts.append(k)

        def quad(G):
            Dxy = np.asarray(st.X - st.Y, np.float64)
            return f(st.Y) + dsum(Dxy * np.asarray(G, np.float64)) + (float(st.L) / 2.) * dsum(Dxy ** 2)

        def ystep():
            tprv = st.t
            st.t = momentum_update(o, st.t, k)
            beta = dt((tprv - 1.) / st.t)
            if mono and k > 0:
                st.Y = st.X + dt(tprv / st.t) * (st.ZZ - st.X) + beta * (st.X - Xprv)
            else:
                st.Y = st.X + beta * (st.X - Xprv)

        if bt == 'standard':
            G = grad(st.Y)
            itbt, ls = 0, True
            while ls and itbt < int(o.get('Backtrack.maxiter', 50)):
                xstep(G)
                F, Q = f(st.X), quad(G)
                if F <= Q:
                    ls = False
                else:
                    st.L = dt(st.L * o.get('Backtrack.gamma_u', 1.2))
                itbt += 1
            ystep()
        elif bt == 'robust':
            if st.Z is None:
                st.Z = st.X.copy()
            st.L = dt(st.L * o.get('Backtrack.gamma_d', 0.9))
            itbt, ls = 0, True
            while ls and itbt < int(o.get('Backtrack.maxiter', 50)):
                L = float(st.L)
                t = float(1. + np.sqrt(1. + 4. * L * st.Tk)) / (2. * L)
                T = st.Tk + t
                st.Y = (dt(st.Tk) * Xprv + dt(t) * st.Z) / dt(T)
                G = grad(st.Y)
                xstep(G)
                F, Q = f(st.X), quad(G)
                if F <= Q:
                    ls = False
                else:
                    st.L = dt(st.L * o.get('Backtrack.gamma_u', 2.0))
                itbt += 1
            st.Tk = T
            st.Z = st.Z + dt(t * float(st.L)) * (st.X - st.Y)
        else:
            G = grad(st.Y)
            if pol is not None:
                if k > 1:
                    G64 = np.asarray(G, np.float64)
                    if pol == 'cauchy':
                        DG = np.asarray(D.dot(G), np.float64)
                        st.L = dsum(DG ** 2) / dsum(G64 ** 2)
                    else:
                        dx = np.asarray(st.X - st.bbx, np.float64)
                        dg = np.asarray(G - st.bbg, np.float64)
                        L = dsum(dg * dg) / dsum(dx * dg)
                        if L < 0.:
                            st.bb_fallbacks = getattr(st, 'bb_fallbacks', []) + [k]
                            L = st.L
                        st.L = L
                if pol == 'bb':
                    st.bbx, st.bbg = st.X, G
            xstep(G)
            ystep()

        if mono and k > 0:
            r = np.sqrt(dsum(np.asarray(st.X - st.Y, np.float64) ** 2))
        else:
            r = np.sqrt(dsum(np.asarray(st.X - Yprv, np.float64) ** 2))
        st.Yprv = Yprv
        obj = st.objfn if mono else objfn(st.X)
        for f_, v in zip(FIELDS, obj + (r, F, Q, itbt, float(st.L))):
            tr[f_].append(v)
        tol = o.get('RelStopTol', 1e-3)
        if o.get('AutoStop.Enabled', False):
            tol = o.get('AutoStop.Tau0', 1e-2) / (1. + k)
        if r < tol:
            break
    st.k += 1
    res = {f_: (np.asarray(v, dtype=np.float64) if v and v[0] is not None else v) for f_, v in tr.items()}
    res.update(X=st.X, Y=st.Y, Lfinal=float(st.L), lmbda=float(lmbda), state=st, reverts=list(st.reverts),
               bb_fallbacks=list(getattr(st, 'bb_fallbacks', [])))
    return res
