"""A NumPy statement of sporco.pgm.cmod CnstrMOD / WeightedCnstrMOD (sporco/pgm/cmod.py:24-407 on the loop of
sporco/pgm/pgm.py:284-702 with the rules of backtrack.py, stepsize.py and momentum.py), in either dtype, and of the
learner sporco.dictlrn.wbpdndl WeightedBPDNDictLearn (``learn``), whose x step is tests/_pgm_bpdn_numpy.py.

TEST INFRASTRUCTURE ONLY.  ``run`` takes the options as a flat dict (``'L'``, ``'MaxMainIter'``, ``'RelStopTol'``,
``'ZeroMean'``, ``'NonNegCoef'``, ``'Monotone'``, ``'AutoStop.Enabled'``, ``'AutoStop.Tau0'``, ``'X0'`` and the rules as
``'Momentum'`` / ``'StepSizePolicy'`` / ``'Backtrack'`` = a kind with its parameters ``'<Slot>.<name>'``) and returns
the final X, Y, L, the IterationStats columns, the iterations at which Monotone reverted and at which the
Barzilai-Borwein rule fell back, and the state a second ``run`` continues from (``state=``, after a ``setcoef``).
Every array operation is done in ``dtype``; the scalars of the rules are Python floats, as in the reference.
"""

import numpy as np

FIELDS = ('DFid', 'Cnstr', 'Rsdl', 'L', 'F_Btrack', 'Q_Btrack', 'IterBTrack')


def normalise(v):
    vn = np.sqrt(np.sum(v ** 2, 0))
    vn[vn == 0] = 1.0
    return np.asarray(v / vn, dtype=v.dtype)


def zeromean(v):
    return v - np.mean(v, 0)


def get_pcn(zm, nnc):
    if zm and nnc:
        raise ValueError('Parameters zm and nnc may not both be True')
    if zm:
        return lambda x: normalise(zeromean(x))
    if nnc:
        return lambda x: normalise(np.clip(x, 0, None))
    return normalise


def weight(W, dtype):
    if W is None:
        return np.array([1.0], dtype=dtype)
    W = np.asarray(W, dtype=dtype)
    if W.ndim == 1:
        W = W.reshape(-1, 1)
    return W


def momentum_t(o, t, k):
    kind = o.get('Momentum', 'nesterov')
    if kind == 'nesterov':
        return 0.5 * float(1. + np.sqrt(1. + 4. * t ** 2))
    if kind == 'linear':
        return (k + o.get('Momentum.b', 2.)) / o.get('Momentum.b', 2.)
    return (k + o.get('Momentum.a', 50.)) / o.get('Momentum.b', 2.)


def run(Z, S, o, W=None, dsz=None, dtype=np.float64, state=None):
    dtype = np.dtype(dtype)
    tp = dtype.type
    S = np.asarray(S, dtype=dtype)
    Z = np.asarray(Z, dtype=dtype)
    W = weight(W, dtype)
    N, M = S.shape[0], Z.shape[0]
    Pcn = get_pcn(o.get('ZeroMean', False), o.get('NonNegCoef', False))
    mono = bool(o.get('Monotone', False))
    bt = o.get('Backtrack')
    pol = None if bt is not None else o.get('StepSizePolicy')

    def grad_f(V):
        return (W * (V.dot(Z) - S)).dot(Z.T)

    def obfn_f(V):
        return 0.5 * float(np.linalg.norm((np.sqrt(W) * (V.dot(Z) - S)).ravel())) ** 2

    def objfn(V):
        return (obfn_f(V), float(np.linalg.norm(Pcn(V) - V)))

    if state is None:
        X = np.zeros((N, M), dtype=dtype) if o.get('X0') is None else np.asarray(o['X0']).astype(dtype)
        st = dict(X=X, Y=X.copy(), L=tp(o.get('L', 500.0)), k=0, t=1, Tk=0.0, Zrb=None, bbx=None, bbg=None, obj=None)
    else:
        st = dict(state)
    X, Y, L, k0, t = st['X'], st['Y'], st['L'], st['k'], st['t']
    Tk, Zrb, bbx, bbg, obj = st['Tk'], st['Zrb'], st['bbx'], st['bbg'], st['obj']
    out = {f: [] for f in FIELDS}
    reverts, fallbacks = [], []
    ZZ = None

    def xstep(k, G):
        """pgm.py:393-422: (X', ZZ, objective, reverted) from Y, G and L."""
        nonlocal L, bbx, bbg
        if pol is not None:
            if k > 1:
                if pol == 'cauchy':
                    HG = G.dot(Z).dot(Z.T)
                    L = np.sum(G * HG) / np.sum(G * G)
                else:
                    dx, dg = X - bbx, G - bbg
                    Ln = np.sum(dg * dg) / np.sum(dx * dg)
                    if Ln < 0.:
                        Ln = L
                        fallbacks.append(k)
                    L = Ln
            if pol == 'bb':
                bbx, bbg = X, G
        V = Y - (tp(1.) / tp(L)) * G
        Xn = Pcn(V)
        return np.asarray(Xn, dtype=dtype)

    for k in range(k0, k0 + int(o['MaxMainIter'])):
        Xprv, Yprv = X, Y
        if mono:
            if k == k0 and obj is None:
                obj = objfn(X)
            obj_prev = obj
        reverted = False

        def monotone(Xn):
            nonlocal obj, reverted, ZZ
            if mono and k > 0:
                ZZ = Xn
                obj = objfn(Xn)
                if obj_prev[0] < obj[0]:
                    obj = obj_prev
                    reverted = True
                    return Xprv
                reverted = False
            return Xn

        F = Q = itb = None
        if bt == 'standard':
            G = grad_f(Y)
            fy = obfn_f(Y)
            itb, ls = 0, True
            while ls and itb < int(o.get('Backtrack.maxiter', 50)):
                Xn = monotone(xstep(k, G))
                F = obfn_f(Xn)
                D = Xn - Y
                Q = fy + float(np.sum(D * G)) + (float(L) / 2.) * float(np.linalg.norm(D.ravel(), 2)) ** 2
                if F <= Q:
                    ls = False
                else:
                    L = tp(L * o.get('Backtrack.gamma_u', 1.2))
                itb += 1
            X = Xn
        elif bt == 'robust':
            if Zrb is None:
                Zrb = X.copy()
            L = tp(L * o.get('Backtrack.gamma_d', 0.9))
            itb, ls = 0, True
            while ls and itb < int(o.get('Backtrack.maxiter', 50)):
                tt = float(1. + np.sqrt(1. + 4. * float(L) * Tk)) / (2. * float(L))
                T = Tk + tt
                Y = (tp(Tk) * Xprv + tp(tt) * Zrb) / tp(T)
                G = grad_f(Y)
                Xn = monotone(xstep(k, G))
                F = obfn_f(Xn)
                D = Xn - Y
                Q = obfn_f(Y) + float(np.sum(D * G)) + (float(L) / 2.) * float(np.linalg.norm(D.ravel(), 2)) ** 2
                if F <= Q:
                    ls = False
                else:
                    L = tp(L * o.get('Backtrack.gamma_u', 2.0))
                itb += 1
            X = Xn
            Tk = T
            Zrb = Zrb + tp(tt * float(L)) * (X - Y)
        else:
            G = grad_f(Y)
            X = monotone(xstep(k, G))
        if reverted:
            reverts.append(k)
        if bt != 'robust':
            tprv = t
            t = momentum_t(o, t, k)
            if mono and k > 0:
                Y = X + tp(tprv / t) * (ZZ - X) + tp((tprv - 1.) / t) * (X - Xprv)
            else:
                Y = X + tp((tprv - 1.) / t) * (X - Xprv)
        # (pgm.py:696-702: under Monotone the residual is taken against the new Y)
        r = float(np.linalg.norm((X - (Y if (mono and k > 0) else Yprv)).ravel()))
        ob = obj if mono else objfn(X)
        for f, v in zip(FIELDS, (ob[0], ob[1], r, float(L), F, Q, itb)):
            out[f].append(v)
        tol = o.get('RelStopTol', 1e-3)
        if o.get('AutoStop.Enabled', False):
            tol = o.get('AutoStop.Tau0', 1e-2) / (1. + k)
        if r < tol:
            break
    res = {f: np.asarray(out[f], dtype=np.float64) for f in FIELDS if out[f] and out[f][0] is not None}
    if 'IterBTrack' in res:
        res['IterBTrack'] = res['IterBTrack'].astype(np.int64)
    res.update(X=X, Y=Y, Lfinal=float(L), reverts=reverts, bb_fallbacks=fallbacks,
               state=dict(X=X, Y=Y, L=L, k=k + 1, t=t, Tk=Tk, Zrb=Zrb, bbx=bbx, bbg=bbg, obj=obj))
    return res


LEARN_FIELDS = ('ObjFun', 'DFid', 'RegL1', 'Cnstr', 'XRsdl', 'XL', 'DRsdl', 'DL')


def learn(D0, S, lmbda, iters, W=None, accurate=False, xo=None, do=None, dtype=np.float64):
    """WeightedBPDNDictLearn (sporco/dictlrn/wbpdndl.py:131-210 on dictlrn.py:293-375): ``iters`` outer iterations of
    one x step (flat options ``xo``) and one D step (``do``); returns the final D and X and the outer columns."""
    import _pgm_bpdn_numpy as pb
    dtype = np.dtype(dtype)
    xo = dict(xo or {}, MaxMainIter=1)
    do = dict(do or {}, MaxMainIter=1)
    S = np.asarray(S, dtype=dtype)
    D = get_pcn(do.get('ZeroMean', False), do.get('NonNegCoef', False))(np.asarray(D0, dtype=np.float64)).astype(dtype)
    do['X0'] = D
    if lmbda is None:
        lmbda = pb.default_lmbda(D, S)
    Wf = weight(W, dtype)
    out = {f: [] for f in LEARN_FIELDS}
    xs = ds = None
    for j in range(iters):
        rx = pb.run(D, S, lmbda, xo, W=W, dtype=dtype, state=xs, iters=1)
        xs = rx['state']
        rd = run(rx['X'], S, do, W=W, dtype=dtype, state=ds)
        ds = rd['state']
        D = rd['X']
        if accurate:
            R = np.asarray(D.dot(rx['X']) - S, np.float64)
            dfd = 0.5 * float(np.sum(np.asarray(Wf, np.float64) * R ** 2))
            rl1 = float(np.sum(np.abs(np.asarray(rx['X'], np.float64))))
            obj = dfd + float(dtype.type(lmbda)) * rl1
        else:
            obj, dfd, rl1 = rx['ObjFun'][-1], rx['DFid'][-1], rx['RegL1'][-1]
        for f, v in zip(LEARN_FIELDS, (obj, dfd, rl1, rd['Cnstr'][-1], rx['Rsdl'][-1], rx['L'][-1], rd['Rsdl'][-1],
                                       rd['L'][-1])):
            out[f].append(float(v))
    res = {f: np.asarray(v, dtype=np.float64) for f, v in out.items()}
    res.update(D=D, X=rx['X'], lmbda=float(lmbda))
    return res
