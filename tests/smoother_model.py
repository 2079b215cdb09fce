"""Host model of the smoother family -- Kalman_smoother (src/EM.cpp:22-131), the penalty of
penalized_likelihood (R/LDS_GA.R:34-40), propagate (src/EM.cpp:295-356), Mstep (src/EM.cpp:139-229) and the EM
loop LDS_EM made of them (src/EM.cpp:245-280) -- in plain numpy, serial in time and vectorised over the rows of a packed theta [n, 6+p+q] =
[A, B(p), C, D(q), Q, R, mu1, V1].  It works in float64 and in numpy.longdouble: the longdouble run is the
extended-precision yardstick that says whether a gap between a device kernel and the fp64 oracle belongs to the
kernel or to the oracle (tests/test_smoother_model_host.py, tests/test_gpu_smoother_family.py; the EM loop:
tests/test_em_model_host.py, tests/test_gpu_em_family.py).

A second statement of the recursions, independent of tests/plgrad_model.py and of oracle/ldsr_oracle.c: the
reference's expressions in the reference's order, its absent-input branches (u or v None), J[T-1] of
src/EM.cpp:98, the likelihood over the finite y_t.  +-Inf in y counts as missing in the filter too (the
project's stated deviation; the reference's update tests is_na only).  Arrays are [n, T]; time is 0-based."""
import numpy as np

PI = 3.141592653589793238463        # src/EM.cpp:3, a double in the reference


def _theta(theta, p, q, dtype):
    th = np.atleast_2d(np.asarray(theta, dtype=dtype))
    if th.shape[1] != 6 + p + q:
        raise ValueError("theta has %d columns, expected 6+p+q = %d" % (th.shape[1], 6 + p + q))
    return (th[:, 0], th[:, 1:1 + p], th[:, 1 + p], th[:, 2 + p:2 + p + q], th[:, 2 + p + q], th[:, 3 + p + q],
            th[:, 4 + p + q], th[:, 5 + p + q])


def _dims(u, v):
    return (1 if u is None else np.asarray(u).shape[0]), (1 if v is None else np.asarray(v).shape[0])


def _inputs(y, u, v, dtype):
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    obs = np.isfinite(y)
    yd = np.where(obs, y, 0.0).astype(dtype)
    u = None if u is None else np.asarray(u, dtype=np.float64).astype(dtype)
    v = None if v is None else np.asarray(v, dtype=np.float64).astype(dtype)
    for a in (u, v):
        if a is not None and (a.ndim != 2 or a.shape[1] != y.size):
            raise ValueError("u and v must be k x T")
    return yd, obs, u, v


def _likelihood(yd, obs, Yp, Vp, C, R, stdlik, dtype):
    """src/EM.cpp:113-124 (and :339-350): Yp, Vp are [T, n].  With nothing observed the sum is empty:
    0 without stdlik, 0/0 = NaN with it."""
    n_obs = int(np.count_nonzero(obs))
    delta = yd[obs, None] - Yp[obs]
    Sigma = C * Vp[obs] * C + R
    acc = np.sum(delta / Sigma * delta + np.log(Sigma), axis=0, dtype=dtype)
    lik = dtype(-0.5) * n_obs * np.log(dtype(2) * dtype(PI)) - dtype(0.5) * acc
    if stdlik:
        lik = lik / dtype(n_obs)
    return lik


def smoother(theta, y, u, v, stdlik=True, dtype=np.float64):
    """Kalman_smoother for every row of theta -> {"X", "Y", "V", "J": [n, T], "lik": [n]} in `dtype`."""
    dtype = np.dtype(dtype).type
    p, q = _dims(u, v)
    A, B, C, D, Q, R, mu1, V1 = _theta(theta, p, q, dtype)
    yd, obs, u, v = _inputs(y, u, v, dtype)
    T, n = yd.size, A.size
    if T < 2:
        raise ValueError("T must be >= 2")
    one = dtype(1)
    with np.errstate(all="ignore"):
        bu = None if u is None else (B @ u).T.copy()        # [T, n]
        dv = None if v is None else (D @ v).T.copy()
        Xp, Vp, Yp, Xu, Vu = (np.empty((T, n), dtype=dtype) for _ in range(5))
        xu = vu = None
        for t in range(T):                                  # :48-90
            if t == 0:
                xp, vp = mu1, V1
            else:
                xp = A * xu if bu is None else A * xu + bu[t - 1]
                vp = A * vu * A + Q
            yp = C * xp if dv is None else C * xp + dv[t]
            if obs[t]:
                K = vp * C * (one / (C * vp * C + R))
                xu = xp + K * (yd[t] - yp)
                vu = (one - K * C) * vp
            else:
                xu, vu = xp, vp
            Xp[t], Vp[t], Yp[t], Xu[t], Vu[t] = xp, vp, yp, xu, vu
        Xs, Vs = Xu.copy(), Vu.copy()                       # :94-104
        J = np.zeros((T, n), dtype=dtype)
        J[T - 1] = Vu[T - 1] * A * (one / (A * Vu[T - 1] * A + Q))
        for t in range(T - 2, -1, -1):
            j = Vu[t] * A * (one / Vp[t + 1])
            Xs[t] = Xu[t] + j * (Xs[t + 1] - Xp[t + 1])
            Vs[t] = Vu[t] + j * (Vs[t + 1] - Vp[t + 1]) * j
            J[t] = j
        Ys = C * Xs if dv is None else C * Xs + dv          # :106-110
        lik = _likelihood(yd, obs, Yp, Vp, C, R, stdlik, dtype)
    return {"X": Xs.T.copy(), "Y": Ys.T.copy(), "V": Vs.T.copy(), "J": J.T.copy(), "lik": lik}


def ssq(theta, X, u):
    """The penalty of R/LDS_GA.R:34-40, sum_t (X_{t+1} - A X_t - B u_t)^2 -> [n], in X's dtype."""
    X = np.atleast_2d(X)
    dtype = X.dtype.type
    p = 1 if u is None else np.asarray(u).shape[0]
    th = np.atleast_2d(np.asarray(theta, dtype=dtype))
    A, B = th[:, 0], th[:, 1:1 + p]
    e = X[:, 1:] - A[:, None] * X[:, :-1]
    if u is not None:
        e = e - B @ np.asarray(u, dtype=np.float64).astype(dtype)[:, :-1]
    return np.sum(e * e, axis=1, dtype=dtype)


def propagate(theta, u, v, y, stdlik=True, dtype=np.float64):
    """propagate: the open-loop forward pass -> {"X", "Y", "V": [n, T], "lik": [n]}."""
    dtype = np.dtype(dtype).type
    p, q = _dims(u, v)
    A, B, C, D, Q, R, mu1, V1 = _theta(theta, p, q, dtype)
    yd, obs, u, v = _inputs(y, u, v, dtype)
    T, n = yd.size, A.size
    with np.errstate(all="ignore"):
        bu = None if u is None else (B @ u).T.copy()
        Xp, Vp = np.empty((T, n), dtype=dtype), np.empty((T, n), dtype=dtype)
        Xp[0], Vp[0] = mu1, V1                               # :318-319
        for t in range(1, T):                               # :322-329
            Xp[t] = A * Xp[t - 1] if bu is None else A * Xp[t - 1] + bu[t - 1]
            Vp[t] = A * Vp[t - 1] * A + Q
        Yp = C * Xp if v is None else C * Xp + (D @ v).T    # :332-336
        lik = _likelihood(yd, obs, Yp, Vp, C, R, stdlik, dtype)
    return {"X": Xp.T.copy(), "Y": Yp.T.copy(), "V": Vp.T.copy(), "lik": lik}


def solve(M, b):
    """x with M x = b by Gauss-Jordan elimination with partial pivoting, in M's dtype (numpy.linalg has no
    longdouble).  M [k, k], b [k]."""
    k = b.size
    W = np.concatenate([M, b[:, None]], axis=1).copy()
    for c in range(k):
        piv = c + int(np.argmax(np.abs(W[c:, c])))
        if not np.abs(W[piv, c]) > 0:
            raise np.linalg.LinAlgError("singular matrix")
        if piv != c:
            W[[c, piv]] = W[[piv, c]]
        W[c] = W[c] / W[c, c]
        for r in range(k):
            if r != c:
                W[r] = W[r] - W[r, c] * W[c]
    return W[:, k]


def mstep(y, u, v, fit, dtype=np.float64):
    """Mstep for every row of fit["X"], fit["V"], fit["J"] ([n, T] or [T]) -> packed theta [n, 6+p+q].
    The reference's two systems x = P inv(M) with symmetric M are solved as M x = P."""
    dtype = np.dtype(dtype).type
    p, q = _dims(u, v)
    yd, obs, u, v = _inputs(y, u, v, dtype)
    T = yd.size
    X, V, J = (np.atleast_2d(np.asarray(fit[k])).astype(dtype) for k in "XVJ")     # (a longdouble fit stays one)
    n = X.shape[0]
    th = np.zeros((n, 6 + p + q), dtype=dtype)              # B, D start at 0 (:154, :186)
    yo, n_obs = yd[obs], dtype(np.count_nonzero(obs))
    vo = None if v is None else v[:, obs]
    with np.errstate(all="ignore"):
        for i in range(n):
            x, Vi, Ji = X[i], V[i], J[i]
            xo = x[obs]
            Syx = yo @ xo                                   # :151-152
            Sxx = xo @ xo + np.sum(Vi[obs], dtype=dtype)
            if vo is not None:                              # :158-170
                P1 = np.concatenate([[Syx], vo @ yo])
                P2 = np.empty((1 + q, 1 + q), dtype=dtype)
                P2[0, 0] = Sxx
                P2[0, 1:] = P2[1:, 0] = vo @ xo
                P2[1:, 1:] = vo @ vo.T
                CD = solve(P2, P1)
                Cn, Dn = CD[0], CD[1:]
                yhat = Cn * xo + Dn @ vo
                th[i, 2 + p:2 + p + q] = Dn
            else:                                           # :172-173
                Cn = Syx * (dtype(1) / Sxx)
                yhat = Cn * xo
            Rn = ((yo - yhat) @ yo) / n_obs                 # :177
            x0, x1 = x[:T - 1], x[1:]
            Tx1x = x1 @ x0 + Vi[1:] @ Ji[:T - 1]            # :180-183
            Txx = x0 @ x0 + np.sum(Vi[:T - 1], dtype=dtype)
            Tx1x1 = x1 @ x1 + np.sum(Vi[1:], dtype=dtype)
            if u is not None:                               # :190-210
                u0 = u[:, :T - 1]
                Tx1u = u0 @ x1
                P3 = np.concatenate([[Tx1x], Tx1u])
                P4 = np.empty((1 + p, 1 + p), dtype=dtype)
                P4[0, 0] = Txx
                P4[0, 1:] = P4[1:, 0] = u0 @ x0
                P4[1:, 1:] = u0 @ u0.T
                AB = solve(P4, P3)
                An, Bn = AB[0], AB[1:]
                Qn = (Tx1x1 - An * Tx1x - Bn @ Tx1u) / dtype(T - 1)
                th[i, 1:1 + p] = Bn
            else:                                           # :212-213
                An = Tx1x * (dtype(1) / Txx)
                Qn = (Tx1x1 - An * Tx1x) / dtype(T - 1)
            th[i, 0], th[i, 1 + p] = An, Cn
            th[i, 2 + p + q], th[i, 3 + p + q] = Qn, Rn
            th[i, 4 + p + q], th[i, 5 + p + q] = x[0], Vi[0]   # :218-219
    return th


def em(theta0, y, u, v, niter=1000, tol=1e-5, dtype=np.float64):
    """LDS_EM (src/EM.cpp:245-280) for every row of theta0, from smoother() and mstep() above: E, M, E, then
    M and E per iteration; a row stops after iteration i >= 2 once |lik_i - lik_{i-1}| and |lik_{i-1} - lik_{i-2}|
    are both below tol (:272), or after niter iterations.  -> {"theta" [n, 6+p+q], "lik" [n], "liks" [n, niter]
    (NaN behind n_iter) in `dtype`, "n_iter" [n] (the reference's lastIter), "margin" [n] float64}.  margin is
    the smallest | |dlik| - tol | over the differences the row's stop decisions read: a result whose liks are
    nearer than margin / 2 to this one's stops at the same iteration."""
    dtype = np.dtype(dtype).type
    if niter < 2:
        raise ValueError("niter must be >= 2 (the reference reads lik[1], src/EM.cpp:256)")
    theta = np.atleast_2d(np.asarray(theta0)).astype(dtype)
    n = theta.shape[0]
    liks = np.full((n, niter), np.nan, dtype=dtype)
    n_iter = np.full(n, 2, dtype=np.int32)
    margin = np.full(n, np.inf)
    fit = smoother(theta, y, u, v, dtype=dtype)                 # i = 0 (:251-253)
    liks[:, 0] = fit["lik"]
    theta = mstep(y, u, v, fit, dtype=dtype)
    fit = smoother(theta, y, u, v, dtype=dtype)                 # i = 1 (:255-256)
    liks[:, 1] = fit["lik"]
    lik = np.array(fit["lik"], dtype=dtype)
    run = np.arange(n)                                          # the rows still iterating
    for i in range(2, niter):                                   # :259-275
        th = mstep(y, u, v, fit, dtype=dtype)
        fit = smoother(th, y, u, v, dtype=dtype)
        theta[run], lik[run], liks[run, i], n_iter[run] = th, fit["lik"], fit["lik"], i + 1
        with np.errstate(invalid="ignore"):
            d1, d2 = np.abs(liks[run, i] - liks[run, i - 1]), np.abs(liks[run, i - 1] - liks[run, i - 2])
            m = np.minimum(np.abs(d1 - dtype(tol)), np.abs(d2 - dtype(tol))).astype(np.float64)
            margin[run] = np.fmin(margin[run], m)
            go = ~((d1 < tol) & (d2 < tol))
        if not go.any():
            break
        run = run[go]
        fit = {k: fit[k][go] for k in "XVJ"}
    return {"theta": theta, "lik": lik, "liks": liks, "n_iter": n_iter, "margin": margin}
