"""Host model of the L-BFGS learner's specification ("The bound-constrained L-BFGS"):
the objective ssqTrain over propagate's recursion, its adjoint gradient and the optimiser, in numpy and
sequential in time.  What the device is compared with -- by properties and known optima, not iterate for
iterate: sums taken in scan order and in serial order differ in the last bits.

The objective works on arrays of any dtype, so it can be evaluated at a complex theta (the complex-step
derivative of the tests)."""
import numpy as np

CONVERGED, MAXIT, LINESEARCH, NONFINITE = 0, 1, 2, 3
LS_TRIALS = 20
ARMIJO = 1e-4
CURV_EPS = 2.2e-16


def split(theta, p, q):
    """A, B[p], C, D[q], mu1 of a packed theta (Q, R, V1 do not enter the objective)."""
    return theta[0], theta[1:1 + p], theta[1 + p], theta[2 + p:2 + p + q], theta[4 + p + q]


def forward(theta, y, u, v):
    """x [T], r [T] (0 where y is not finite); u: p x T or None, v: q x T or None."""
    T = y.size
    p = 1 if u is None else u.shape[0]
    q = 1 if v is None else v.shape[0]
    A, B, C, D, mu1 = split(theta, p, q)
    dt = np.result_type(theta.dtype, np.float64)
    x = np.zeros(T, dtype=dt)
    x[0] = mu1
    for t in range(T - 1):
        x[t + 1] = A * x[t] + (B @ u[:, t] if u is not None else 0.0)
    Y = C * x + (D @ v if v is not None else 0.0)
    obs = np.isfinite(y)
    r = np.where(obs, np.where(obs, y, 0.0) - Y, 0.0)
    return x, r


def ssq(theta, y, u, v):
    theta = np.asarray(theta)
    with np.errstate(all="ignore"):
        _, r = forward(theta, np.asarray(y, dtype=np.float64), u, v)
        return np.sum(r * r)


def ssq_grad(theta, y, u, v):
    """-> f, grad [P] by the adjoint recursion lam_t = -2 C r_t + A lam_{t+1}."""
    theta = np.asarray(theta, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    T = y.size
    p = 1 if u is None else u.shape[0]
    q = 1 if v is None else v.shape[0]
    A, _, C, _, _ = split(theta, p, q)
    with np.errstate(all="ignore"):
        x, r = forward(theta, y, u, v)
        lam = np.zeros(T + 1)
        for t in range(T - 1, -1, -1):
            lam[t] = -2.0 * C * r[t] + A * lam[t + 1]
        g = np.zeros(theta.size)
        g[0] = np.sum(lam[1:T] * x[:T - 1])
        if u is not None:
            g[1:1 + p] = u[:, :T - 1] @ lam[1:T]
        g[1 + p] = -2.0 * np.sum(r * x)
        if v is not None:
            g[2 + p:2 + p + q] = -2.0 * (v @ r)
        g[4 + p + q] = lam[0]
        return np.sum(r * r), g


def select(values, select_max):
    """First largest (select_max) or first smallest finite value; -1 if none."""
    values = np.asarray(values, dtype=np.float64)
    fin = np.isfinite(values)
    if not fin.any():
        return -1
    v = np.where(fin, values, -np.inf if select_max else np.inf)
    return int(np.argmax(v) if select_max else np.argmin(v))


def minimise(fun, fun_grad, par0, lb, ub, maxit=100, lmm=5, factr=1e7, pgtol=0.0):
    """The optimiser of the specification on any objective: fun(x) -> f, fun_grad(x) -> f, g.
    Returns dict par, value, n_iter, n_eval, status."""
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    par0 = np.asarray(par0, dtype=np.float64)
    ftol = factr * 2.0 ** -52
    x = np.clip(par0, lb, ub)
    with np.errstate(all="ignore"):
        f, g = fun_grad(x)
    n_eval, k = 1, 0
    if not np.isfinite(f):
        return {"par": par0.copy(), "value": np.nan, "n_iter": 0, "n_eval": 1, "status": NONFINITE}
    pairs = []                                   # (s, y), newest first
    while True:
        active = (lb == ub) | ((x <= lb) & (g > 0)) | ((x >= ub) & (g < 0))
        pg = np.where(active, 0.0, g)
        pgn = np.max(np.abs(pg)) if not np.any(np.isnan(pg)) else np.nan
        if pgn <= pgtol:
            status = CONVERGED
            break
        if k >= maxit:
            status = MAXIT
            break
        d = -pg
        if pairs:
            free = ~active
            use, al = [], []
            qv = pg.copy()
            gamma = None
            for s, yv in pairs:
                sy, yy = np.sum(s[free] * yv[free]), np.sum(yv[free] * yv[free])
                ok = sy > CURV_EPS * yy
                use.append((ok, sy))
                a = 0.0
                if ok:
                    a = np.sum(s[free] * qv[free]) / sy
                    qv[free] -= a * yv[free]
                    if gamma is None:
                        gamma = sy / yy
                al.append(a)
            qv *= 1.0 if gamma is None else gamma
            for j in range(len(pairs) - 1, -1, -1):
                ok, sy = use[j]
                if ok:
                    s, yv = pairs[j]
                    be = np.sum(yv[free] * qv[free]) / sy
                    qv[free] += (al[j] - be) * s[free]
            d = np.where(active, 0.0, -qv)
        gd = np.sum(g * d)
        if pairs and not gd < 0.0:
            pairs = []
            d = -pg
            gd = np.sum(g * d)
        alpha = min(1.0, 1.0 / pgn) if k == 0 else 1.0
        ok = False
        for _ in range(LS_TRIALS):
            xt = np.clip(x + alpha * d, lb, ub)
            with np.errstate(all="ignore"):
                ft = fun(xt)
            n_eval += 1
            if np.isfinite(ft) and ft <= f + ARMIJO * np.sum(g * (xt - x)):
                ok = True
                break
            alpha *= 0.5
        if not ok:
            status = LINESEARCH
            break
        with np.errstate(all="ignore"):
            ft, gt = fun_grad(xt)
        n_eval += 1
        s, yv = xt - x, gt - g
        if np.sum(s * yv) > CURV_EPS * np.sum(yv * yv):
            pairs = ([(s, yv)] + pairs)[:lmm]
        drop = (f - ft) / max(abs(f), abs(ft), 1.0)
        x, f, g = xt, ft, gt
        k += 1
        if drop <= ftol:
            status = CONVERGED
            break
    return {"par": x, "value": float(f), "n_iter": k, "n_eval": n_eval, "status": status}


def bfgs(y, u, v, par0, lb, ub, **kw):
    """minimise() on ssqTrain of one series from one start point."""
    return minimise(lambda x: ssq(x, y, u, v), lambda x: ssq_grad(x, y, u, v), par0, lb, ub, **kw)
