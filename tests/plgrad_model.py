"""Host model of the penalised-likelihood objective of LDS_BFGS_with_update (R/LDS_GA.R:90-127): the
forward recursions of Kalman_smoother(stdlik = FALSE) and penalized_likelihood, serial in time, and the
hand-derived reverse-mode gradient, in numpy.  What a device implementation of this learner is to be
compared with (the project has none yet); the optimiser is bfgs_model.minimise on f = -pl.

Time is 0-based, o_t = 1 where y_t is finite:
    Xp_0 = mu1, Vp_0 = V1;  t >= 1: Xp_t = A Xu_{t-1} + B.u_{t-1},  Vp_t = A^2 Vu_{t-1} + Q
    S_t = C^2 Vp_t + R,  d_t = y_t - C Xp_t - D.v_t,  K_t = o_t Vp_t C / S_t
    Xu_t = Xp_t + K_t d_t,  Vu_t = (1 - K_t C) Vp_t
    lik = -1/2 sum_{o_t} (log 2 pi + log S_t + d_t^2 / S_t)
    J_t = Vu_t A / Vp_{t+1} (t <= T-2),  Xs_{T-1} = Xu_{T-1},  Xs_t = Xu_t + J_t (Xs_{t+1} - Xp_{t+1})
    e_t = Xs_{t+1} - A Xs_t - B.u_t (t <= T-2),  ssq = sum e_t^2,  pl = lik - lambda ssq

The forward pass works on arrays of any dtype: complex (the complex-step derivative of the tests) and
numpy.longdouble (the yardstick of the model's own rounding error)."""
import numpy as np

import bfgs_model as B

LOG_2PI = 1.8378770664093453


def _dims(u, v):
    return (1 if u is None else u.shape[0]), (1 if v is None else v.shape[0])


def _unpack(theta, p, q):
    return (theta[0], theta[1:1 + p], theta[1 + p], theta[2 + p:2 + p + q], theta[2 + p + q], theta[3 + p + q],
            theta[4 + p + q], theta[5 + p + q])


def forward(theta, y, u, v, lam):
    """-> dict of the forward quantities ([T] each, J and e with a 0 in slot T-1) and lik, ssq, pl."""
    theta = np.asarray(theta)
    dt = np.result_type(theta.dtype, np.float64)
    T = y.size
    p, q = _dims(u, v)
    A, Bv, C, D, Q, R, mu1, V1 = _unpack(theta, p, q)
    obs = np.isfinite(y)
    y0 = np.where(obs, y, 0.0).astype(dt)
    bu = (Bv @ u if u is not None else np.zeros(T)).astype(dt)
    dv = (D @ v if v is not None else np.zeros(T)).astype(dt)
    Xp, Vp, S, d, K, Xu, Vu, Xs, J, e = (np.zeros(T, dtype=dt) for _ in range(10))
    lik = dt.type(0)
    for t in range(T):
        Xp[t] = mu1 if t == 0 else A * Xu[t - 1] + bu[t - 1]
        Vp[t] = V1 if t == 0 else A * A * Vu[t - 1] + Q
        S[t] = C * C * Vp[t] + R
        if obs[t]:
            d[t] = y0[t] - C * Xp[t] - dv[t]
            K[t] = Vp[t] * C / S[t]
            lik = lik - 0.5 * (LOG_2PI + np.log(S[t]) + d[t] * d[t] / S[t])
        Xu[t] = Xp[t] + K[t] * d[t]
        Vu[t] = (1 - K[t] * C) * Vp[t]
    Xs[T - 1] = Xu[T - 1]
    for t in range(T - 2, -1, -1):
        J[t] = Vu[t] * A / Vp[t + 1]
        Xs[t] = Xu[t] + J[t] * (Xs[t + 1] - Xp[t + 1])
    e[:T - 1] = Xs[1:] - A * Xs[:T - 1] - bu[:T - 1]
    ssq = np.sum(e * e)
    return {"obs": obs, "Xp": Xp, "Vp": Vp, "S": S, "d": d, "K": K, "Xu": Xu, "Vu": Vu, "Xs": Xs, "J": J, "e": e,
            "lik": lik, "ssq": ssq, "pl": lik - lam * ssq}


def pl(theta, y, u, v, lam):
    with np.errstate(all="ignore"):
        return forward(theta, np.asarray(y, dtype=np.float64), u, v, lam)["pl"]


def pl_grad(theta, y, u, v, lam, dtype=np.float64):
    """-> pl, d pl / d theta [P].  Three linear recurrences over the stored forward pass:
    a_t (adjoint of Xs_t) runs forward with coefficient J_{t-1}; xp_t (of Xp_t) and vp_t (of Vp_t) run
    backward with A (1 - K_t C) and its square."""
    theta = np.asarray(theta, dtype=dtype)
    y = np.asarray(y, dtype=np.float64)
    T = y.size
    p, q = _dims(u, v)
    A, _, C, _, _, _, _, _ = _unpack(theta, p, q)
    with np.errstate(all="ignore"):
        F = forward(theta, y, u, v, lam)
        obs, Xp, Vp, S, d, K, Xu, Vu, Xs, J, e = (F[k] for k in ("obs", "Xp", "Vp", "S", "d", "K", "Xu", "Vu", "Xs",
                                                                "J", "e"))
        dt = Xp.dtype
        eb = -2 * lam * e                                   # adjoint of e_t (0 at T-1)
        g = np.zeros(theta.size, dtype=dt)
        gA = gQ = gC = gR = dt.type(0)
        gB, gD = np.zeros(p, dtype=dt), np.zeros(q, dtype=dt)
        # the smoothed means, forward: Xs_t feeds e_{t-1}, e_t and Xs_{t-1}
        a = np.zeros(T, dtype=dt)
        for t in range(T):
            a[t] = (eb[t - 1] if t > 0 else 0) - A * eb[t] + (J[t - 1] * a[t - 1] if t > 0 else 0)
        Jb = np.zeros(T, dtype=dt)                          # adjoint of J_t
        Jb[:T - 1] = a[:T - 1] * (Xs[1:] - Xp[1:])
        # the filter, backward
        xp1 = vp1 = dt.type(0)                              # adjoints of Xp_{t+1}, Vp_{t+1}
        for t in range(T - 1, -1, -1):
            xu = a[t] + A * xp1
            vu = A * A * vp1
            if t < T - 1:
                vu = vu + Jb[t] * A / Vp[t + 1]
                gA = gA - Xs[t] * eb[t] + Jb[t] * Vu[t] / Vp[t + 1] + xp1 * Xu[t] + 2 * A * Vu[t] * vp1
                if u is not None:
                    gB = gB + u[:, t] * (xp1 - eb[t])
                gQ = gQ + vp1
            xp = xu - (J[t - 1] * a[t - 1] if t > 0 else 0)
            vp = vu - (Jb[t - 1] * J[t - 1] / Vp[t] if t > 0 else 0)
            if obs[t]:
                Kb = xu * d[t] - C * Vp[t] * vu
                Sb = -0.5 * (1 / S[t] - d[t] * d[t] / (S[t] * S[t])) - Kb * K[t] / S[t]
                db = -d[t] / S[t] + K[t] * xu
                gC = gC - K[t] * Vp[t] * vu + Kb * Vp[t] / S[t] - db * Xp[t] + 2 * C * Vp[t] * Sb
                if v is not None:
                    gD = gD - db * v[:, t]
                gR = gR + Sb
                xp = xp - C * db
                vp = vp - K[t] * C * vu + Kb * C / S[t] + C * C * Sb
            xp1, vp1 = xp, vp
        g[0] = gA
        if u is not None:
            g[1:1 + p] = gB
        g[1 + p] = gC
        if v is not None:
            g[2 + p:2 + p + q] = gD
        g[2 + p + q], g[3 + p + q], g[4 + p + q], g[5 + p + q] = gQ, gR, xp1, vp1
        return F["pl"], g


def neg_pl(theta, y, u, v, lam):
    return -pl(theta, y, u, v, lam)


def neg_pl_grad(theta, y, u, v, lam):
    f, g = pl_grad(theta, y, u, v, lam)
    return -f, -g


def bfgs(y, u, v, par0, lb, ub, lam=1.0, **kw):
    """bfgs_model.minimise on f = -pl of one series from one start point."""
    return B.minimise(lambda x: float(neg_pl(x, y, u, v, lam)), lambda x: neg_pl_grad(x, y, u, v, lam), par0, lb, ub,
                      **kw)
