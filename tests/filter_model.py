"""Host model of the Kalman filter's outputs and the innovation diagnostics in plain
numpy, serial in time and vectorised over the rows of a packed theta [n, 6+p+q] = [A, B(p), C, D(q), Q, R, mu1, V1].
It works in float64 and in numpy.longdouble; the longdouble run is the yardstick of tests/test_gpu_filter.py.

Its own statement of section 12's definitions, line by line, independent of tests/smoother_model.py and of
tests/plgrad_model.py (tests/test_filter_host.py compares it with the first).  Time is 0-based; obs_t =
isfinite(y_t); an absent u (v) drops the B u (D v) term.  Arrays are [n, T]."""
import numpy as np

ROWS = ("Xp", "Vp", "Yp", "Xu", "Vu", "e", "S", "ll")
LOG_2PI = "1.837877066409345483560659472811235279722794947275566825634"     # log(2 pi)


def _cast(a, dtype):
    return None if a is None else np.asarray(a, dtype=np.float64).astype(dtype)


def acf_holes(z, obs, n_lags):
    """Section 12's autocorrelations of z [n, T] (any values where obs [T] is False): pairs (t, t + k) with both
    steps observed, one common mean and denominator.  -> zmean [n], zvar [n], acf [n, n_lags] in z's dtype."""
    z = np.atleast_2d(z)
    dtype = z.dtype.type
    obs = np.asarray(obs, dtype=bool)
    n, T = z.shape
    n_obs = int(np.count_nonzero(obs))
    nan = dtype(np.nan)
    with np.errstate(all="ignore"):
        if n_obs == 0:
            return np.full(n, nan), np.full(n, nan), np.full((n, n_lags), nan)
        zo = z[:, obs]
        zmean = np.sum(zo, axis=1, dtype=dtype) / dtype(n_obs)
        dev = np.where(obs[None, :], z - zmean[:, None], dtype(0))
        den = np.sum(dev * dev, axis=1, dtype=dtype)
        zvar = den / dtype(n_obs)
        acf = np.full((n, n_lags), nan)
        for k in range(1, n_lags + 1):
            pair = obs[:T - k] & obs[k:]
            if not pair.any():
                continue
            num = np.sum(dev[:, :T - k][:, pair] * dev[:, k:][:, pair], axis=1, dtype=dtype)
            acf[:, k - 1] = np.where(den != 0, num / den, nan)
    return zmean, zvar, acf


def kalman_filter(theta, y, u, v, stdlik=True, n_lags=0, dtype=np.float64):
    """-> {"Xp", "Vp", "Yp", "Xu", "Vu", "e", "S", "ll": [n, T], "lik", "zmean", "zvar": [n], "acf": [n, n_lags],
    "n_obs": int} in `dtype`."""
    dtype = np.dtype(dtype).type
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    T = y.size
    obs = np.isfinite(y)
    yd = np.where(obs, y, 0.0).astype(dtype)
    u, v = _cast(u, dtype), _cast(v, dtype)
    p = 1 if u is None else u.shape[0]
    q = 1 if v is None else v.shape[0]
    th = np.atleast_2d(np.asarray(theta, dtype=dtype))
    assert th.shape[1] == 6 + p + q
    A, B, C, D = th[:, 0], th[:, 1:1 + p], th[:, 1 + p], th[:, 2 + p:2 + p + q]
    Q, R, mu1, V1 = th[:, 2 + p + q], th[:, 3 + p + q], th[:, 4 + p + q], th[:, 5 + p + q]
    n = th.shape[0]
    zero, one, half, nan = dtype(0), dtype(1), dtype("0.5"), dtype(np.nan)
    log2pi = dtype(LOG_2PI)
    out = {k: np.empty((n, T), dtype=dtype) for k in ROWS}
    z = np.full((n, T), nan, dtype=dtype)
    with np.errstate(all="ignore"):
        for t in range(T):
            if t == 0:
                xp, vp = mu1.copy(), V1.copy()
            else:
                xp = A * xu
                if u is not None:
                    xp = xp + B @ u[:, t - 1]
                vp = A * vu * A + Q
            yp = C * xp
            if v is not None:
                yp = yp + D @ v[:, t]
            S = C * vp * C + R
            if obs[t]:
                e = yd[t] - yp
                K = vp * C / S
                xu = xp + K * e
                vu = (one - K * C) * vp
                ll = -half * (log2pi + np.log(S) + e * e / S)
                z[:, t] = e / np.sqrt(S)
            else:
                e = np.full(n, nan, dtype=dtype)
                xu, vu = xp, vp
                ll = np.full(n, zero, dtype=dtype)
            for k, a in zip(ROWS, (xp, vp, yp, xu, vu, e, S, ll)):
                out[k][:, t] = a
        n_obs = int(np.count_nonzero(obs))
        lik = np.sum(out["ll"], axis=1, dtype=dtype)
        if stdlik:
            lik = lik / dtype(n_obs)
        out["lik"] = lik
        out["zmean"], out["zvar"], out["acf"] = acf_holes(z, obs, n_lags)
    out["n_obs"] = n_obs
    return out


def ljung_box(acf, n_obs):
    """Q = n (n + 2) sum_k acf_k^2 / (n - k), n = n_obs, over the rows of acf [n, n_lags] -> [n] float64"""
    acf = np.atleast_2d(np.asarray(acf, dtype=np.float64))
    k = np.arange(1, acf.shape[1] + 1)
    return n_obs * (n_obs + 2.0) * np.sum(acf * acf / (n_obs - k), axis=1)
