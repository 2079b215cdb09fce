"""The Kalman filter's own outputs and the innovation diagnostics over
ldsr_filter_batch: the one-step-ahead prediction, the filtered state, the innovation and its variance, the
per-step likelihood terms -- what Kalman_smoother (src/EM.cpp:43-90,115-120) computes on its way and discards --
and the whiteness statistics of the standardised innovations, the adequacy check of a fitted state-space model."""
import math

import numpy as np

from . import _lib
from .api import _d, _dims, _i, _offsets, _series, pack_theta

ROWS = ("Xp", "Vp", "Yp", "Xu", "Vu", "e", "S", "ll")


def filter_batch(y, u, v, theta, cell_offsets=None, stdlik=True, n_lags=0, rows=ROWS, device=0):
    """One filter pass per cell's theta, packed [n_cells, 6+p+q]; all cells in one launch.  rows: which of
    Xp, Vp, Yp, Xu, Vu, e, S, ll ([n_cells, T] each) to bring back -- a row not named is neither written nor
    copied.  -> dict of the requested rows, lik [n_cells], n_obs [n_cells], zmean, zvar [n_cells], status
    [n_cells] and, with n_lags > 0, acf [n_cells, n_lags]."""
    rows = tuple(rows)
    for r in rows:
        if r not in ROWS:
            raise ValueError("unknown row %r: the rows are %s" % (r, ", ".join(ROWS)))
    Y, U, V, S, T, p, q, shared = _series(y, u, v)
    theta = np.ascontiguousarray(np.atleast_2d(theta), dtype=np.float64)
    if theta.shape[1] != 6 + p + q:
        raise ValueError("theta must be [n_cells, %d]" % (6 + p + q))
    n = theta.shape[0]
    off = _offsets(cell_offsets, S, n)
    n_lags = int(n_lags)
    out = {r: np.empty((n, T)) for r in rows}
    lik, zstat, status = np.empty(n), np.empty((n, 2)), np.empty(n, dtype=np.int32)
    acf = np.empty((n, n_lags)) if n_lags > 0 else None
    _lib.check(_lib.lib().ldsr_filter_batch(device, S, T, p, q, _d(Y), _d(U), _d(V), shared, _i(off), _d(theta),
                                            int(bool(stdlik)), n_lags, *[_d(out.get(r)) for r in ROWS], _d(lik),
                                            _d(zstat), _d(acf), _i(status)))
    n_series_obs = np.isfinite(Y).sum(axis=1)
    out.update(lik=lik, zmean=zstat[:, 0].copy(), zvar=zstat[:, 1].copy(), status=status,
               n_obs=np.repeat(n_series_obs, np.diff(off)).astype(np.int64))
    if acf is not None:
        out["acf"] = acf
    return out


def Kalman_filter(y, u, v, theta, stdlik=True, device=0):
    """The filter at one theta list, as Kalman_smoother takes it.
    -> {"Xp","Vp","Yp","Xu","Vu","e","S","ll": 1 x T arrays, "lik": float}"""
    p, q = _dims(u, v)
    r = filter_batch(y, u, v, pack_theta(theta, p, q)[None, :], stdlik=stdlik, device=device)
    out = {k: r[k] for k in ROWS}
    out["lik"] = float(r["lik"][0])
    return out


# ---- the chi-square tail (no scipy in this project) ------------------------------------------------------------
def _gamma_q(a, x):
    """Regularised upper incomplete gamma Q(a, x): the series of P below x < a + 1, the continued fraction of Q
    (modified Lentz) above."""
    if not (a > 0.0) or x != x:
        return float("nan")
    if x <= 0.0:
        return 1.0
    if x == float("inf"):
        return 0.0
    front = math.exp(a * math.log(x) - x - math.lgamma(a))
    if x < a + 1.0:
        term = total = 1.0 / a
        for k in range(1, 100000):
            term *= x / (a + k)
            total += term
            if abs(term) <= abs(total) * 1e-17:
                break
        return 1.0 - front * total
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for k in range(1, 100000):
        an = -k * (k - a)
        b += 2.0
        d = an * d + b
        d = 1.0 / (d if abs(d) > tiny else tiny)
        c = b + an / c
        c = c if abs(c) > tiny else tiny
        h *= d * c
        if abs(d * c - 1.0) < 1e-16:
            break
    return front * h


def chi2_sf(x, df):
    """P(X > x) for X chi-square with df degrees of freedom."""
    return _gamma_q(0.5 * float(df), 0.5 * float(x))


def ljung_box(acf, n_obs):
    """Q = n (n + 2) sum_k acf_k^2 / (n - k) over the rows of acf [n_cells, n_lags], n = n_obs [n_cells], and its
    chi-square upper tail with n_lags degrees of freedom.  NaN where an acf_k is NaN or n <= n_lags."""
    acf = np.atleast_2d(np.asarray(acf, dtype=np.float64))
    n = np.asarray(n_obs, dtype=np.float64).reshape(-1, 1)
    k = np.arange(1, acf.shape[1] + 1, dtype=np.float64)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        Q = (n * (n + 2.0))[:, 0] * np.sum(acf * acf / (n - k), axis=1)
    Q = np.where((n[:, 0] > acf.shape[1]), Q, np.nan)
    pv = np.array([chi2_sf(x, acf.shape[1]) if np.isfinite(x) else np.nan for x in Q])
    return Q, pv


def innovation_diagnostics(y, u, v, theta_packed, cell_offsets=None, n_lags=10, device=0):
    """Are the standardised innovations of each cell's theta white, with mean 0 and variance 1?  One launch, no
    rows: only scalars cross PCIe.  -> {"n_obs", "zmean", "zvar", "status": [n_cells], "acf": [n_cells, n_lags],
    "Q": the Ljung-Box statistic, "p_value": its chi-square upper tail with n_lags degrees of freedom}."""
    if n_lags < 1:
        raise ValueError("n_lags must be >= 1")
    r = filter_batch(y, u, v, theta_packed, cell_offsets=cell_offsets, stdlik=True, n_lags=n_lags, rows=(),
                     device=device)
    Q, pv = ljung_box(r["acf"], r["n_obs"])
    return {"n_obs": r["n_obs"], "zmean": r["zmean"], "zvar": r["zvar"], "acf": r["acf"], "Q": Q, "p_value": pv,
            "status": r["status"]}
