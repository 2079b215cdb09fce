"""LDS_BFGS of the reference (R/LDS_GA.R:155-184): learn theta by a bound-constrained L-BFGS that
minimises ssqTrain from num_restarts random start points -- the BFGS and BFGS_smooth arms of
call_method (R/LDS_reconstruction.R:70-86).

Everything numeric runs on the GPU behind one library call (ldsr_bfgs_batch, include/ldsr_hip.h): one
persistent wavefront per restart runs the whole optimisation, the winner is picked on the device and only
its model crosses PCIe.  The optimiser is this project's own specification ("The
bound-constrained L-BFGS"); it does not reproduce the iterates of the L-BFGS-B code behind stats::optim.
LDS_BFGS_with_update (R/LDS_GA.R:90-127) is the same optimiser on f = -penalized_likelihood
(ldsr_bfgs_update_batch; the objective and its exact gradient: pl_grad).
This module only marshals and draws the start points -- there is no host implementation of the objectives
or of the optimiser."""
import numpy as np

from . import _lib
from .api import _d, _dims, _i, _offsets, _series, unpack_theta

CONVERGED, MAXIT, LINESEARCH, NONFINITE, INTERRUPTED = 0, 1, 2, 3, 4
_START_STREAM = 1 << 40       # counter-mode stream of restart r: _START_STREAM + r


def _value_grad(entry, lam, y, u, v, theta_packed, cell_offsets, grad, device):
    """ssq_train / pl_grad: marshal, call `entry` (lam: the argument only one of the two takes, else None) and
    return the values, with grad=True (values, gradients)"""
    Y, U, V, S, T, p, q, shared = _series(y, u, v)
    theta = np.ascontiguousarray(np.atleast_2d(theta_packed), dtype=np.float64)
    if theta.shape[1] != 6 + p + q:
        raise ValueError("theta must be [n, %d]" % (6 + p + q))
    n = theta.shape[0]
    off = _offsets(cell_offsets, S, n)
    f = np.empty(n)
    g = np.empty_like(theta) if grad else None
    _lib.check(getattr(_lib.lib(), entry)(device, S, T, p, q, _d(Y), _d(U), _d(V), shared, _i(off), _d(theta),
                                          *([] if lam is None else [float(lam)]), _d(f), _d(g)))
    return (f, g) if grad else f


def ssq_train(y, u, v, theta_packed, cell_offsets=None, grad=False, device=0):
    """ssqTrain (R/LDS_GA.R:143-147) for a batch of packed thetas [n, 6+p+q]: the sum over the observed
    y_t of (y_t - propagate(theta)$Y_t)^2.  With grad=True -> (ssq [n], gradient [n, 6+p+q])."""
    return _value_grad("ldsr_ssq_grad_batch", None, y, u, v, theta_packed, cell_offsets, grad, device)


def _bfgs_call(entry, lam, y, u, v, par0, lb, ub, cell_offsets, maxit, lmm, factr, pgtol, select, with_J, fit_mode,
               device, return_all):
    """bfgs_batch / bfgs_update_batch: marshal, call `entry` (lam, fit_mode: the arguments only one of the two
    takes, None where it takes none) and shape the result"""
    if select not in ("reference", "min"):
        raise ValueError('select must be "reference" or "min"')
    Y, U, V, S, T, p, q, shared = _series(y, u, v)
    P = 6 + p + q
    par0 = np.ascontiguousarray(np.atleast_2d(par0), dtype=np.float64)
    if par0.shape[1] != P:
        raise ValueError("par0 must be [n_cells, %d]" % P)
    lb = np.ascontiguousarray(lb, dtype=np.float64).reshape(-1)
    ub = np.ascontiguousarray(ub, dtype=np.float64).reshape(-1)
    if lb.size != P or ub.size != P:
        raise ValueError("lb and ub must have 6+p+q = %d entries" % P)
    n = par0.shape[0]
    off = _offsets(cell_offsets, S, n)
    out = {"winner": np.empty(S, dtype=np.int32), "theta": np.empty((S, P)), "value": np.empty(S),
           "lik": np.empty(S), "X": np.empty((S, T)), "Y": np.empty((S, T)), "V": np.empty((S, T))}
    if with_J:
        out["J"] = np.empty((S, T))
    a = {}
    if return_all:
        a = {"par": np.empty((n, P)), "value": np.empty(n), "n_iter": np.empty(n, dtype=np.int32),
             "n_eval": np.empty(n, dtype=np.int32), "status": np.empty(n, dtype=np.int32)}
    _lib.check(getattr(_lib.lib(), entry)(
        device, S, T, p, q, _d(Y), _d(U), _d(V), shared, _i(off), _d(par0), _d(lb), _d(ub),
        *([] if lam is None else [float(lam)]), int(maxit), int(lmm), float(factr), float(pgtol),
        int(select == "reference"), *([] if fit_mode is None else [int(fit_mode)]),
        _d(a.get("par")), _d(a.get("value")), _i(a.get("n_iter")), _i(a.get("n_eval")), _i(a.get("status")),
        _i(out["winner"]), _d(out["theta"]), _d(out["value"]), _d(out["lik"]), _d(out["X"]), _d(out["Y"]),
        _d(out["V"]), _d(out.get("J"))))
    if return_all:
        out["all"] = a
    return out


def bfgs_batch(y, u, v, par0, lb, ub, cell_offsets=None, maxit=100, lmm=5, factr=1e7, pgtol=0.0,
               select="reference", smooth=False, device=0, return_all=True):
    """One L-BFGS run per row of par0 [n_cells, 6+p+q], all in one call.  y: [T], or [S, T] (the folds of
    cvLDS with shared u, v) with cell_offsets [S+1].  select: "reference" is the reference's literal
    which.max(optim.vals) (R/LDS_GA.R:174: the LARGEST of the minimised values), "min" the smallest.

    Returns dict: winner [S] (global cell index, -1 = none), theta [S, P], value [S], lik [S],
    X / Y / V [S, T] (J too with smooth=True: the fit is Kalman_smoother's, else propagate's); plus
    "all" (per-cell par, value, n_iter, n_eval, status) when return_all."""
    return _bfgs_call("ldsr_bfgs_batch", None, y, u, v, par0, lb, ub, cell_offsets, maxit, lmm, factr, pgtol, select,
                      bool(smooth), bool(smooth), device, return_all)


def pl_grad(y, u, v, theta_packed, lam, cell_offsets=None, grad=False, device=0):
    """penalized_likelihood (R/LDS_GA.R:28-44) for a batch of packed thetas [n, 6+p+q]: lik(stdlik=FALSE) -
    lam * ssq, one wavefront per theta.  With grad=True -> (pl [n], d pl / d theta [n, 6+p+q])."""
    return _value_grad("ldsr_pl_grad_batch", lam, y, u, v, theta_packed, cell_offsets, grad, device)


def bfgs_update_batch(y, u, v, par0, lb, ub, lam=1.0, cell_offsets=None, maxit=100, lmm=5, factr=1e7, pgtol=0.0,
                      select="reference", device=0, return_all=True):
    """bfgs_batch on f = -penalized_likelihood at lam: one L-BFGS run per row of par0 [n_cells, 6+p+q].
    select: "reference" is the reference's literal which.max(optim.vals) (R/LDS_GA.R:116: the LARGEST of the
    minimised values), "min" the smallest.

    Returns dict: winner [S], theta [S, P], value [S] (the minimised -pl), lik [S], X / Y / V / J [S, T] (the
    fit is Kalman_smoother's); plus "all" (per-cell par, value, n_iter, n_eval, status) when return_all."""
    return _bfgs_call("ldsr_bfgs_update_batch", lam, y, u, v, par0, lb, ub, cell_offsets, maxit, lmm, factr, pgtol,
                      select, True, None, device, return_all)


def start_points(lb, ub, num_restarts, seed=None, r_seed=None, first=0):
    """[num_restarts, P] start points lb + (ub - lb) U.  r_seed=k: the draws of R's
    `set.seed(k); replicate(num.restarts, runif(P, lb, ub))` (ldsr_amd/rrng.py; a coordinate with
    lb == ub takes no uniform, as R's runif returns a without drawing when a == b).  Otherwise restart r
    draws from counter-mode stream `first + r` of synth.py, so a restart's start point does not depend on
    how many others share the call."""
    lb = np.asarray(lb, dtype=np.float64).reshape(-1)
    ub = np.asarray(ub, dtype=np.float64).reshape(-1)
    n, P = int(num_restarts), lb.size
    out = np.tile(lb, (n, 1))
    if r_seed is not None:
        from .rrng import RUniform
        free = lb != ub
        nf = int(free.sum())
        if nf:
            U = RUniform(r_seed).unif_rand(n * nf).reshape(n, nf)
            out[:, free] = lb[free] + (ub[free] - lb[free]) * U
        return out
    from .synth import uniform
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1)[0])
    for r in range(n):
        out[r] = lb + (ub - lb) * uniform(seed, _START_STREAM + first + r, P)
    return out


def _learn(name, batch, y, u, v, ub, lb, num_restarts, seed, r_seed, kwargs):
    """LDS_BFGS / LDS_BFGS_with_update: draw the start points, run `batch` (bfgs_batch / bfgs_update_batch, with
    kwargs) on the one series and shape the reference's list; the fit has J where the batch gave one"""
    if ub is None or lb is None:
        raise ValueError("%s needs ub and lb" % name)     # R/LDS_reconstruction.R:176
    p, q = _dims(u, v)
    par0 = start_points(lb, ub, num_restarts, seed=seed, r_seed=r_seed)
    r = batch(y, u, v, par0, lb, ub, **kwargs)
    if r["theta"].shape[0] != 1:
        raise ValueError("%s takes one series; %s runs several" % (name, batch.__name__))
    k = int(r["winner"][0])
    if k < 0:
        raise _lib.LdsrError("%s: no restart has a finite objective value" % name)
    fit = {key: r[key][0:1].copy() for key in ("X", "Y", "V", "J") if key in r}
    fit["lik"] = float(r["lik"][0])
    return {"theta": unpack_theta(r["theta"][0], p, q), "fit": fit, "lik": fit["lik"], "pl": float(r["value"][0]),
            "all": dict(r["all"], selected=k, par0=par0)}


def LDS_BFGS(y, u, v, ub=None, lb=None, num_restarts=100, seed=None, r_seed=None, select="reference",
             smooth=False, maxit=100, device=0):
    """-> {"theta", "fit", "lik", "pl", "all"}   (R/LDS_GA.R:176-183): theta as the reference's list, fit =
    propagate(theta, u, v, y) with the standardised likelihood (smooth=True: Kalman_smoother(y, u, v,
    theta), the BFGS_smooth arm, R/LDS_reconstruction.R:79-85), lik = fit's, pl = the selected restart's
    minimised ssq; "all" = the per-restart par / value / n_iter / n_eval / status (+ selected, par0)."""
    return _learn("LDS_BFGS", bfgs_batch, y, u, v, ub, lb, num_restarts, seed, r_seed,
                  dict(maxit=maxit, select=select, smooth=smooth, device=device))


def LDS_BFGS_with_update(y, u, v, lambda_=1.0, ub=None, lb=None, num_restarts=100, seed=None, r_seed=None,
                         select="reference", maxit=100, device=0):
    """-> {"theta", "fit", "lik", "pl", "all"}   (R/LDS_GA.R:118-126): theta as the reference's list, fit =
    Kalman_smoother(y, u, v, theta) with the standardised likelihood, lik = fit's, pl = the selected restart's
    minimised -penalized_likelihood; "all" = the per-restart par / value / n_iter / n_eval / status (+ selected,
    par0)."""
    return _learn("LDS_BFGS_with_update", bfgs_update_batch, y, u, v, ub, lb, num_restarts, seed, r_seed,
                  dict(lam=lambda_, maxit=maxit, select=select, device=device))
