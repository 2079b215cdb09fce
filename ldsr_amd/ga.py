"""LDS_GA of the reference (R/LDS_GA.R:54-82): learn theta by an island genetic algorithm that
maximises penalized_likelihood inside a box.

The whole algorithm runs on the GPU behind one library call (ldsr_ga_batch, include/ldsr_hip.h):
the populations never leave the device, a generation is two kernel launches.  It is an island GA of
the family of GA::gaisl, which the reference delegates to, by this project's own specification
("The island GA"); it does not reproduce gaisl's random stream.  This module only
marshals -- there is no host implementation."""
import numpy as np

from . import _lib
from .api import Kalman_smoother, _d, _dims, _i, _series, unpack_theta


def ga_batch(y, u, v, lb, ub, lambda_=1.0, num_islands=4, pop_per_island=100, maxiter=1000, run=100,
             seed=0, suggestions=None, device=0, return_population=False):
    """One GA per series of y ([T] or [S, T]; u, v as everywhere: k x T shared by the series, or
    S x k x T), all in one call.  lb, ub: packed bounds [6+p+q].  suggestions: [n_sugg, P] (one
    series) or [S, n_sugg, P], the first individuals of island 0.  Problem s draws under seed + s.

    Returns dict: theta [S, P], pl [S], n_gen [S], trace [S, maxiter] (best so far, NaN beyond
    n_gen); with return_population also population [S, K, n, P] and fitness [S, K, n] of the last
    evaluated generation."""
    Y, U, V, S, T, p, q, shared = _series(y, u, v)
    P = 6 + p + q
    lb = np.ascontiguousarray(lb, dtype=np.float64).reshape(-1)
    ub = np.ascontiguousarray(ub, dtype=np.float64).reshape(-1)
    if lb.size != P or ub.size != P:
        raise ValueError("lb and ub must have 6+p+q = %d entries" % P)
    K, n = int(num_islands), int(pop_per_island)
    sug, n_sugg = None, 0
    if suggestions is not None:
        sug = np.ascontiguousarray(suggestions, dtype=np.float64)
        if sug.ndim == 2:
            sug = sug[None]
        if sug.ndim != 3 or sug.shape[0] != S or sug.shape[2] != P:
            raise ValueError("suggestions must be [n_sugg, %d] or [%d, n_sugg, %d]" % (P, S, P))
        sug = np.ascontiguousarray(sug)
        n_sugg = sug.shape[1]
    theta = np.empty((S, P))
    pl = np.empty(S)
    n_gen = np.empty(S, dtype=np.int32)
    trace = np.empty((S, max(int(maxiter), 0)))
    pop = np.empty((S, max(K, 0), max(n, 0), P)) if return_population else None
    fit = np.empty((S, max(K, 0), max(n, 0))) if return_population else None
    _lib.check(_lib.lib().ldsr_ga_batch(
        device, S, T, p, q, _d(Y), _d(U), _d(V), shared, _d(lb), _d(ub), float(lambda_), K, n,
        int(maxiter), int(run), int(seed) & 0xFFFFFFFFFFFFFFFF, _d(sug), n_sugg, _d(theta), _d(pl),
        _i(n_gen), _d(trace), _d(pop), _d(fit)))
    out = {"theta": theta, "pl": pl, "n_gen": n_gen, "trace": trace}
    if return_population:
        out["population"] = pop
        out["fitness"] = fit
    return out


def LDS_GA(y, u, v, lambda_=1, ub=None, lb=None, num_islands=4, pop_per_island=100, niter=1000, run=100,
           seed=None, suggestions=None, device=0):
    """-> {"theta", "fit", "lik", "pl"}   (R/LDS_GA.R:78-81): theta as the reference's list, fit =
    Kalman_smoother(y, u, v, theta) with the standardised likelihood ("so that it's comparable with
    EM"), lik = fit's, pl = the best penalised likelihood found (ga_batch also tells the generations
    used and the trace)."""
    if ub is None or lb is None:
        raise ValueError("LDS_GA needs ub and lb")     # R/LDS_reconstruction.R:176
    if seed is None:
        seed = int(np.random.SeedSequence().generate_state(1)[0])
    p, q = _dims(u, v)
    r = ga_batch(y, u, v, lb, ub, lambda_=lambda_, num_islands=num_islands, pop_per_island=pop_per_island,
                 maxiter=niter, run=run, seed=seed, suggestions=suggestions, device=device)
    if r["theta"].shape[0] != 1:
        raise ValueError("LDS_GA takes one series; ga_batch runs several")
    theta = unpack_theta(r["theta"][0], p, q)
    fit = Kalman_smoother(y, u, v, theta, device=device)
    return {"theta": theta, "fit": fit, "lik": fit["lik"], "pl": float(r["pl"][0])}
