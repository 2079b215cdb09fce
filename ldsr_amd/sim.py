"""Stochastic replicates of a fitted LDS model on the GPU: the reference's R/stochastics.R
(one_LDS_rep :18-46, LDS_rep :58-63), through ldsr_simulate_batch of include/ldsr_hip.h.

    r_seed=k   reproduces set.seed(k); LDS_rep(...): the host draws the uniforms R would consume
               (rrng.RUniform, ldsr_simulate_draw_count of them) and the GPU does the rest.  An
               rrng.RUniform may be passed instead of k: its stream continues from call to call, as
               consecutive LDS_rep calls after one set.seed do.
    seed=s     counter mode: the uniforms are SplitMix64 of (s, model, replicate, position) on the
               device, so replicate k is the same whichever call or batch it is computed in.
    neither    counter mode with a fresh entropy seed, as R is when unseeded.

Nothing is simulated on the host: without a GPU the calls raise LdsrError.
"""
import ctypes as C

import numpy as np

from . import _lib
from .api import _d, pack_theta
from .rrng import RUniform

_llp = C.POINTER(C.c_longlong)


def _widths(theta, u, v, p, q, P):
    """p, q of the packed theta layout: from u / v when given, else from the caller or a dict theta."""
    if u is not None:
        p = np.asarray(u).shape[-2] if np.ndim(u) >= 2 else 1
    if v is not None:
        q = np.asarray(v).shape[-2] if np.ndim(v) >= 2 else 1
    if isinstance(theta, dict):
        p = np.size(theta["B"]) if p is None else p
        q = np.size(theta["D"]) if q is None else q
    if p is None and q is None:
        if P != 8:
            raise ValueError("cannot tell p and q from a packed theta of %d entries: pass p and q, "
                             "or theta as a dict" % P)
        p = q = 1
    p = P - 6 - q if p is None else p
    q = P - 6 - p if q is None else q
    if p < 1 or q < 1 or 6 + p + q != P:
        raise ValueError("theta has %d entries, expected 6+p+q with p = %s, q = %s" % (P, p, q))
    return int(p), int(q)


def _inputs(a, n_models, T, name):
    """None | [k, T'] (one series for all models) | [n_models, k, T'] -> time-major [.][T][k]; columns
    beyond T are ignored, as the reference indexes u[, t] for t = 1..n only."""
    if a is None:
        return None, True
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 1:
        a = a[None, :]
    if a.shape[-1] < T:
        raise ValueError("%s has %d columns, fewer than T = %d" % (name, a.shape[-1], T))
    if a.ndim == 2:
        return np.ascontiguousarray(a[:, :T].T), True
    if a.ndim == 3 and a.shape[0] == n_models:
        return np.ascontiguousarray(np.transpose(a[:, :, :T], (0, 2, 1))), False
    raise ValueError("%s must be k x T or n_models x k x T" % name)


def _packed(theta_packed, p, q):
    th = np.ascontiguousarray(np.atleast_2d(np.asarray(theta_packed, dtype=np.float64)))
    if th.ndim != 2 or th.shape[1] != 6 + p + q:
        raise ValueError("theta must be [n_models, %d]" % (6 + p + q))
    return th


def draw_count(theta_packed, T, num_reps, p=1, q=1):
    """(uniforms one R-stream call consumes, per-model offsets [n_models + 1]) -- R's rnorm rules
    decide which draws exist (ldsr_simulate_draw_count)."""
    th = _packed(theta_packed, p, q)
    off = np.empty(th.shape[0] + 1, dtype=np.int64)
    n = _lib.lib().ldsr_simulate_draw_count(th.shape[0], int(T), p, q, _d(th), int(num_reps),
                                            off.ctypes.data_as(_llp))
    if n < 0:
        _lib.check(-n)
    return int(n), off


def simulate_batch(theta_packed, u, v, T, num_reps, mu=None, exp_trans=True, seed=None, uniforms=None,
                   first_rep=0, device=0, p=None, q=None, outputs=("simX", "simY", "simQ")):
    """num_reps replicates of T steps for each row of theta_packed [n_models, 6+p+q] in one launch.
    u / v: p x T / q x T shared by every model, [n_models, p, T] per model, or None (term dropped;
    then p / q come from the arguments, default 1).  mu: scalar or [n_models].  uniforms: R-stream
    mode (R's unif_rand() values in LDS_rep's order, draw_count() of them); otherwise counter mode
    with `seed`.  Returns {"simX", "simY", "simQ"} (those named in `outputs`), each
    [n_models, num_reps, T]."""
    T, num_reps = int(T), int(num_reps)
    P = np.atleast_2d(np.asarray(theta_packed)).shape[-1]
    p, q = _widths(None, u, v, p, q, P)
    th = _packed(theta_packed, p, q)
    n = th.shape[0]
    U, us = _inputs(u, n, T, "u")
    V, vs = _inputs(v, n, T, "v")
    shared = 1 if (us and vs) else 0
    if not shared:          # one series for one input, per-model series for the other: replicate
        if U is not None and us:
            U = np.ascontiguousarray(np.broadcast_to(U, (n,) + U.shape))
        if V is not None and vs:
            V = np.ascontiguousarray(np.broadcast_to(V, (n,) + V.shape))
    MU = None if mu is None else np.ascontiguousarray(np.broadcast_to(np.asarray(mu, dtype=np.float64), (n,)))
    if uniforms is not None:
        uniforms = np.ascontiguousarray(uniforms, dtype=np.float64).reshape(-1)
        need, _ = draw_count(th, T, num_reps, p, q)
        if uniforms.size != need:
            raise ValueError("R-stream mode consumes %d uniforms here, got %d" % (need, uniforms.size))
        seed = 0
    elif seed is None:
        seed = int(np.random.SeedSequence().generate_state(1, np.uint64)[0])
    out = {k: np.empty((n, num_reps, T)) for k in ("simX", "simY", "simQ") if k in outputs}
    _lib.check(_lib.lib().ldsr_simulate_batch(
        int(device), n, T, p, q, _d(U), _d(V), shared, _d(th), _d(MU), num_reps, int(first_rep),
        1 if exp_trans else 0, int(seed) & 0xFFFFFFFFFFFFFFFF, _d(uniforms), _d(out.get("simX")),
        _d(out.get("simY")), _d(out.get("simQ"))))
    return out


def _rep_call(theta, u, v, years, num_reps, first_rep, rep_ids, mu, exp_trans, r_seed, seed, device):
    if years is None:
        raise ValueError("years is required (the study horizon; n = len(years))")
    years = np.asarray(years)
    n = years.size
    if u is None:
        v = None            # the reference's no-input branch drops D v_t too (R/stochastics.R:28-33)
    elif v is None:
        raise ValueError("v is required when u is given (the reference indexes v[, t])")
    p, q = _widths(theta, u, v, None, None, _theta_size(theta))
    th = pack_theta(theta, p, q)
    uniforms = None
    if r_seed is not None:
        g = r_seed if isinstance(r_seed, RUniform) else RUniform(r_seed)
        uniforms = g.unif_rand(draw_count(th, n, num_reps, p, q)[0])
    r = simulate_batch(th, u, v, n, num_reps, mu=mu, exp_trans=exp_trans, seed=seed, uniforms=uniforms,
                       first_rep=first_rep, device=device, p=p, q=q)
    return {"year": np.tile(years, num_reps), "simX": r["simX"].reshape(-1), "simY": r["simY"].reshape(-1),
            "simQ": r["simQ"].reshape(-1), "rep": np.repeat(np.asarray(rep_ids), n)}


def _theta_size(theta):
    if isinstance(theta, dict):
        return sum(np.size(theta[k]) for k in ("A", "B", "C", "D", "Q", "R", "mu1", "V1"))
    return np.size(theta)


def LDS_rep(theta, u=None, v=None, years=None, num_reps=100, mu=0, exp_trans=True, r_seed=None, seed=None,
            device=0):
    """LDS_rep (R/stochastics.R:58-63): the reference's long format as 1-D arrays in replicate-major
    order -- {"year", "simX", "simY", "simQ", "rep"}, rep = 1..num_reps.  theta: dict or packed;
    u / v: p x T' / q x T' (T' >= len(years); u = None drops B u_t AND D v_t, as the reference)."""
    return _rep_call(theta, u, v, years, int(num_reps), 0, np.arange(1, int(num_reps) + 1), mu, exp_trans,
                     r_seed, seed, device)


def one_LDS_rep(rep_num, theta, u=None, v=None, years=None, mu=0, exp_trans=True, r_seed=None, seed=None,
                device=0):
    """one_LDS_rep (R/stochastics.R:18-46): one replicate with rep column rep_num.  In counter mode
    it is replicate rep_num of LDS_rep with the same seed."""
    return _rep_call(theta, u, v, years, 1, int(rep_num) - 1, [rep_num], mu, exp_trans, r_seed, seed, device)
