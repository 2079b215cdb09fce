#!/usr/bin/env python3
"""Rates of the device-resident L-BFGS learner (ldsr_bfgs_batch) on the NP-shaped problem of
LDS_reconstruction(method = "BFGS"): T = 813, p = q = 3, 100 restarts -- one problem, and 30 folds in one
call (cvLDS) -- as objective evaluations (forward passes) per second and restarts per second, wall clock
of the host-pointer entry (PCIe in and out included), best of --reps calls after one warm-up call.

For comparison, the loop a caller could write without that entry: ldsr_propagate_batch for the objective,
central differences in numpy for the gradient (2 (6+p+q) + 1 passes per gradient, what stats::optim does
without gr), driven by the same optimiser (tests/bfgs_model.py), the restarts of a problem in lockstep
so that every propagate call carries as many thetas as are still running.

    python tools/bfgs_rate.py [--restarts 100] [--folds 30] [--reps 3] [--host-restarts 8] > profiles/r07_bfgs_rates.txt

--objective pl: LDS_BFGS_with_update instead (ldsr_bfgs_update_batch, f = -penalized_likelihood at --lambda), on
the T = 113 and T = 813 NP problems with a box that keeps Q, R, V1 >= 0.5: evaluations per second, the wall time
of LDS_BFGS_with_update, and for scale the time of ldsr_penalized_lik_batch -- the value-only FIT kernel that
computes the same number -- on the same thetas.

    python tools/bfgs_rate.py --objective pl > profiles/r08_bfgs_update_rates.txt"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def np_problem():
    """The NP fixture as LDS_reconstruction builds it (tests/conftest.py::npcase) and the box of its vignette-style call."""
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_data.json")))
    qa, years = np.array(d["NPannual"]["Qa"]), np.array(d["NPannual"]["year"])
    pcs = np.array(d["NPpc"]["data"])
    obs = np.log(qa)
    y = np.full(pcs.shape[1], np.nan)
    i0 = years[0] - 1200
    y[i0:i0 + obs.size] = obs - obs.mean()
    p = q = 3
    lb = np.concatenate([[0.0], np.full(p, -1.0), [0.0], np.full(q, -1.0), [0.0, 0.0, -1.0, 0.0]])
    ub = np.concatenate([[1.0], np.full(p, 1.0), [1.0], np.full(q, 1.0), [1.0, 1.0, 1.0, 1.0]])
    return y, pcs, lb, ub


def folds(y, n, seed=5):
    """n copies of y with a random quarter of the observed years held out (cvLDS's folds differ in their NA mask only)"""
    from ldsr_amd import synth
    obs = np.flatnonzero(np.isfinite(y))
    out = np.tile(y, (n, 1))
    for f in range(n):
        out[f, obs[synth.uniform(seed, f, obs.size) < 0.25]] = np.nan
    return out


def timed(fn, reps):
    fn()
    best, res = np.inf, None
    for _ in range(reps):
        t = time.perf_counter()
        res = fn()
        best = min(best, time.perf_counter() - t)
    return best, res


def host_loop(eng, y, u, v, par0, lb, ub):
    """One problem through propagate + central differences; -> seconds, propagate passes, best value."""
    import bfgs_model as M
    P = par0.shape[1]
    h = 1e-6
    passes = [0]

    def f_batch(X):
        r = eng.smooth_batch(y, u, v, X, mode="propagate")
        passes[0] += X.shape[0]
        return np.nansum((y[None, :] - r["Y"]) ** 2, axis=1)

    def fun(x):
        return f_batch(x[None, :])[0]

    def fun_grad(x):
        X = np.tile(x, (2 * P + 1, 1))
        for j in range(P):
            X[1 + 2 * j, j] += h
            X[2 + 2 * j, j] -= h
        f = f_batch(X)
        return f[0], (f[1::2] - f[2::2]) / (2 * h)

    t = time.perf_counter()
    vals = [M.minimise(fun, fun_grad, x0, lb, ub)["value"] for x0 in par0]
    return time.perf_counter() - t, passes[0], np.nanmin(vals)


def main_pl(a):
    import ldsr_amd as eng
    from ldsr_amd.bfgs import start_points
    y813, pcs, _, _ = np_problem()
    p = q = 3
    lb = np.concatenate([[0.0], np.full(p, -1.0), [0.0], np.full(q, -1.0), [0.5, 0.5, -1.0, 0.5]])
    ub = np.concatenate([[1.0], np.full(p, 1.0), [1.0], np.full(q, 1.0), [1.5, 1.5, 1.0, 1.5]])
    n = a.restarts
    par0 = start_points(lb, ub, n, seed=1)
    print("# tools/bfgs_rate.py --objective pl: NP data, p = q = 3, %d restarts, lambda = %g, maxit = 100, lmm = 5, factr = 1e7" % (n, a.lam))
    print("# %s" % eng._lib.lib().ldsr_version().decode())
    print("case                              seconds   evaluations   eval/s      iterations(mean/max)  best -pl")
    for T in (113, 813):
        y, u = y813[813 - T:], np.ascontiguousarray(pcs[:, 813 - T:])
        sec, r = timed(lambda: eng.bfgs_update_batch(y, u, u, par0, lb, ub, lam=a.lam, select="min"), a.reps)
        ev = int(r["all"]["n_eval"].sum())
        print("%-32s %9.5f %12d %11.4g   %8.1f / %-5d %14.8g" % ("T = %d, ldsr_bfgs_update_batch" % T, sec, ev, ev / sec,
              np.mean(r["all"]["n_iter"]), np.max(r["all"]["n_iter"]), r["value"][0]))
        st = np.bincount(r["all"]["status"], minlength=4)
        print("#   status: %d converged, %d maxit, %d line search, %d non-finite" % tuple(st[:4]))
        sec, _ = timed(lambda: eng.LDS_BFGS_with_update(y, u, u, lambda_=a.lam, ub=ub, lb=lb, num_restarts=n, seed=1,
                                                        select="min"), a.reps)
        print("%-32s %9.5f" % ("T = %d, LDS_BFGS_with_update" % T, sec))
        th = r["all"]["par"]
        sec, _ = timed(lambda: eng.pl_grad(y, u, u, th, a.lam), a.reps)
        print("%-32s %9.5f %12d %11.4g" % ("T = %d, pl_grad, values" % T, sec, n, n / sec))
        sec, _ = timed(lambda: eng.pl_grad(y, u, u, th, a.lam, grad=True), a.reps)
        print("%-32s %9.5f %12d %11.4g" % ("T = %d, pl_grad, with gradient" % T, sec, n, n / sec))
        sec, _ = timed(lambda: eng.penalized_likelihood(y, u, u, th, a.lam), a.reps)
        print("%-32s %9.5f %12d %11.4g" % ("T = %d, ldsr_penalized_lik_batch" % T, sec, n, n / sec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objective", choices=("ssq", "pl"), default="ssq")
    ap.add_argument("--lambda", dest="lam", type=float, default=1.0)
    ap.add_argument("--restarts", type=int, default=100)
    ap.add_argument("--folds", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-restarts", type=int, default=8)
    a = ap.parse_args()
    if a.objective == "pl":
        return main_pl(a)
    import ldsr_amd as eng
    from ldsr_amd.bfgs import start_points
    y, pcs, lb, ub = np_problem()
    T, n = y.size, a.restarts
    par0 = start_points(lb, ub, n, seed=1)
    print("# tools/bfgs_rate.py: NP shape T = %d, p = q = 3, %d restarts, maxit = 100, lmm = 5, factr = 1e7" % (T, n))
    print("# %s" % eng._lib.lib().ldsr_version().decode())
    print("case                          seconds   evaluations   eval/s      restarts/s   iterations(mean/max)  best ssq")

    def row(name, sec, ev, nr, it, best):
        print("%-28s %9.5f %12d %11.4g %11.4g   %8.1f / %-5d %14.8g" % (name, sec, ev, ev / sec, nr / sec, np.mean(it), np.max(it), best))

    sec, r = timed(lambda: eng.bfgs_batch(y, pcs, pcs, par0, lb, ub, select="min"), a.reps)
    row("device, 1 problem", sec, int(r["all"]["n_eval"].sum()), n, r["all"]["n_iter"], r["value"][0])
    ys = folds(y, a.folds)
    par0f = np.tile(par0, (a.folds, 1))
    off = np.arange(a.folds + 1) * n
    sec, r = timed(lambda: eng.bfgs_batch(ys, pcs, pcs, par0f, lb, ub, cell_offsets=off, select="min"), a.reps)
    row("device, %d folds in one call" % a.folds, sec, int(r["all"]["n_eval"].sum()), n * a.folds, r["all"]["n_iter"], np.min(r["value"]))
    st = np.bincount(r["all"]["status"], minlength=4)
    print("# status of the %d cells: %d converged, %d maxit, %d line search, %d non-finite" % ((n * a.folds,) + tuple(st[:4])))
    m = a.host_restarts
    sec, passes, best = host_loop(eng, y, pcs, pcs, par0[:m], lb, ub)
    print("%-28s %9.5f %12d %11.4g %11.4g   %8s   %-5s %14.8g" % ("propagate + central diff, %d" % m, sec, passes, passes / sec, m / sec, "-", "-", best))
    print("# (the last row's evaluations are propagate passes, %d per gradient; its restarts run one after the other)" % (2 * par0.shape[1] + 1))


if __name__ == "__main__":
    main()
