"""LDS_GA on the Nakhon Phanom data (the reference's bundled NPannual / NPpc, T = 813): the island GA on
the GPU, once from a random population and once seeded with the winner of LDS_EM_restart
(`suggestions`); prints the penalised likelihood and the generations used.
usage: python examples/ga_reconstruction.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ldsr_amd  # noqa: E402


def main():
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_data.json")))
    qa, years = np.array(ref["NPannual"]["Qa"]), np.array(ref["NPannual"]["year"])
    u = np.ascontiguousarray(np.array(ref["NPpc"]["data"]))          # 3 x 813, years 1200..2012
    obs = np.log(qa)
    y = np.full(u.shape[1], np.nan)
    y[years[0] - 1200:years[0] - 1200 + len(obs)] = obs - obs.mean()
    p = q = 3
    lam = 1.0

    em = ldsr_amd.LDS_EM_restart(y, u, u, ldsr_amd.make_init(p, q, 50, seed=1), niter=1000, tol=1e-5)
    th_em = ldsr_amd.pack_theta(em["theta"], p, q)
    pl_em = ldsr_amd.penalized_likelihood(y, u, u, th_em, lam)[0]
    print("EM winner:        lik %.6f  pl %.6f" % (em["lik"], pl_em))

    lb = np.minimum(np.concatenate([[0.0], np.full(p, -1.0), [0.0], np.full(q, -1.0), [0.01, 0.01, -1.0, 0.01]]), th_em - 0.1)
    ub = np.maximum(np.concatenate([[1.0], np.full(p, 1.0), [1.0], np.full(q, 1.0), [2.0, 2.0, 1.0, 2.0]]), th_em + 0.1)
    for name, sugg in (("GA, unseeded:    ", None), ("GA, seeded by EM:", th_em[None])):
        r = ldsr_amd.ga_batch(y, u, u, lb, ub, lambda_=lam, num_islands=4, pop_per_island=100, maxiter=1000,
                              run=100, seed=7, suggestions=sugg)
        fit = ldsr_amd.Kalman_smoother(y, u, u, r["theta"][0])
        print("%s lik %.6f  pl %.6f  after %d generations" % (name, fit["lik"], r["pl"][0], r["n_gen"][0]))


if __name__ == "__main__":
    main()
