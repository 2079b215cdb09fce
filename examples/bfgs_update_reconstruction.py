"""LDS_BFGS_with_update on the Nakhon Phanom data (the reference's bundled NPannual / NPpc, T = 813): 100
restarts of the bound-constrained L-BFGS over -penalized_likelihood on the GPU (R/LDS_GA.R:90-127), under the
reference's selection rule (which.max of the minimised values, R/LDS_GA.R:116) and under the smallest value, at
two penalties.  The fit is Kalman_smoother(theta) of the selected restart.
usage: python examples/bfgs_update_reconstruction.py"""
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
    # (variances bounded away from 0: S_t = C^2 Vp_t + R > 0 at every start)
    lb = np.concatenate([[0.0], np.full(p, -1.0), [0.0], np.full(q, -1.0), [0.01, 0.01, -1.0, 0.01]])
    ub = np.concatenate([[1.0], np.full(p, 1.0), [1.0], np.full(q, 1.0), [1.0, 1.0, 1.0, 1.0]])

    for lam in (1.0, 10.0):
        for select in ("reference", "min"):
            m = ldsr_amd.LDS_BFGS_with_update(y, u, u, lambda_=lam, ub=ub, lb=lb, num_restarts=100, r_seed=1,
                                              select=select)
            a = m["all"]
            print("lambda = %-4g select = %-9s restart %3d of 100: -pl %.6f  lik %.6f  (%d iterations, %d evaluations; "
                  "all restarts: -pl %.4f .. %.4f)" % (
                      lam, select, a["selected"], m["pl"], m["lik"], a["n_iter"][a["selected"]],
                      a["n_eval"][a["selected"]], np.nanmin(a["value"]), np.nanmax(a["value"])))


if __name__ == "__main__":
    main()
