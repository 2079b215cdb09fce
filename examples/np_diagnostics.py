#!/usr/bin/env python3
"""Is the package's fitted model of the Mekong at Nakhon Phanom adequate?  The standard check of a state-space
fit: the standardised innovations z_t = e_t / sqrt(S_t) of the Kalman filter at the fitted theta should be
white, with mean 0 and variance 1.  The filter runs on the GPU (ldsr_filter_batch)
at the stored NPlds theta; only the scalars come back.

    python examples/np_diagnostics.py [n_lags]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ldsr_amd  # noqa: E402


def main():
    n_lags = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_data.json")))
    years_obs = np.array(d["NPannual"]["year"])
    obs = np.log(np.array(d["NPannual"]["Qa"]))      # transform = 'log' (R/LDS_reconstruction.R:164-182)
    pcs = np.array(d["NPpc"]["data"])                # 3 x 813, years 1200..2012
    y = np.full(pcs.shape[1], np.nan)
    y[years_obs[0] - 1200:years_obs[0] - 1200 + obs.size] = obs - obs.mean()
    theta = ldsr_amd.pack_theta(d["NPlds"]["theta"], 3, 3)

    kf = ldsr_amd.Kalman_filter(y, pcs, pcs, d["NPlds"]["theta"])
    r = ldsr_amd.innovation_diagnostics(y, pcs, pcs, theta[None, :], n_lags=n_lags)
    print("Nakhon Phanom, T = %d, %d observed years, theta = NPlds" % (y.size, r["n_obs"][0]))
    print("lik %.9f (package's NPlds$lik: %.9f)" % (kf["lik"], d["NPlds"]["lik"][0]))
    print("standardised innovations: mean %+.4f   variance %.4f" % (r["zmean"][0], r["zvar"][0]))
    print("autocorrelations, lags 1..%d: %s" % (n_lags, " ".join("%+.3f" % a for a in r["acf"][0])))
    print("  (a white series of %d values stays within +-%.3f at 95 %%)" % (r["n_obs"][0], 1.96 / np.sqrt(r["n_obs"][0])))
    print("Ljung-Box Q(%d) = %.3f   p = %.4f   -> %s" % (
        n_lags, r["Q"][0], r["p_value"][0],
        "no evidence against white innovations" if r["p_value"][0] > 0.05 else "the innovations are autocorrelated"))
    worst = int(np.nanargmax(np.abs(kf["e"][0] / np.sqrt(kf["S"][0]))))
    print("largest |z_t|: %.2f in %d" % (abs(kf["e"][0, worst]) / np.sqrt(kf["S"][0, worst]), 1200 + worst))


if __name__ == "__main__":
    main()
