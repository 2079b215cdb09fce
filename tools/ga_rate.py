"""GA generations per second on the GPU box (not part of any test): ldsr_ga_batch against the loop a
caller could write without it -- breeding on the host (tests/ga_model.py) and one
ldsr_amd.penalized_likelihood call per generation.  NP shape (T = 813, the fixture's u, v), 4 x 100
individuals, `run` large so that every generation runs; (a) one problem, (b) 30 problems (cross-validation
folds: the instrumental years of one fold masked each) as one call.  Medians and min / max of the
repetitions after one warm-up.  usage: python tools/ga_rate.py [--gens 200] [--host-gens-b 20] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ga_model as M  # noqa: E402
import ldsr_amd  # noqa: E402


def np_case():
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_data.json")))
    qa, years = np.array(ref["NPannual"]["Qa"]), np.array(ref["NPannual"]["year"])
    u = np.ascontiguousarray(np.array(ref["NPpc"]["data"]))          # 3 x 813, years 1200..2012
    obs = np.log(qa)
    y = np.full(u.shape[1], np.nan)
    i0 = years[0] - 1200
    y[i0:i0 + len(obs)] = obs - obs.mean()
    return y, u, i0, len(obs)


def folds(y, i0, n_obs, S):
    Y = np.repeat(y[None], S, axis=0)
    for s in range(1, S):               # fold s hides a block of instrumental years (fold 0: none)
        a = i0 + (s * 7) % (n_obs - 6)
        Y[s, a:a + 6] = np.nan
    return Y


def host_loop(Y, u, lb, ub, K, n, gens, seed):
    S, P = Y.shape[0], lb.size
    pops = np.stack([M.initial_population(seed, s, K, n, lb, ub) for s in range(S)])
    off = (np.arange(S + 1) * K * n).astype(np.int32)
    states = [M.new_state(P) for _ in range(S)]
    for g in range(gens):
        fit = ldsr_amd.penalized_likelihood(Y, u, u, pops.reshape(-1, P), 1.0, cell_offsets=off).reshape(S, K, n)
        for s in range(S):
            states[s] = M.bookkeeping(states[s], pops[s], fit[s], g, gens, 10 ** 9)
            if g + 1 < gens:
                pops[s] = M.breed(pops[s], fit[s], g, seed, s, lb, ub)
    return [st["best"] for st in states]


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return np.array(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gens", type=int, default=200)
    ap.add_argument("--host-gens-b", type=int, default=20, help="generations of the host loop in case (b)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-only", action="store_true", help="one run of case (a) on the device (for rocprofv3)")
    a = ap.parse_args()
    y, u, i0, n_obs = np_case()
    K, n, seed = 4, 100, 2026
    lb = np.concatenate([[0.0], np.full(3, -1.0), [0.0], np.full(3, -1.0), [0.01, 0.01, -1.0, 0.01]])
    ub = np.concatenate([[1.0], np.full(3, 1.0), [1.0], np.full(3, 1.0), [2.0, 2.0, 1.0, 2.0]])
    if a.device_only:
        r = ldsr_amd.ga_batch(y, u, u, lb, ub, maxiter=a.gens, run=10 ** 9, seed=seed)
        print("pl %.6f after %d generations" % (r["pl"][0], r["n_gen"][0]))
        return
    lines = ["GA rates, NP shape (T = %d, p = q = 3), %d x %d individuals, lambda = 1, run = off; %d repetitions after one warm-up"
             % (y.size, K, n, a.reps)]
    for name, Y, host_gens in (("(a) 1 problem", y[None], a.gens), ("(b) 30 problems, one call", folds(y, i0, n_obs, 30), a.host_gens_b)):
        S = Y.shape[0]
        out = {}
        td = timed(lambda: out.update(d=ldsr_amd.ga_batch(Y if S > 1 else Y[0], u, u, lb, ub, maxiter=a.gens, run=10 ** 9, seed=seed)), a.reps)
        th = timed(lambda: out.update(h=host_loop(Y, u, lb, ub, K, n, host_gens, seed)), a.reps)
        assert np.all(out["d"]["n_gen"] == a.gens)
        rd, rh = a.gens / td, host_gens / th
        lines.append("%s" % name)
        lines.append("  (i)  ldsr_ga_batch, %d generations:            median %8.1f generations/s (min %.1f, max %.1f); %.1f ms a generation"
                     % (a.gens, np.median(rd), rd.min(), rd.max(), 1e3 * np.median(td) / a.gens))
        lines.append("  (ii) host breeding + penalized_likelihood, %d generations: median %8.1f generations/s (min %.1f, max %.1f)"
                     % (host_gens, np.median(rh), rh.min(), rh.max()))
        lines.append("  ratio of the medians (i) / (ii): %.1f" % (np.median(rd) / np.median(rh)))
        if host_gens == a.gens:
            lines.append("  best pl: device %.9f, host loop %.9f" % (out["d"]["pl"][0], out["h"][0]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
