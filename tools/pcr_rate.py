#!/usr/bin/env python3
"""Rates of the batched principal-component regression (ldsr_pcr_batch, R/PCR.R) on two shapes:

  NP        cvPCR on the bundled Nakhon Phanom data: 1 member x 30 folds, n = 46, k = 3
  ensemble  PCR_ensemble_selection's device call: 1000 members x 30 folds, n = 46, k drawn from 1..8

as least-squares fits (cells) per second, wall clock of the host-pointer entry (PCIe in and out included,
the call ends in a stream synchronise), best of --reps calls after one warm-up call; the ensemble shape
repeats the call until --min-seconds have passed per measurement.  Beside it the loop a caller could write
without the entry: numpy.linalg.lstsq per cell on the host (the same fits, one core), timed the same way.

    python tools/pcr_rate.py [--members 1000] [--reps 5] > profiles/r13_pcr_rates.txt"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def np_problem():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_data.json")))
    qa, years = np.array(d["NPannual"]["Qa"]), np.array(d["NPannual"]["year"])
    pc = np.ascontiguousarray(np.array(d["NPpc"]["data"]).T)
    Z = [np.array(z) - 1 for z in d["NPcv"]["Z"]]
    held = np.zeros((len(Z), qa.size), dtype=np.uint8)
    for f, z in enumerate(Z):
        held[f, z] = 1
    return pc[years - 1200], np.log(qa), held


def timed(fn, reps, min_seconds):
    fn()
    best = np.inf
    for _ in range(reps):
        n, t = 0, time.perf_counter()
        while True:
            res = fn()
            n += 1
            dt = time.perf_counter() - t
            if dt >= min_seconds:
                break
        best = min(best, dt / n)
    return best, res


def lstsq_loop(members, y, held):
    out = np.empty((len(members), held.shape[0], y.size))
    one = np.ones((y.size, 1))
    for m, X in enumerate(members):
        D = np.concatenate([one, X], axis=1)
        for f in range(held.shape[0]):
            keep = held[f] == 0
            out[m, f] = D @ np.linalg.lstsq(D[keep], y[keep], rcond=None)[0]      # one_pcr_cv, R/PCR.R:101-107
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    a = ap.parse_args()
    from ldsr_amd import _lib, pcr
    if _lib.lib().ldsr_device_count() < 1:
        sys.exit("tools/pcr_rate.py: no GPU visible -- a rate is measured on the device or not at all")
    X, y, held = np_problem()
    rng = np.random.default_rng(13)
    pool = np.column_stack([X, rng.standard_normal((y.size, 13))])
    ens = [pool[:, np.sort(rng.choice(16, k, replace=False))] for k in rng.integers(1, 9, a.members)]
    print("# tools/pcr_rate.py: n = 46, 30 folds of 12 held-out points (NPcv's); seconds per call, best of %d x >= %.2f s" % (a.reps, a.min_seconds))
    print("# %s" % _lib.lib().ldsr_version().decode())
    print("case                                   cells   device s/call   device cells/s   lstsq loop s   loop cells/s   speed-up   max |pred diff|")
    for name, members in (("NP: 1 member, k = 3", [X]), ("ensemble: %d members, k in 1..8" % a.members, ens)):
        cells = len(members) * held.shape[0]
        sec, r = timed(lambda: pcr.pcr_batch(members, y, held, coef=False, sigma=False), a.reps, a.min_seconds)
        assert np.all(r["status"] == 0)
        hsec, ref = timed(lambda: lstsq_loop(members, y, held), 1 if cells > 1000 else a.reps, 0.0 if cells > 1000 else a.min_seconds)
        print("%-36s %7d %15.6f %16.4g %14.5f %14.4g %10.1f %17.3g" % (name, cells, sec, cells / sec, hsec, cells / hsec, hsec / sec,
                                                                     np.max(np.abs(r["pred"] - ref))))
    print("# (device: ldsr_pcr_batch through ldsr_amd.pcr.pcr_batch, packing of the member blocks in numpy included;")
    print("#  loop: numpy.linalg.lstsq per cell, one host core)")


if __name__ == "__main__":
    main()
