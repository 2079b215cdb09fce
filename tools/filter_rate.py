#!/usr/bin/env python3
"""Rates of the Kalman filter entry (ldsr_filter_batch_device) on two shapes,

  NP     T = 813, p = q = 3  (the Nakhon Phanom shape: 1200..2012, the last tenth observed)
  short  T = 1000, p = 1, q = 2, fully observed

at --cells cells each (one series, that many thetas), measured twice: with all eight rows written, and with
scalars only at n_lags = 10 (what innovation_diagnostics asks for).  The operands are resident on the device;
a measurement is the time between two HIP events around ONE launch on the current stream, the median of --reps
launches after --warmup warm-up launches.  Beside them, on the same cells:

  ldsr_filter_batch   the host-pointer entry, scalars only, n_lags = 10: wall clock of the call (upload, launch,
                      copy back; the call ends in a stream synchronise), median of --host-reps calls
  ldsr_smooth_batch   Kalman_smoother on the same cells through its host-pointer entry, all four rows, timed the
                      same way

    python tools/filter_rate.py [--cells 4096] [--reps 50] > profiles/r15_filter_rates.txt"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    import ldsr_amd
    from ldsr_amd import _lib, synth
    L = _lib.lib()
    if L.ldsr_device_count() < 1 or not torch.cuda.is_available():
        sys.exit("tools/filter_rate.py: no GPU visible -- a rate is measured on the device or not at all")
    n = a.cells
    print("# tools/filter_rate.py: %d cells (one series, %d thetas of make_init's distribution); device entry: HIP events around one"
          % (n, n))
    print("# launch, median of %d after %d warm-up launches; host entries: wall clock of the call, median of %d after one warm-up call"
          % (a.reps, a.warmup, a.host_reps))
    print("# %s" % L.ldsr_version().decode())
    print("%-62s %12s %14s %12s" % ("measurement", "ms", "cells/s", "GB/s written"))
    dev = torch.device("cuda:0")
    for name, T, p, q, mask in (("NP shape: T = 813, p = q = 3, last tenth observed", 813, 3, 3, "paleo"),
                                ("T = 1000, p = 1, q = 2, fully observed", 1000, 1, 2, "dense")):
        y, u, v = synth.make_series(T, p, q, series_id=15, mask=mask)
        theta = synth.make_init_packed(p, q, n, seed=15)
        d_y = torch.from_numpy(y).to(dev)
        d_u = torch.from_numpy(np.ascontiguousarray(u.T)).to(dev)
        d_v = torch.from_numpy(np.ascontiguousarray(v.T)).to(dev)
        d_th = torch.from_numpy(theta).to(dev)
        rows = [torch.empty(n * T, dtype=torch.float64, device=dev) for _ in range(ROWS)]
        d_lik = torch.empty(n, dtype=torch.float64, device=dev)
        d_zs = torch.empty(2 * n, dtype=torch.float64, device=dev)
        d_acf = torch.empty(10 * n, dtype=torch.float64, device=dev)
        d_st = torch.empty(n, dtype=torch.int32, device=dev)
        off = (C.c_int * 2)(0, n)
        wsb = L.ldsr_filter_workspace_bytes(1, T, p, q, n, 10)
        ws = torch.empty(wsb + 256, dtype=torch.uint8, device=dev)
        ws_ptr = (ws.data_ptr() + 255) // 256 * 256
        vp = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def launch(with_rows, n_lags):
            rp = [vp(r) if with_rows else None for r in rows]
            rc = L.ldsr_filter_batch_device(0, stream, 1, T, p, q, vp(d_y), vp(d_u), vp(d_v), 0, off, vp(d_th), 1, n_lags,
                                            *rp, vp(d_lik), vp(d_zs), vp(d_acf) if n_lags else None, vp(d_st),
                                            C.c_void_p(ws_ptr), wsb)
            if rc:
                sys.exit("ldsr_filter_batch_device: " + L.ldsr_last_error().decode())

        def events(fn):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            return statistics.median(ms)

        def wall(fn):
            fn()
            s = []
            for _ in range(a.host_reps):
                t = time.perf_counter()
                fn()
                s.append(time.perf_counter() - t)
            return 1e3 * statistics.median(s)

        print("# " + name)
        ms = events(lambda: launch(True, 0))
        print("%-62s %12.4f %14.4g %12.1f" % ("ldsr_filter_batch_device, all 8 rows, n_lags = 0", ms, n / ms * 1e3,
                                              8.0 * ROWS * n * T / ms / 1e6))
        ms = events(lambda: launch(False, 10))
        print("%-62s %12.4f %14.4g %12.1f" % ("ldsr_filter_batch_device, scalars only, n_lags = 10", ms, n / ms * 1e3,
                                              8.0 * n * T / ms / 1e6))
        lik_dev = d_lik.cpu().numpy()
        ms = wall(lambda: ldsr_amd.filter_batch(y, u, v, theta, n_lags=10, rows=()))
        print("%-62s %12.4f %14.4g %12s" % ("ldsr_filter_batch (host pointers), scalars only, n_lags = 10", ms, n / ms * 1e3, "-"))
        ms = wall(lambda: ldsr_amd.smooth_batch(y, u, v, theta))
        print("%-62s %12.4f %14.4g %12s" % ("ldsr_smooth_batch (host pointers), X, Y, V, J", ms, n / ms * 1e3, "-"))
        sm = ldsr_amd.smooth_batch(y, u, v, theta)["lik"]
        print("#   max |lik(filter) - lik(smoother)| over the cells: %.3g" % np.nanmax(np.abs(lik_dev - sm)))
    print("# (GB/s written: the rows' bytes, or the strip of z for the lag pass, over the launch time; the reads are T (1 + p + q)")
    print("#  doubles per cell and hit the L2 after the first wave of a series)")


if __name__ == "__main__":
    main()
