#!/usr/bin/env python3
"""bench.py -- restart x EM-iteration throughput of the EM/Kalman hot path on MI355X.

One "step" = one pass of the hot path over one batch: a single ldsr_em_batch_device call
(series preparation + the EM kernel) on BASELINE.json's config 2 -- synthetic T=1000, p=1,
q=2, 4096 restarts per GPU, niter=100, tol=0 (the stop rule of src/EM.cpp:272 can never fire,
so every cell runs exactly 100 E-steps) = 409 600 restart x EM-iteration units per GPU.
Inputs (y, u, v, theta0) are resident in HBM before the timed region.  --workload selects the
other BASELINE configs (cfg3 per GPU; cfg4 / cfg5 fixed grids) for DESIGN.md's table.

N > 1: one process per GPU.  `python bench.py --gpus N` invoked plainly starts the N ranks
itself (a child `python -m torch.distributed.run`, before this process touches the GPU); under
torch.distributed.run it is a rank.  Restarts shard embarrassingly -- every rank takes its part of
each series' restarts (ldsr_amd/shard.py), no data-path collective (R/LDS_reconstruction.R:46 is a
%dopar% over independent tasks).  The
headline fields are WEAK scaling (every rank its own 4096 restarts; restart index = global
position in the counter-based generator); for the single-series workloads the same run also
times the STRONG split of BASELINE config 2 (4096 restarts / N per rank) and reports it in
"strong_scaling".  cfg4 / cfg5 are fixed grids -> "strong" by construction.

Prints ONE JSON line on rank 0: metric, value, unit, higher_is_better, dtype, ms_per_step (one
timed step), steps, warmup, config.  A plain run does only what
the headline needs: set up, warm up, time --steps steps, write the outputs of the last timed step
(--dump-outputs DIR), print the line.  --full adds the objects below (and, for N > 1, the
strong-scaling run); --no-verify / --no-host-entry / --no-cpu-baseline drop single legs of it.
  --dump-outputs DIR   theta.npy [cells, 6+p+q], lik.npy, n_iter.npy, status.npy [cells] of the last
                timed launch, float64 (n_iter / status are exact small integers), rank 0's cells;
                rank r > 0 writes <name>_rank<r>.npy.  Above 64 MB in all, a fixed seeded sample of
                cells is written instead, with its cell indices in sample_index.npy.  The inputs are
                a function of the arguments alone (ldsr_amd/synth.py is seeded), so two builds can
                be compared output for output.
Objects of --full:
  roofline      the binding resource is fp64 VALU issue, not HBM: achieved = algorithmic flops
                ((6p+6q+50)*T per unit) / EM-kernel time measured with HIP events
                on the launch stream, against the 78.6 TFLOP/s fp64 vector peak.  The nominal HBM
                figure of BASELINE.json (16*T*(3+p+q) logical bytes per unit) is
                kept as hbm_logical_*: it is NOT traffic -- the series lives in LDS and the
                filtered states in registers, so it can exceed the 8 TB/s peak.  Counter-measured
                numbers (HBM bytes per launch, VALU instructions) come from committed rocprofv3
                --pmc passes of this same command (profiles/pmc_summary.json) and are emitted
                only when an entry for this workload AND this kernel instantiation exists.
  host_entry    the same workload through ldsr_em_batch (host pointers, PCIe in/out) -- what the R shim
                calls; reported beside `value`, never as it
  cpu_baseline  the CPU oracle (a port of src/EM.cpp, not RcppArmadillo) on the host cores
  verified      a 64-cell sample of the last timed launch against the CPU oracle (outside the
                timed region): identical iteration counts, theta and lik within the parity bar
"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# BASELINE.json configs.  cfg2 (the metric's config) and cfg3 are quoted per GPU -> weak scaling
# (every rank gets `restarts` restarts of the one series); cfg4 / cfg5 are fixed grids "sharded
# across the GPUs" -> strong scaling (every rank takes its part of each series' restarts).
WORKLOADS = {
    "cfg2": dict(T=1000, p=1, q=2, series=1, restarts=4096, niter=100, scaling="weak"),
    "cfg3": dict(T=1000, p=4, q=8, series=1, restarts=8192, niter=100, scaling="weak"),
    "cfg4": dict(T=2000, p=1, q=4, series=10, restarts=1024, niter=100, scaling="strong",
                 kind="cvfolds"),      # 10 CV folds of one series: shared u, v; own NA mask
    "cfg5": dict(T=813, p=1, q=3, series=48, restarts=512, niter=100, scaling="strong",
                 kind="stations"),     # 48 independent series, observed tail of 30..90 steps
}

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8.0 TB/s spec
FP64_VALU_PEAK_TFLOPS = 78.6  # 256 CUs x 4 SIMDs x 16 fp64 lanes/clk x 2 flop x 2.4 GHz (AMD spec)
N_SIMD, CLOCK_HZ = 1024, 2.4e9


def build_problem(name, mask, world, rank, scaling=None):
    """Host arrays of this rank's slice of the workload's (series, restart) grid:
    Y [S,T], U [S or 1,T,p], V [S or 1,T,q] (time-major), shared_uv, cell_offsets [S+1],
    theta0 [cells, P], plus the global cell count.  scaling="strong" on a single-series
    workload splits its `restarts` over the ranks instead of giving every rank that many."""
    from ldsr_amd import shard, synth
    w = WORKLOADS[name]
    T, p, q, S, R = w["T"], w["p"], w["q"], w["series"], w["restarts"]
    kind = w.get("kind", "single")
    if kind == "single":
        y, u, v = synth.make_series(T, p, q, series_id=0, mask=mask)
        n_global = R if scaling == "strong" else world * R   # weak: R restarts per rank
        lo, hi = shard.rank_slice(n_global, world, rank)
        th0 = synth.make_init_packed(p, q, hi - lo, seed=1, first=lo)
        return (y[None], np.ascontiguousarray(u.T[None]), np.ascontiguousarray(v.T[None]), 0,
                np.array([0, hi - lo], np.int32), th0, n_global)
    if kind == "cvfolds":
        # cvLDS (R/LDS_reconstruction.R:270-285): instrumental period = last 200 steps, fold k
        # hides a contiguous block of 21 instrumental points (make_Z blocks, R/utils.R:89-96)
        y, u, v = synth.make_series(T, p, q, series_id=4, mask="paleo", n_tail=200)
        Y = np.repeat(y[None], S, axis=0)
        for k in range(S):
            Y[k, T - 200 + 18 * k:T - 200 + 18 * k + 21] = np.nan
        U, V, shared = np.ascontiguousarray(u.T[None]), np.ascontiguousarray(v.T[None]), 1
    else:
        ys, us, vs = zip(*[synth.make_series(T, p, q, series_id=500 + s_, mask="paleo",
                                             n_tail=30 + (s_ * 60) // max(S - 1, 1))
                           for s_ in range(S)])
        Y = np.stack(ys)
        U = np.ascontiguousarray(np.stack([a.T for a in us]))
        V = np.ascontiguousarray(np.stack([a.T for a in vs]))
        shared = 0
    off = (np.arange(S + 1) * R).astype(np.int64)
    n_global = int(off[-1])
    # striped cut (ldsr_amd/shard.py): this rank's share of EVERY series' restarts; a restart's
    # initial theta is a function of its global cell id
    g_lo, loc = shard.rank_stripes(off, world, rank)
    th0 = np.concatenate([synth.make_init_packed(p, q, int(loc[s_ + 1] - loc[s_]), seed=1, first=int(g_lo[s_]))
                          for s_ in range(S)])
    return Y, U, V, shared, loc, th0, n_global


def bytes_per_unit(T, p, q):
    """Logical bytes of one E+M unit: y, u, v read twice, (Xu, Vu) written+read."""
    return 16 * T * (3 + p + q)


def flops_per_unit(T, p, q):
    """Algorithmic fp64 flops of one E+M unit, divides and logs counted as 1."""
    return (6 * p + 6 * q + 50) * T


def load_pmc(workload, mask, kernel, niter, tol):
    """The committed rocprofv3 --pmc summary for this workload (profiles/pmc_summary.json).
    PMC counters cannot be collected from inside the timed run; they come from separate
    rocprofv3 passes of this same command.  Returns (entry, stale): the entry recorded for this
    workload, and whether it was measured on ANOTHER kernel instantiation / iteration setup than
    the one being timed now (then its numbers describe an older build and are flagged)."""
    path = os.path.join(ROOT, "profiles", "pmc_summary.json")
    try:
        with open(path) as f:
            entries = json.load(f).get("entries", [])
    except (OSError, ValueError):
        return None, None
    # (several rounds may hold an entry for the same workload and kernel name: the latest round counts)
    best = exact = None
    for e in sorted(entries, key=lambda e_: str(e_.get("round", "")), reverse=True):
        if e.get("workload") != workload or e.get("mask", "dense") != mask:
            continue
        if e.get("kernel") == kernel and e.get("niter") == niter and e.get("tol") == tol:
            exact = exact or e
        best = best or e
    if exact:
        return exact, False
    return (best, True) if best else (None, None)


def host_cores():
    """Usable host cores: affinity mask, capped by the cgroup CPU quota (the GPU box exposes
    256 CPUs but grants a 16-core share)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(round(int(quota) / int(period)))))
    except (OSError, ValueError):
        pass
    return n


def rscript_reference_probe(T, p, q, niter):
    """if (and only if) Rscript with the ldsr package is installed on this
    box, time the real RcppArmadillo path (LDS_EM on one restart) and report it separately.
    Never assumed: the build image and the GPU boxes seen so far have no R."""
    import shutil
    rs = shutil.which("Rscript")
    if not rs:
        return {"available": False, "why": "Rscript not found on PATH"}
    code = ("suppressMessages(library(ldsr)); set.seed(1); T <- %d; p <- %d; q <- %d;"
            "u <- matrix(rnorm(p*T), p, T); v <- matrix(rnorm(q*T), q, T); y <- matrix(rnorm(T), 1, T);"
            "th <- make_init(p, q, 1)[[1]]; t0 <- proc.time()[3];"
            "for (i in 1:8) r <- ldsr:::LDS_EM(y, u, v, th, %d, 0); cat(8 * %d / (proc.time()[3] - t0))"
            % (T, p, q, niter, niter))
    try:
        out = subprocess.run([rs, "-e", code], capture_output=True, text=True, timeout=120)
        if out.returncode != 0:
            return {"available": False, "why": "Rscript present but ldsr not usable: "
                    + out.stderr.strip().splitlines()[-1][:120] if out.stderr.strip() else "error"}
        return {"available": True, "value": float(out.stdout.strip().split()[-1]),
                "unit": "restart*EM-iter/s", "cores": 1, "kind": "reference",
                "sample": "8 x LDS_EM(niter=%d, tol=0) on one R process" % niter}
    except Exception as e:   # noqa: BLE001 -- a probe must never break the benchmark
        return {"available": False, "why": "probe failed: %s" % type(e).__name__}


def cpu_baseline(p, q, niter, Y, U, V, seed, target_s=12.0):
    """The CPU oracle on the first series of the workload (Y [S,T], U [.,T,p], V [.,T,q]):
    a short pilot sizes a sample of about `target_s` seconds on every usable host core."""
    from oracle import oracle as O
    from ldsr_amd import synth
    cores = host_cores()
    Y = np.ascontiguousarray(Y[:1])
    U = np.ascontiguousarray(U[:1])
    V = np.ascontiguousarray(V[:1])
    pilot = 64 * cores
    th0 = synth.make_init_packed(p, q, pilot, seed=seed)
    O.em_batch(Y, U, V, np.zeros(cores, np.int32), th0[:cores], 3, 0.0, n_threads=cores)   # warm
    t0 = time.perf_counter()
    O.em_batch(Y, U, V, np.zeros(pilot, np.int32), th0, niter, 0.0, n_threads=cores)
    rate = pilot * niter / (time.perf_counter() - t0)
    cells = int(min(max(rate * target_s / niter, pilot), 1 << 18)) // cores * cores
    th0 = synth.make_init_packed(p, q, cells, seed=seed)
    t0 = time.perf_counter()
    O.em_batch(Y, U, V, np.zeros(cells, np.int32), th0, niter, 0.0, n_threads=cores)
    dt = time.perf_counter() - t0
    return {"value": cells * niter / dt, "unit": "restart*EM-iter/s", "cores": cores,
            "kind": "port",
            "sample": "%d restarts x %d EM iterations of the same series, %d host threads, %.1f s "
                      "(CPU oracle = scalar fp64 port of src/EM.cpp, not RcppArmadillo)"
                      % (cells, niter, cores, dt)}


def verify_sample(job, p, q, niter, tol, n_sample=64):
    """Outside the timed region: what the LAST timed launch left in HBM against the CPU oracle on
    a sample of its cells (evenly spaced over the rank's grid) -- identical iteration counts, then
    theta and lik within 1e-6 relative + 1e-9 absolute.  The oracle is the
    checker here, as in tests/ (the full-size check of this same launch is
    tests/test_gpu_full_configs.py::test_bench_launch_matches_oracle)."""
    from oracle import oracle as O
    th = job.d_th.cpu().numpy()
    lik = job.d_lik.cpu().numpy()
    nit = job.d_nit.cpu().numpy()
    Y, U, V = job.d_y.cpu().numpy(), job.d_u.cpu().numpy(), job.d_v.cpu().numpy()
    S = Y.shape[0]
    if U.shape[0] != S:
        U, V = np.repeat(U, S, axis=0), np.repeat(V, S, axis=0)
    n = th.shape[0]
    idx = np.unique(np.linspace(0, n - 1, min(n_sample, n)).astype(np.int64))
    soc = (np.searchsorted(job.loc_off, idx, side="right") - 1).astype(np.int32)
    th0 = job.d_th0.cpu().numpy()[idx]
    r_th, r_lik, r_nit, _ = O.em_batch(Y, U, V, soc, th0, niter, tol, n_threads=host_cores())
    same_it = bool(np.array_equal(r_nit, nit[idx]))
    fin = np.isfinite(r_lik)
    d_th = np.abs(th[idx] - r_th)[fin]
    d_lk = np.abs(lik[idx] - r_lik)[fin]
    bar_th = (1e-6 * np.abs(r_th) + 1e-9)[fin]
    bar_lk = (1e-6 * np.abs(r_lik) + 1e-9)[fin]
    ok = same_it and bool(np.all(d_th <= bar_th)) and bool(np.all(d_lk <= bar_lk))
    rel = float(max((d_th / bar_th).max(), (d_lk / bar_lk).max())) if d_th.size else 0.0
    return {"cells": int(idx.size), "against": "CPU oracle (port of src/EM.cpp), same niter / tol",
            "n_iter_equal": same_it, "max_dev_over_bar": rel,
            "bar": "|d| <= 1e-6 |ref| + 1e-9 on every theta entry and on lik", "ok": ok}


def host_entry_rate(L, job, T, p, q, niter, tol, algo, units_rank, steps=10, warmup=2):
    """The same workload through the HOST-POINTER entry the R shim calls (ldsr_em_batch: operands in
    host memory, one pinned->device copy in, kernels, one copy back, one synchronisation; the lead /
    fully-observed fact is found from y by the library) -- timed outside the headline loop, reported
    next to it, never `value`.  Plain ctypes on preallocated arrays: no Python wrapper in the loop."""
    from ldsr_amd import _lib
    Y = np.ascontiguousarray(job.d_y.cpu().numpy())
    U = np.ascontiguousarray(job.d_u.cpu().numpy())
    V = np.ascontiguousarray(job.d_v.cpu().numpy())
    th0 = np.ascontiguousarray(job.d_th0.cpu().numpy())
    n, P = th0.shape
    th = np.empty_like(th0)
    lik = np.empty(n)
    nit = np.empty(n, np.int32)
    st = np.empty(n, np.int32)
    off = (C.c_int * (job.S + 1))(*[int(x) for x in job.loc_off])
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    pi = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))

    def call():
        _lib.check(L.ldsr_em_batch(job.local_rank, job.S, T, p, q, pd(Y), pd(U), pd(V), job.shared_uv,
                                   off, pd(th0), niter, tol, algo, pd(th), pd(lik), pi(nit), pi(st),
                                   None))
    for _ in range(warmup):
        call()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    dt = (time.perf_counter() - t0) / steps
    units = int(nit.sum())
    return {"entry": "ldsr_em_batch (host pointers: PCIe in and out, lead found from y by the library)",
            "ms_per_call": dt * 1e3, "value": units / dt, "unit": "restart*EM-iter/s", "steps": steps,
            "units_per_call": units, "same_units_as_device_entry": units == units_rank,
            "bytes_in": int(Y.nbytes + U.nbytes + V.nbytes + th0.nbytes),
            "bytes_out": int(th.nbytes + lik.nbytes + nit.nbytes + st.nbytes)}


def roofline(workload, mask, kernel_name, niter, tol, T, p, q, units_rank, kern_ms):
    """--full: the roofline object of the timed launches (kern_ms = their mean HIP-event kernel time)."""
    kern_s = kern_ms * 1e-3
    fpu, bpu = flops_per_unit(T, p, q), bytes_per_unit(T, p, q)
    tflops = fpu * units_rank / kern_s / 1e12             # this GPU's kernel
    logical_gbs = bpu * units_rank / kern_s / 1e9
    pmc, stale = load_pmc(workload, mask, kernel_name, niter, tol)
    roof = {"bound": "fp64_valu", "achieved": tflops, "peak": FP64_VALU_PEAK_TFLOPS,
            "unit": "TFLOP/s", "frac": tflops / FP64_VALU_PEAK_TFLOPS,
            "traffic": None, "kernel": kernel_name, "kernel_ms": kern_ms,
            "algorithmic_flops_per_unit": fpu, "units_per_launch": units_rank,
            "hbm_logical_bytes_per_unit": bpu, "hbm_logical_gbs": logical_gbs,
            "hbm_logical_frac": logical_gbs / HBM_PEAK_GBS, "hbm_peak_gbs": HBM_PEAK_GBS,
            "flops_are": "reference-equivalent: what src/EM.cpp spends on these units, (6p+6q+50) T "
                         "each; kernels with a closed-form lead or steady-state sweeps execute "
                         "fewer -- fp64_executed_frac is what the SQ counters saw",
            "note": "fp64 VALU issue is the binding resource; hbm_logical_* is BASELINE.json's "
                    "nominal byte figure (not traffic: the series is served from LDS, the "
                    "filtered states never leave registers) and may exceed 1; traffic / "
                    "hbm_measured_* / issue_frac are rocprofv3 PMC numbers of the committed "
                    "passes named in pmc_source"}
    if pmc is not None:
        roof["traffic"] = pmc.get("hbm_bytes_per_launch")
        roof["pmc_source"] = pmc.get("source")
        roof["pmc_stale"] = bool(stale)
        if pmc.get("hbm_bytes_per_launch") is not None:
            roof["hbm_measured_gbs"] = pmc["hbm_bytes_per_launch"] / kern_s / 1e9
            roof["hbm_measured_frac"] = roof["hbm_measured_gbs"] / HBM_PEAK_GBS
        if pmc.get("valu_insts_per_unit") is not None:
            # wave-instructions issued per second against 1024 SIMDs x one fp64 issue / 4 clk
            roof["valu_insts_per_unit"] = pmc["valu_insts_per_unit"]
            roof["issue_frac"] = (pmc["valu_insts_per_unit"] * units_rank / kern_s
                                  / (N_SIMD * CLOCK_HZ / 4.0))
        if pmc.get("fp64_flops_executed_per_unit"):
            # what the kernel actually executes (FMA = 2 flops, counted by the SQ): the
            # parallel-in-time formulation does ~1.9x the algorithmic flops
            roof["fp64_executed_tflops"] = pmc["fp64_flops_executed_per_unit"] * units_rank / kern_s / 1e12
            roof["fp64_executed_frac"] = roof["fp64_executed_tflops"] / FP64_VALU_PEAK_TFLOPS
        if pmc.get("valu_active_per_wave_cycle") is not None:
            roof["valu_busy_frac"] = 2.0 * pmc["valu_active_per_wave_cycle"]   # two waves per SIMD
        if pmc.get("sustained_clock_ghz"):
            # `peak` assumes the 2.4 GHz boost clock; under fp64 load the chip holds less
            # (GRBM_GUI_ACTIVE / 8 XCDs / kernel duration of the committed PMC pass): the same
            # achieved rate against the peak AT THAT CLOCK separates clock from code
            clk = pmc["sustained_clock_ghz"]
            roof["sustained_clock_ghz"] = clk
            roof["peak_at_sustained_clock"] = FP64_VALU_PEAK_TFLOPS * clk / (CLOCK_HZ / 1e9)
            roof["frac_at_sustained_clock"] = tflops / roof["peak_at_sustained_clock"]
    return roof


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(job, out_dir, rank, world, cap_bytes=DUMP_CAP_BYTES):
    """--dump-outputs: what the caller of ldsr_em_batch_device_lead receives from the last timed
    launch (theta, lik, n_iter, status of every cell of this rank), as float64 .npy files.  Past
    the cap (shared over the ranks) a fixed seeded sample of cells, indices in sample_index.npy."""
    arrays = {"theta": job.d_th.cpu().numpy(), "lik": job.d_lik.cpu().numpy(),
              "n_iter": job.d_nit.cpu().numpy(), "status": job.d_st.cpu().numpy()}
    arrays = {k: np.ascontiguousarray(a, dtype=np.float64) for k, a in arrays.items()}
    n = job.cells
    row_bytes = sum(a.nbytes for a in arrays.values()) // max(n, 1)
    keep = (cap_bytes // world) // max(row_bytes + 8, 1)
    if n > keep:
        idx = np.sort(np.random.default_rng(12345).choice(n, size=keep, replace=False))
        arrays = {k: a[idx] for k, a in arrays.items()}
        arrays["sample_index"] = idx.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    suffix = "" if rank == 0 else "_rank%d" % rank
    for k, a in arrays.items():
        np.save(os.path.join(out_dir, k + suffix + ".npy"), a)


def spawn_ranks(n):
    """`python bench.py --gpus N` invoked plainly: start the N ranks as a CHILD
    `python -m torch.distributed.run` (this parent never imports torch or touches the GPU, and
    nothing is exec'ed from a process that has), forward its output and exit with its code."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % n,
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "1")
    return subprocess.call(cmd, env=env)


class Job:
    """Device-resident operands of one rank's slice and the one-call step over them."""

    def __init__(self, L, torch, dev, local_rank, prob, T, p, q, niter, tol, algo):
        from ldsr_amd import _lib
        Y, U, V, self.shared_uv, loc_off, th0, self.n_global = prob
        self.local_rank = local_rank
        self.loc_off = np.asarray(loc_off, dtype=np.int64)
        self.S, self.cells = Y.shape[0], th0.shape[0]
        self.d_y = torch.from_numpy(Y).to(dev)          # [S][T]
        self.d_u = torch.from_numpy(U).to(dev)          # [S or 1][T][p]
        self.d_v = torch.from_numpy(V).to(dev)          # [S or 1][T][q]
        self.d_th0 = torch.from_numpy(th0).to(dev)
        self.d_th = torch.empty_like(self.d_th0)
        self.d_lik = torch.empty(self.cells, dtype=torch.float64, device=dev)
        self.d_nit = torch.empty(self.cells, dtype=torch.int32, device=dev)
        self.d_st = torch.empty(self.cells, dtype=torch.int32, device=dev)
        self.wsb = L.ldsr_em_workspace_bytes(self.S, T, p, q, self.cells, algo)
        assert self.wsb > 0
        self.d_ws = torch.empty(self.wsb + 256, dtype=torch.uint8, device=dev)
        ws_ptr = (self.d_ws.data_ptr() + 255) & ~255
        off = (C.c_int * (self.S + 1))(*[int(x) for x in loc_off])
        stream = torch.cuda.current_stream(dev)
        # what the generator knows about its own mask and hands over like the host-pointer entries
        # find it from y: the number of leading steps that are missing in EVERY series
        fin = np.isfinite(Y)
        self.lead = int(min((np.argmax(r) if r.any() else Y.shape[1]) for r in fin)) if os.environ.get(
            "LDSR_BENCH_NO_LEAD") is None else 0
        if fin.all() and os.environ.get("LDSR_BENCH_NO_LEAD") is None:
            self.lead = -1         # every y_t observed (ldsr_hip.h: AUTO keeps the pair family with tol > 0)

        def step():
            _lib.check(L.ldsr_em_batch_device_lead(
                local_rank, C.c_void_p(stream.cuda_stream), self.S, T, p, q, self.d_y.data_ptr(),
                self.d_u.data_ptr(), self.d_v.data_ptr(), self.shared_uv, off,
                self.d_th0.data_ptr(), niter, tol, algo, self.d_th.data_ptr(),
                self.d_lik.data_ptr(), self.d_nit.data_ptr(), self.d_st.data_ptr(), None,
                C.c_void_p(ws_ptr), self.wsb, self.lead))
        self.step = step

    def units(self, niter, tol):
        """E-steps this rank executes per step, after checking the run did the work it claims."""
        nit = self.d_nit.cpu().numpy()
        st = self.d_st.cpu().numpy()
        if tol == 0.0:
            assert np.all(nit == niter), "cells stopped early"
        assert np.all(st == 0), "non-finite likelihoods in the bench batch"
        return int(nit.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="cfg2", choices=sorted(WORKLOADS) + ["custom"])
    ap.add_argument("--shape", default=None, help="custom workload: T,p,q,restarts (one series, weak scaling)")
    ap.add_argument("--algo", type=int, default=0, help="0 auto, 1 serial, 2 scan (1-4 waves per cell), 3 pair (two cells per wave)")
    ap.add_argument("--mask", default="dense", choices=["dense", "paleo"])
    ap.add_argument("--niter", type=int, default=None, help="EM iteration cap (default: the workload's 100)")
    ap.add_argument("--tol", type=float, default=0.0,
                    help="stop tolerance; > 0 lets cells converge at their own pace and the "
                         "units are the iterations actually executed")
    ap.add_argument("--scaling", default=None, choices=["weak", "strong"],
                    help="headline split of a single-series workload over the ranks (default weak: "
                         "the per-GPU configuration of BASELINE.json; strong: its restarts / N)")
    ap.add_argument("--full", action="store_true",
                    help="also the legs beside the headline: roofline (HIP-event kernel time, committed "
                         "PMC figures), the oracle check of the last timed launch, host_entry, "
                         "cpu_baseline and, for N > 1, the strong-scaling run")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the last timed launch's theta / lik / n_iter / status as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU oracle baseline")
    ap.add_argument("--no-host-entry", action="store_true",
                    help="--full without the host-pointer-entry leg (ldsr_em_batch, PCIe-inclusive; reported beside value)")
    ap.add_argument("--no-verify", action="store_true",
                    help="--full without the oracle check of a 64-cell sample of the last timed launch")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args.gpus))

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # Rehearsal on a one-GPU box: LDSR_BENCH_ONE_GPU=1 lets several ranks share cuda:0 over gloo
    # (the driver's real runs use one GPU per rank over RCCL).
    one_gpu = os.environ.get("LDSR_BENCH_ONE_GPU") == "1"
    backend = os.environ.get("LDSR_BENCH_BACKEND", "gloo" if one_gpu else "nccl")
    if one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    from ldsr_amd import _lib
    L = _lib.lib()

    if args.workload == "custom":     # diagnostics only (kernel studies); never the reported metric
        cT, cp, cq, cr = [int(x) for x in args.shape.split(",")]
        WORKLOADS["custom"] = dict(T=cT, p=cp, q=cq, series=1, restarts=cr, niter=100, scaling="weak")
    w = WORKLOADS[args.workload]
    T, p, q, niter = w["T"], w["p"], w["q"], (args.niter or w["niter"])
    single = w["series"] == 1
    scaling = (args.scaling or w["scaling"]) if single else w["scaling"]
    job = Job(L, torch, dev, local_rank,
              build_problem(args.workload, args.mask, world, rank, scaling), T, p, q, niter,
              args.tol, args.algo)
    name_buf = C.create_string_buffer(160)
    algo_resolved = L.ldsr_em_plan_lead(T, p, q, niter, args.tol, args.algo, job.lead, name_buf, 160)
    kernel_name = name_buf.value.decode()      # (replaced below by what the first launch really ran)

    def barrier():
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    def reduce_over_ranks(dt, units_rank):
        if world == 1:
            return dt, units_rank
        tdev = dev if backend == "nccl" else "cpu"
        tmax = torch.tensor([dt], dtype=torch.float64, device=tdev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        usum = torch.tensor([units_rank], dtype=torch.int64, device=tdev)
        dist.all_reduce(usum, op=dist.ReduceOp.SUM)
        return float(tmax.item()), int(usum.item())

    def timed(j, profile):
        """W warm-up steps, then exactly K steps between barrier + synchronize brackets."""
        for _ in range(args.warmup):
            j.step()
        barrier()
        if profile:
            L.ldsr_profile_enable(1)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            j.step()
        barrier()
        dt = time.perf_counter() - t0
        kern_ms = None
        if profile:
            tot_ms, n_l = C.c_double(), C.c_int()
            _lib.check(L.ldsr_profile_collect(C.byref(tot_ms), C.byref(n_l)))
            L.ldsr_profile_enable(0)
            kern_ms = tot_ms.value / max(n_l.value, 1)
        units_rank = j.units(niter, args.tol)
        dt, units_all = reduce_over_ranks(dt, units_rank)
        return dt, units_rank, units_all, kern_ms

    def units_by_rank(units_rank):
        """E-steps every rank executed per step (the load balance of the cut)."""
        if world == 1:
            return [units_rank]
        tdev = dev if backend == "nccl" else "cpu"
        mine = torch.tensor([units_rank], dtype=torch.int64, device=tdev)
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine)
        return [int(x.item()) for x in parts]

    dt, units_rank, units_all, kern_ms = timed(job, args.full)   # HIP-event kernel times: --full only
    if args.dump_outputs:
        dump_outputs(job, args.dump_outputs, rank, world)
    per_rank = units_by_rank(units_rank)
    if L.ldsr_last_em_kernel(local_rank, name_buf, 160) == 0:      # the kernel the timed launches ran
        kernel_name = name_buf.value.decode()

    strong = None
    if args.full and world > 1 and single and scaling == "weak":
        # the same run, BASELINE config 2 as ONE job split N ways (restarts / N per rank)
        sjob = Job(L, torch, dev, local_rank,
                   build_problem(args.workload, args.mask, world, rank, "strong"), T, p, q, niter,
                   args.tol, args.algo)
        sdt, _, sunits_all, _ = timed(sjob, False)
        strong = {"scaling": "strong", "cells_total": sjob.n_global, "cells_rank0": sjob.cells,
                  "value": sunits_all * args.steps / sdt, "unit": "restart*EM-iter/s",
                  "ms_per_step": sdt / args.steps * 1e3, "units_per_step": sunits_all}

    if rank == 0:
        value = units_all * args.steps / dt
        out = {
            "metric": "restart x EM-iteration / s (T=%d, p=%d, q=%d)" % (T, p, q),
            "value": value, "unit": "restart*EM-iter/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": "f64",
            "data": "synthetic",
            "config": {"workload": "%s: synthetic T=%d p=%d q=%d, %d series x %d restarts%s, "
                                   "niter=%d, tol=%g, %s mask"
                                   % (args.workload, T, p, q, w["series"], w["restarts"],
                                      "/GPU" if scaling == "weak" else " in total", niter, args.tol,
                                      args.mask if single else "paleo-style"),
                       "cells_rank0": job.cells, "cells_total": job.n_global, "niter": niter,
                       "tol": args.tol, "algo": algo_resolved, "units_per_step": units_all,
                       "sharding": "rank r = the r-th of %d parts of every series' restarts, no collective" % world,
                       "units_per_rank": per_rank,
                       "imbalance_max_over_mean": max(per_rank) * len(per_rank) / max(sum(per_rank), 1)},
        }
        if args.full:
            out["roofline"] = roofline(args.workload, args.mask, kernel_name, niter, args.tol,
                                       T, p, q, units_rank, kern_ms)
        if strong is not None:
            out["strong_scaling"] = strong
        if args.full and not args.no_verify:
            out["verified"] = verify_sample(job, p, q, niter, args.tol)
            if not out["verified"]["ok"]:
                print(json.dumps(out), flush=True)
                sys.exit("bench.py: the timed launch does not match the CPU oracle")
        if args.full and world == 1 and not args.no_host_entry:
            he = host_entry_rate(L, job, T, p, q, niter, args.tol, args.algo, units_rank)
            he["vs_device_resident"] = he["value"] / (units_rank * args.steps / dt)
            out["host_entry"] = he
        if args.full and world == 1 and not args.no_cpu_baseline:
            Y, U, V = (job.d_y.cpu().numpy(), job.d_u.cpu().numpy(), job.d_v.cpu().numpy())
            out["cpu_baseline"] = cpu_baseline(p, q, niter, Y, U, V, seed=1)
            out["cpu_baseline"]["rscript_reference"] = rscript_reference_probe(T, p, q, niter)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
