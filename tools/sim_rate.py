#!/usr/bin/env python3
"""Rates of the stochastic-replicate kernel (simulate.hip; LDS_rep of the reference's R/stochastics.R).

    python tools/sim_rate.py                 # vignette call + large device-resident job (GPU)
    python tools/sim_rate.py --large-only    # the large job alone (for a rocprofv3 --kernel-trace run)
    python tools/sim_rate.py --static        # VALU instructions per step from the ISA (no GPU)

Vignette call: set.seed(100); LDS_rep(NPlds$theta, t(NPpc), t(NPpc), 1200:2012, mu = mean(log(Qa))),
100 replicates x 813 steps, split into host uniforms, the host entry's copies and the kernel, against
a plain serial loop of the same recursion on the host.  Large job: 48 models x 10 000 replicates x
813 steps, p = q = 3, counter mode, simX / simY / simQ written (24 B per step), device buffers."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBS = 6.29          # measured float4-copy rate of the MI355X (TB/s)


def np_case():
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_data.json")))
    th = ref["NPlds"]["theta"]
    theta = np.concatenate([th["A"][:1], np.ravel(th["B"]), th["C"][:1], np.ravel(th["D"]), th["Q"][:1], th["R"][:1],
                            th["mu1"][:1], th["V1"][:1]]).astype(np.float64)
    pcs = np.array(ref["NPpc"]["data"], dtype=np.float64)          # 3 x 813
    mu = float(np.log(np.array(ref["NPannual"]["Qa"])).mean())
    return theta, pcs, mu


def med(f, n):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def serial_loop(theta, u, n, reps, z):
    """The reference's loop (R/stochastics.R:34-37) on the host, normals already drawn."""
    A, B, Cc, D, sq, sr = theta[0], theta[1:4], theta[4], theta[5:8], np.sqrt(theta[8]), np.sqrt(theta[9])
    out = np.empty((reps, n))
    for k in range(reps):
        x = np.sqrt(theta[11]) * z[k, 0]
        for t in range(n):
            out[k, t] = Cc * x + D @ u[:, t] + sr * z[k, 1 + n + t]
            x = A * x + B @ u[:, t] + sq * z[k, 1 + t]
    return out


def kernel_ms(L, C, torch, args, iters):
    """Median kernel time of ldsr_simulate_batch_device from HIP events on the launch stream."""
    from ldsr_amd import _lib
    stream = torch.cuda.current_stream()
    ts = []
    for i in range(iters + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        _lib.check(L.ldsr_simulate_batch_device(0, C.c_void_p(stream.cuda_stream), *args))
        b.record(stream)
        b.synchronize()
        if i >= 2:
            ts.append(a.elapsed_time(b))
    return float(np.median(ts)), ts


def vignette(L, C, torch):
    import ldsr_amd
    from ldsr_amd import rrng
    theta, pcs, mu = np_case()
    n, reps = 813, 100
    years = np.arange(1200, 2013)
    count, off = ldsr_amd.sim.draw_count(theta, n, reps, 3, 3)
    ldsr_amd.LDS_rep(theta, pcs, pcs, years=years, num_reps=reps, mu=mu, r_seed=100)       # warm-up
    t_unif = med(lambda: rrng.RUniform(100).unif_rand(count), 20)
    t_e2e = med(lambda: ldsr_amd.LDS_rep(theta, pcs, pcs, years=years, num_reps=reps, mu=mu, r_seed=100), 20)
    uni = rrng.RUniform(100).unif_rand(count)
    t_host = med(lambda: ldsr_amd.simulate_batch(theta, pcs, pcs, n, reps, mu=mu, uniforms=uni), 20)
    dev = torch.device("cuda:0")
    d_th = torch.from_numpy(theta[None].copy()).to(dev)
    d_u = torch.from_numpy(np.ascontiguousarray(pcs.T)).to(dev)
    d_mu = torch.tensor([mu], dtype=torch.float64, device=dev)
    d_uni = torch.from_numpy(uni).to(dev)
    d_off = torch.zeros(1, dtype=torch.int64, device=dev)
    outs = [torch.empty((1, reps, n), dtype=torch.float64, device=dev) for _ in range(3)]
    k_ms, _ = kernel_ms(L, C, torch, (1, n, 3, 3, d_u.data_ptr(), d_u.data_ptr(), 1, d_th.data_ptr(), d_mu.data_ptr(),
                                      reps, 0, 1, 0, d_uni.data_ptr(), d_off.data_ptr(),
                                      *[o.data_ptr() for o in outs]), 50)
    z = rrng.RUniform(100).norm_rand(reps * (1 + 2 * n)).reshape(reps, 1 + 2 * n)
    t0 = time.perf_counter()
    serial_loop(theta, pcs, n, reps, z)
    t_loop = (time.perf_counter() - t0) * 1e3
    print("== vignette call: LDS_rep(NPlds theta, t(NPpc), t(NPpc), 1200:2012, mu, r_seed = 100), 100 x 813")
    print("uniforms drawn on the host       %8d (%.1f MB)" % (count, count * 8 / 1e6))
    print("end-to-end LDS_rep               %8.3f ms  (median of 20)" % t_e2e)
    print("  host uniforms (RUniform)       %8.3f ms" % t_unif)
    print("  host entry, uniforms given     %8.3f ms  (copies in / out + launch + kernel)" % t_host)
    print("    kernel (HIP events)          %8.4f ms  (median of 50, device entry)" % k_ms)
    print("    copies + host marshalling    %8.3f ms  (host entry - kernel)" % (t_host - k_ms))
    print("  rest (Python, long format)     %8.3f ms" % (t_e2e - t_unif - t_host))
    print("serial host loop (numpy, normals given) %8.1f ms  = %.0fx the end-to-end call" % (t_loop, t_loop / t_e2e))


def large(L, C, torch, iters):
    theta, pcs, _ = np_case()
    M, reps, n = 48, 10000, 813
    th = np.repeat(theta[None], M, axis=0)
    th[:, 0] = np.linspace(0.3, 0.9, M)                   # 48 different members
    dev = torch.device("cuda:0")
    d_th = torch.from_numpy(th).to(dev)
    d_u = torch.from_numpy(np.ascontiguousarray(pcs.T)).to(dev)
    d_mu = torch.full((M,), 9.0, dtype=torch.float64, device=dev)
    outs = [torch.empty((M, reps, n), dtype=torch.float64, device=dev) for _ in range(3)]
    ms, ts = kernel_ms(L, C, torch, (M, n, 3, 3, d_u.data_ptr(), d_u.data_ptr(), 1, d_th.data_ptr(), d_mu.data_ptr(),
                                     reps, 0, 1, 12345, None, None, *[o.data_ptr() for o in outs]), iters)
    steps = M * reps * n
    gb = steps * 24 / 1e9
    print("== large job: 48 models x 10 000 replicates x 813 steps, p = q = 3, counter mode, 3 outputs")
    print("kernel (HIP events)      %.3f ms median of %d  (all: %s)" % (ms, len(ts), " ".join("%.3f" % t for t in ts)))
    print("steps/s                  %.3e" % (steps / (ms * 1e-3)))
    print("written                  %.2f GB -> %.2f TB/s = %.2f of the %.2f TB/s measured HBM rate"
          % (gb, gb / ms, gb / ms / HBM_TBS, HBM_TBS))
    print("write bound              %.3f ms" % (gb / HBM_TBS))
    assert bool(torch.isfinite(outs[2]).all())


def static():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import loop_mix
    import resource_usage
    csrc = os.path.join(ROOT, "ldsr_amd", "csrc")
    for r in resource_usage.table(os.path.join(csrc, "simulate.hip")):
        print("resources  %s: VGPR %d, AGPR %d, VGPR spill %d, scratch %d B/lane, occupancy %d waves/SIMD, SGPR %d"
              % (r[0], r[1], r[2], r[3], r[4], r[5], r[6]))
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "sim.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-I" + csrc, "--offload-arch=gfx950",
                        "--cuda-device-only", "-S", os.path.join(csrc, "simulate.hip"), "-o", asm],
                       check=True, capture_output=True)
        found = loop_mix.loops(asm, "ldsr_simulate_kernel")
    # hipcc unswitches the chunk loop into one copy per combination of (u, v, R-stream / counter
    # uniforms); each copy holds both qnorm tails, of which the r > 5 one runs for p < 1.4e-11 only
    for name, lo, hi, c, ops, n in found:
        valu = sum(v for k, v in c.items() if k.startswith("valu"))
        if valu < 100:
            continue                  # the p / q loops of B u_t, D v_t
        print("chunk loop copy, %4d instructions (= per step: one lane per step): VALU %d (%s); SALU %d, VMEM %d, "
              "scratch %d" % (hi - lo, valu, ", ".join("%s %d" % (k[5:], v) for k, v in sorted(c.items())
                                                         if k.startswith("valu")),
                              c.get("salu", 0), c.get("vmem", 0), c.get("scratch", 0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large-only", action="store_true")
    ap.add_argument("--static", action="store_true")
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    if a.static:
        static()
        return
    import ctypes as C

    import torch
    from ldsr_amd import _lib
    L = _lib.lib()
    if not a.large_only:
        vignette(L, C, torch)
    large(L, C, torch, a.iters)


if __name__ == "__main__":
    main()
