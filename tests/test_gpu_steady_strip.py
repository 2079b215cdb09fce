"""B u_t without the LDS strip in the steady sweeps of the pair kernel (em_pair_impl.h, em_pair_body_steady,
REREAD_U): with one input (padded p = 1) F1 no longer stores B u_t; F2 and the on-demand likelihood pass rebuild
it from the series image's own u values.  Checked against the CPU oracle at the suite's bar (SURVEY.md Appendix B:
identical n_iter, |d| <= 1e-6 |ref| + 1e-9 on theta and lik) and against the serial kernel (algo = 1), on eight
cells of one fully observed series: the chunk shapes of the steady form (T = 737: L = 24, the shortest; 993: L = 32
with lane 0 alone owning a predicated step; 1000; 1024: every lane predicated), the widths on either side of the
predicate ((1,1), (1,2): re-read; (2,1), (2,2), (4,2): strip kept; u absent: B u_t = 0), the three paths that
read it (likelihood on the last iteration only, in every iteration for the trace, the work-queue member) and a
batch with a slow cell, whose wave leaves the S loop for the G phase -- which still keeps h_t in the strip --
and returns.  ldsr_last_em_kernel names the kernel that ran.  At T = 1000 the eight strips leave room for the
series image up to two 16-byte pairs per step: (2,2) and (4,2) get whatever kernel the plan gives them there,
and are run once more at the longest series that takes the steady form (T = 928: L = 29; T = 864: L = 27).
One test without a GPU reads the listing of config 2's kernel: no ds_write_b64 and no scratch in its S loop."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from conftest import parity_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 1e-6, 1e-9
AUTO, SERIAL, PAIR = 0, 1, 3
NCELL, NITER = 8, 6


def _pad(n):
    return 1 if n <= 1 else 2 if n <= 2 else 4


def _steady_fits(T, p, q):
    """em_pair_impl.h pair_steady(): image + eight strips + transient block within 160 KiB, chunks of 24+ steps."""
    L, K = -(-T // 32), 1 + _pad(p) + _pad(q)
    img = 64 * (L * (K // 2) + (K & 1) * ((L + 1) // 2))
    return L >= 24 and (img + 8 * 64 * (L - 1) + 64 * ((K + 1) // 2)) * 8 <= 160 * 1024


@functools.lru_cache(maxsize=None)
def _problem(T, p, q, slow=False):
    from ldsr_amd import synth
    y, u, v = synth.make_series(T, p, q, series_id=1400 + T + 10 * p + q)
    th0 = synth.make_init_packed(p, q, NCELL, seed=T + 7 * p + q)
    if slow:
        th0[2, 0], th0[2, 1 + p] = 0.97, 0.03        # A, C: fails the verdict for tens of iterations
    return y, u, v, th0


@functools.lru_cache(maxsize=None)
def _oracle(T, p, q, niter, tol, has_u=True, slow=False):
    from oracle import oracle as O
    y, u, v, th0 = _problem(T, p, q, slow)
    return O.em_batch(y[None], np.ascontiguousarray(u.T[None]) if has_u else None, np.ascontiguousarray(v.T[None]),
                      np.zeros(NCELL, np.int32), th0, niter, tol, n_threads=8)


def _last_kernel():
    from ldsr_amd import _lib
    buf = C.create_string_buffer(160)
    assert _lib.lib().ldsr_last_em_kernel(0, buf, 160) == 0
    return buf.value.decode()


def _case(T, p, q, niter=NITER, tol=0.0, trace=False, has_u=True, slow=False):
    """One call on the pair kernel (the plan's own choice where the shape has no steady member), checked against
    the oracle and the serial kernel; -> the call's result."""
    import ldsr_amd
    y, u, v, th0 = _problem(T, p, q, slow)
    uu = u if has_u else None
    what = "T=%d p=%d q=%d niter=%d tol=%g trace=%d has_u=%d slow=%d" % (T, p, q, niter, tol, trace, has_u, slow)
    steady = _steady_fits(T, p, q)
    r = ldsr_amd.em_batch(y, uu, v, th0, niter=niter, tol=tol, algo=PAIR if steady else AUTO, return_liks=trace)
    if steady:
        assert _last_kernel() == "em_pair_kernel<%d, %d, %d, 32, %s, false>" % (
            _pad(p), _pad(q), -(-T // 32), "true" if tol > 0 else "false"), what
    ref_th, ref_lik, ref_it, ref_st = _oracle(T, p, q, niter, tol, has_u, slow)
    assert np.all(np.isfinite(ref_th)) and np.all(np.isfinite(ref_lik)), what
    assert np.array_equal(r["n_iter"], ref_it), what
    assert np.array_equal(r["status"], ref_st), what
    assert parity_close(r["theta"], ref_th, RTOL, ATOL), what
    assert parity_close(r["lik"], ref_lik, RTOL, ATOL), what
    s = ldsr_amd.em_batch(y, uu, v, th0, niter=niter, tol=tol, algo=SERIAL)
    assert np.array_equal(r["n_iter"], s["n_iter"]), what
    assert parity_close(r["theta"], s["theta"], RTOL, ATOL) and parity_close(r["lik"], s["lik"], RTOL, ATOL), what
    if tol == 0.0:
        assert np.all(r["n_iter"] == niter), what
    if trace:
        k = r["n_iter"]
        assert np.array_equal(r["liks"][np.arange(NCELL), k - 1], r["lik"]), what
        for c in range(NCELL):
            assert np.all(np.isfinite(r["liks"][c, :k[c]])), what
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("T", [737, 993, 1000, 1024])
def test_chunk_shapes(T):
    """L = 24 and 32; rp = 1 (T = 993: lane 0 alone owns a predicated step, whose B u_t stays in a register),
    rp = 8 and rp = 32."""
    assert _steady_fits(T, 1, 2)
    _case(T, 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("T,p,q", [(1000, 1, 1), (1000, 1, 2), (1000, 2, 1), (1000, 2, 2), (928, 2, 2),
                                   (1000, 4, 2), (864, 4, 2)])
def test_widths(T, p, q):
    """One u read per step on the new path; padded p = 2 and 4 keep the strip and must still agree."""
    assert _steady_fits(T, p, q) == ((T, p, q) not in ((1000, 2, 2), (1000, 4, 2)))
    _case(T, p, q)


@pytest.mark.gpu
def test_absent_u():
    """has_u false: B stays an exact zero and B u_t = 0 from the image's zero column as from the strip."""
    r = _case(1000, 1, 2, has_u=False)
    assert np.all(r["theta"][:, 1] == 0.0)


@pytest.mark.gpu
def test_paths_that_read_bu():
    """tol = 0 without the trace: the likelihood pass runs in the last iteration only; with the trace it runs in
    every iteration and reads u too -- the same bits; tol > 0: the work-queue member, likelihood inside F2."""
    plain = _case(1000, 1, 2)
    traced = _case(1000, 1, 2, trace=True)
    for k in ("theta", "lik", "n_iter", "status"):
        assert np.array_equal(plain[k], traced[k]), k
    r = _case(1000, 1, 2, niter=200, tol=1e-5)
    assert np.all(r["n_iter"] < 200)


@pytest.mark.gpu
@pytest.mark.parametrize("tol", [0.0, 1e-5])
def test_slow_cell_leaves_for_the_g_phase_and_returns(tol):
    """Cell 2 starts at A = 0.97, C = 0.03: its wave runs generic iterations (h_t in the strip) until the cell
    passes the verdict, then steady ones again; the other waves stay in the S loop throughout."""
    _case(1000, 1, 2, niter=100, tol=tol, slow=True)


def test_s_loop_of_config2_holds_no_strip_store_and_no_scratch():
    """Listing of em_pair_kernel<1, 2, 32, 32, false, false> (BASELINE config 2): its S loop -- the largest loop
    without the call of pair_steady_g_phase inside the loop that holds the call -- has no ds_write_b64 (the strip
    store of B u_t was the only LDS store of the steady sweeps) and no scratch instruction."""
    import subprocess
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import loop_mix
    csrc = os.path.join(ROOT, "ldsr_amd", "csrc")
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "one.hip")
        with open(src, "w") as f:
            f.write('#include "em_pair_impl.h"\n'
                    'template __global__ void em_pair_kernel<1, 2, 32, 32, false, false>(EmParams);\n')
        asm = os.path.join(td, "one.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-I" + csrc, "--offload-arch=gfx950",
                        "--cuda-device-only", "-S", src, "-o", asm], check=True, capture_output=True)
        found = loop_mix.loops(asm, "em_pair_kernelILi1ELi2ELi32ELi32ELb0ELb0EE")
    outer = max((f for f in found if f[4].get("s_swappc_b64", 0)), key=lambda f: f[2] - f[1])
    inner = [f for f in found if f[1] >= outer[1] and f[2] <= outer[2] and not f[4].get("s_swappc_b64", 0)]
    _, lo, hi, classes, ops, _ = max(inner, key=lambda f: f[2] - f[1])
    assert hi - lo > 1500 and ops.get("ds_read_b128", 0) >= 100, (lo, hi, ops.most_common(8))   # the S loop it is
    assert ops.get("ds_write_b64", 0) == 0, ops
    assert not any(op.startswith("ds_write") for op in ops), [op for op in ops if op.startswith("ds_write")]
    assert classes.get("scratch", 0) == 0, classes
