"""Likelihood on demand in fixed-count EM runs (tol = 0, static schedule) of the pair kernel's steady
form (em_pair_impl.h, pair_need_lik): the likelihood of an iteration is evaluated only where it is read --
by the trace (liks), by a cell's last iteration, at an interrupt poll.  A call that asks for the trace
evaluates every likelihood, so it is the yardstick for one that does not: theta, lik, n_iter and status
must agree bit for bit, and both must meet the oracle at the suite's bar (identical
n_iter, |d| <= 1e-6 |ref| + 1e-9).  Through ldsr_em_batch_device, on the smallest steady shapes: T = 737
(the shortest series that takes the form, chunks of 24 steps), 1000 and 1024; a third of the cells start
slow (A = 0.97, C = 0.03, as tests/test_gpu_pair.py builds them) and the cell count is odd, so that S loop,
G phase, mixed waves, waiting halves and an idle half all occur.  With (p, q) = (2, 4) the pair kernel ends
at T = 896 (eight waves' strips must fit the CU's LDS): T = 896 is added for it, and its T = 1000 / 1024 cases
run whatever kernel the plan gives such a call -- they guard that kernel the way the masked series does."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import parity_close

pytestmark = pytest.mark.gpu

AUTO, PAIR = 0, 3              # LDSR_ALGO_AUTO, LDSR_ALGO_PAIR
NCELL = 95
NITERS = (2, 3, 5, 70)         # 70 crosses the interrupt poll of the wave's 64th iteration
SHAPES = [(T, p, q) for T in (737, 1000, 1024) for (p, q) in ((1, 2), (1, 1), (2, 4))] + [(896, 2, 4)]
NOT_PAIR = [(1000, 2, 4), (1024, 2, 4)]       # no pair kernel for these: the plan's own choice


def _series(T, p, q):
    from ldsr_amd import synth
    return synth.make_series(T, p, q, series_id=300 + T + 10 * p + q)


def _theta0(T, p, q, n=NCELL):
    from ldsr_amd import synth
    th0 = synth.make_init_packed(p, q, n, seed=T + p + q)
    th0[0::3, 0], th0[0::3, 1 + p] = 0.97, 0.03          # A, C: slow for tens of iterations
    return th0


def _device_run(y, u, v, th0, niter, trace, algo=PAIR):
    """One ldsr_em_batch_device call (tol = 0) -> theta, lik, n_iter, status[, liks]."""
    import torch
    from ldsr_amd import _lib
    L = _lib.lib()
    T, p, q, n = y.shape[0], u.shape[0], v.shape[0], th0.shape[0]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    d_y = torch.from_numpy(np.ascontiguousarray(y)).to(dev)
    d_u = torch.from_numpy(np.ascontiguousarray(u.T)).to(dev)
    d_v = torch.from_numpy(np.ascontiguousarray(v.T)).to(dev)
    d_th0 = torch.from_numpy(np.ascontiguousarray(th0)).to(dev)
    d_th = torch.full(th0.shape, np.nan, dtype=torch.float64, device=dev)
    d_lik = torch.full((n,), np.nan, dtype=torch.float64, device=dev)
    d_nit = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    d_liks = torch.full((n, niter), np.nan, dtype=torch.float64, device=dev) if trace else None
    wsb = L.ldsr_em_workspace_bytes(1, T, p, q, n, algo)
    ws = torch.empty(wsb + 256, dtype=torch.uint8, device=dev)
    off_c = (C.c_int * 2)(0, n)
    _lib.check(L.ldsr_em_batch_device(
        0, C.c_void_p(stream.cuda_stream), 1, T, p, q, d_y.data_ptr(), d_u.data_ptr(), d_v.data_ptr(), 1, off_c,
        d_th0.data_ptr(), niter, 0.0, algo, d_th.data_ptr(), d_lik.data_ptr(), d_nit.data_ptr(), d_st.data_ptr(),
        d_liks.data_ptr() if trace else None, C.c_void_p((ws.data_ptr() + 255) & ~255), wsb))
    torch.cuda.synchronize(dev)
    r = {"theta": d_th.cpu().numpy(), "lik": d_lik.cpu().numpy(), "n_iter": d_nit.cpu().numpy(),
         "status": d_st.cpu().numpy()}
    if trace:
        r["liks"] = d_liks.cpu().numpy()
    return r


def _oracle(y, u, v, th0, niter):
    from oracle import oracle as O
    return O.em_batch(y[None], np.ascontiguousarray(u.T[None]), np.ascontiguousarray(v.T[None]),
                      np.zeros(th0.shape[0], np.int32), th0, niter, 0.0, n_threads=16)


def _same_bits(a, b, what):
    for k in ("theta", "lik", "n_iter", "status"):
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), "%s: %s differs" % (what, k)


def _last_of_trace(r):
    return r["liks"][np.arange(r["liks"].shape[0]), r["n_iter"] - 1]


@functools.lru_cache(maxsize=None)
def _runs(T, p, q):
    """niter -> (call without the trace, call with it, oracle); computed once per shape for both tests."""
    from ldsr_amd import _lib
    buf = C.create_string_buffer(160)
    algo = AUTO if (T, p, q) in NOT_PAIR else PAIR
    if algo == PAIR:
        assert _lib.lib().ldsr_em_plan(T, p, q, 100, 0.0, PAIR, buf, 160) == PAIR
        name = buf.value.decode()                   # two cells per wave, chunks of 24+ steps, static schedule
        assert name.endswith(", 32, false, false>") and int(name.split(",")[2]) >= 24, name
    y, u, v = _series(T, p, q)
    th0 = _theta0(T, p, q)
    return {niter: (_device_run(y, u, v, th0, niter, False, algo), _device_run(y, u, v, th0, niter, True, algo),
                    _oracle(y, u, v, th0, niter)) for niter in NITERS}


@pytest.mark.parametrize("T,p,q", SHAPES)
def test_untraced_call_equals_traced_call_bit_for_bit(T, p, q):
    for niter, (plain, traced, _) in _runs(T, p, q).items():
        what = "T=%d p=%d q=%d niter=%d" % (T, p, q, niter)
        _same_bits(plain, traced, what)
        assert np.all(plain["n_iter"] == niter), what
        assert np.array_equal(_last_of_trace(traced), traced["lik"], equal_nan=True), what
        assert np.all(np.isfinite(traced["liks"])), what       # every iteration's likelihood is in the trace


@pytest.mark.parametrize("T,p,q", SHAPES)
def test_both_calls_match_the_oracle(T, p, q):
    for niter, (plain, traced, ref) in _runs(T, p, q).items():
        ref_th, ref_lik, ref_it, ref_st = ref
        assert np.all(np.isfinite(ref_lik)) and np.all(np.isfinite(ref_th))     # the slow cells stay finite
        for r, name in ((plain, "plain"), (traced, "traced")):
            what = "%s T=%d p=%d q=%d niter=%d" % (name, T, p, q, niter)
            assert np.array_equal(r["n_iter"], ref_it), what
            assert np.array_equal(r["status"], ref_st), what
            assert parity_close(r["theta"], ref_th, 1e-6, 1e-9), what
            assert parity_close(r["lik"], ref_lik, 1e-6, 1e-9), what


def test_negative_sigma_in_the_last_iteration_is_still_reported():
    """A negative variance in theta0 (tests/test_gpu_parity.py builds its negative-variance cells the same way).
    A negative R is repaired by the first M-step, so Q = -0.5 is the one set here: by the oracle's account it
    leaves cell 9 (a slow one) with 108 negative Sigma_t in iteration 1 and cell 32 (whose wave partner is idle)
    with R < 0, 999 negative Sigma_t, in iteration 2.  Where that iteration is the last, its likelihood is the log
    of a negative number -- NaN, status 1 -- and theta is whatever the M-steps made of it: the same bits as in
    the traced run."""
    T, p, q = 1000, 1, 2
    y, u, v = _series(T, p, q)
    th0 = _theta0(T, p, q, 33)
    bad = [4, 9, 32]                                   # a fast cell, a slow one, the one with an idle partner
    th0[bad, 2 + p + q] = -0.5
    ok = np.setdiff1d(np.arange(33), bad)
    for niter, c in ((2, 9), (3, 32)):
        ref_th, ref_lik, ref_it, _ = _oracle(y, u, v, th0, niter)
        assert np.isnan(ref_lik[c]) and np.all(np.isfinite(ref_th[c]))           # (what the case is there for)
        plain, traced = _device_run(y, u, v, th0, niter, False), _device_run(y, u, v, th0, niter, True)
        _same_bits(plain, traced, "niter=%d" % niter)
        assert np.isnan(plain["lik"][c]) and plain["status"][c] == 1 and plain["n_iter"][c] == niter
        assert np.isnan(traced["liks"][c, niter - 1])
        assert np.all((plain["status"] == 0) == np.isfinite(plain["lik"]))
        assert np.array_equal(plain["n_iter"], ref_it)
        assert parity_close(plain["theta"][ok], ref_th[ok], 1e-6, 1e-9) and parity_close(plain["lik"][ok], ref_lik[ok], 1e-6, 1e-9)


def test_series_with_an_unobserved_value_keeps_its_body():
    """One unobserved y_t sends the series to the masked generic body, which evaluates the likelihood in every
    iteration as before: traced and untraced calls agree bit for bit, and with the oracle."""
    T, p, q = 1000, 1, 2
    y, u, v = _series(T, p, q)
    y = y.copy()
    y[417] = np.nan
    th0 = _theta0(T, p, q, 33)
    for niter in (3, 70):
        plain, traced = _device_run(y, u, v, th0, niter, False), _device_run(y, u, v, th0, niter, True)
        _same_bits(plain, traced, "niter=%d" % niter)
        assert np.array_equal(_last_of_trace(traced), traced["lik"], equal_nan=True)
        ref_th, ref_lik, ref_it, ref_st = _oracle(y, u, v, th0, niter)
        assert np.array_equal(plain["n_iter"], ref_it) and np.array_equal(plain["status"], ref_st)
        assert parity_close(plain["theta"], ref_th, 1e-6, 1e-9) and parity_close(plain["lik"], ref_lik, 1e-6, 1e-9)
