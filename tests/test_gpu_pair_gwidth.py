"""The generic (G) iterations of the steady pair kernel run a lone slow cell on all 64 lanes of its wave and two
slow cells side by side on 32 lanes each (em_pair_impl.h, LDSR_G_SUBCHUNK).  Both widths are drivers of one
sub-chunk body and must give a cell the same bits: the same slow cells are launched (a) paired with each other,
(b) each with a fast partner, (c) each alone in its wave, under the static schedule (tol = 0) and through the
work queue (a tol that stops no one), and theta / lik / n_iter / status of every slow cell must be exactly
equal in all six; each launch also meets the oracle at the pair family's bar (identical n_iter,
|d| <= 1e-6 |ref| + 1e-9).

Which cells share a wave: series_prep sorts the cells of a launch by predicted slowness (stable, slowest
first) and a launch of up to 16 cells is one workgroup whose wave w takes sorted cells 2w, 2w + 1.  So (a) is one
launch of the slow cells alone (an even count), (b) one launch of two cells per slow cell (the slow one sorts
first), (c) one launch of one cell each.

That the cells are what the test needs is checked on the CPU first: the kernel's verdict (pair_var_block: the
Riccati recursion from V1 reaches its fixed point to 2^-48 within the L-1 steps of the first chunk, J^2 < 0.8)
is replayed on the oracle's theta of every iteration with a margin on either side -- a factor four in the bound
(2^-50 for "steady", 2^-46 for "slow"; the kernel's Vp comes out of a scan of 2x2 products and differs from the
sequential recursion's by a few ulp, the bound is 32 ulp) and two steps -- so that a rounding difference between
the replay and the kernel cannot change a cell's class."""
import numpy as np
import pytest

from conftest import parity_close

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-9
PAIR = 3
NITER = 12
TOL_Q = 1e-300      # > 0: the work-queue members; |lik - lik1| < 1e-300 stops no one
# (T, p, q): L = 32 (sub-chunks of 16 + 16), L = 24 (12 + 12) and L = 25 (13 + 12: the odd length has a third
# power of the step block and other image offsets for `b`), one input pair per step (K = 4) and wider: p = 2 with
# an odd K = 5 (the odd value's pairs), q = 4 (K = 6)
CASES = [(1000, 1, 2), (737, 1, 2), (800, 1, 2), (1000, 2, 1), (737, 2, 2), (800, 2, 2), (737, 1, 4)]


@pytest.fixture(scope="module")
def eng():
    import ldsr_amd
    return ldsr_amd


def _oracle(y, u, v, th0, niter, tol):
    from oracle import oracle as O
    return O.em_batch(np.atleast_2d(y), np.ascontiguousarray(u.T[None]), np.ascontiguousarray(v.T[None]),
                      np.zeros(len(th0), np.int32), th0, niter, tol, n_threads=8)


def _settled(th, p, q, steps, bound):
    """pair_var_block's verdict with `steps` transient steps and `bound` for 2^-48, sequentially in float64."""
    A, C, Q, R, V1 = th[0], th[1 + p], th[2 + p + q], th[3 + p + q], th[5 + p + q]
    Vp = V1
    for _ in range(steps):
        Vp = A * A * (R * Vp / (C * C * Vp + R)) + Q
    Vu = R * Vp / (C * C * Vp + R)
    Vp1 = A * A * Vu + Q
    J = A * Vu / Vp1
    return abs(Vp1 - Vp) <= bound * abs(Vp) and Vp > 0.0 and J * J < 0.8


def _slow_iterations(y, u, v, th0, p, q, L):
    """Per cell: in how many of the NITER iterations it is surely slow / surely steady (theta of iteration k is
    what a run of k + 1 iterations returns, the theta that produced the last fit; the oracle runs two or more)."""
    slow = np.zeros(len(th0), int)
    fast = np.zeros(len(th0), int)
    for k in range(NITER):
        th = _oracle(y, u, v, th0, k + 1, 0.0)[0] if k else th0
        for c in range(len(th0)):
            slow[c] += not _settled(th[c], p, q, L - 1 + 2, 2.0 ** -46)
            fast[c] += bool(_settled(th[c], p, q, L - 1 - 2, 2.0 ** -50))
    return slow, fast


def _same(r, i, s, k, what):
    assert np.array_equal(r["theta"][i], s["theta"][k]), what
    assert r["lik"][i] == s["lik"][k] and r["n_iter"][i] == s["n_iter"][k] and r["status"][i] == s["status"][k], what


@pytest.mark.parametrize("T,p,q", CASES)
def test_a_slow_cell_has_the_same_bits_on_32_and_on_64_lanes(eng, T, p, q):
    from ldsr_amd import _lib, synth
    import ctypes as C
    L = -(-T // 32)
    buf = C.create_string_buffer(160)
    for tol, queue in ((0.0, "false"), (TOL_Q, "true")):
        _lib.lib().ldsr_em_plan(T, p, q, NITER, float(tol), PAIR, buf, 160)
        pp, qq = (1 if p <= 1 else 2 if p <= 2 else 4), (1 if q <= 1 else 2 if q <= 2 else 4)
        assert buf.value.decode() == "em_pair_kernel<%d, %d, %d, 32, %s, false>" % (pp, qq, L, queue)
    y, u, v = synth.make_series(T, p, q, series_id=300 + T + 10 * p + q)
    pool = synth.make_init_packed(p, q, 24, seed=T + p + q)
    slow0 = pool[:6].copy()
    slow0[:4, 0], slow0[:4, 1 + p] = 0.97, 0.03          # like cell 132 of the bench grid: slow for tens of iterations
    slow0[4:, 0], slow0[4:, 1 + p] = 0.85, 0.10          # a handful of iterations, then steady: the wave changes width
    ns, _ = _slow_iterations(y, u, v, slow0, p, q, L)
    assert np.all(ns[:4] >= 6) and np.all(ns >= 1), ns
    _, nf = _slow_iterations(y, u, v, pool[6:], p, q, L)
    fast0 = pool[6:][nf == NITER][:6]
    assert len(fast0) == 6, nf
    ref = _oracle(y, u, v, slow0, NITER, 0.0)
    base = None
    for tol in (0.0, TOL_Q):
        # (a) slow with slow
        a = eng.em_batch(y, u, v, slow0, niter=NITER, tol=tol, algo=PAIR)
        assert np.all(a["n_iter"] == ref[2]), "T=%d tol=%g: iteration counts" % (T, tol)
        assert parity_close(a["lik"], ref[1], RTOL, ATOL) and parity_close(a["theta"], ref[0], RTOL, ATOL)
        if base is None:
            base = a
        for i in range(6):
            _same(base, i, a, i, "T=%d (%d,%d) cell %d: tol = 0 against the work queue" % (T, p, q, i))
            # (b) with a fast partner (the slow cell sorts first: half 0 of the wave; a lone slow cell in half 1
            # is what (a) has whenever the cell in half 0 settles before its partner)
            b = eng.em_batch(y, u, v, np.stack([slow0[i], fast0[i]]), niter=NITER, tol=tol, algo=PAIR)
            _same(base, i, b, 0, "T=%d (%d,%d) cell %d tol=%g: slow partner against fast partner" % (T, p, q, i, tol))
            # (c) alone in its wave
            c = eng.em_batch(y, u, v, slow0[i:i + 1].copy(), niter=NITER, tol=tol, algo=PAIR)
            _same(base, i, c, 0, "T=%d (%d,%d) cell %d tol=%g: slow partner against no partner" % (T, p, q, i, tol))
