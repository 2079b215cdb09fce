"""Kalman_smoother and penalized_likelihood on a series whose Svv / Tuu is singular (run with -m gpu).  The scan
kernel whitens the inputs by these matrices and flags such a series instead of answering, but the smoother
(src/EM.cpp:22-131) needs neither: ldsr_smooth_batch and ldsr_penalized_lik_batch run the flagged series' cells
on the serial kernel.  Checked against the CPU oracle under the project's parity bar, and bit for bit against the
calls that hold one series alone."""
import numpy as np
import pytest

from conftest import parity_close
from test_gpu_bfgs import _mask, _thetas
from test_plgrad_host import oracle_pl

pytestmark = pytest.mark.gpu

LAM = 0.25


@pytest.fixture(scope="module")
def eng():
    import ldsr_amd
    from ldsr_amd import _lib
    assert _lib.lib().ldsr_device_count() >= 1, "no GPU visible"
    return ldsr_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _series(T, p, q, mask):
    from ldsr_amd import synth
    y, u, v = synth.make_series(T, p, q, series_id=T + p)
    return _mask(y, mask), u, v


# one observation for three columns of v (Svv), T = 65 and T = 3; one transition for three columns of u (Tuu)
@pytest.mark.parametrize("T,p,q,mask", [(65, 3, 3, "last"), (3, 3, 3, "last"), (65, 3, 3, "first"), (2, 3, 1, "none")])
def test_singular_series_against_the_oracle(eng, O, T, p, q, mask):
    y, u, v = _series(T, p, q, mask)
    th = _thetas(p, q, (0.0, 0.5, -0.9, 0.999))
    assert np.all(eng.em_batch(y, u, v, th, niter=3, tol=0.0)["status"] == 2)         # the series is a singular one
    pl = eng.penalized_likelihood(y, u, v, th, LAM)
    for stdlik in (True, False):
        fit = eng.smooth_batch(y, u, v, th, stdlik=stdlik)
        for i, t in enumerate(th):
            ref = O.kalman_smoother(y, u, v, t, stdlik=stdlik)
            for k in ("X", "Y", "V", "J"):
                assert parity_close(fit[k][i], np.asarray(ref[k]).reshape(-1)), (k, i, stdlik)
            assert np.isfinite(fit["lik"][i]) and parity_close(fit["lik"][i], ref["lik"]), (i, stdlik)
    for i, t in enumerate(th):
        assert np.isfinite(pl[i]) and parity_close(pl[i], oracle_pl(O, t, y, u, v, LAM)), (i, pl[i])


def test_a_singular_series_next_to_a_regular_one(eng):
    """Each series' rows are those of the call that holds it alone, whatever shares the call."""
    y1, u, v = _series(65, 3, 3, "last")
    y0 = _mask(np.where(np.isfinite(y1), y1, 0.1), "random30")
    th = _thetas(3, 3, (0.0, 0.5, -0.9, 0.999, 0.3))
    for ys, off in ((np.stack([y0, y1]), [0, 2, 5]), (np.stack([y1, y0, y1]), [0, 1, 3, 5])):
        pl = eng.penalized_likelihood(ys, u, v, th, LAM, cell_offsets=off)
        fit = eng.smooth_batch(ys, u, v, th, cell_offsets=off)
        assert np.all(np.isfinite(pl)) and np.all(np.isfinite(fit["lik"]))
        for s in range(len(off) - 1):
            c = slice(off[s], off[s + 1])
            assert np.array_equal(pl[c], eng.penalized_likelihood(ys[s], u, v, th[c], LAM)), s
            alone = eng.smooth_batch(ys[s], u, v, th[c])
            for k in alone:
                assert np.array_equal(fit[k][c], alone[k]), (s, k)


def test_the_learners_fit_of_a_singular_series_is_kalman_smoothers(eng):
    """fit = Kalman_smoother(theta_w), also where the scan kernel has no answer; next to a regular series too"""
    from ldsr_amd.bfgs import start_points
    y1, u, v = _series(65, 3, 3, "last")
    y0 = _mask(np.where(np.isfinite(y1), y1, 0.1), "random30")
    lb = np.concatenate([[0.0], np.full(3, -1.0), [0.0], np.full(3, -1.0), [0.5, 0.5, -1.0, 0.5]])
    ub = np.concatenate([[1.0], np.full(3, 1.0), [1.0], np.full(3, 1.0), [1.5, 1.5, 1.0, 1.5]])
    m = eng.LDS_BFGS_with_update(y1, u, v, lambda_=LAM, ub=ub, lb=lb, num_restarts=4, seed=3, maxit=5)
    fit = eng.Kalman_smoother(y1, u, v, m["theta"])
    assert np.isfinite(m["lik"]) and m["lik"] == fit["lik"]
    for k in ("X", "Y", "V", "J"):
        assert np.all(np.isfinite(m["fit"][k])) and np.array_equal(m["fit"][k], fit[k]), k
    par0 = start_points(lb, ub, 4, seed=3)
    ys = np.stack([y0, y1])
    for r in (eng.bfgs_update_batch(ys, u, v, par0, lb, ub, lam=LAM, cell_offsets=[0, 2, 4], maxit=5),
              eng.bfgs_batch(ys, u, v, par0, lb, ub, cell_offsets=[0, 2, 4], maxit=5, smooth=True)):
        for s in range(2):
            alone = eng.smooth_batch(ys[s], u, v, r["theta"][s:s + 1])
            assert np.isfinite(r["lik"][s]) and r["lik"][s] == alone["lik"][0], s
            for k in ("X", "Y", "V", "J"):
                assert np.array_equal(r[k][s], alone[k][0]), (s, k)
