"""The host model of LDS_BFGS_with_update's objective (tests/plgrad_model.py, R/LDS_GA.R:90-127): it has the
oracle's penalised likelihood, a hand-derived gradient equal to the complex-step derivative of its own
forward pass on every case of the table below, and its L-BFGS finds an optimum known in closed form.  The
model is the yardstick a device implementation of the objective is to be compared with; the project has no
device implementation yet.

The bar such a comparison uses on the gradient is |d_i| <= 1e-6 |ref_i| + 1e-9 max(1, max_j |ref_j|).  The model's own
rounding error -- its float64 gradient against the same recursions in numpy.longdouble -- must stay below a
tenth of that bar on every listed case, so that a failure of the comparison is the device's and not an
ill-conditioned input's."""
import numpy as np
import pytest

import bfgs_model as B
import plgrad_model as M
from conftest import parity_close
from test_gpu_bfgs import _VG_CASES, _mask, _thetas

# A = 0.999 is the near-unit value of test_gpu_bfgs.py; it passes the longdouble check below on every case,
# so no theta of the table had to be replaced.
A_ALL = (0.0, 0.5, -0.9, 0.999)
LONG_T = 1639                         # a series of many chunks of 64 steps
LAMBDAS = (1.0, 0.25, 3.0)


def grad_close(g, ref, scale=1.0):
    """The bar (scale = 1): the project's parity bar with its absolute floor scaled to the vector -- a sum
    taken in another order errs relative to its largest term, not to a component that cancels to nearly nothing."""
    g, ref = np.asarray(g, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool(np.all(np.abs(g - ref) <= scale * (1e-6 * np.abs(ref) + 1e-9 * max(1.0, np.max(np.abs(ref))))))


def vg_cases():
    """(tag, y, u, v, thetas [n, P], lam) of every value-and-gradient case: the shapes of
    test_gpu_bfgs._VG_CASES, the three absent-input combinations at T = 2, 65, 130, and one long series."""
    from ldsr_amd import synth
    out = []
    for i, (T, p, q, mask) in enumerate(_VG_CASES):
        y, u, v = synth.make_series(T, p, q, series_id=T + p)
        out.append(("T=%d p=%d q=%d %s" % (T, p, q, mask), _mask(y, mask), u, v, _thetas(p, q, A_ALL),
                    LAMBDAS[i % 3]))
    for T in (2, 65, 130):
        y, u, v = synth.make_series(T, 3, 2, series_id=9)
        y = _mask(y, "random30" if T > 2 else "none")
        for uu, vv in ((None, v), (u, None), (None, None)):
            p, q = (1 if uu is None else 3), (1 if vv is None else 2)
            out.append(("T=%d u=%s v=%s" % (T, uu is not None, vv is not None), y, uu, vv, _thetas(p, q, A_ALL[1:3]),
                        1.0))
    T = LONG_T
    y, u, v = synth.make_series(T, 3, 3, series_id=T + 3)
    out.append(("T=%d p=3 q=3 random30" % T, _mask(y, "random30"), u, v, _thetas(3, 3, A_ALL), 1.0))
    return out


def oracle_pl(O, th, y, u, v, lam):
    """lik - lam * ssq from the oracle's Kalman smoother (stdlik = 0), as penalized_likelihood forms it"""
    p = 1 if u is None else u.shape[0]
    fit = O.kalman_smoother(y, u, v, th, stdlik=False)
    X = fit["X"]
    bu = th[1:1 + p] @ u if u is not None else np.zeros(y.size)
    return fit["lik"] - lam * np.sum((X[1:] - th[0] * X[:-1] - bu[:-1]) ** 2)


_N_CASES = len(_VG_CASES) + 9 + 1


def test_case_table_is_what_the_count_says():
    assert len(vg_cases()) == _N_CASES


@pytest.mark.parametrize("k", range(_N_CASES))
def test_model_value_and_gradient(k):
    from oracle import oracle as O
    tag, y, u, v, thetas, lam = vg_cases()[k]
    h = 1e-30
    for th in thetas:
        f, g = M.pl_grad(th, y, u, v, lam)
        ref = oracle_pl(O, th, y, u, v, lam)
        assert np.isfinite(f) and parity_close(f, ref), (tag, f, ref)
        assert f == M.pl(th, y, u, v, lam)
        cs = np.empty_like(th)
        for j in range(th.size):
            z = th.astype(np.complex128)
            z[j] += 1j * h
            cs[j] = M.pl(z, y, u, v, lam).imag / h
        _, gl = M.pl_grad(th, y, u, v, lam, dtype=np.longdouble)
        bar = 1e-6 * np.abs(g) + 1e-9 * max(1.0, np.max(np.abs(g)))
        gap = np.max(np.abs(np.asarray(g - gl, dtype=np.float64)) / bar)
        print("%s A=%g lam=%g: pl %.12g (oracle %.12g), complex-step gap %.3g, longdouble gap %.3g of the bar" % (
            tag, th[0], lam, f, ref, np.max(np.abs(g - cs) / bar), gap))
        assert grad_close(g, cs, 0.1), (tag, g, cs)
        assert gap < 0.1, (tag, th[0], gap)
        p, q = (1 if u is None else u.shape[0]), (1 if v is None else v.shape[0])
        zero = ([1] if u is None else []) + ([2 + p] if v is None else [])
        assert np.all(g[zero] == 0.0) and np.all(cs[zero] == 0.0), tag


def test_model_missing_values():
    """+-Inf in y counts as missing; with nothing observed pl = -lam ssq and C, D, R cannot move it."""
    tag, y, u, v, thetas, lam = vg_cases()[11]          # T = 130, p = q = 16, none
    p, q = u.shape[0], v.shape[0]
    th = thetas[1]
    yi, yn = y.copy(), y.copy()
    yi[::3], yn[::3] = np.inf, np.nan
    yi[1::7], yn[1::7] = -np.inf, np.nan
    a, b = M.pl_grad(th, yi, u, v, lam), M.pl_grad(th, yn, u, v, lam)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    F = M.forward(th, np.full(y.size, np.nan), u, v, lam)
    f, g = M.pl_grad(th, np.full(y.size, np.nan), u, v, lam)
    assert F["lik"] == 0.0 and f == -lam * F["ssq"]
    assert np.all(g[1 + p:2 + p + q] == 0.0) and g[3 + p + q] == 0.0


# ---- the model's optimiser on an optimum known in closed form ------------------------------------------

def known_optimum_case(bounded):
    """C = 0 and A, B, Q, mu1, V1 pinned by lb == ub: the filter never updates, ssq is exactly 0 and
    f = -pl = 1/2 sum_obs (log 2 pi R + (y_t - D.v_t)^2 / R): the optimum is OLS for D over the observed steps
    and R* = RSS / n, f* = n/2 (log 2 pi R* + 1).  bounded: an upper bound on D_0 below its unconstrained
    optimum -- RSS is convex in D, so the optimum has D_0 on that bound and the rest from OLS with D_0 fixed.
    -> y, u, v, lb, ub, par0 [4, P], f*, index of D_0."""
    from ldsr_amd import synth
    T, p, q = 65, 2, 3
    y, u, v = synth.make_series(T, p, q, series_id=23)
    y = y.copy()
    y[synth.uniform(3, 2, T) < 0.2] = np.nan
    P = 6 + p + q
    iD, iR = 2 + p, 3 + p + q
    pin = np.zeros(P)
    pin[0], pin[1:1 + p] = 0.5, 0.3
    pin[2 + p + q], pin[4 + p + q], pin[5 + p + q] = 0.5, 0.1, 1.0      # Q, mu1, V1 (C stays 0)
    lb, ub = pin.copy(), pin.copy()
    lb[iD:iD + q], ub[iD:iD + q] = -3.0, 3.0
    lb[iR], ub[iR] = 1e-3, 10.0
    obs = np.isfinite(y)
    Z, n = v.T[obs], int(obs.sum())
    sol = np.linalg.lstsq(Z, y[obs], rcond=None)[0]
    if bounded:
        b = 0.5 * sol[0] if sol[0] > 0 else 2.0 * sol[0] - 0.5       # an upper bound below the optimum
        ub[iD] = b
        rest = np.linalg.lstsq(Z[:, 1:], y[obs] - b * Z[:, 0], rcond=None)[0]
        sol = np.concatenate([[b], rest])
    assert np.all(np.abs(sol) < 3.0) and lb[iD] < ub[iD]
    Rstar = float(np.sum((y[obs] - Z @ sol) ** 2)) / n
    assert lb[iR] < Rstar < ub[iR]
    fstar = 0.5 * n * (np.log(2 * np.pi * Rstar) + 1.0)
    par0 = lb + (ub - lb) * synth.uniform(21, 5, 4 * P).reshape(4, P)
    return y, u, v, lb, ub, par0, fstar, iD


@pytest.mark.parametrize("bounded", [False, True])
def test_model_optimiser_reaches_the_known_optimum(bounded):
    y, u, v, lb, ub, par0, fstar, iD = known_optimum_case(bounded)
    for x0 in par0:
        r = M.bfgs(y, u, v, x0, lb, ub, lam=1.0)
        gap = r["value"] - fstar
        print("bounded=%s: f* %.12g, gap %.3g after %d iterations, %d evaluations, status %d" % (
            bounded, fstar, gap, r["n_iter"], r["n_eval"], r["status"]))
        assert gap <= 1e-6 * max(1.0, abs(fstar))
        assert gap >= -1e-9 * max(1.0, abs(fstar))                 # (nothing beats the exact optimum)
        assert r["n_eval"] >= r["n_iter"] + 1
        assert np.all(r["par"] >= lb) and np.all(r["par"] <= ub)
        assert np.array_equal(r["par"][lb == ub], lb[lb == ub])
        if bounded:
            assert r["par"][iD] == ub[iD]


def test_model_optimiser_edge_cases():
    y, u, v, lb, ub, par0, fstar, iD = known_optimum_case(False)
    r = M.bfgs(y, u, v, par0[0], lb, lb)                            # a degenerate box
    assert (r["n_iter"], r["status"], r["n_eval"]) == (0, B.CONVERGED, 1) and np.array_equal(r["par"], lb)
    assert r["value"] == -M.pl(lb, y, u, v, 1.0)
    r = M.bfgs(y, u, v, par0[0], lb, ub, maxit=1)
    assert (r["n_iter"], r["status"]) == (1, B.MAXIT) and r["value"] < -M.pl(par0[0], y, u, v, 1.0)
    lo = lb.copy()
    lo[3 + 2 + 3] = -2.0                                            # R < 0: S_t < 0 with C = 0
    bad = par0[0].copy()
    bad[3 + 2 + 3] = -1.0
    r = M.bfgs(y, u, v, bad, lo, ub)
    assert r["status"] == B.NONFINITE and np.isnan(r["value"]) and np.array_equal(r["par"], bad)
