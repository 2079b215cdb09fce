"""LDS_BFGS without a GPU: the entries exist on every layer, their argument errors surface before any
device call, nothing computes on the host -- and the host model of the specification (tests/bfgs_model.py,
the yardstick of the GPU tests) has the objective of the oracle's propagate, an exact gradient, and finds
optima that are known in closed form."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bfgs_model as M
from conftest import parity_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bfgs_entries_are_declared_exported_and_bound():
    import ldsr_amd
    from ldsr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ldsr_hip.h")).read()
    so = C.CDLL(_lib.SO_PATH)
    for name in ("ldsr_ssq_grad_batch", "ldsr_bfgs_batch"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(so, name), name
    assert callable(ldsr_amd.LDS_BFGS) and callable(ldsr_amd.bfgs_batch) and callable(ldsr_amd.ssq_train)
    for name, want in (("CONVERGED", M.CONVERGED), ("MAXIT", M.MAXIT), ("LINESEARCH", M.LINESEARCH),
                       ("NONFINITE", M.NONFINITE)):
        m = re.search(r"#define\s+LDSR_BFGS_%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == want == getattr(ldsr_amd.bfgs, name), name


def _call(L, **kw):
    """ldsr_bfgs_batch on a tiny valid problem (T = 4, p = q = 1, 2 restarts) with single arguments replaced."""
    P = 8
    a = dict(device=0, n_series=1, T=4, p=1, q=1, y=(C.c_double * 4)(0.1, -0.2, 0.3, 0.0), u=None, v=None,
             shared_uv=0, off=(C.c_int * 2)(0, 2), par0=(C.c_double * (2 * P))(*([0.5] * (2 * P))),
             lb=(C.c_double * P)(*([0.1] * P)), ub=(C.c_double * P)(*([0.9] * P)), maxit=10, lmm=5, factr=1e7,
             pgtol=0.0, select_max=1, fit_mode=0, winner=(C.c_int * 1)(), theta_w=(C.c_double * P)(),
             value_w=(C.c_double * 1)())
    a.update(kw)
    return L.ldsr_bfgs_batch(a["device"], a["n_series"], a["T"], a["p"], a["q"], a["y"], a["u"], a["v"],
                             a["shared_uv"], a["off"], a["par0"], a["lb"], a["ub"], a["maxit"], a["lmm"],
                             a["factr"], a["pgtol"], a["select_max"], a["fit_mode"], None, None, None, None, None,
                             a["winner"], a["theta_w"], a["value_w"], None, None, None, None, None)


def test_bfgs_argument_errors_without_gpu():
    from ldsr_amd import _lib
    L = _lib.lib()
    P = 8
    EINVAL, EUNSUPPORTED = 1, 2

    def bounds(i, x):
        b = [0.5] * P
        b[i] = x
        return (C.c_double * P)(*b)

    cases = [
        (dict(lb=bounds(3, 0.95)), EINVAL, b"lb must be <= ub"),
        (dict(lb=bounds(0, float("-inf"))), EINVAL, b"finite"),
        (dict(ub=bounds(7, float("nan"))), EINVAL, b"finite"),
        (dict(lb=bounds(1, -1e308), ub=bounds(1, 1e308)), EINVAL, b"finite"),
        (dict(lb=None), EINVAL, b"lb and ub"),
        (dict(maxit=0), EINVAL, b"maxit"),
        (dict(lmm=0), EINVAL, b"lmm"),
        (dict(lmm=9), EINVAL, b"lmm"),
        (dict(factr=-1.0), EINVAL, b"factr"),
        (dict(factr=float("nan")), EINVAL, b"factr"),
        (dict(pgtol=-1e-3), EINVAL, b"pgtol"),
        (dict(fit_mode=2), EINVAL, b"fit_mode"),
        (dict(off=(C.c_int * 2)(1, 2)), EINVAL, b"cell_offsets[0]"),
        (dict(n_series=2, off=(C.c_int * 3)(0, 2, 1)), EINVAL, b"non-decreasing"),
        (dict(off=None), EINVAL, b"cell_offsets"),
        (dict(n_series=0), EINVAL, b"n_series"),
        (dict(T=1), EINVAL, b"T must be"),
        (dict(p=0), EINVAL, b"p and q"),
        (dict(p=17), EUNSUPPORTED, b"not supported"),
        (dict(q=17), EUNSUPPORTED, b"not supported"),
        (dict(y=None), EINVAL, b"y"),
        (dict(par0=None), EINVAL, b"par0"),
        (dict(winner=None), EINVAL, b"winner"),
    ]
    for kw, code, msg in cases:
        rc = _call(L, **kw)
        assert rc == code, (kw.keys(), rc)
        assert msg in L.ldsr_last_error(), (kw.keys(), L.ldsr_last_error())
    # ... and of the objective's entry
    y, th, f = (C.c_double * 4)(0.1, -0.2, 0.3, 0.0), (C.c_double * P)(*([0.5] * P)), (C.c_double * 1)()
    off = (C.c_int * 2)(0, 1)
    for kw, code in ((dict(T=1), EINVAL), (dict(p=17), EUNSUPPORTED), (dict(q=17), EUNSUPPORTED),
                     (dict(theta=None), EINVAL), (dict(ssq=None), EINVAL), (dict(off=(C.c_int * 2)(1, 1)), EINVAL)):
        a = dict(T=4, p=1, q=1, theta=th, ssq=f, off=off)
        a.update(kw)
        assert L.ldsr_ssq_grad_batch(0, 1, a["T"], a["p"], a["q"], y, None, None, 0, a["off"], a["theta"],
                                     a["ssq"], None) == code, kw.keys()


def test_bfgs_has_no_host_implementation():
    """A valid call without a GPU fails loudly (the rule of test_no_cpu_fallback)."""
    import ldsr_amd
    from ldsr_amd import _lib, synth
    src = open(os.path.join(ROOT, "ldsr_amd", "bfgs.py")).read()
    assert "bfgs_model" not in src and "oracle" not in src
    with pytest.raises(ValueError):
        ldsr_amd.LDS_BFGS(*synth.make_series(50, 1, 2))      # the reference stops without bounds too
    if _lib.lib().ldsr_device_count() > 0:
        return                                               # (with a GPU the calls below succeed)
    y, u, v = synth.make_series(50, 1, 2)
    lb, ub = np.full(9, 0.05), np.full(9, 0.95)
    with pytest.raises(_lib.LdsrError):
        ldsr_amd.ssq_train(y, u, v, np.full(9, 0.5))
    with pytest.raises(_lib.LdsrError):
        ldsr_amd.bfgs_batch(y, u, v, np.full((3, 9), 0.5), lb, ub)
    with pytest.raises(_lib.LdsrError):
        ldsr_amd.LDS_BFGS(y, u, v, ub=ub, lb=lb, num_restarts=3, seed=1)


# ---- the model's objective and gradient -----------------------------------------------------------

def _cases(npcase):
    """(name, y, u, v): masked and unmasked, u absent, v absent, and the NP fixture."""
    from ldsr_amd import synth
    out = []
    y, u, v = synth.make_series(130, 3, 2, series_id=5)
    out.append(("dense", y, u, v))
    ym = y.copy()
    ym[synth.uniform(9, 1, y.size) < 0.3] = np.nan
    out.append(("random30", ym, u, v))
    yp, up, vp = synth.make_series(130, 3, 2, series_id=5, mask="paleo")
    out.append(("paleo", yp, up, vp))
    out.append(("no_u", ym, None, v))
    out.append(("no_v", ym, u, None))
    out.append(("no_uv", y, None, None))
    c = npcase(1900)
    out.append(("np1900", c["y"], c["u"], c["v"]))
    return out


def _thetas(p, q, n=3, seed=4):
    from ldsr_amd import synth
    th = synth.make_init_packed(p, q, n, seed=seed)
    th[:, 4 + p + q] = np.linspace(-0.4, 0.6, n)      # mu1 != 0: its gradient is exercised
    return th


def test_model_objective_is_the_oracles_propagate(npcase):
    from oracle import oracle as O
    for name, y, u, v in _cases(npcase):
        p, q = (1 if u is None else u.shape[0]), (1 if v is None else v.shape[0])
        for th in _thetas(p, q):
            ref = np.nansum((y - O.propagate(th, u, v, y)["Y"]) ** 2)
            assert parity_close(M.ssq(th, y, u, v), ref), name
            assert parity_close(M.ssq_grad(th, y, u, v)[0], ref), name


def test_model_gradient_is_the_complex_step_derivative(npcase):
    """f is a polynomial in theta, so Im f(theta + i h e_j) / h with h = 1e-30 is its derivative to
    rounding: no finite-difference tolerance."""
    h = 1e-30
    for name, y, u, v in _cases(npcase):
        p, q = (1 if u is None else u.shape[0]), (1 if v is None else v.shape[0])
        for th in _thetas(p, q):
            f, g = M.ssq_grad(th, y, u, v)
            ref = np.empty_like(th)
            for j in range(th.size):
                z = th.astype(np.complex128)
                z[j] += 1j * h
                ref[j] = M.ssq(z, y, u, v).imag / h
            assert parity_close(g, ref), (name, g, ref)
            # what cannot move the objective has gradient exactly 0
            zero = [2 + p + q, 3 + p + q, 5 + p + q] + ([1] if u is None else []) + ([2 + p] if v is None else [])
            assert np.all(g[zero] == 0.0) and np.all(ref[zero] == 0.0), name
    # +-Inf in y counts as missing, and nothing observed means nothing to fit
    y, u, v = _cases(npcase)[0][1:]
    yi, yn = y.copy(), y.copy()
    yi[::3], yn[::3] = np.inf, np.nan
    yi[1::7], yn[1::7] = -np.inf, np.nan
    th = _thetas(3, 2)[0]
    a, b = M.ssq_grad(th, yi, u, v), M.ssq_grad(th, yn, u, v)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    f, g = M.ssq_grad(th, np.full(y.size, np.nan), u, v)
    assert f == 0.0 and np.all(g == 0.0)


def test_r_seed_start_points_are_the_r_uniform_stream_in_the_box():
    from ldsr_amd.bfgs import start_points
    from ldsr_amd.rrng import RUniform
    lb = np.array([0.0, -1.0, 0.3, 0.0, 1.0, 1.0, -2.0, 1.0])
    ub = np.array([1.0, 1.0, 0.3, 2.0, 1.0, 1.0, 2.0, 1.0])      # four coordinates with lb == ub
    n = 5
    got = start_points(lb, ub, n, r_seed=42)
    g = RUniform(42)
    want = np.empty((n, lb.size))
    for r in range(n):
        for c in range(lb.size):       # runif(P, lb, ub): element by element, no draw where a == b
            want[r, c] = lb[c] if lb[c] == ub[c] else lb[c] + (ub[c] - lb[c]) * g.unif_rand(1)[0]
    assert np.array_equal(got, want)
    assert np.all(got >= lb) and np.all(got <= ub) and np.all(got[:, lb == ub] == lb[lb == ub])
    # set.seed(1); runif(2): the widely published first draws
    assert np.allclose(start_points([0.0, 0.0], [1.0, 1.0], 1, r_seed=1)[0], [0.2655087, 0.3721239], atol=5e-8)
    # counter mode: a restart's start point does not depend on how many others share the call
    a, b = start_points(lb, ub, 3, seed=7), start_points(lb, ub, 9, seed=7)
    assert np.array_equal(a, b[:3]) and np.array_equal(start_points(lb, ub, 4, seed=7, first=5), b[5:])
    assert np.all(b >= lb) and np.all(b <= ub) and len({tuple(r) for r in b}) == 9


# ---- the model's optimiser on optima known in closed form --------------------------------------------

def convex_case(bounded):
    """A, B and mu1 pinned by lb == ub: the objective is linear least squares in (C, D), whose optimum
    numpy.linalg.lstsq gives exactly.  bounded: an upper bound on C below its unconstrained optimum --
    the objective is convex, so the bounded optimum has C at that bound and D from lstsq with C fixed.
    -> y, u, v, lb, ub, par0 [4, P], f*, C index."""
    from ldsr_amd import synth
    T, p, q = 80, 2, 3
    y, u, v = synth.make_series(T, p, q, series_id=11)
    y = y.copy()
    y[synth.uniform(3, 2, T) < 0.2] = np.nan
    P = 6 + p + q
    iC = 1 + p
    pin = np.array([0.8, 0.3, 0.3] + [0.0] * (P - 3))      # (A, B: what the series was made with)
    pin[4 + p + q] = 0.1
    lb, ub = pin.copy(), pin.copy()
    lb[iC], ub[iC] = -2.0, 2.0
    lb[2 + p:2 + p + q], ub[2 + p:2 + p + q] = -2.0, 2.0
    lb[[2 + p + q, 3 + p + q, 5 + p + q]] = 0.5      # Q, R, V1: free in the box, absent from the objective
    ub[[2 + p + q, 3 + p + q, 5 + p + q]] = 1.5
    x, _ = M.forward(pin, y, u, v)
    obs = np.isfinite(y)
    Z = np.column_stack([x, v.T])[obs]
    sol = np.linalg.lstsq(Z, y[obs], rcond=None)[0]
    assert 0.2 < sol[0] < 2.0                        # (the unconstrained C is inside the box)
    if bounded:
        ub[iC] = 0.5 * sol[0]
        d = np.linalg.lstsq(Z[:, 1:], y[obs] - ub[iC] * Z[:, 0], rcond=None)[0]
        sol = np.concatenate([[ub[iC]], d])
        lb[iC] = -2.0
    assert np.all(np.abs(sol[1:]) < 2.0)
    fstar = float(np.sum((y[obs] - Z @ sol) ** 2))
    par0 = lb + (ub - lb) * synth.uniform(21, 5, 4 * P).reshape(4, P)
    return y, u, v, lb, ub, par0, fstar, iC


@pytest.mark.parametrize("bounded", [False, True])
def test_model_optimiser_reaches_the_known_optimum(bounded):
    y, u, v, lb, ub, par0, fstar, iC = convex_case(bounded)
    for x0 in par0:
        r = M.bfgs(y, u, v, x0, lb, ub)
        gap = r["value"] - fstar
        print("bounded=%s: f* %.12g, gap %.3g after %d iterations, %d evaluations, status %d" % (
            bounded, fstar, gap, r["n_iter"], r["n_eval"], r["status"]))
        assert gap <= 1e-6 * max(1.0, fstar)
        assert gap >= -1e-9 * max(1.0, fstar)                      # (nothing beats the exact optimum)
        assert r["status"] == M.CONVERGED and r["n_eval"] >= r["n_iter"] + 1
        assert np.all(r["par"] >= lb) and np.all(r["par"] <= ub)
        assert np.array_equal(r["par"][lb == ub], lb[lb == ub])
        assert np.array_equal(r["par"][-4:-2], np.clip(x0, lb, ub)[-4:-2])     # Q, R never move
        if bounded:
            assert r["par"][iC] == ub[iC]


def test_model_optimiser_edge_cases():
    y, u, v, lb, ub, par0, fstar, iC = convex_case(False)
    r = M.bfgs(y, u, v, par0[0], lb, lb)                            # a degenerate box
    assert (r["n_iter"], r["status"]) == (0, M.CONVERGED) and np.array_equal(r["par"], lb)
    assert r["value"] == M.ssq(lb, y, u, v)
    r = M.bfgs(y, u, v, par0[0], lb, ub, maxit=1)
    assert (r["n_iter"], r["status"]) == (1, M.MAXIT) and r["value"] < M.ssq(par0[0], y, u, v)
    big = par0[0].copy()
    lo, hi = lb.copy(), ub.copy()
    lo[0], hi[0], big[0] = -60.0, 60.0, 50.0
    yl = np.tile(y, 11)[:813]
    r = M.bfgs(yl, np.tile(u, 11)[:, :813], np.tile(v, 11)[:, :813], big, lo, hi)
    assert r["status"] == M.NONFINITE and np.isnan(r["value"]) and np.array_equal(r["par"], big)
    assert M.select([3.0, np.nan, 5.0, 5.0, 1.0, 1.0], True) == 2 and M.select([3.0, np.nan, 5.0, 1.0, 1.0], False) == 3
    assert M.select([np.nan, np.nan], True) == -1 and M.select([], False) == -1
