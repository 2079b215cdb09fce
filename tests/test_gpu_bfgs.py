"""LDS_BFGS on the GPU (run with -m gpu).  The objective is checked against the CPU oracle's propagate and
the gradient against the host model's adjoint gradient (tests/bfgs_model.py, itself pinned to the
complex-step derivative in test_bfgs_host.py), bar |d| <= 1e-6 |ref| + 1e-9.  The optimiser is NOT
compared with the model iterate for iterate -- sums in scan order and in serial order differ in the last
bits and a quasi-Newton iteration amplifies that -- but by properties every run must have and against
optima known in closed form, with the model's own gap as the yardstick."""
import numpy as np
import pytest

import bfgs_model as M
from conftest import parity_close
from test_bfgs_host import convex_case

pytestmark = pytest.mark.gpu


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


def _mask(y, kind):
    from ldsr_amd import synth
    y = y.copy()
    T = y.size
    if kind == "paleo":                 # all but the last 40 steps (or all but the last, for tiny T)
        y[:max(T - 40, 0) if T > 40 else T - 1] = np.nan
    elif kind == "random30":
        y[synth.uniform(77, T, T) < 0.3] = np.nan
    elif kind == "first":
        y[1:] = np.nan
    elif kind == "last":
        y[:-1] = np.nan
    elif kind == "all":
        y[:] = np.nan
    else:
        assert kind == "none"
    return y


def _thetas(p, q, A_values):
    from ldsr_amd import synth
    th = synth.make_init_packed(p, q, len(A_values), seed=4 + p + 17 * q)
    th[:, 0] = A_values
    th[:, 4 + p + q] = np.linspace(-0.4, 0.6, len(A_values))
    return th


def _check(eng, O, y, u, v, th, tag):
    """device value vs oracle, device gradient vs model, values with and without the gradient"""
    f, g = eng.ssq_train(y, u, v, th, grad=True)
    f_only = eng.ssq_train(y, u, v, th)
    assert np.array_equal(f, f_only), tag
    for i, t in enumerate(th):
        with np.errstate(all="ignore"):
            ref = np.nansum((y - O.propagate(t, u, v, y)["Y"]) ** 2)
            mf, mg = M.ssq_grad(t, y, u, v)
        print("%s A=%g: f %.12g (oracle %.12g), max |dg| %.3g" % (tag, t[0], f[i], ref, np.max(np.abs(g[i] - mg))))
        assert parity_close(f[i], ref), (tag, i, f[i], ref)
        assert parity_close(g[i], mg), (tag, i, g[i], mg)
    return f, g


A_ALL = (0.0, 0.5, -0.9, 0.999)
# every chunk boundary of the lane-per-step mapping, each with another width and mask; then every width
# and every mask at a length with a partial last chunk
_VG_CASES = [(2, 1, 1, "none"), (3, 3, 3, "last"), (63, 7, 2, "random30"), (64, 16, 16, "paleo"),
             (65, 3, 3, "first"), (128, 1, 1, "random30"), (130, 7, 2, "paleo"), (813, 3, 3, "random30")]
_VG_CASES += [(130, p, q, "none") for (p, q) in ((1, 1), (3, 3), (16, 16))]
_VG_CASES += [(65, 3, 3, m) for m in ("none", "paleo", "random30", "last")] + [(130, 3, 3, "first")]


@pytest.mark.parametrize("T,p,q,mask", _VG_CASES)
def test_value_and_gradient(eng, O, T, p, q, mask):
    from ldsr_amd import synth
    y, u, v = synth.make_series(T, p, q, series_id=T + p)
    y = _mask(y, mask)
    _check(eng, O, y, u, v, _thetas(p, q, A_ALL), "T=%d p=%d q=%d %s" % (T, p, q, mask))


@pytest.mark.parametrize("T", [2, 65, 130])
def test_value_and_gradient_with_an_absent_input(eng, O, T):
    from ldsr_amd import synth
    y, u, v = synth.make_series(T, 3, 2, series_id=9)
    y = _mask(y, "random30" if T > 2 else "none")
    for uu, vv, zero in ((None, v, [1]), (u, None, [2 + 3]), (None, None, [1, 3])):
        p, q = (1 if uu is None else 3), (1 if vv is None else 2)
        _, g = _check(eng, O, y, uu, vv, _thetas(p, q, A_ALL[1:3]), "T=%d u=%s v=%s" % (T, uu is not None, vv is not None))
        zero = [1] * (uu is None) + [2 + p] * (vv is None) + [2 + p + q, 3 + p + q, 5 + p + q]
        assert np.all(g[:, zero] == 0.0)


def test_nothing_observed_and_infinite_observations(eng):
    from ldsr_amd import synth
    y, u, v = synth.make_series(130, 3, 3, series_id=2)
    th = _thetas(3, 3, A_ALL)
    f, g = eng.ssq_train(_mask(y, "all"), u, v, th, grad=True)
    assert np.all(f == 0.0) and np.all(g == 0.0)
    yi, yn = y.copy(), y.copy()
    yi[::3], yn[::3] = np.inf, np.nan
    yi[1::7], yn[1::7] = -np.inf, np.nan
    a, b = eng.ssq_train(yi, u, v, th, grad=True), eng.ssq_train(yn, u, v, th, grad=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_np_fixture_and_several_series_with_shared_inputs(eng, O, npcase):
    c = npcase(1200)                                     # T = 813
    _check(eng, O, c["y"], c["u"], c["v"], _thetas(3, 3, (0.3, 0.95)), "NP")
    masks = ("none", "paleo", "random30", "first")
    base = np.where(np.isfinite(c["y"]), c["y"], 0.1)
    ys = np.stack([_mask(base, m) for m in masks])
    th = np.concatenate([_thetas(3, 3, (0.5, -0.9)) for _ in masks])
    off = np.arange(len(masks) + 1) * 2
    f, g = eng.ssq_train(ys, c["u"], c["v"], th, cell_offsets=off, grad=True)
    for s in range(len(masks)):
        fs, gs = eng.ssq_train(ys[s], c["u"], c["v"], th[2 * s:2 * s + 2], grad=True)
        assert np.array_equal(f[2 * s:2 * s + 2], fs) and np.array_equal(g[2 * s:2 * s + 2], gs)
        for i in range(2):
            mf, mg = M.ssq_grad(th[2 * s + i], ys[s], c["u"], c["v"])
            assert parity_close(f[2 * s + i], mf) and parity_close(g[2 * s + i], mg), masks[s]


# ---- the optimiser ---------------------------------------------------------------------------------------

def _np_problem(npcase, n=8, seed=12):
    from ldsr_amd.bfgs import start_points
    c = npcase(1900)                                     # T = 113
    p = q = 3
    lb = np.concatenate([[0.0], np.full(p, -1.0), [0.0], np.full(q, -1.0), [0.5, 0.5, -1.0, 0.5]])
    ub = np.concatenate([[1.0], np.full(p, 1.0), [1.0], np.full(q, 1.0), [1.5, 1.5, 1.0, 1.5]])
    return c, lb, ub, start_points(lb, ub, n, seed=seed)


@pytest.fixture(scope="module")
def np_run(eng, npcase):
    c, lb, ub, par0 = _np_problem(npcase)
    return c, lb, ub, par0, eng.bfgs_batch(c["y"], c["u"], c["v"], par0, lb, ub)


def test_per_cell_properties(eng, np_run):
    c, lb, ub, par0, r = np_run
    a = r["all"]
    f0 = eng.ssq_train(c["y"], c["u"], c["v"], par0)
    print("f0", f0, "\nvalue", a["value"], "\nn_iter", a["n_iter"], "n_eval", a["n_eval"], "status", a["status"])
    assert np.all(a["value"] <= f0)
    assert np.all(a["par"] >= lb) and np.all(a["par"] <= ub)
    assert np.array_equal(a["par"][:, [8, 9, 11]], par0[:, [8, 9, 11]])        # Q, R, V1
    assert parity_close(a["value"], eng.ssq_train(c["y"], c["u"], c["v"], a["par"]))
    assert np.all(a["n_eval"] >= a["n_iter"] + 1) and np.all(a["n_iter"] <= 100)
    assert set(a["status"]) <= {M.CONVERGED, M.MAXIT, M.LINESEARCH, M.NONFINITE}
    # (for the record, not a check: where the model ends from the same starts)
    print("model", [M.bfgs(c["y"], c["u"], c["v"], x0, lb, ub)["value"] for x0 in par0])


def test_selection_and_reference_list_shape(eng, np_run, npcase):
    c, lb, ub, par0, r = np_run
    val = r["all"]["value"]
    assert r["winner"][0] == M.select(val, True) == int(np.argmax(val))
    assert r["value"][0] == val.max() and np.array_equal(r["theta"][0], r["all"]["par"][r["winner"][0]])
    rmin = eng.bfgs_batch(c["y"], c["u"], c["v"], par0, lb, ub, select="min", return_all=False)
    assert rmin["winner"][0] == M.select(val, False) == int(np.argmin(val)) and rmin["value"][0] == val.min()
    # ties take the first index
    tie = eng.bfgs_batch(c["y"], c["u"], c["v"], par0[[3, 1, 3, 1]], lb, ub)
    assert tie["winner"][0] == int(np.argmax(val[[3, 1]])) and np.array_equal(tie["all"]["value"][:2], tie["all"]["value"][2:])
    for smooth in (False, True):
        m = eng.LDS_BFGS(c["y"], c["u"], c["v"], ub=ub, lb=lb, num_restarts=8, seed=12, select="min", smooth=smooth)
        assert np.array_equal(m["all"]["par0"], par0) and m["all"]["selected"] == rmin["winner"][0]
        assert m["pl"] == val.min()
        fit = (eng.Kalman_smoother(c["y"], c["u"], c["v"], m["theta"]) if smooth
               else eng.propagate(m["theta"], c["u"], c["v"], c["y"]))
        assert sorted(m["fit"]) == sorted(fit)
        for k in fit:
            assert np.array_equal(m["fit"][k], fit[k]), (smooth, k)
        assert m["lik"] == fit["lik"] and np.isfinite(m["lik"])
        assert eng.pack_theta(m["theta"], 3, 3).tolist() == rmin["theta"][0].tolist()


@pytest.mark.parametrize("bounded", [False, True])
def test_known_optimum(eng, bounded):
    """Device gap <= 10 x max(the model's gap on the same starts, 1e-9 max(1, f*)): the factor allows for
    the other summation order; the model is the yardstick, not the device."""
    y, u, v, lb, ub, par0, fstar, iC = convex_case(bounded)
    r = eng.bfgs_batch(y, u, v, par0, lb, ub)["all"]
    for i, x0 in enumerate(par0):
        mgap = M.bfgs(y, u, v, x0, lb, ub)["value"] - fstar
        gap = r["value"][i] - fstar
        print("bounded=%s start %d: device gap %.3g (%d it, status %d), model gap %.3g" % (
            bounded, i, gap, r["n_iter"][i], r["status"][i], mgap))
        assert gap <= 10.0 * max(mgap, 1e-9 * max(1.0, fstar))
        assert np.array_equal(r["par"][i][lb == ub], lb[lb == ub])
        if bounded:
            assert r["par"][i][iC] == ub[iC]


def test_determinism_and_independence(eng, np_run, npcase):
    c, lb, ub, par0, r = np_run
    again = eng.bfgs_batch(c["y"], c["u"], c["v"], par0, lb, ub)
    for k in ("winner", "theta", "value", "lik", "X", "Y", "V"):
        assert np.array_equal(r[k], again[k]), k
    for k in r["all"]:
        assert np.array_equal(r["all"][k], again["all"][k]), k
    alone = eng.bfgs_batch(c["y"], c["u"], c["v"], par0[5:6], lb, ub)["all"]
    y2 = np.stack([_mask(np.where(np.isfinite(c["y"]), c["y"], 0.0), "random30"), c["y"]])
    two = eng.bfgs_batch(y2, c["u"], c["v"], np.concatenate([par0[:3], par0[5:6], par0[:2]]), lb, ub,
                         cell_offsets=[0, 3, 6])
    assert two["winner"][0] in (0, 1, 2) and two["winner"][1] in (3, 4, 5)
    for k in ("par", "value", "n_iter", "status", "n_eval"):
        assert np.array_equal(alone[k][0], r["all"][k][5]), k
        assert np.array_equal(two["all"][k][3], r["all"][k][5]), k


def test_edge_cases(eng, npcase):
    c, lb, ub, par0 = _np_problem(npcase)
    y, u, v = c["y"], c["u"], c["v"]
    r = eng.bfgs_batch(y, u, v, par0[:2], par0[0], par0[0])["all"]                # a degenerate box
    assert np.all(r["n_iter"] == 0) and np.all(r["status"] == M.CONVERGED) and np.all(r["par"] == par0[0])
    assert np.array_equal(r["value"], eng.ssq_train(y, u, v, par0[[0, 0]])) and np.all(r["n_eval"] == 1)
    full = eng.bfgs_batch(y, u, v, par0, lb, ub)["all"]
    one = eng.bfgs_batch(y, u, v, par0, lb, ub, maxit=1)["all"]
    conv1 = (full["n_iter"] == 1) & (full["status"] == M.CONVERGED)      # one step was enough
    assert np.all(one["n_iter"] == 1) and not np.all(conv1)
    assert np.array_equal(one["status"], np.where(conv1, M.CONVERGED, M.MAXIT))
    # the objective overflows at |A| = 50 over 813 steps
    c8 = npcase(1200)
    lo, hi = lb.copy(), ub.copy()
    lo[0], hi[0] = -60.0, 60.0
    bad = par0[:3].copy()
    bad[1, 0] = 50.0
    rb = eng.bfgs_batch(c8["y"], c8["u"], c8["v"], bad, lo, hi)
    assert rb["all"]["status"][1] == M.NONFINITE and np.isnan(rb["all"]["value"][1])
    assert np.array_equal(rb["all"]["par"][1], bad[1]) and rb["winner"][0] in (0, 2)
    assert np.all(np.isfinite(rb["all"]["value"][[0, 2]]))
    # a series whose restarts are all non-finite, next to one that is fine
    bad2 = bad[[1, 1, 0]].copy()
    bad2[1, 0] = -50.0
    y2 = np.stack([c8["y"], c8["y"]])
    rs = eng.bfgs_batch(y2, c8["u"], c8["v"], bad2, lo, hi, cell_offsets=[0, 2, 3])
    assert list(rs["winner"]) == [-1, 2] and np.isnan(rs["value"][0]) and np.isfinite(rs["value"][1])
    for k in ("theta", "X", "Y", "V"):
        assert np.all(np.isnan(rs[k][0])) and np.all(np.isfinite(rs[k][1])), k
    assert np.isnan(rs["lik"][0]) and np.isfinite(rs["lik"][1])
    from ldsr_amd import _lib
    lo[0], hi[0] = 49.0, 50.0
    with pytest.raises(_lib.LdsrError, match="finite"):
        eng.LDS_BFGS(c8["y"], c8["u"], c8["v"], ub=hi, lb=lo, num_restarts=4, seed=1)
