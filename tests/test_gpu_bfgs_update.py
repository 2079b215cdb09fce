"""LDS_BFGS_with_update on the GPU (run with -m gpu).  The objective is checked against the CPU oracle's
lik - lambda ssq, the project's older device entry for the same number (penalized_likelihood) and the host model
(tests/plgrad_model.py, itself pinned to the complex-step derivative in test_plgrad_host.py); the bars are the
project's own: parity_close on values, test_plgrad_host.grad_close at scale 1 on gradients.  The optimiser is
compared by properties and against an optimum known in closed form, with the model's own gap as the yardstick
(the rule of test_gpu_bfgs.py).  The tests run in file order: the first device call of the new kernels is the
smallest one, T = 2 with p = q = 1 and no gradient."""
import numpy as np
import pytest

import bfgs_model as B
import plgrad_model as M
from conftest import parity_close
from test_gpu_bfgs import _mask, _np_problem
from test_plgrad_host import grad_close, known_optimum_case, oracle_pl, vg_cases

pytestmark = pytest.mark.gpu

_CASES = vg_cases()


def _case(tag):
    (c,) = [c for c in _CASES if c[0] == tag]
    return c


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


def _tiny():
    tag, y, u, v, thetas, lam = _CASES[0]
    assert y.size == 2 and u.shape[0] == 1 and v.shape[0] == 1
    return y, u, v, thetas[1:2], lam


def test_first_call_value_only_at_T2(eng):
    y, u, v, th, lam = _tiny()
    f = eng.pl_grad(y, u, v, th, lam)
    ref = M.pl(th[0], y, u, v, lam)
    old = eng.penalized_likelihood(y, u, v, th, lam)
    print("pl %.17g model %.17g penalized_likelihood %.17g" % (f[0], ref, old[0]))
    assert f.shape == (1,) and np.isfinite(f[0])
    assert parity_close(f[0], ref) and parity_close(f[0], old[0])


def test_first_call_with_gradient_at_T2(eng):
    y, u, v, th, lam = _tiny()
    f, g = eng.pl_grad(y, u, v, th, lam, grad=True)
    mf, mg = M.pl_grad(th[0], y, u, v, lam)
    print("pl %.17g model %.17g\ngrad  %s\nmodel %s" % (f[0], mf, g[0], mg))
    assert parity_close(f[0], mf) and parity_close(f[0], eng.penalized_likelihood(y, u, v, th, lam)[0])
    assert g.shape == (1, 8) and grad_close(g[0], mg, scale=1)
    assert np.array_equal(f, eng.pl_grad(y, u, v, th, lam))


@pytest.mark.parametrize("k", range(len(_CASES)))
def test_value_and_gradient(eng, O, k):
    tag, y, u, v, thetas, lam = _CASES[k]
    f, g = eng.pl_grad(y, u, v, thetas, lam, grad=True)
    assert np.array_equal(f, eng.pl_grad(y, u, v, thetas, lam)), tag       # bit-equal with and without grad
    p, q = (1 if u is None else u.shape[0]), (1 if v is None else v.shape[0])
    zero = ([1] if u is None else []) + ([2 + p] if v is None else [])
    for i, th in enumerate(thetas):
        ref = oracle_pl(O, th, y, u, v, lam)
        mf, mg = M.pl_grad(th, y, u, v, lam)
        bar = 1e-6 * np.abs(mg) + 1e-9 * max(1.0, np.max(np.abs(mg)))
        print("%s A=%g lam=%g: pl %.12g (oracle %.12g), gradient gap %.3g of the bar" % (
            tag, th[0], lam, f[i], ref, np.max(np.abs(g[i] - mg) / bar)))
        assert np.isfinite(f[i]) and parity_close(f[i], ref), (tag, i, f[i], ref)
        assert grad_close(g[i], mg, scale=1), (tag, i, g[i], mg)
        assert np.all(g[i][zero] == 0.0), tag


@pytest.mark.parametrize("k", range(len(_CASES)))
def test_value_against_penalized_likelihood(eng, k):
    """The same cases against the device entry that has computed this number since the GA work.  Five of them are
    series whose Svv / Tuu is singular (a single observed y_t for three columns of v; T = 2 with three columns of
    u): there penalized_likelihood answers from the serial smoother (tests/test_gpu_singular_smoother.py)."""
    tag, y, u, v, thetas, lam = _CASES[k]
    f = eng.pl_grad(y, u, v, thetas, lam)
    old = eng.penalized_likelihood(y, u, v, thetas, lam)
    print("%s: pl_grad %s\n    penalized_likelihood %s" % (tag, f, old))
    assert np.all(np.isfinite(f)) and parity_close(f, old), (tag, f, old)


def test_missing_values(eng):
    tag, y, u, v, thetas, lam = _case("T=130 p=16 q=16 none")
    p, q = u.shape[0], v.shape[0]
    yi, yn = y.copy(), y.copy()
    yi[::3], yn[::3] = np.inf, np.nan
    yi[1::7], yn[1::7] = -np.inf, np.nan
    a, b = eng.pl_grad(yi, u, v, thetas, lam, grad=True), eng.pl_grad(yn, u, v, thetas, lam, grad=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    nothing = np.full(y.size, np.nan)
    f, g = eng.pl_grad(nothing, u, v, thetas, lam, grad=True)
    for i, th in enumerate(thetas):
        F = M.forward(th, nothing, u, v, lam)
        assert F["lik"] == 0.0 and parity_close(f[i], -lam * F["ssq"])
        assert grad_close(g[i], M.pl_grad(th, nothing, u, v, lam)[1], scale=1)
    assert np.all(g[:, 1 + p:2 + p + q] == 0.0) and np.all(g[:, 3 + p + q] == 0.0)      # C, D, R


@pytest.mark.parametrize("off", [[0, 3, 5], [0, 0, 5]])
def test_several_series_with_shared_inputs(eng, off):
    tag, y, u, v, thetas, lam = _case("T=65 p=3 q=3 paleo")
    base = np.where(np.isfinite(y), y, 0.1)
    ys = np.stack([_mask(base, "random30"), y])
    th = np.concatenate([thetas, thetas[:1]])
    f, g = eng.pl_grad(ys, u, v, th, lam, cell_offsets=off, grad=True)
    for s in range(2):
        if off[s] == off[s + 1]:
            continue
        fs, gs = eng.pl_grad(ys[s], u, v, th[off[s]:off[s + 1]], lam, grad=True)
        assert np.array_equal(f[off[s]:off[s + 1]], fs) and np.array_equal(g[off[s]:off[s + 1]], gs), s


# ---- the optimiser ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("bounded", [False, True])
def test_known_optimum(eng, bounded):
    """Device gap <= 10 x max(the model's gap from the same start, 1e-9 max(1, f*)): the factor allows for
    the other summation order; the model is the yardstick, not the device."""
    y, u, v, lb, ub, par0, fstar, iD = known_optimum_case(bounded)
    r = eng.bfgs_update_batch(y, u, v, par0, lb, ub, lam=1.0)["all"]
    for i, x0 in enumerate(par0):
        mgap = M.bfgs(y, u, v, x0, lb, ub, lam=1.0)["value"] - fstar
        gap = r["value"][i] - fstar
        print("bounded=%s start %d: device gap %.3g (%d it, status %d), model gap %.3g" % (
            bounded, i, gap, r["n_iter"][i], r["status"][i], mgap))
        assert gap <= 10.0 * max(mgap, 1e-9 * max(1.0, fstar))
        assert np.array_equal(r["par"][i][lb == ub], lb[lb == ub])
        if bounded:
            assert r["par"][i][iD] == ub[iD]


LAM = 1.0


@pytest.fixture(scope="module")
def np_run(eng, npcase):
    c, lb, ub, par0 = _np_problem(npcase)
    return c, lb, ub, par0, eng.bfgs_update_batch(c["y"], c["u"], c["v"], par0, lb, ub, lam=LAM)


def test_per_cell_properties(eng, np_run):
    c, lb, ub, par0, r = np_run
    a = r["all"]
    f0 = -eng.pl_grad(c["y"], c["u"], c["v"], par0, LAM)
    print("f0", f0, "\nvalue", a["value"], "\nn_iter", a["n_iter"], "n_eval", a["n_eval"], "status", a["status"])
    assert np.all(np.isfinite(f0)) and np.all(a["value"] <= f0)
    assert np.all(a["par"] >= lb) and np.all(a["par"] <= ub)
    assert parity_close(a["value"], -eng.pl_grad(c["y"], c["u"], c["v"], a["par"], LAM))
    assert np.all(a["n_eval"] >= a["n_iter"] + 1) and np.all(a["n_iter"] <= 100)
    assert set(a["status"]) <= {B.CONVERGED, B.MAXIT, B.LINESEARCH, B.NONFINITE}


def test_selection_and_reference_list_shape(eng, np_run):
    c, lb, ub, par0, r = np_run
    val = r["all"]["value"]
    assert r["winner"][0] == B.select(val, True) == int(np.argmax(val))
    assert r["value"][0] == val.max() and np.array_equal(r["theta"][0], r["all"]["par"][r["winner"][0]])
    rmin = eng.bfgs_update_batch(c["y"], c["u"], c["v"], par0, lb, ub, lam=LAM, select="min", return_all=False)
    assert rmin["winner"][0] == B.select(val, False) == int(np.argmin(val)) and rmin["value"][0] == val.min()
    # ties take the first index
    tie = eng.bfgs_update_batch(c["y"], c["u"], c["v"], par0[[3, 1, 3, 1]], lb, ub, lam=LAM)
    assert tie["winner"][0] == int(np.argmax(val[[3, 1]]))
    assert np.array_equal(tie["all"]["value"][:2], tie["all"]["value"][2:])
    for select, pick in (("min", np.argmin), ("reference", np.argmax)):
        m = eng.LDS_BFGS_with_update(c["y"], c["u"], c["v"], lambda_=LAM, ub=ub, lb=lb, num_restarts=8, seed=12,
                                     select=select)
        assert sorted(m) == ["all", "fit", "lik", "pl", "theta"]
        assert np.array_equal(m["all"]["par0"], par0) and m["all"]["selected"] == int(pick(val))
        assert m["pl"] == val[int(pick(val))]
        fit = eng.Kalman_smoother(c["y"], c["u"], c["v"], m["theta"])
        assert sorted(m["fit"]) == sorted(fit) == ["J", "V", "X", "Y", "lik"]
        for k in fit:
            assert np.array_equal(m["fit"][k], fit[k]), k
        assert m["lik"] == fit["lik"] and np.isfinite(m["lik"])
        assert eng.pack_theta(m["theta"], 3, 3).tolist() == r["all"]["par"][int(pick(val))].tolist()


def test_determinism_and_independence(eng, np_run):
    c, lb, ub, par0, r = np_run
    again = eng.bfgs_update_batch(c["y"], c["u"], c["v"], par0, lb, ub, lam=LAM)
    for k in ("winner", "theta", "value", "lik", "X", "Y", "V", "J"):
        assert np.array_equal(r[k], again[k]), k
    for k in r["all"]:
        assert np.array_equal(r["all"][k], again["all"][k]), k
    alone = eng.bfgs_update_batch(c["y"], c["u"], c["v"], par0[5:6], lb, ub, lam=LAM)["all"]
    y2 = np.stack([_mask(np.where(np.isfinite(c["y"]), c["y"], 0.0), "random30"), c["y"]])
    two = eng.bfgs_update_batch(y2, c["u"], c["v"], np.concatenate([par0[:3], par0[5:6], par0[:2]]), lb, ub, lam=LAM,
                                cell_offsets=[0, 3, 6])
    assert two["winner"][0] in (0, 1, 2) and two["winner"][1] in (3, 4, 5)
    for k in ("par", "value", "n_iter", "status", "n_eval"):
        assert np.array_equal(alone[k][0], r["all"][k][5]), k
        assert np.array_equal(two["all"][k][3], r["all"][k][5]), k


def test_edge_cases(eng, npcase):
    c, lb, ub, par0 = _np_problem(npcase)
    y, u, v = c["y"], c["u"], c["v"]
    r = eng.bfgs_update_batch(y, u, v, par0[:2], par0[0], par0[0], lam=LAM)["all"]          # a degenerate box
    assert np.all(r["n_iter"] == 0) and np.all(r["status"] == B.CONVERGED) and np.all(r["par"] == par0[0])
    assert np.array_equal(r["value"], -eng.pl_grad(y, u, v, par0[[0, 0]], LAM)) and np.all(r["n_eval"] == 1)
    full = eng.bfgs_update_batch(y, u, v, par0, lb, ub, lam=LAM)["all"]
    one = eng.bfgs_update_batch(y, u, v, par0, lb, ub, lam=LAM, maxit=1)["all"]
    conv1 = (full["n_iter"] == 1) & (full["status"] == B.CONVERGED)      # one step was enough
    assert np.all(one["n_iter"] == 1) and not np.all(conv1)
    assert np.array_equal(one["status"], np.where(conv1, B.CONVERGED, B.MAXIT))
    # R = -1 with C = 0: S_t = R < 0 at every step
    iC, iR = 1 + 3, 3 + 3 + 3
    lo = lb.copy()
    lo[iR] = -2.0
    bad = par0[:3].copy()
    bad[1, iC], bad[1, iR] = 0.0, -1.0
    rb = eng.bfgs_update_batch(y, u, v, bad, lo, ub, lam=LAM)
    assert rb["all"]["status"][1] == B.NONFINITE and np.isnan(rb["all"]["value"][1])
    assert np.array_equal(rb["all"]["par"][1], bad[1]) and rb["winner"][0] in (0, 2)
    assert np.all(np.isfinite(rb["all"]["value"][[0, 2]]))
    # a series whose restarts are all non-finite, next to one that is fine
    bad2 = bad[[1, 1, 0]].copy()
    bad2[1, iR] = -1.5
    y2 = np.stack([y, y])
    rs = eng.bfgs_update_batch(y2, u, v, bad2, lo, ub, lam=LAM, cell_offsets=[0, 2, 3])
    assert list(rs["winner"]) == [-1, 2] and np.isnan(rs["value"][0]) and np.isfinite(rs["value"][1])
    for k in ("theta", "X", "Y", "V", "J"):
        assert np.all(np.isnan(rs[k][0])) and np.all(np.isfinite(rs[k][1])), k
    assert np.isnan(rs["lik"][0]) and np.isfinite(rs["lik"][1])
    from ldsr_amd import _lib
    lo[iC], hi = 0.0, ub.copy()
    hi[iC], hi[iR], lo[iR] = 0.0, -1.0, -2.0
    with pytest.raises(_lib.LdsrError, match="finite"):
        eng.LDS_BFGS_with_update(y, u, v, lambda_=LAM, ub=hi, lb=lo, num_restarts=4, seed=1)
