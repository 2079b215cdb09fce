"""The extended-precision yardstick of the smoother family (tests/smoother_model.py), checked without a GPU on
every case of the table of tests/test_gpu_smoother_family.py:

 * the float64 and the numpy.longdouble model equal the oracle's kalman_smoother, propagate and mstep at the
   project's bar, and reproduce the reference's known-answer numbers pinned in test_oracle_golden.py;
 * THE CAP CONDITION: the oracle's gap to the longdouble model, max |oracle - ld| / (1e-6 |ld| + 1e-9) over all
   outputs, is at most 1/1000 of the bar on every case.  That is what lets the GPU tests hold a device kernel
   to 1/10 of the bar against the model: a larger gap is the kernel's, not an ill-conditioned input's.  A case
   that misses the condition gets another input, never a wider condition;
 * the table runs every FIT kernel ldsr_smooth_plan can name, and the serial smoother for both of its reasons."""
import ctypes as C

import numpy as np
import pytest

import smoother_model as SM
import test_gpu_smoother_family as F
from conftest import parity_close

CAP = F.ORACLE_CAP


def _check(tag, orc, f64, ld, keys):
    for k in keys:
        assert np.asarray(f64[k]).dtype == np.float64 and np.asarray(ld[k]).dtype == np.longdouble, k
        assert parity_close(f64[k], orc[k]), (tag, "float64 model", k)
        assert parity_close(np.asarray(ld[k], dtype=np.float64), orc[k]), (tag, "longdouble model", k)
    g = F.worst_gap(orc, ld, keys)
    print("GAP %-52s oracle %.3e float64 model %.3e" % (tag, g, F.worst_gap(f64, ld, keys)))
    assert g <= CAP, (tag, g)


def _with_liks(r, y, th, u, lam_dtype):
    """the model's dict with lik0 (stdlik = False), lik (lik0 / n_obs) and pl"""
    r = dict(r)
    r["lik0"] = r["lik"]
    with np.errstate(invalid="ignore", divide="ignore"):
        r["lik"] = r["lik0"] / lam_dtype(np.count_nonzero(np.isfinite(y)))
    if "J" in r:
        r["pl"] = r["lik0"] - lam_dtype(F.LAM) * SM.ssq(th, r["X"], u)
    return r


@pytest.mark.parametrize("c", F.smoother_cases(), ids=lambda c: c["id"])
def test_smoother_model_against_oracle(c):
    y, u, v, th, orc, ld = F.smoother_refs(c)
    f64 = _with_liks(SM.smoother(th, y, u, v, stdlik=False), y, th, u, np.float64)
    _check(c["id"], orc, f64, ld, F.SMOOTH_KEYS)
    # the switch: stdlik = True is the same pass divided by the number of observations
    std = SM.smoother(th, y, u, v, stdlik=True)
    assert np.array_equal(std["lik"], f64["lik"], equal_nan=True) and np.array_equal(std["X"], f64["X"])
    if c["mask"] == "none":
        assert np.all(np.isnan(orc["lik"])) and np.all(orc["lik0"] == 0.0)


@pytest.mark.parametrize("T,p,q,shared", F.MULTI_CASES)
def test_smoother_model_against_oracle_several_series(T, p, q, shared):
    for s, i, ys, us, vs, th, orc, ld in F.multi_refs(T, p, q, shared):
        f64 = _with_liks(SM.smoother(th, ys, us, vs, stdlik=False), ys, th, us, np.float64)
        f64 = {k: f64[k][0] for k in F.SMOOTH_KEYS}
        _check("several-T%d-p%d-q%d-%s series %d cell %d" % (T, p, q, "shared" if shared else "own", s, i), orc, f64, ld,
               F.SMOOTH_KEYS)


@pytest.mark.parametrize("c", F.propagate_cases(), ids=lambda c: c["id"])
def test_propagate_model_against_oracle(c):
    y, u, v, th, orc, ld = F.propagate_refs(c)
    f64 = _with_liks(SM.propagate(th, u, v, y, stdlik=False), y, th, u, np.float64)
    _check(c["id"], orc, f64, ld, F.PROP_KEYS)
    assert np.array_equal(SM.propagate(th, u, v, y)["lik"], f64["lik"], equal_nan=True)


@pytest.mark.parametrize("c", F.mstep_cases(), ids=lambda c: c["id"])
def test_mstep_model_against_oracle(c):
    y, u, v, fit, orc, ld = F.mstep_refs(c)
    assert np.all(np.isfinite(orc))
    f64 = SM.mstep(y, u, v, fit)
    _check(c["id"], {"theta": orc}, {"theta": f64}, {"theta": ld}, ("theta",))
    p, q = (1 if u is None else c["p"]), (1 if v is None else c["q"])
    if u is None:
        assert np.all(f64[:, 1] == 0.0)                     # B stays at the zero it starts from
    if v is None:
        assert np.all(f64[:, 2 + p] == 0.0)


def test_mstep_model_two_series():
    for i, s, ys, us, vs, row, orc, ld in F.mstep_two_series_refs()[1]:
        _check("mstep two-series row %d" % i, {"theta": orc}, {"theta": SM.mstep(ys, us, vs, row)[0]}, {"theta": ld},
               ("theta",))


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_model_reproduces_the_reference_known_answers(p1case, npcase, refdata, dtype):
    """tests/testthat/test-LDS-EM.R:21-41 (two E/M rounds) at the reference's 1e-6, the 17-digit regression
    pins and NPlds$lik of test_oracle_golden.py, from the model instead of the oracle."""
    from oracle import oracle as O
    c = p1case
    y, u, v = c["y"], c["u"], c["v"]
    s1 = SM.smoother(c["theta0"], y, u, v, dtype=dtype)
    t1 = SM.mstep(y, u, v, {k: np.asarray(s1[k], dtype=np.float64) for k in "XVJ"}, dtype=dtype)
    s2 = SM.smoother(np.asarray(t1, dtype=np.float64), y, u, v, dtype=dtype)
    t2 = SM.mstep(y, u, v, {k: np.asarray(s2[k], dtype=np.float64) for k in "XVJ"}, dtype=dtype)
    th1 = O.unpack_theta(np.asarray(t1[0], dtype=np.float64), 7, 7)
    th2 = O.unpack_theta(np.asarray(t2[0], dtype=np.float64), 7, 7)
    tol = 1e-6
    assert float(s1["lik"][0]) == pytest.approx(-11.678657, rel=tol)
    assert float(s1["X"][0, 0]) == pytest.approx(1.293356, rel=tol)
    assert float(s1["X"][0, 84]) == pytest.approx(-0.987671, rel=tol)
    assert th1["A"] == pytest.approx(0.606066, rel=tol)
    assert th1["C"] == pytest.approx(-0.005995, abs=1e-6)
    assert th1["Q"] == pytest.approx(3.640236, rel=tol)
    assert float(s2["lik"][0]) == pytest.approx(-0.114224, abs=1e-6)
    assert th2["A"] == pytest.approx(0.603945, rel=tol)
    assert th2["C"] == pytest.approx(-0.012004, abs=1e-6)
    assert th2["Q"] == pytest.approx(3.644322, rel=tol)
    assert float(s1["lik"][0]) == pytest.approx(-11.678656588814256, rel=1e-12)
    assert float(s1["V"][0, 0]) == pytest.approx(0.76393202250021031, rel=1e-12)
    assert float(s1["J"][0, 0]) == pytest.approx(0.33333333333333337, rel=1e-12)
    assert th1["R"] == pytest.approx(0.074517883051681055, rel=1e-12)
    assert th1["mu1"] == pytest.approx(1.293355756908821, rel=1e-12)
    # propagate is the open-loop forward pass
    pr = SM.propagate(c["theta0"], u, v, y, dtype=dtype)
    x = np.empty(85)
    x[0] = 1.0
    for t in range(1, 85):
        x[t] = 0.5 * x[t - 1] + np.full(7, 0.5) @ u[:, t - 1]
    np.testing.assert_allclose(np.asarray(pr["X"][0], dtype=np.float64), x, rtol=1e-13)
    # one E-step at the bundled NPlds theta gives NPlds$lik
    n = npcase(1200)
    th = refdata["NPlds"]["theta"]
    theta = O.pack_theta(th["A"][0], th["B"], th["C"][0], th["D"], th["Q"][0], th["R"][0], th["mu1"][0], th["V1"][0])
    s = SM.smoother(theta, n["y"], n["u"], n["v"], dtype=dtype)
    assert float(s["lik"][0]) == pytest.approx(refdata["NPlds"]["lik"][0], rel=1e-9)


def test_model_em_loop_reproduces_the_reference_convergence(p1case):
    for dtype in (np.float64, np.longdouble):
        _em_loop_reproduces_the_reference_convergence(p1case, dtype)


def _em_loop_reproduces_the_reference_convergence(p1case, dtype):
    """LDS_EM (src/EM.cpp:245-280) as the model's em(): 68 iterations to lik = -0.039093, the reference's own
    known answer (tests/testthat/test-LDS-EM.R:36-41), in float64 and in longdouble; the trace, the margin of
    the stop decisions and the rows' independence."""
    c = p1case
    y, u, v, tol = c["y"], c["u"], c["v"], 1e-5
    r = SM.em(c["theta0"], y, u, v, niter=100, tol=tol, dtype=dtype)
    assert r["theta"].dtype == dtype and r["liks"].dtype == dtype and r["liks"].shape == (1, 100)
    assert r["n_iter"][0] == 68 and float(r["lik"][0]) == pytest.approx(-0.039093, abs=1e-6)
    assert float(r["theta"][0, 0]) == pytest.approx(0.59893129323481986, rel=1e-9)
    liks = r["liks"][0]
    assert np.all(np.isfinite(liks[:68])) and np.all(np.isnan(liks[68:])) and liks[67] == r["lik"][0]
    d = np.abs(np.diff(np.asarray(liks[:68], dtype=np.float64)))
    assert d[66] < tol and d[65] < tol and not (d[65] < tol and d[64] < tol)      # stopped exactly there
    assert 0 < r["margin"][0] <= min(abs(d[66] - tol), abs(d[65] - tol), abs(d[64] - tol)) * (1 + 1e-6)
    # a row stops on its own: a second row goes on to the cap and the first keeps what it had when it stopped
    # (to rounding: numpy sums B u in another order for two rows)
    th2 = np.stack([c["theta0"], c["theta0"]])
    th2[1, 0], th2[1, 8] = 0.9, 0.1
    r2 = SM.em(th2, y, u, v, niter=80, tol=tol, dtype=dtype)
    assert r2["n_iter"][0] == 68 and r2["n_iter"][1] != 68 and np.all(np.isnan(r2["liks"][0, 68:]))
    assert parity_close(np.asarray(r2["liks"][0, :68], dtype=np.float64), np.asarray(liks[:68], dtype=np.float64), 1e-10, 0)
    assert parity_close(np.asarray(r2["theta"][0], dtype=np.float64), np.asarray(r["theta"][0], dtype=np.float64), 1e-9, 1e-12)
    assert np.all(SM.em(c["theta0"], y, u, v, niter=2, tol=tol, dtype=dtype)["n_iter"] == 2)


def test_model_missing_values_and_solver():
    """+-Inf in y is missing (the same bits as NaN there); the Gauss-Jordan solve against numpy's."""
    c = F._case("x", 60, 2, 3, "scattered30")
    y, u, v, th = F.case_inputs(c)
    yi = y.copy()
    yi[np.nonzero(np.isnan(y))[0][::2]] = np.inf
    yi[np.nonzero(np.isnan(y))[0][1::4]] = -np.inf
    a, b = SM.smoother(th, y, u, v), SM.smoother(th, yi, u, v)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    rng = np.random.default_rng(5)
    M, rhs = rng.normal(size=(9, 9)), rng.normal(size=9)
    M[0, 0] = 0.0                                            # a pivot that has to move
    np.testing.assert_allclose(SM.solve(M, rhs), np.linalg.solve(M, rhs), rtol=1e-11)
    xl = SM.solve(M.astype(np.longdouble), rhs.astype(np.longdouble))
    assert xl.dtype == np.longdouble and np.max(np.abs(M.astype(np.longdouble) @ xl - rhs)) < 1e-16
    with pytest.raises(np.linalg.LinAlgError):
        SM.solve(np.zeros((2, 2)), np.ones(2))


def test_case_table_runs_every_fit_kernel():
    """ldsr_smooth_plan over T = 2 .. 8192 and p, q in {1, 2, 3, 4, 5, 8} names the FIT kernels a call can run;
    the table runs every one of them at least once, and the serial smoother once because p or q exceeds 8 and
    once because T exceeds 8192.  A member added to em_members.h without a case fails here."""
    from ldsr_amd import _lib
    L = _lib.lib()
    name = C.create_string_buffer(160)

    def plan(T, p, q):
        a = L.ldsr_smooth_plan(T, p, q, name, 160)
        assert a in (1, 2), (T, p, q, a)
        return name.value.decode() if a == 2 else None

    reachable, serial_shapes = set(), set()
    for p in (1, 2, 3, 4, 5, 8):
        for q in (1, 2, 3, 4, 5, 8):
            for T in range(2, 8193):
                k = plan(T, p, q)
                if k is None:
                    serial_shapes.add((T, p, q))
                else:
                    reachable.add(k)
    members = set()
    for k in reachable:
        assert k.startswith("em_scan_kernel<") and k.endswith(", true>"), k
        PP, QQ, Lc, W = (int(x) for x in k[len("em_scan_kernel<"):].split(", ")[:4])
        members.add((Lc, W))
    assert members == set(F.SCAN_MEMBERS), sorted(members ^ set(F.SCAN_MEMBERS))
    assert not serial_shapes, sorted(serial_shapes)[:5]      # p, q <= 8 and T <= 8192: always the scan kernel

    ran, serial_wide, serial_long = set(), 0, 0
    for c in F.smoother_cases():
        p, q = (c["p"] if c["u"] else 1), (c["q"] if c["v"] else 1)
        k = plan(c["T"], p, q)
        if k is not None:
            ran.add(k)
        elif c["T"] > 8192:
            serial_long += 1
        else:
            assert p > 8 or q > 8, c["id"]
            serial_wide += 1
    assert sorted(reachable - ran) == []
    assert serial_wide >= 1 and serial_long >= 1
    # the member rule is on the lengths it names: both ends of every member's range and a T in between
    for Lc, W in F.SCAN_MEMBERS:
        lo, mid, hi = F.member_lengths(Lc, W)
        for T in (lo, mid, hi):
            want = "em_scan_kernel<1, 2, %d, %d, false, %s, true>" % (Lc, W, "true" if W > 1 else "false")
            assert plan(T, 1, 2) == want, (Lc, W, T)
        assert lo == 2 or plan(lo - 1, 1, 2) != plan(lo, 1, 2)
        assert hi == 8192 or plan(hi + 1, 1, 2) != plan(hi, 1, 2)
        nl = -(-mid // Lc)
        assert mid % Lc and (mid - nl * (Lc - 1)) not in (1, nl)
