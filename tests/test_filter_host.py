"""The Kalman filter entries without a GPU: the host model of INTEGRATION.md section 12 (tests/filter_model.py)
against the smoother's model, the autocorrelation specification on hand-made series, the chi-square tail against
closed forms, and the argument checks of ldsr_filter_batch / ldsr_filter_batch_device."""
import ctypes as C
import math

import numpy as np
import pytest

import filter_cases as FC
import filter_model as FM
import smoother_model as SM

LD = np.longdouble
EINVAL, EUNSUPPORTED, EHIP = 1, 2, 3


def _assert_close(a, ref, frac, what):
    ok, worst = FC.close(a, ref, frac)
    assert ok, "%s: %.3g of the allowance (%g of the bar)" % (what, worst, frac)


# ---- the model against the smoother's model, in longdouble: a thousandth of the bar ---------------------------
@pytest.mark.parametrize("name", FC.NAMES)
def test_model_agrees_with_the_smoother_model(name):
    c = FC.case(name)
    T = c["T"]
    for s in range(c["S"]):
        a, b = c["off"][s], c["off"][s + 1]
        if b == a:
            continue
        y, u, v = c["series"](s)
        th = c["theta"][a:b]
        for stdlik in (True, False):
            f = FC.reference(name, stdlik)
            sm = SM.smoother(th, y, u, v, stdlik=stdlik, dtype=LD)
            _assert_close(f["lik"][a:b], sm["lik"], 1e-3, "%s series %d lik (stdlik=%s)" % (name, s, stdlik))
        # the smoother's terminal condition (src/EM.cpp:94-95)
        _assert_close(f["Xu"][a:b, T - 1], sm["X"][:, T - 1], 1e-3, "%s series %d Xu[T-1]" % (name, s))
        _assert_close(f["Vu"][a:b, T - 1], sm["V"][:, T - 1], 1e-3, "%s series %d Vu[T-1]" % (name, s))
        # with nothing observed the prediction is propagate's open-loop state
        blind = FM.kalman_filter(th, np.full(T, np.nan), u, v, dtype=LD)
        pr = SM.propagate(th, u, v, y, dtype=LD)
        _assert_close(blind["Xp"], pr["X"], 1e-3, "%s series %d Xp against propagate" % (name, s))
        _assert_close(blind["Vp"], pr["V"], 1e-3, "%s series %d Vp against propagate" % (name, s))
        assert np.all(np.isnan(blind["e"])) and np.all(blind["ll"] == 0)


@pytest.mark.parametrize("name", FC.NAMES)
def test_float64_model_is_within_a_thousandth_of_the_bar(name):
    """so a device result a tenth of the bar from the longdouble model is that close to the float64 one too"""
    c = FC.case(name)
    ref = FC.reference(name)
    f64 = FC.run_model(c, dtype=np.float64)
    for k in FM.ROWS + ("lik", "zmean", "zvar", "acf"):
        _assert_close(f64[k], ref[k], 1e-3, "%s %s" % (name, k))


def test_definitions_on_a_two_step_series_by_hand():
    # A = 0.5, B = 2, C = 3, D = -1, Q = 0.25, R = 1, mu1 = 1, V1 = 2; y = (7, NaN), u = (1, .), v = (1, 4)
    th = np.array([[0.5, 2.0, 3.0, -1.0, 0.25, 1.0, 1.0, 2.0]])
    r = FM.kalman_filter(th, [7.0, np.nan], np.array([[1.0, 9.0]]), np.array([[1.0, 4.0]]), stdlik=False, n_lags=1)
    S0, e0 = 3 * 2 * 3 + 1.0, 7.0 - (3 * 1.0 - 1.0)
    K0 = 2 * 3 / S0
    Xu0, Vu0 = 1.0 + K0 * e0, (1 - K0 * 3) * 2
    np.testing.assert_allclose(r["Xp"][0], [1.0, 0.5 * Xu0 + 2.0], rtol=1e-15)
    np.testing.assert_allclose(r["Vp"][0], [2.0, 0.25 * Vu0 + 0.25], rtol=1e-15)
    np.testing.assert_allclose(r["Yp"][0], [2.0, 3 * (0.5 * Xu0 + 2.0) - 4.0], rtol=1e-15)
    np.testing.assert_allclose(r["S"][0], [S0, 9 * (0.25 * Vu0 + 0.25) + 1.0], rtol=1e-15)
    np.testing.assert_allclose(r["Xu"][0], [Xu0, 0.5 * Xu0 + 2.0], rtol=1e-15)
    np.testing.assert_allclose(r["Vu"][0], [Vu0, 0.25 * Vu0 + 0.25], rtol=1e-15)
    assert r["e"][0, 0] == e0 and np.isnan(r["e"][0, 1]) and r["ll"][0, 1] == 0
    ll0 = -0.5 * (math.log(2 * math.pi) + math.log(S0) + e0 * e0 / S0)
    assert r["ll"][0, 0] == pytest.approx(ll0, rel=1e-15) and r["lik"][0] == pytest.approx(ll0, rel=1e-15)
    assert r["zmean"][0] == pytest.approx(e0 / math.sqrt(S0), rel=1e-15) and r["zvar"][0] == 0
    assert np.isnan(r["acf"][0, 0])           # one observation: no pair, and a zero denominator


# ---- the autocorrelations of a series with holes, by hand ---------------------------------------------------------
def test_acf_specification_by_hand():
    nan = np.nan
    # 6 steps, dense: z = 1, 2, 3, 4, 5, 6 -> mean 3.5, deviations -2.5 .. 2.5, denominator 17.5
    z = np.array([[1.0, 2, 3, 4, 5, 6]])
    zm, zv, acf = FM.acf_holes(z, np.ones(6, bool), 3)
    assert zm[0] == 3.5 and zv[0] == 17.5 / 6
    np.testing.assert_allclose(acf[0], [(3.75 + 0.75 - 0.25 + 0.75 + 3.75) / 17.5, (1.25 - 0.75 - 0.75 + 1.25) / 17.5,
                                        (-1.25 - 2.25 - 1.25) / 17.5], rtol=1e-15)
    # 7 steps with holes at 2 and 5: observed z = 2, 4, ., 6, 0, ., 3 -> mean 3, deviations -1, 1, ., 3, -3, ., 0
    z = np.array([[2.0, 4, 99, 6, 0, -99, 3]])
    obs = np.array([1, 1, 0, 1, 1, 0, 1], bool)
    zm, zv, acf = FM.acf_holes(z, obs, 6)
    assert zm[0] == 3 and zv[0] == 20 / 5
    want = [(-1 * 1 + 3 * -3) / 20,          # lag 1: pairs (0,1), (3,4)
            (1 * 3 + -3 * 0) / 20,           # lag 2: (1,3), (4,6)
            (-1 * 3 + 1 * -3 + 3 * 0) / 20,  # lag 3: (0,3), (1,4), (3,6)
            (-1 * -3) / 20,                  # lag 4: (0,4)
            (1 * 0) / 20,                    # lag 5: (1,6)
            (-1 * 0) / 20]                   # lag 6: (0,6)
    np.testing.assert_allclose(acf[0], want, rtol=0, atol=1e-16)
    # 8 steps observed at 0, 3, 6 only: pairs exist at lags 3 and 6 and nowhere else
    obs = np.array([1, 0, 0, 1, 0, 0, 1, 0], bool)
    z = np.array([[1.0, nan, nan, 2, nan, nan, 6, nan]])
    zm, zv, acf = FM.acf_holes(z, obs, 7)
    assert zm[0] == 3 and zv[0] == 14 / 3
    assert np.array_equal(np.isnan(acf[0]), [True, True, False, True, True, False, True])
    np.testing.assert_allclose(acf[0, [2, 5]], [(-2 * -1 + -1 * 3) / 14, (-2 * 3) / 14], rtol=1e-15)
    # a constant series: the denominator is 0; nothing observed: everything NaN
    _, zv, acf = FM.acf_holes(np.full((1, 6), 2.0), np.ones(6, bool), 2)
    assert zv[0] == 0 and np.all(np.isnan(acf))
    zm, zv, acf = FM.acf_holes(np.full((1, 6), 2.0), np.zeros(6, bool), 2)
    assert np.isnan(zm[0]) and np.isnan(zv[0]) and np.all(np.isnan(acf))


# ---- the chi-square tail and the Ljung-Box statistic --------------------------------------------------------------
@pytest.mark.parametrize("x", [0.1, 1.0, 10.0, 50.0])
def test_chi_square_tail_against_closed_forms(x):
    from ldsr_amd.filter import chi2_sf
    assert chi2_sf(x, 2) == pytest.approx(math.exp(-x / 2), rel=1e-12)
    assert chi2_sf(x, 4) == pytest.approx(math.exp(-x / 2) * (1 + x / 2), rel=1e-12)
    assert chi2_sf(x, 1) == pytest.approx(math.erfc(math.sqrt(x / 2)), rel=1e-12)


def test_ljung_box_statistic():
    from ldsr_amd.filter import chi2_sf, ljung_box
    acf = np.array([[0.5, -0.25], [0.1, np.nan]])
    Q, pv = ljung_box(acf, [10, 10])
    assert Q[0] == pytest.approx(10 * 12 * (0.25 / 9 + 0.0625 / 8), rel=1e-15)
    assert pv[0] == pytest.approx(chi2_sf(Q[0], 2), rel=1e-15) and np.isnan(Q[1]) and np.isnan(pv[1])
    assert FM.ljung_box(acf[:1], 10)[0] == pytest.approx(Q[0], rel=1e-15)
    Q, pv = ljung_box(acf[:1], [2])           # n_obs <= n_lags: no statistic
    assert np.isnan(Q[0]) and np.isnan(pv[0])


# ---- the argument checks: no device is touched before they pass -----------------------------------------------------
def _lib():
    from ldsr_amd import _lib
    return _lib.lib()


class _Args:
    """a valid ldsr_filter_batch call (T = 8, p = 1, q = 2, two cells), fields replaceable"""

    def __init__(self, **kw):
        self.device, self.n_series, self.T, self.p, self.q = 0, 1, 8, 1, 2
        self.y = (C.c_double * 64)(*([0.1] * 64))
        self.u = (C.c_double * 1024)()
        self.v = (C.c_double * 1024)()
        self.shared_uv = 0
        self.off = (C.c_int * 2)(0, 2)
        self.theta = (C.c_double * 256)(*([0.5] * 256))
        self.stdlik, self.n_lags = 1, 3
        self.rows = [None] * 8
        self.lik = (C.c_double * 2)()
        self.zstat = (C.c_double * 4)()
        self.acf = (C.c_double * 64)()
        self.status = (C.c_int * 2)()
        for k, val in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, val)

    def host(self):
        return _lib().ldsr_filter_batch(self.device, self.n_series, self.T, self.p, self.q, self.y, self.u, self.v,
                                        self.shared_uv, self.off, self.theta, self.stdlik, self.n_lags, *self.rows,
                                        self.lik, self.zstat, self.acf, self.status)

    def dev(self, ws=None, ws_bytes=0):
        as_vp = lambda a: None if a is None else C.cast(a, C.c_void_p)      # noqa: E731
        return _lib().ldsr_filter_batch_device(self.device, None, self.n_series, self.T, self.p, self.q, as_vp(self.y),
                                               as_vp(self.u), as_vp(self.v), self.shared_uv, self.off, as_vp(self.theta),
                                               self.stdlik, self.n_lags, *([None] * 8), as_vp(self.lik),
                                               as_vp(self.zstat), as_vp(self.acf), as_vp(self.status), ws, ws_bytes)


ERRORS = [
    (dict(n_series=0), EINVAL, b"n_series must be >= 1"),
    (dict(T=1, n_lags=0), EINVAL, b"T must be >= 2"),
    (dict(p=0), EINVAL, b"p and q must be >= 1"),
    (dict(p=17), EUNSUPPORTED, b"p and q above 16 are not supported by this build"),
    (dict(q=17), EUNSUPPORTED, b"p and q above 16 are not supported by this build"),
    (dict(y=None), EINVAL, b"y and cell_offsets must not be NULL"),
    (dict(off=None), EINVAL, b"y and cell_offsets must not be NULL"),
    (dict(off=(C.c_int * 2)(1, 2)), EINVAL, b"cell_offsets[0] must be 0"),
    (dict(off=(C.c_int * 2)(0, -1)), EINVAL, b"cell_offsets must be non-decreasing"),
    (dict(theta=None), EINVAL, b"theta and lik must not be NULL"),
    (dict(lik=None), EINVAL, b"theta and lik must not be NULL"),
    (dict(n_lags=-1), EINVAL, b"n_lags must be in 0 .. 32"),
    (dict(n_lags=33, T=64), EINVAL, b"n_lags must be in 0 .. 32"),
    (dict(n_lags=8), EINVAL, b"n_lags must be smaller than T"),
    (dict(acf=None), EINVAL, b"acf must not be NULL when n_lags > 0"),
]


@pytest.mark.parametrize("change,code,text", ERRORS, ids=[t.decode()[:40] + "/" + ",".join(c) for c, _, t in ERRORS])
def test_argument_errors_have_their_code_and_message(change, code, text):
    L = _lib()
    for entry in ("host", "dev"):
        a = _Args(**change)
        rc = getattr(a, entry)()
        msg = L.ldsr_last_error()
        assert rc == code and msg.startswith(text), (entry, rc, msg)
        assert list(a.lik) == [0.0, 0.0] if a.lik is not None else True


def test_workspace_bytes_and_a_short_workspace():
    L = _lib()
    wb = L.ldsr_filter_workspace_bytes
    assert wb(1, 8, 1, 2, 2, 0) > 0
    for bad in ((0, 8, 1, 2, 2, 0), (1, 1, 1, 2, 2, 0), (1, 8, 0, 2, 2, 0), (1, 8, 17, 2, 2, 0), (1, 8, 1, 17, 2, 0),
                (1, 8, 1, 2, -1, 0), (1, 8, 1, 2, 2, -1), (1, 8, 1, 2, 2, 8), (1, 64, 1, 2, 2, 33)):
        assert wb(*bad) == 0, bad
    for T, n in ((8, 2), (813, 8), (65, 7)):
        assert wb(1, T, 1, 2, n, 1) - wb(1, T, 1, 2, n, 0) >= 8 * T * n
        assert wb(1, T, 1, 2, n, min(32, T - 1)) == wb(1, T, 1, 2, n, 1)        # one strip of z whatever the lags
    # the device entry refuses a missing or short workspace before it touches a device
    a = _Args()
    need = wb(1, 8, 1, 2, 2, 3)
    assert a.dev(None, need) == EINVAL and L.ldsr_last_error().startswith(b"workspace must not be NULL")
    fake = C.c_void_p(1 << 20)      # never dereferenced: the size is checked first
    assert a.dev(fake, need - 256) == EINVAL
    assert L.ldsr_last_error() == b"workspace too small: need %d bytes" % need
    assert a.dev(C.c_void_p((1 << 20) + 8), need) == EINVAL
    assert L.ldsr_last_error().startswith(b"workspace must be 256-byte aligned")


def test_no_cpu_fallback():
    """a valid call on a device that does not exist is LDSR_EHIP: nothing is computed on the host"""
    L = _lib()
    a = _Args(device=L.ldsr_device_count() + 64)
    assert a.host() == EHIP, L.ldsr_last_error()
    assert list(a.lik) == [0.0, 0.0]
    from ldsr_amd import _lib as lib_mod
    import ldsr_amd
    y = np.linspace(-1, 1, 8)
    with pytest.raises(lib_mod.LdsrError):
        ldsr_amd.filter_batch(y, None, None, np.full((1, 8), 0.5), device=a.device)
    # an empty batch is answered without a device, as by the other entries
    assert _Args(off=(C.c_int * 2)(0, 0), device=a.device).host() == 0
