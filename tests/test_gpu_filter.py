"""ldsr_filter_batch / ldsr_filter_batch_device on the device against the longdouble
host model of tests/filter_model.py, over the case table of tests/filter_cases.py: chunk edges in T, narrow and
wide inputs, absent inputs, every kind of mask, several series, ragged cells, lags across the chunk boundary.

The margin is a tenth of the project's bar |d| <= 1e-6 |ref| + 1e-9 against the longdouble model -- the margin
and the reasoning of tests/test_gpu_smoother_family.py: a fraction of the bar, not a figure measured on the
device; tests/test_filter_host.py shows the float64 model a thousandth of the bar from the longdouble one."""
import numpy as np
import pytest

import filter_cases as FC
import filter_model as FM
import filter_runs as FR
from extents import same_bits

pytestmark = pytest.mark.gpu

ROWS = FM.ROWS
OK, NONFINITE = 0, 1


@pytest.fixture(scope="module")
def eng():
    import ldsr_amd
    from ldsr_amd import _lib
    assert _lib.lib().ldsr_device_count() >= 1, "no GPU visible"
    return ldsr_amd


_base = {}


def base_run(name):
    """the case through the host entry with every row, stdlik = True: computed once"""
    if name not in _base:
        _base[name] = FR.host_run(FC.case(name))
    return _base[name]


def assert_close(got, ref, frac, what):
    ok, worst = FC.close(got, ref, frac)
    print("%-40s %.3g of the allowance" % (what, worst))
    assert ok, "%s: %.3g of the allowance (%g of the bar)" % (what, worst, frac)


@pytest.mark.parametrize("name", FC.NAMES)
def test_against_the_longdouble_model(eng, name):
    c = FC.case(name)
    ref = FC.reference(name)
    got = base_run(name)
    for k in ROWS + ("lik",):
        assert_close(got[k], ref[k], 0.1, "%s %s" % (name, k))
    assert_close(got["zstat"][:, 0], ref["zmean"], 0.1, name + " zmean")
    assert_close(got["zstat"][:, 1], ref["zvar"], 0.1, name + " zvar")
    if c["n_lags"]:
        assert_close(got["acf"], ref["acf"], 0.1, name + " acf")
    assert np.array_equal(np.isnan(got["e"]), np.repeat(~np.isfinite(c["Y"]), np.diff(c["off"]), axis=0))
    assert np.array_equal(got["status"], np.full(c["n"], OK)), got["status"]
    # the unstandardised likelihood, and every lag count the ABI allows at this T
    raw = FR.host_run(c, stdlik=False, rows=())
    assert_close(raw["lik"], FC.reference(name, False)["lik"], 0.1, name + " lik (stdlik = False)")
    for n_lags in sorted(set((0, 1, min(8, c["T"] - 1))) - {c["n_lags"]}):
        r = FR.host_run(c, n_lags=n_lags, rows=())
        same_bits({k: r[k] for k in ("lik", "zstat", "status")}, {k: got[k] for k in ("lik", "zstat", "status")},
                  "n_lags = %d and %d" % (n_lags, c["n_lags"]))
        if n_lags:
            assert_close(r["acf"], FC.run_model(c, n_lags=n_lags)["acf"], 0.1, "%s acf (n_lags = %d)" % (name, n_lags))


@pytest.mark.parametrize("name", FC.NAMES)
def test_likelihood_against_the_penalised_likelihood_at_lambda_zero(eng, name):
    """the same innovations likelihood from the smoother family's kernels (another summation order): the bar"""
    c = FC.case(name)
    raw = FR.host_run(c, stdlik=False, rows=())
    pl = eng.penalized_likelihood(c["Y"] if c["S"] > 1 else c["Y"][0], c["u"], c["v"], c["theta"], 0.0,
                                  cell_offsets=list(c["off"]))
    assert_close(raw["lik"], pl, 1.0, name + " lik against penalized_likelihood(lambda = 0)")


@pytest.mark.parametrize("name", FC.NAMES)
def test_outputs_do_not_depend_on_the_rows_requested(eng, name):
    c = FC.case(name)
    full = base_run(name)
    small = [k for k in full if k not in ROWS]
    for rows in [()] + [(k,) for k in ROWS] + [("Xu", "e", "ll"), ("Vp", "S")]:
        r = FR.host_run(c, rows=rows)
        assert set(r) == set(small) | set(rows)
        same_bits(r, {k: full[k] for k in r}, "rows = %s and all rows" % (rows,))


@pytest.mark.parametrize("name", FC.NAMES)
def test_outputs_do_not_depend_on_stdlik(eng, name):
    c = FC.case(name)
    full = base_run(name)
    raw = FR.host_run(c, stdlik=False)
    keep = [k for k in full if k != "lik"]
    same_bits({k: raw[k] for k in keep}, {k: full[k] for k in keep}, "stdlik = False and True")
    n_obs = np.repeat(np.isfinite(c["Y"]).sum(axis=1), np.diff(c["off"]))
    with np.errstate(invalid="ignore", divide="ignore"):       # (0 / 0 with nothing observed: NaN on both sides)
        assert np.array_equal(raw["lik"] / n_obs, full["lik"], equal_nan=True), (raw["lik"] / n_obs, full["lik"])


@pytest.mark.parametrize("name", FC.NAMES)
def test_outputs_do_not_depend_on_the_place_in_the_batch(eng, name):
    c = FC.case(name)
    full = base_run(name)
    # every series' cells in reverse order
    perm = np.concatenate([np.arange(c["off"][s], c["off"][s + 1])[::-1] for s in range(c["S"])]).astype(int)
    r = FR.host_run(c, theta=c["theta"][perm])
    same_bits(r, {k: v[perm] for k, v in full.items()}, "the cells reversed and in order")
    # the last cell alone, with its series alone
    s = max(s for s in range(c["S"]) if c["off"][s + 1] > c["off"][s])
    y, u, v = c["series"](s)
    one = dict(c, S=1, Y=y[None], u=u, v=v, n=1, off=np.array([0, 1], np.int32), theta=c["theta"][-1:])
    r = FR.host_run(one)
    same_bits(r, {k: v[-1:] for k, v in full.items()}, "the last cell alone and in the batch")


@pytest.mark.parametrize("name", FC.NAMES)
def test_device_entry_gives_the_host_entry_s_bits(eng, name):
    c = FC.case(name)
    same_bits(FR.device_run(c), base_run(name), "the device entry and the host entry")
    raw = FR.device_run(c, stdlik=False, rows=("e", "S"))
    same_bits(raw, FR.host_run(c, stdlik=False, rows=("e", "S")), "the device entry and the host entry (stdlik = False)")


@pytest.mark.parametrize("name", ["T65_dense", "T129_three_series", "T200_wide_dense"])
def test_a_cell_with_negative_innovation_variance_is_flagged_and_alone(eng, name):
    """R < 0 so that S_0 = C^2 V1 + R < 0 at the observed first step: log S_0 is NaN, the cell is
    LDSR_CELL_NONFINITE, and its neighbours are what they are without it"""
    c = FC.case(name)
    p, q = c["p"], c["q"]
    assert np.isfinite(c["Y"][0, 0])
    full = base_run(name)
    th = c["theta"].copy()
    bad = 1
    th[bad, 3 + p + q] = -(th[bad, 1 + p] ** 2 * th[bad, 5 + p + q]) - 0.5
    r = FR.host_run(c, theta=th)
    want = np.full(c["n"], OK)
    want[bad] = NONFINITE
    assert np.array_equal(r["status"], want), r["status"]
    assert not np.isfinite(r["lik"][bad]) and r["S"][bad, 0] < 0
    others = np.arange(c["n"]) != bad
    same_bits({k: v[others] for k, v in r.items()}, {k: v[others] for k, v in full.items()},
              "the neighbours with and without the cell")


def test_nakhon_phanom_at_the_stored_theta(eng, npcase, refdata):
    """the anchored case: T = 813, p = q = 3, the bundled NPlds theta; lik is NPlds$lik to 1e-9 (DESIGN.md
    section 2's soft pin) and the diagnostics are the model's"""
    from oracle import oracle as O
    n = npcase(1200)
    th = refdata["NPlds"]["theta"]
    theta = O.pack_theta(th["A"][0], th["B"], th["C"][0], th["D"], th["Q"][0], th["R"][0], th["mu1"][0], th["V1"][0])[None, :]
    r = eng.filter_batch(n["y"], n["u"], n["v"], theta, rows=())
    assert float(r["lik"][0]) == pytest.approx(refdata["NPlds"]["lik"][0], rel=1e-9)
    kf = eng.Kalman_filter(n["y"], n["u"], n["v"], O.unpack_theta(theta[0], 3, 3))
    assert kf["lik"] == float(r["lik"][0]) and kf["Xp"].shape == (1, 813)
    d = eng.innovation_diagnostics(n["y"], n["u"], n["v"], theta, n_lags=10)
    ref = FM.kalman_filter(theta, n["y"], n["u"], n["v"], n_lags=10, dtype=np.longdouble)
    assert d["n_obs"][0] == ref["n_obs"] == int(np.isfinite(n["y"]).sum())
    for k in ROWS:
        assert_close(kf[k], ref[k], 0.1, "NP " + k)
    for k in ("zmean", "zvar", "acf"):
        assert_close(d[k], ref[k], 0.1, "NP " + k)
    Q = FM.ljung_box(np.asarray(ref["acf"], dtype=np.float64), ref["n_obs"])
    assert d["Q"][0] == pytest.approx(Q[0], rel=1e-6)
    from ldsr_amd.filter import chi2_sf
    assert d["p_value"][0] == chi2_sf(d["Q"][0], 10) and 0.0 <= d["p_value"][0] <= 1.0
