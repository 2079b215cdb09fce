"""ldsr_pcr_batch on the GPU (run with -m gpu) against the extended-precision model of tests/pcr_model.py.

Two bars.  (a) the project's: parity_close, |d| <= 1e-6 |ref| + 1e-9, on every case.  (b) on ill-conditioned
designs the yardstick is measured at run time: the worst error of fp64 numpy.linalg.lstsq against the model over
the same cells, predictions scaled by max |pred|; the device must stay within 16 x that value (Householder
against LAPACK's SVD: the constants differ), which the normal equations miss by more than 100 x (measured on
the CPU: lstsq 7.5e-12 / 3.9e-11 / 2.5e-12 against 8.7e-8 / 8.3e-6 / 7.3e-6 for the three designs below).
The tests run in file order: the first device call is the smallest, one cell of 3 rows."""
import numpy as np
import pytest

import pcr_model as M
from conftest import parity_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from ldsr_amd import _lib, pcr
    assert _lib.lib().ldsr_device_count() >= 1, "no GPU visible"
    return pcr


@pytest.fixture(scope="module")
def npdata(refdata):
    qa = np.array(refdata["NPannual"]["Qa"])
    years = np.array(refdata["NPannual"]["year"])
    pc = np.ascontiguousarray(np.array(refdata["NPpc"]["data"]).T)        # 813 x 3
    Z = [np.array(z, dtype=np.int64) - 1 for z in refdata["NPcv"]["Z"]]
    return {"Qa": {"year": years, "Qa": qa}, "pc": pc, "Z": Z, "X": pc[years - 1200], "y": np.log(qa)}


def _held(Z, n):
    h = np.zeros((len(Z), n), dtype=np.uint8)
    for f, z in enumerate(Z):
        h[f, np.asarray(z, dtype=np.int64)] = 1
    return h


def _design(n, k, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, k)) * rng.uniform(0.5, 3.0, k) + rng.uniform(-1, 1, k)
    y = 0.3 + X @ rng.uniform(-1, 1, k) + 0.5 * rng.standard_normal(n)
    return X, y


def _check(dev, ref, coef=True):
    """bar (a) on everything the call returned"""
    assert np.array_equal(dev["status"], ref["status"]) and np.array_equal(dev["df"], ref["df"])
    for key in ("pred", "lev", "sigma") + (("coef",) if coef else ()):
        if dev[key] is not None:
            assert dev[key].shape == ref[key].shape
            assert parity_close(dev[key], ref[key].astype(np.float64)), key


def _both(eng, members, y, held, pred_members=None):
    dev = eng.pcr_batch(members, y, held, pred_members=pred_members, lev=True)
    return dev, M.pcr_batch_ld(members, y, held, pred_members)


def test_first_call_one_cell_of_three_rows(eng):
    X = np.array([[0.0], [1.0], [3.0]])
    y = np.array([1.0, 2.0, 2.5])
    dev, ref = _both(eng, [X], y, np.zeros((1, 3), np.uint8))
    _check(dev, ref)
    assert dev["status"][0, 0] == 0 and dev["df"][0, 0] == 1 and np.all(np.isnan(dev["coef"][0, 0, 2:]))


def test_np_folds(eng, npdata):
    """NP data, NPcv's 30 folds (cond <= 8.3)."""
    dev, ref = _both(eng, [npdata["X"]], npdata["y"], _held(npdata["Z"], 46))
    assert np.all(dev["status"] == 0) and np.all(dev["df"] == 30)
    _check(dev, ref)


_SHAPES = [(n, k) for k in (1, 3, 8, 16) for n in sorted({k + 2, 13, 46, 64, 65, 130, 257}) if n >= k + 2]


@pytest.mark.parametrize("n,k", _SHAPES)
def test_shapes(eng, n, k):
    """one, two and more rows per lane, a ragged last pass, every compiled width"""
    X, y = _design(n, k, 100 * n + k)
    rng = np.random.default_rng(n + k)
    nh = max(1, (n - k - 1) // 3)
    Z = [[], list(range(nh)), sorted(rng.choice(n, nh, replace=False))]
    dev, ref = _both(eng, [X], y, _held(Z, n))
    assert np.all(dev["status"] == 0)
    _check(dev, ref)


@pytest.mark.parametrize("n", [451, 452, 1024])
def test_long_designs(eng, n):
    """k = 16: the last n whose cell fits the default 64 KiB of LDS, the first that needs the raised limit, and
    the entry's upper limit (16 rows per lane, 144.5 KiB)"""
    X, y = _design(n, 16, n)
    dev, ref = _both(eng, [X], y, _held([[], list(range(5, n, 7))], n))
    assert np.all(dev["status"] == 0)
    _check(dev, ref)


def test_fold_types(eng):
    n, k = 46, 3
    X, y = _design(n, k, 7)
    rng = np.random.default_rng(8)
    Z = [[], [17], list(range(9)), list(range(n - 9, n)), sorted(rng.choice(n, 11, replace=False)),
         list(range(k + 1, n)),            # exactly k + 1 training rows: df = 0
         list(range(k, n))]                # k training rows
    dev, ref = _both(eng, [X], y, _held(Z, n))
    _check(dev, ref)
    assert list(dev["status"][0]) == [0, 0, 0, 0, 0, 0, 2]
    assert list(dev["df"][0]) == [42, 41, 33, 33, 31, 0, -1]
    assert np.isnan(dev["sigma"][0, 5]) and np.all(np.isfinite(dev["pred"][0, 5])) and np.all(np.isfinite(dev["coef"][0, 5, :4]))
    assert parity_close(dev["pred"][0, 5, :k + 1], y[:k + 1])               # an exact interpolation of its rows
    assert all(np.all(np.isnan(dev[key][0, 6])) for key in ("pred", "lev", "coef", "sigma"))
    # NaN (and Inf) in y on rows a fold trains on: those rows drop out, as held-out rows do
    y2 = y.copy()
    y2[[2, 30]] = np.nan
    y2[40] = np.inf
    dev2, ref2 = _both(eng, [X], y2, _held(Z[:5], n))
    _check(dev2, ref2)
    assert list(dev2["df"][0]) == [39, 38, 31, 31, 31 - 3 + len(set(Z[4]) & {2, 30, 40})]
    Z3 = [sorted(set(z) | {2, 30, 40}) for z in Z[:5]]
    dev3 = eng.pcr_batch([X], y, _held(Z3, n), lev=True)
    for key in ("pred", "lev", "coef", "sigma", "df"):
        assert np.array_equal(dev2[key], dev3[key], equal_nan=True), key    # bit for bit the same training set


_ILL = [(13, 3, 1e-5), (70, 8, 1e-6), (130, 16, 1e-6)]


def _ill_design(n, k, eps):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((n, k))
    X[:, -1] = X[:, 0] + eps * rng.standard_normal(n)
    y = 1.0 + X @ rng.uniform(-1, 1, k) + 0.3 * rng.standard_normal(n)
    nh = max(1, (n - k - 1) // 4)
    Z = [[], list(range(nh)), list(range(n - nh, n)), sorted(rng.choice(n, nh, replace=False))]
    return X, y, Z


@pytest.mark.parametrize("n,k,eps", _ILL)
def test_ill_conditioned(eng, n, k, eps):
    """bar (b): within 16 x the error fp64 lstsq makes on the same cells (and bar (a) on pred, lev, sigma)"""
    X, y, Z = _ill_design(n, k, eps)
    held = _held(Z, n)
    dev, ref = _both(eng, [X], y, held)
    assert np.all(dev["status"] == 0)
    D = np.column_stack([np.ones(n), X])
    e_ls = e_dev = 0.0
    for f in range(len(Z)):
        keep = held[f] == 0
        want = ref["pred"][0, f]
        scale = float(np.max(np.abs(want)))
        ls = D @ np.linalg.lstsq(D[keep], y[keep], rcond=None)[0]
        e_ls = max(e_ls, float(np.max(np.abs(ls.astype(M.LD) - want))) / scale)
        e_dev = max(e_dev, float(np.max(np.abs(dev["pred"][0, f].astype(M.LD) - want))) / scale)
    print("n = %d k = %d eps = %g cond = %.3g: lstsq error %.3g, device error %.3g (%.2f x)"
          % (n, k, eps, np.linalg.cond(D), e_ls, e_dev, e_dev / e_ls))
    assert e_dev <= 16.0 * e_ls
    _check(dev, ref, coef=False)


def test_duplicated_column_is_singular_and_alone(eng):
    n = 46
    X, y = _design(n, 3, 21)
    Xd = np.column_stack([X, X[:, 1]])
    Z = [[], list(range(5)), [7, 20, 33]]
    held = _held(Z, n)
    mixed = eng.pcr_batch([X, Xd, X[:, :2]], y, held, lev=True)
    assert np.all(mixed["status"][1] == 2) and np.all(mixed["status"][[0, 2]] == 0)
    assert all(np.all(np.isnan(mixed[key][1])) for key in ("pred", "lev", "coef", "sigma"))
    clean = eng.pcr_batch([X, X[:, :2]], y, held, lev=True)
    for key in ("pred", "lev", "coef", "sigma", "df", "status"):
        assert np.array_equal(mixed[key][[0, 2]], clean[key], equal_nan=True), key
    _check(clean, M.pcr_batch_ld([X, X[:, :2]], y, held))


@pytest.mark.parametrize("ks", [(3, 2), (16, 1)])
def test_members_of_different_width(eng, npdata, ks):
    """each member bit-identical to being run alone; the ensemble's Ycv is the member mean"""
    rng = np.random.default_rng(31)
    pc = np.column_stack([npdata["pc"], rng.standard_normal((813, 13))])
    members = [pc[:, :k] for k in ks]
    Xs = [m[npdata["Qa"]["year"] - 1200] for m in members]
    held = _held(npdata["Z"], 46)
    both = eng.pcr_batch(Xs, npdata["y"], held, lev=True)
    for m, X in enumerate(Xs):
        alone = eng.pcr_batch([X], npdata["y"], held, lev=True)
        for key in ("pred", "lev", "coef", "sigma", "df", "status"):
            assert np.array_equal(both[key][m], alone[key][0], equal_nan=True), (key, m)
    _check(both, M.pcr_batch_ld(Xs, npdata["y"], held))
    cvr = eng.cvPCR(npdata["Qa"], members, 1200, Z=npdata["Z"], metric_space="transformed")
    assert np.array_equal(cvr["Ycv"], np.mean(both["pred"], axis=0))


def test_reconstruction_mode(eng, npdata):
    """N = 813 prediction rows from a fit on 46"""
    dev, ref = _both(eng, [npdata["X"]], npdata["y"], np.zeros((1, 46), np.uint8), pred_members=[npdata["pc"]])
    assert dev["pred"].shape == (1, 1, 813) and dev["df"][0, 0] == 42
    _check(dev, ref)
    a = eng.PCR_reconstruction(npdata["Qa"], npdata["pc"], 1200)
    b = eng.PCR_reconstruction(npdata["Qa"], npdata["pc"], 1200, engine=M.pcr_batch)
    for key in ("Q", "Ql", "Qu"):
        assert parity_close(a["rec"][key], b["rec"][key]), key
    assert parity_close(a["coeffs"], b["coeffs"]) and parity_close(a["sigma"], b["sigma"])
    ea = eng.PCR_reconstruction(npdata["Qa"], [npdata["pc"], npdata["pc"][:, :2]], 1200)
    eb = eng.PCR_reconstruction(npdata["Qa"], [npdata["pc"], npdata["pc"][:, :2]], 1200, engine=M.pcr_batch)
    assert parity_close(ea["rec"]["Q"], eb["rec"]["Q"])
    assert all(parity_close(x["Q"], w["Q"]) and parity_close(x["coeffs"], w["coeffs"]) for x, w in zip(ea["ensemble"], eb["ensemble"]))


def test_many_members(eng, npdata):
    """512 members x 30 folds: indexing over many workgroups; 64 sampled cells against the model"""
    rng = np.random.default_rng(77)
    pool = np.column_stack([npdata["X"], rng.standard_normal((46, 13))])
    ks = rng.integers(1, 9, 512)
    members = [pool[:, np.sort(rng.choice(16, k, replace=False))] for k in ks]
    held = _held(npdata["Z"], 46)
    dev = eng.pcr_batch(members, npdata["y"], held, lev=True)
    assert dev["pred"].shape == (512, 30, 46) and np.all(dev["status"] == 0)
    assert np.array_equal(dev["df"], np.repeat((46 - 12 - 1 - ks)[:, None], 30, axis=1))
    for c in rng.choice(512 * 30, 64, replace=False):
        m, f = divmod(int(c), 30)
        ref = M.fit_cell(members[m], npdata["y"], held[f], members[m])
        assert parity_close(dev["pred"][m, f], ref["pred"].astype(np.float64)), (m, f)
        assert parity_close(dev["lev"][m, f], ref["lev"].astype(np.float64)), (m, f)
        assert parity_close(dev["coef"][m, f, :ks[m] + 1], ref["coef"].astype(np.float64)), (m, f)
        assert np.all(np.isnan(dev["coef"][m, f, ks[m] + 1:]))
        assert parity_close(dev["sigma"][m, f], float(ref["sigma"])), (m, f)


def test_ensemble_selection_equals_its_engine_twin(eng, npdata):
    pc = npdata["pc"]
    members = [pc[:, :1], pc, pc[:, :2], pc[:, [0, 2]]]
    for agg in ("best member", "best overall"):
        for crit in ("RE", "KGE"):
            a = eng.PCR_ensemble_selection(npdata["Qa"], members, 1200, Z=npdata["Z"], agg_type=agg, criterion=crit,
                                           return_all_metrics=True)
            b = eng.PCR_ensemble_selection(npdata["Qa"], members, 1200, Z=npdata["Z"], agg_type=agg, criterion=crit,
                                           return_all_metrics=True, engine=M.pcr_batch)
            assert a["choice"] == b["choice"] and a["member"] == b["member"]
            for k in b["all_metrics"]:
                assert parity_close(a["all_metrics"][k], b["all_metrics"][k]), k
            for k in b["cv"]["metrics"]:
                assert parity_close(a["cv"]["metrics"][k], b["cv"]["metrics"][k]), k
            assert parity_close(a["cv"]["Ycv"], b["cv"]["Ycv"])
