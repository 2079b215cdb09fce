"""Principal-component regression without a GPU: the extended-precision model of the kernel
(tests/pcr_model.py) against numpy's least squares on the reference's Nakhon Phanom folds, the argument
checks of ldsr_pcr_batch, the Student-t quantile, and the host logic of ldsr_amd/pcr.py (cvPCR,
PCR_reconstruction, PCR_ensemble_selection) run on the model through `engine=`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pcr_model  # noqa: E402


@pytest.fixture(scope="module")
def npdata(refdata):
    qa = np.array(refdata["NPannual"]["Qa"])
    years = np.array(refdata["NPannual"]["year"])
    pc = np.ascontiguousarray(np.array(refdata["NPpc"]["data"]).T)        # 813 x 3, years 1200..2012
    Z = [np.array(z, dtype=np.int64) - 1 for z in refdata["NPcv"]["Z"]]   # stored 1-based
    inst = years - 1200
    return {"Qa": {"year": years, "Qa": qa}, "pc": pc, "Z": Z, "X": pc[inst], "y": np.log(qa)}


def _held(Z, n):
    h = np.zeros((len(Z), n), dtype=np.uint8)
    for f, z in enumerate(Z):
        h[f, z] = 1
    return h


def test_model_matches_lstsq_on_the_np_folds(npdata):
    """The design's condition number is <= 8.3 here, so LAPACK's fp64 answer is good to ~1e-14."""
    X, y, Z = npdata["X"], npdata["y"], npdata["Z"]
    assert len(Z) == 30 and all(len(z) == 12 for z in Z) and X.shape == (46, 3)
    r = pcr_model.pcr_batch_ld([X], y, _held(Z, 46))
    D = np.column_stack([np.ones(46), X])
    for f, z in enumerate(Z):
        keep = np.setdiff1d(np.arange(46), z)
        assert np.linalg.cond(D[keep]) <= 8.3
        beta, rss, _, _ = np.linalg.lstsq(D[keep], y[keep], rcond=None)
        assert r["status"][0, f] == 0 and r["df"][0, f] == 46 - 12 - 4
        assert np.max(np.abs(r["coef"][0, f, :4].astype(float) - beta)) <= 1e-12
        assert np.max(np.abs(r["pred"][0, f].astype(float) - D @ beta)) <= 1e-12
        assert abs(float(r["sigma"][0, f]) - np.sqrt(rss[0] / 30)) <= 1e-12
        H = D @ np.linalg.inv(D[keep].T @ D[keep]) @ D.T
        assert np.max(np.abs(r["lev"][0, f].astype(float) - np.diag(H))) <= 1e-11
    assert np.all(np.isnan(r["coef"][0, :, 4:].astype(float)))


def test_model_rank_rule_and_training_rule():
    rng = np.random.default_rng(2)
    X = rng.standard_normal((12, 3))
    y = rng.standard_normal(12)
    held = np.zeros(12, bool)
    dup = np.column_stack([X, X[:, 0]])
    assert pcr_model.fit_cell(dup, y, held, dup)["status"] == 2
    assert np.all(np.isnan(pcr_model.fit_cell(dup, y, held, dup)["pred"].astype(float)))
    held[:8] = True                       # 4 training rows, 4 coefficients: df = 0
    c = pcr_model.fit_cell(X, y, held, X)
    assert c["status"] == 0 and c["df"] == 0 and np.isnan(float(c["sigma"])) and np.all(np.isfinite(c["pred"].astype(float)))
    assert np.max(np.abs(c["pred"][8:].astype(float) - y[8:])) <= 1e-12      # an exact interpolation
    held[8] = True                        # 3 training rows
    assert pcr_model.fit_cell(X, y, held, X)["status"] == 2
    y2 = y.copy()
    y2[3] = np.nan                        # a missing y row never trains
    h2 = np.zeros(12, bool)
    h3 = h2.copy()
    h3[3] = True
    a, b = pcr_model.fit_cell(X, y2, h2, X), pcr_model.fit_cell(X, y, h3, X)
    assert a["df"] == b["df"] == 7 and np.array_equal(a["pred"], b["pred"])


def test_pcr_argument_validation_without_gpu():
    from ldsr_amd import _lib
    L = _lib.lib()
    n, F = 6, 2
    X = (C.c_double * (n * 17))(*np.random.default_rng(0).standard_normal(n * 17))
    y = (C.c_double * n)(*range(n))
    held = (C.c_ubyte * (F * n))()
    pred = (C.c_double * (F * n))()
    st = (C.c_int * F)()

    def call(k=3, X=X, y=y, n_folds=F, held=held, n=n, N=n):
        kk = (C.c_int * 1)(k)
        return L.ldsr_pcr_batch(0, 1, n, kk, X, y, n_folds, held, N, None, pred, None, None, None, None, st)

    assert call(k=17) == 2 and b"ldsr_pcr_batch" in L.ldsr_last_error() and b"k[0] = 17" in L.ldsr_last_error()
    assert call(k=0) == 1 and b"k[0] must be >= 1" in L.ldsr_last_error()
    assert call(n_folds=0) == 1 and b"ldsr_pcr_batch: n_folds must be >= 1" in L.ldsr_last_error()
    assert call(y=None) == 1 and b"ldsr_pcr_batch: y must not be NULL" in L.ldsr_last_error()
    assert call(X=None) == 1 and b"ldsr_pcr_batch: X must not be NULL" in L.ldsr_last_error()
    bad = (C.c_ubyte * (F * n))()
    bad[7] = 2
    assert call(held=bad) == 1 and b"heldout must hold 0 / 1 only (byte 7)" in L.ldsr_last_error()
    assert call(n=1, N=1) == 1 and b"n must be >= 2" in L.ldsr_last_error()
    assert call(N=5) == 1 and b"N must equal n" in L.ldsr_last_error()
    # a design beyond what LDS holds is refused before any HIP call (n = 1025 at k = 16)
    kk = (C.c_int * 1)(16)
    big = 1025
    Xb, yb, hb = (C.c_double * (big * 16))(), (C.c_double * big)(), (C.c_ubyte * big)()
    pb = (C.c_double * big)()
    assert L.ldsr_pcr_batch(0, 1, big, kk, Xb, yb, 1, hb, big, None, pb, None, None, None, None, st) == 2
    assert b"18432" in L.ldsr_last_error()


@pytest.mark.parametrize("df,want", [(1, 12.706204736), (2, 4.302652730), (10, 2.228138852), (30, 2.042272456),
                                     (42, 2.018081703), (120, 1.979930405)])
def test_qt(df, want):
    from ldsr_amd.pcr import qt
    assert abs(qt(0.975, df) - want) <= 1e-8
    assert abs(qt(0.025, df) + want) <= 1e-8 and qt(0.5, df) == 0.0


def test_cvpcr_on_the_model(npdata):
    from ldsr_amd import cv, pcr
    Z, y, X = npdata["Z"], npdata["y"], npdata["X"]
    for space, target in (("original", npdata["Qa"]["Qa"]), ("transformed", y)):
        r = pcr.cvPCR(npdata["Qa"], npdata["pc"], 1200, Z=Z, metric_space=space, use_robust_mean=False,
                      engine=pcr_model.pcr_batch)
        assert r["Ycv"].shape == (30, 46) and np.array_equal(r["target"]["y"], target)
        D = np.column_stack([np.ones(46), X])
        for f, z in enumerate(Z):
            keep = np.setdiff1d(np.arange(46), z)
            fit = D @ np.linalg.lstsq(D[keep], y[keep], rcond=None)[0]     # one_pcr_cv, R/PCR.R:101-107
            fit = np.exp(fit) if space == "original" else fit
            assert np.allclose(r["Ycv"][f], fit, rtol=1e-11, atol=0)
            want = cv.calculate_metrics(r["Ycv"][f], target, z)
            for k, v in want.items():
                assert r["metrics_dist"][k][f] == v
        for k in r["metrics"]:
            assert r["metrics"][k] == float(np.mean(r["metrics_dist"][k]))
    rb = pcr.cvPCR(npdata["Qa"], npdata["pc"], 1200, Z=Z, engine=pcr_model.pcr_batch)
    assert rb["metrics"]["KGE"] == cv.tbrm(rb["metrics_dist"]["KGE"])
    # one_pcr_cv is one cell of it
    one = pcr.one_pcr_cv(X, y, Z[4], engine=pcr_model.pcr_batch)
    assert np.array_equal(np.exp(one), rb["Ycv"][4])
    # a list of members: the fold mean of the member predictions (R/PCR.R:164)
    two = pcr.cvPCR(npdata["Qa"], [npdata["pc"], npdata["pc"][:, :2]], 1200, Z=Z, metric_space="transformed",
                    engine=pcr_model.pcr_batch)
    b = pcr.cvPCR(npdata["Qa"], npdata["pc"][:, :2], 1200, Z=Z, metric_space="transformed", engine=pcr_model.pcr_batch)
    a = pcr.cvPCR(npdata["Qa"], npdata["pc"], 1200, Z=Z, metric_space="transformed", engine=pcr_model.pcr_batch)
    assert np.allclose(two["Ycv"], 0.5 * (a["Ycv"] + b["Ycv"]), rtol=1e-15, atol=0)
    with pytest.raises(ValueError):
        pcr.cvPCR(npdata["Qa"], npdata["pc"][:700], 1200, Z=Z, engine=pcr_model.pcr_batch)     # ends in 1899
    with pytest.raises(ValueError):
        pcr.cvPCR(npdata["Qa"], npdata["pc"], 1200, transform="boxcox", Z=Z, engine=pcr_model.pcr_batch)
    with pytest.raises(RuntimeError):
        pcr.cvPCR(npdata["Qa"], np.column_stack([npdata["pc"], npdata["pc"][:, 0]]), 1200, Z=Z, engine=pcr_model.pcr_batch)


def test_reconstruction_on_the_model(npdata):
    from ldsr_amd import pcr
    X, y = npdata["X"], npdata["y"]
    r = pcr.PCR_reconstruction(npdata["Qa"], npdata["pc"], 1200, engine=pcr_model.pcr_batch)
    D = np.column_stack([np.ones(46), X])
    beta, rss, _, _ = np.linalg.lstsq(D, y, rcond=None)
    sigma = np.sqrt(rss[0] / 42)
    assert np.allclose(r["coeffs"], beta, rtol=1e-11) and abs(r["sigma"] - sigma) <= 1e-13
    assert np.array_equal(r["rec"]["year"], np.arange(1200, 2013))
    P = np.column_stack([np.ones(813), npdata["pc"]])
    fit = P @ beta
    h = np.einsum("ij,jk,ik->i", P, np.linalg.inv(D.T @ D), P)
    upr = fit + 2.018081703 * sigma * np.sqrt(1 + h)                        # predict.lm, qt(0.975, 42)
    sd = (upr - fit) / 1.96                                                 # R/PCR.R:53
    assert np.allclose(r["rec"]["Q"], np.exp(fit), rtol=1e-11)
    # exp_ci, R/utils.R:122-125: qlnorm(c(0.05, 0.95), fit, sd), qnorm(0.95) = 1.6448536269514722
    assert np.allclose(r["rec"]["Ql"], np.exp(fit - 1.6448536269514722 * sd), rtol=1e-9)
    assert np.allclose(r["rec"]["Qu"], np.exp(fit + 1.6448536269514722 * sd), rtol=1e-9)
    assert np.all(r["rec"]["Ql"] < r["rec"]["Q"]) and np.all(r["rec"]["Q"] < r["rec"]["Qu"])
    # transform = "none": predict.lm's interval itself
    rn = pcr.PCR_reconstruction(npdata["Qa"], npdata["pc"], 1200, transform="none", engine=pcr_model.pcr_batch)
    bn, rssn, _, _ = np.linalg.lstsq(D, npdata["Qa"]["Qa"], rcond=None)
    half = 2.018081703 * np.sqrt(rssn[0] / 42) * np.sqrt(1 + h)
    assert np.allclose(rn["rec"]["Q"], P @ bn, rtol=1e-11)
    assert np.allclose(rn["rec"]["Qu"] - rn["rec"]["Q"], half, rtol=1e-8)
    assert np.allclose(rn["rec"]["Q"] - rn["rec"]["Ql"], half, rtol=1e-8)
    # a list: member fits in the transformed space and the back-transformed row mean (R/PCR.R:72-88)
    e = pcr.PCR_reconstruction(npdata["Qa"], [npdata["pc"], npdata["pc"][:, :2]], 1200, engine=pcr_model.pcr_batch)
    assert len(e["ensemble"]) == 2 and e["ensemble"][1]["coeffs"].shape == (3,)
    assert np.allclose(e["ensemble"][0]["Q"], fit, rtol=1e-11) and abs(e["ensemble"][0]["sigma"] - sigma) <= 1e-13
    assert np.allclose(e["rec"]["Q"], np.exp(0.5 * (e["ensemble"][0]["Q"] + e["ensemble"][1]["Q"])), rtol=1e-15)
    assert set(e["rec"]) == {"year", "Q"}
    # boxcox with an explicit lambda: the back-transformed interval (R/PCR.R:60)
    rb = pcr.PCR_reconstruction(npdata["Qa"], npdata["pc"], 1200, transform="boxcox", lambda_=0.5, engine=pcr_model.pcr_batch)
    yb = (npdata["Qa"]["Qa"] ** 0.5 - 1) / 0.5
    assert np.allclose(rb["rec"]["Q"], (P @ np.linalg.lstsq(D, yb, rcond=None)[0] * 0.5 + 1) ** 2, rtol=1e-10)
    r0 = pcr.PCR_reconstruction(npdata["Qa"], npdata["pc"], 1200, transform="boxcox", lambda_=0.005, engine=pcr_model.pcr_batch)
    assert np.array_equal(r0["rec"]["Qu"], r["rec"]["Qu"])                  # |lambda| < 0.01: the log transform


def test_ensemble_selection_on_the_model(npdata):
    from ldsr_amd import pcr
    Qa, pc, Z = npdata["Qa"], npdata["pc"], npdata["Z"]
    members = [pc[:, :1], pc, pc[:, :2]]
    calls = []

    def engine(*a, **kw):
        calls.append(1)
        return pcr_model.pcr_batch(*a, **kw)

    cvs = [pcr.cvPCR(Qa, m, 1200, Z=Z, engine=pcr_model.pcr_batch) for m in members]
    ens = pcr.cvPCR(Qa, members, 1200, Z=Z, engine=pcr_model.pcr_batch)
    for crit in ("RE", "CE", "nRMSE", "KGE"):
        scores = [c["metrics"][crit] for c in cvs]
        best = int(np.argmax(scores))
        del calls[:]
        r = pcr.PCR_ensemble_selection(Qa, members, 1200, Z=Z, agg_type="best member", criterion=crit, engine=engine,
                                       return_all_metrics=True)
        assert len(calls) == 1                                             # one device call for every member's CV
        assert r["choice"] == best + 1 and r["member"] == best
        assert np.array_equal(r["cv"]["Ycv"], cvs[best]["Ycv"]) and r["cv"]["metrics"] == cvs[best]["metrics"]
        assert np.array_equal(r["all_metrics"][crit], scores)
        o = pcr.PCR_ensemble_selection(Qa, members, 1200, Z=Z, agg_type="best overall", criterion=crit, engine=engine,
                                       return_all_metrics=True)
        assert o["all_metrics"][crit][-1] == ens["metrics"][crit] and o["all_metrics"][crit].shape == (4,)
        if ens["metrics"][crit] > scores[best]:
            assert o["choice"] == 0 and o["member"] is None and np.array_equal(o["cv"]["Ycv"], ens["Ycv"])
        else:
            assert o["choice"] == best + 1 and np.array_equal(o["cv"]["Ycv"], cvs[best]["Ycv"])
    # 'best overall' picks the ensemble (choice = 0) when its score is the highest: two members whose errors cancel
    n = 46
    rng = np.random.default_rng(11)
    sig = rng.standard_normal(813)
    e = rng.standard_normal(813)
    Qs = {"year": Qa["year"], "Qa": np.exp(sig[Qa["year"] - 1200] + 0.05 * rng.standard_normal(n))}
    o = pcr.PCR_ensemble_selection(Qs, [(sig + 0.7 * e)[:, None], (sig - 0.7 * e)[:, None]], 1200, Z=Z,
                                   agg_type="best overall", criterion="RE", engine=engine, return_all_metrics=True)
    assert o["choice"] == 0 and o["all_metrics"]["RE"][2] > max(o["all_metrics"]["RE"][:2])
    # ties go to the first index (which.max)
    t = pcr.PCR_ensemble_selection(Qa, [pc, pc], 1200, Z=Z, criterion="RE", engine=engine)
    assert t["choice"] == 1
    # a member with a rank-deficient fold is never chosen
    s = pcr.PCR_ensemble_selection(Qa, [np.column_stack([pc, pc[:, 0]]), pc[:, :2]], 1200, Z=Z, criterion="RE", engine=engine)
    assert s["choice"] == 2
    # Z = None: the folds are drawn once, for every member
    z = pcr.PCR_ensemble_selection(Qa, members, 1200, criterion="RE", engine=engine, rng=np.random.default_rng(3))
    assert len(z["cv"]["Z"]) == 30
    with pytest.raises(ValueError):
        pcr.PCR_ensemble_selection(Qa, members, 1200, Z=Z, agg_type="mean", engine=engine)


def test_product_path_refuses_without_a_gpu(npdata):
    """No CPU fall-back: without a device the raw call fails with the library's error."""
    from ldsr_amd import _lib, pcr
    if _lib.lib().ldsr_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.LdsrError):
        pcr.pcr_batch([npdata["X"]], npdata["y"], np.zeros((1, 46), np.uint8))
