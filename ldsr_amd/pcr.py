"""Principal-component regression on the GPU: the reference's benchmark model R/PCR.R
(PCR_reconstruction :20-91, one_pcr_cv :101-107, cvPCR :124-191, PCR_ensemble_selection :210-238) through
ldsr_pcr_batch of include/ldsr_hip.h.

Every least-squares fit -- each (member, fold) of a cross-validation, each member of a reconstruction -- is
one cell of ONE device call (a Householder QR per wavefront, ldsr_amd/csrc/pcr.hip); transforms, fold
averaging, metrics and the selection rule are host code here.  Nothing is fitted on the host: without a GPU
the calls raise LdsrError, unless `engine=` names another implementation of pcr_batch (tests run this host
logic on an extended-precision model).

Conventions: `Qa` is a dict with "year" and "Qa" (or a 2-column array), `pc` an N x k array -- rows are the
years start_year .. start_year + N - 1, columns the principal components, as the reference's data.frame -- or
a list of such arrays for an ensemble.  Folds `Z` hold 0-based indices into the instrumental period (R's are
1-based), as in cv.py.

Deviations from the reference, stated in INTEGRATION.md section 11: a rank-deficient design is an error
(status LDSR_CELL_SINGULAR) where .lm.fit would pivot; PCR_ensemble_selection with Z=None draws the folds
once for all members; transform="boxcox" needs an explicit lambda_ (MASS::boxcox is third-party)."""
import ctypes as C
import math

import numpy as np

from . import _lib, cv
from .api import _d, _i
from .rrng import qnorm

CELL_OK, CELL_SINGULAR = 0, 2
COEF_STRIDE = 17
_ubp = C.POINTER(C.c_ubyte)


# ---- Student's t quantile (stats::qt of predict.lm's interval) ------------------------------------------
def _betacf(a, b, x):
    """Continued fraction of the regularised incomplete beta function (modified Lentz)."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (d if abs(d) > tiny else tiny)
    h = d
    for m in range(1, 10000):
        m2 = 2 * m
        for aa in (m * (b - m) * x / ((qam + m2) * (a + m2)), -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + aa * d
            d = 1.0 / (d if abs(d) > tiny else tiny)
            c = 1.0 + aa / c
            c = c if abs(c) > tiny else tiny
            h *= d * c
        if abs(d * c - 1.0) < 1e-16:
            break
    return h


def _betainc(a, b, x):
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    front = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x))
    if x < (a + 1.0) / (a + b + 2.0):
        return front * _betacf(a, b, x) / a
    return 1.0 - front * _betacf(b, a, 1.0 - x) / b


def _pt_upper(t, df):
    """P(T > t) for t >= 0."""
    return 0.5 * _betainc(0.5 * df, 0.5, df / (df + t * t))


def qt(p, df):
    """Quantile of Student's t with df > 0 degrees of freedom (not necessarily whole): Newton's iteration on
    the upper tail from the normal quantile.  The tail is convex beyond 0, so the iterates rise monotonically
    to the root."""
    p, df = float(p), float(df)
    if not (0.0 < p < 1.0) or not df > 0.0:
        return float("nan")
    if p == 0.5:
        return 0.0
    if p < 0.5:
        return -qt(1.0 - p, df)
    up = 1.0 - p
    lc = math.lgamma(0.5 * (df + 1.0)) - math.lgamma(0.5 * df) - 0.5 * math.log(df * math.pi)
    t = float(qnorm(np.array([p]))[0])
    for _ in range(200):
        dens = math.exp(lc - 0.5 * (df + 1.0) * math.log1p(t * t / df))
        step = (_pt_upper(t, df) - up) / dens
        t += step
        if abs(step) <= 1e-15 * abs(t):
            break
    return t


# ---- the raw call ------------------------------------------------------------------------------------------
def _blocks(members, rows, name):
    out = []
    for m, a in enumerate(members):
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 1:
            a = a[:, None]
        if a.ndim != 2 or a.shape[0] != rows:
            raise ValueError("%s[%d] must be %d x k, got %s" % (name, m, rows, a.shape))
        out.append(a)
    return out


def pcr_batch(members, y, heldout, pred_members=None, lev=False, coef=True, sigma=True, device=0):
    """All (member, fold) fits of y ~ 1 + members[m] in one launch.
    members: list of n x k_m arrays; y [n] (non-finite rows never train); heldout [n_folds, n] of 0 / 1;
    pred_members: list of N x k_m arrays to predict, None = the members' own rows.
    -> {"pred" [M, F, N], "lev" (or None), "coef" [M, F, 17] (NaN beyond k_m + 1; or None), "sigma" [M, F]
    (or None), "df" [M, F], "status" [M, F]}."""
    y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
    n = y.size
    Xs = _blocks(members, n, "members")
    M = len(Xs)
    if M < 1:
        raise ValueError("members must not be empty")
    k = np.array([a.shape[1] for a in Xs], dtype=np.int32)
    held = np.ascontiguousarray(np.atleast_2d(np.asarray(heldout)).astype(np.uint8))
    if held.shape[1] != n:
        raise ValueError("heldout must be n_folds x %d" % n)
    F = held.shape[0]
    X = np.concatenate([a.T.ravel() for a in Xs])           # column-major blocks
    Xp, N = None, n
    if pred_members is not None:
        Ps = _blocks(pred_members, np.asarray(pred_members[0]).shape[0], "pred_members")
        if [a.shape[1] for a in Ps] != list(k):
            raise ValueError("pred_members must have the members' columns")
        N = Ps[0].shape[0]
        Xp = np.concatenate([a.T.ravel() for a in Ps])
    out = {"pred": np.empty((M, F, N)), "lev": np.empty((M, F, N)) if lev else None,
           "coef": np.empty((M, F, COEF_STRIDE)) if coef else None, "sigma": np.empty((M, F)) if sigma else None,
           "df": np.empty((M, F), dtype=np.int32), "status": np.empty((M, F), dtype=np.int32)}
    _lib.check(_lib.lib().ldsr_pcr_batch(int(device), M, n, _i(k), _d(X), _d(y), F, held.ctypes.data_as(_ubp), N,
                                         _d(Xp), _d(out["pred"]), _d(out["lev"]), _d(out["coef"]),
                                         _d(out["sigma"]), _i(out["df"]), _i(out["status"])))
    return out


# ---- the reference's operators ---------------------------------------------------------------------------
def _transform(qa, transform, lambda_):
    """-> (y, lambda or None)   R/PCR.R:30-40"""
    if transform == "log":
        return np.log(qa), None
    if transform == "boxcox":
        if lambda_ is None:
            raise ValueError('transform = "boxcox" needs lambda_: the reference takes it from MASS::boxcox, which '
                             "is not part of this package")
        if abs(lambda_) < 0.01:                              # :36-38
            return np.log(qa), 0.0
        return (qa ** lambda_ - 1.0) / lambda_, float(lambda_)
    if transform != "none":
        raise ValueError('Accepted transformations are "log", "boxcox" and "none" only.')
    return qa.copy(), None


def inv_boxcox(x, lambda_):
    """R/utils.R:112-114"""
    return np.exp(x) if lambda_ == 0 else (np.asarray(x) * lambda_ + 1.0) ** (1.0 / lambda_)


def _back(x, transform, lam):
    if transform == "log":
        return np.exp(x)
    if transform == "boxcox":
        return inv_boxcox(x, lam)
    return x


def exp_ci(y, sigma):
    """R/utils.R:122-125: the 5 % and 95 % quantiles of a log-normal -> (Q, Ql, Qu)."""
    z = qnorm(np.array([0.05, 0.95]))
    return np.exp(y), np.exp(y + sigma * z[0]), np.exp(y + sigma * z[1])


def _prep(Qa, pc, start_year, transform, lambda_):
    if isinstance(Qa, dict):
        qyears, qa = np.asarray(Qa["year"]), np.asarray(Qa["Qa"], dtype=np.float64)
    else:
        Qa = np.asarray(Qa, dtype=np.float64)
        qyears, qa = Qa[:, 0].astype(np.int64), Qa[:, 1]
    single = not isinstance(pc, (list, tuple))
    pcs = [np.asarray(a, dtype=np.float64) for a in ([pc] if single else pc)]
    pcs = [a[:, None] if a.ndim == 1 else a for a in pcs]
    N = pcs[0].shape[0]
    end_year = start_year + N - 1                            # :26
    if end_year < qyears[-1]:
        raise ValueError("The last year of the principal components is earlier than the last year of the "
                         "instrumental period.")
    y, lam = _transform(qa, transform, lambda_)
    years = np.arange(start_year, end_year + 1)
    inst = np.nonzero(np.isin(years, qyears))[0]             # :43
    if inst.size != y.size:
        raise ValueError("every year of Qa must lie within start_year .. start_year + nrow(pc) - 1")
    return {"single": single, "pcs": pcs, "y": y, "qa": qa, "qyears": qyears, "years": years, "inst": inst, "lam": lam}


def _heldout(Z, n):
    held = np.zeros((len(Z), n), dtype=np.uint8)
    for f, z in enumerate(Z):
        held[f, np.asarray(z, dtype=np.int64)] = 1
    return held


def _engine(engine, device):
    if engine is not None:
        return engine
    return lambda *a, **kw: pcr_batch(*a, device=device, **kw)


def one_pcr_cv(Xmat, y, z, device=0, engine=None):
    """one_pcr_cv (R/PCR.R:101-107): fit without the points z (0-based), predict every row of Xmat."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    r = _engine(engine, device)([Xmat], y, _heldout([z], y.size), coef=False, sigma=False)
    if r["status"][0, 0] != CELL_OK:
        raise RuntimeError("one_pcr_cv: rank-deficient design (or fewer training rows than coefficients)")
    return r["pred"][0, 0]


def _cv_result(pred, p, transform, Z, metric_space, use_robust_mean):
    """cvPCR from the members' predictions pred [M', F, n] on: fold mean :164, back-transform :166-175,
    metrics :177-180."""
    Ycv = np.mean(pred, axis=0)
    if metric_space == "original":
        Ycv = _back(Ycv, transform, p["lam"])
        target = p["qa"]
    else:
        target = p["y"]
    if np.any(np.isnan(Ycv)):            # a rank-deficient cell (PCR_ensemble_selection): no score
        dist = {k: np.full(len(Z), np.nan) for k in ("R2", "RE", "CE", "nRMSE", "KGE")}
        mean = {k: float("nan") for k in dist}
    else:
        dist, mean = cv.cv_metrics(Ycv, target, Z, robust_mean=use_robust_mean)
    return {"metrics_dist": dist, "metrics": mean, "target": {"year": p["qyears"], "y": target}, "Ycv": Ycv, "Z": Z}


def _bad_cell(status):
    m, f = np.argwhere(status != CELL_OK)[0]
    return "member %d, fold %d: rank-deficient design (or fewer training rows than coefficients)" % (m, f)


def cvPCR(Qa, pc, start_year, transform="log", Z=None, metric_space="original", use_robust_mean=True, lambda_=None,
          rng=None, device=0, engine=None):
    """cvPCR (R/PCR.R:124-191): every member x fold fit in one device call.
    -> {"metrics_dist": {name: [n_folds]}, "metrics": {name: mean}, "target": {"year", "y"}, "Ycv" [n_folds, n]
    (the reference's long table, one row per fold), "Z"}."""
    if metric_space not in ("original", "transformed"):
        raise ValueError('metric_space must be "original" or "transformed"')
    p = _prep(Qa, pc, start_year, transform, lambda_)
    if Z is None:
        Z = cv.make_Z(p["y"], rng=rng)                        # :158
    elif not isinstance(Z, (list, tuple)):
        raise ValueError("Please provide the cross-validation folds (Z) in a list.")
    Xmats = [a[p["inst"]] for a in p["pcs"]]                  # :155
    r = _engine(engine, device)(Xmats, p["y"], _heldout(Z, p["y"].size), coef=False, sigma=False)
    if np.any(r["status"] != CELL_OK):
        raise RuntimeError("cvPCR: " + _bad_cell(r["status"]))
    return _cv_result(r["pred"], p, transform, Z, metric_space, use_robust_mean)


def PCR_reconstruction(Qa, pc, start_year, transform="log", lambda_=None, device=0, engine=None):
    """PCR_reconstruction (R/PCR.R:20-91).  Single model: {"rec": {"year", "Q", "Ql", "Qu"}, "coeffs", "sigma"},
    the interval being predict.lm's fit +- qt(0.975, df) sigma sqrt(1 + h_t) put through the reference's own
    sdY = (upr - fit) / 1.96 and exp_ci (:51-66).  List: {"rec": {"year", "Q"}, "ensemble": [{"Q", "coeffs",
    "sigma"}]} with Q the back-transformed row mean (:72-88)."""
    p = _prep(Qa, pc, start_year, transform, lambda_)
    y, lam = p["y"], p["lam"]
    Xmats = [a[p["inst"]] for a in p["pcs"]]                  # :48, :75
    r = _engine(engine, device)(Xmats, y, np.zeros((1, y.size), dtype=np.uint8), pred_members=p["pcs"],
                                lev=p["single"], coef=True, sigma=True)
    if np.any(r["status"] != CELL_OK):
        raise RuntimeError("PCR_reconstruction: " + _bad_cell(r["status"]))
    ks = [a.shape[1] for a in Xmats]
    if not p["single"]:
        ens = [{"Q": r["pred"][m, 0], "coeffs": r["coef"][m, 0, :ks[m] + 1], "sigma": float(r["sigma"][m, 0])}
               for m in range(len(ks))]
        Q = _back(np.mean(r["pred"][:, 0], axis=0), transform, lam)          # :81-86
        return {"rec": {"year": p["years"], "Q": Q}, "ensemble": ens}
    fit, h, sig, df = r["pred"][0, 0], r["lev"][0, 0], float(r["sigma"][0, 0]), int(r["df"][0, 0])
    half = (qt(0.975, df) if df > 0 else float("nan")) * sig * np.sqrt(1.0 + h)      # predict.lm, interval = "prediction"
    lwr, upr = fit - half, fit + half
    if transform == "log" or (transform == "boxcox" and lam == 0):
        Q, Ql, Qu = exp_ci(fit, (upr - fit) / 1.96)           # :53-54, :57-58
    elif transform == "boxcox":
        Q, Ql, Qu = (inv_boxcox(a, lam) for a in (fit, lwr, upr))            # :60
    else:
        Q, Ql, Qu = fit, lwr, upr
    return {"rec": {"year": p["years"], "Q": Q, "Ql": Ql, "Qu": Qu}, "coeffs": r["coef"][0, 0, :ks[0] + 1], "sigma": sig}


def _which_max(x):
    """R's which.max: first index of the maximum, NaN ignored; -1 when there is none."""
    x = np.asarray(x, dtype=np.float64)
    return -1 if np.all(np.isnan(x)) else int(np.nanargmax(x))


def PCR_ensemble_selection(Qa, pc, start_year, transform="log", Z=None, agg_type="best member", criterion="RE",
                           return_all_metrics=False, lambda_=None, rng=None, device=0, engine=None):
    """PCR_ensemble_selection (R/PCR.R:210-238) with ONE device call for every member's cross-validation; the
    ensemble's cross-validation (:228) is built from the same member predictions.  The criterion is maximised
    (which.max, :222, first index on ties) whichever it is, as the reference does.
    -> {"choice": the reference's 1-based member number, 0 = the ensemble mean; "member": 0-based index or None;
    "cv": the choice's cvPCR result; "all_metrics": {name: [M] or [M + 1]} if asked}.
    A member with a rank-deficient fold has NaN metrics and is never chosen."""
    if agg_type not in ("best member", "best overall"):
        raise ValueError('agg.type must be either "best member" or "best overall".')
    if criterion not in ("RE", "CE", "nRMSE", "KGE"):
        raise ValueError("Criterion must be either RE, CE, nRMSE or KGE")
    if not isinstance(pc, (list, tuple)):
        raise ValueError("pc must be a list of principal-component matrices")
    p = _prep(Qa, pc, start_year, transform, lambda_)
    if Z is None:
        Z = cv.make_Z(p["y"], rng=rng)
    Xmats = [a[p["inst"]] for a in p["pcs"]]
    r = _engine(engine, device)(Xmats, p["y"], _heldout(Z, p["y"].size), coef=False, sigma=False)
    pred = np.where((r["status"] == CELL_OK)[:, :, None], r["pred"], np.nan)
    member_cv = [_cv_result(pred[m:m + 1], p, transform, Z, "original", True) for m in range(len(Xmats))]    # :220
    keys = list(member_cv[0]["metrics"])
    allm = {k: [c["metrics"][k] for c in member_cv] for k in keys}
    best = _which_max(allm[criterion])                        # :222
    if best < 0:
        raise RuntimeError("PCR_ensemble_selection: no member has a finite " + criterion)
    ans = {"choice": best + 1, "member": best, "cv": member_cv[best]}
    if agg_type == "best overall":
        ens_cv = _cv_result(pred, p, transform, Z, "original", True)          # :228
        if ens_cv["metrics"][criterion] > allm[criterion][best]:              # :230
            ans = {"choice": 0, "member": None, "cv": ens_cv}
        for k in keys:
            allm[k] = allm[k] + [ens_cv["metrics"][k]]
    if return_all_metrics:
        ans["all_metrics"] = {k: np.array(v) for k, v in allm.items()}
    return ans
