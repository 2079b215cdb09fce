"""Host model of ldsr_pcr_batch (include/ldsr_hip.h) in numpy.longdouble: the same Householder QR of
[1 X_m] on the training rows (not held out, y finite), intercept first, no pivoting, with the same rank rule
(a column whose remaining norm is <= 1e-7 of its original norm, or fewer training rows than columns: SINGULAR,
NaN outputs), leverage h_t = |R^-T x_t|^2 and sigma = sqrt(RSS / df), NaN at df = 0.  pcr_batch() has the
signature and the result of ldsr_amd.pcr.pcr_batch, so it also serves as its `engine=`."""
import numpy as np

LD = np.longdouble
CELL_OK, CELL_SINGULAR = 0, 2
COEF_STRIDE = 17


def fit_cell(X, y, held, Xpred):
    """One cell.  X [n, k], y [n], held [n] bool, Xpred [N, k] -> dict of longdouble results."""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, k = X.shape
    K, N = k + 1, Xpred.shape[0]
    tr = ~np.asarray(held, dtype=bool) & np.isfinite(y)
    nt = int(tr.sum())
    nan = {"pred": np.full(N, np.nan, LD), "lev": np.full(N, np.nan, LD), "coef": np.full(K, np.nan, LD),
           "sigma": LD(np.nan), "df": nt - K, "status": CELL_SINGULAR}
    if nt < K:
        return nan
    A = np.concatenate([np.ones((nt, 1), LD), X[tr].astype(LD)], axis=1)
    b = y[tr].astype(LD)
    osq = np.sum(A * A, axis=0)
    for j in range(K):
        x = A[j:, j].copy()
        nrm = np.sqrt(np.sum(x * x))
        if not nrm > LD(1e-7) * np.sqrt(osq[j]):
            return nan
        alpha = x[0]
        bet = -nrm if alpha >= 0 else nrm
        x[0] = alpha - bet
        tau = LD(1) / (nrm * (nrm + abs(alpha)))
        for c in range(j + 1, K):
            A[j:, c] -= (tau * np.sum(x * A[j:, c])) * x
        b[j:] -= (tau * np.sum(x * b[j:])) * x
        A[j, j] = bet
        A[j + 1:, j] = 0
    R = A[:K, :K]
    beta = np.zeros(K, LD)
    for r in range(K - 1, -1, -1):
        beta[r] = (b[r] - np.sum(R[r, r + 1:] * beta[r + 1:])) / R[r, r]
    P = np.concatenate([np.ones((N, 1), LD), np.asarray(Xpred, dtype=np.float64).astype(LD)], axis=1)
    pred = np.sum(P * beta[None, :], axis=1)
    Zs = np.zeros((N, K), LD)                        # R' z = x_t
    for r in range(K):
        Zs[:, r] = (P[:, r] - np.sum(Zs[:, :r] * R[:r, r][None, :], axis=1)) / R[r, r]
    df = nt - K
    sigma = np.sqrt(np.sum(b[K:] * b[K:]) / df) if df > 0 else LD(np.nan)
    return {"pred": pred, "lev": np.sum(Zs * Zs, axis=1), "coef": beta, "sigma": sigma, "df": df, "status": CELL_OK}


def pcr_batch_ld(members, y, heldout, pred_members=None):
    """Every (member, fold) cell in longdouble -> dict of arrays shaped as ldsr_amd.pcr.pcr_batch's."""
    members = [np.asarray(a, dtype=np.float64).reshape(len(y), -1) for a in members]
    preds = members if pred_members is None else [np.asarray(a, dtype=np.float64).reshape(-1, m.shape[1])
                                                  for a, m in zip(pred_members, members)]
    held = np.atleast_2d(np.asarray(heldout)).astype(bool)
    M, F, N = len(members), held.shape[0], preds[0].shape[0]
    out = {"pred": np.empty((M, F, N), LD), "lev": np.empty((M, F, N), LD), "coef": np.full((M, F, COEF_STRIDE), np.nan, LD),
           "sigma": np.empty((M, F), LD), "df": np.empty((M, F), np.int32), "status": np.empty((M, F), np.int32)}
    for m in range(M):
        for f in range(F):
            c = fit_cell(members[m], y, held[f], preds[m])
            out["pred"][m, f], out["lev"][m, f], out["sigma"][m, f] = c["pred"], c["lev"], c["sigma"]
            out["coef"][m, f, :c["coef"].size] = c["coef"]
            out["df"][m, f], out["status"][m, f] = c["df"], c["status"]
    return out


def pcr_batch(members, y, heldout, pred_members=None, lev=False, coef=True, sigma=True, device=0):
    """ldsr_amd.pcr.pcr_batch on the model, rounded to fp64 (an `engine=` for the host logic)."""
    r = pcr_batch_ld(members, y, heldout, pred_members)
    out = {k: (v if v.dtype == np.int32 else v.astype(np.float64)) for k, v in r.items()}
    if not lev:
        out["lev"] = None
    if not coef:
        out["coef"] = None
    if not sigma:
        out["sigma"] = None
    return out
