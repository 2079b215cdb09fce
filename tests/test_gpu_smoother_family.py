"""Every FIT smoother kernel -- the FIT form of em_scan_kernel for each compiled (L, W) member at each padded
width, and the serial smooth_kernel where the scan plan does not hold -- and the propagate and M-step entries,
against the fp64 oracle AND against the extended-precision model tests/smoother_model.py.

Three assertions per case:
 1. the project's bar against the oracle: |d| <= 1e-6 |ref| + 1e-9 (conftest.parity_close);
 2. the gap to the numpy.longdouble model is at most a TENTH of that bar.  The margin is a fraction of the
    project's own bar, not a figure measured on the device (the precedent is tests/test_plgrad_host.py); it is
    sound because tests/test_smoother_model_host.py proves, without a GPU, that the oracle itself sits within a
    thousandth of the bar of the model on every case of this table;
 3. an output depends on nothing but its own cell: X, Y, V, J are bit-equal between stdlik = True and False,
    lik(stdlik = False) and penalized_likelihood(lambda = 0) are bit-equal, and a cell's outputs are bit-equal
    for any position in the batch.

Each test prints, per case, the device's and the oracle's gap to the model as fractions of the bar
(profiles/r09_smoother_gaps.txt is that output of one run).  A case is one launch shape of 4 cells and a host
reference of at most 8193 steps."""
import numpy as np
import pytest

import smoother_model as SM
from conftest import parity_close

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-9
LAM = 0.4
DEVICE_CAP = 0.1          # of the bar: the device against the longdouble model
ORACLE_CAP = 1e-3         # of the bar: the oracle against the longdouble model (test_smoother_model_host.py)

# The compiled (chunk length L, waves per cell W) members of the scan family, restated from
# ldsr_amd/csrc/em_members.h.  test_smoother_model_host.py enumerates ldsr_smooth_plan and fails when a member
# exists that no case of the table below runs: a new member needs an entry here.
SCAN_MEMBERS = ((2, 1), (3, 1), (4, 1), (6, 1), (8, 1), (10, 1), (12, 1), (13, 1), (14, 1), (15, 1), (16, 1), (20, 1),
                (24, 1), (28, 1), (32, 1), (20, 2), (24, 2), (28, 2), (32, 2), (20, 4), (24, 4), (28, 4), (32, 4))
PADDED = (1, 2, 4, 8)                 # the widths the scan family is instantiated for
WIDTHS = (1, 2, 3, 5, 8)              # 3 and 5 run the identity padding of 4 and 8
BODY_T = (100, 250, 1000, 1100, 1500, 2600, 5000)


def member_lengths(L, W):
    """(smallest, interior, largest) T the plan maps to the member: 64 W L_prev + 1 and 64 W L, and between
    them a T that L does not divide with rp = T - nl (L - 1) neither 1 nor nl (nl = ceil(T / L) active lanes,
    the first rp of them with L steps)."""
    prev = [l for l, w in SCAN_MEMBERS if w == W and l < L]
    lo = 64 * W * max(prev) + 1 if prev else {1: 2, 2: 2049, 4: 4097}[W]
    hi = 64 * W * L
    for T in range((lo + hi) // 2, hi):
        nl = -(-T // L)
        rp = T - nl * (L - 1)
        if T % L and rp not in (1, nl) and T > lo:
            return lo, T, hi
    raise AssertionError("no interior length for member (%d, %d)" % (L, W))


def _case(rule, T, p, q, mask, u=True, v=True):
    tag = "%s-T%d-p%d-q%d-%s" % (rule, T, p, q, mask)
    if not (u and v):
        tag += "-no" + ("" if u else "u") + ("" if v else "v")
    return {"id": tag, "rule": rule, "T": T, "p": p, "q": q, "mask": mask, "u": u, "v": v}


def smoother_cases():
    """The single-series cases of smooth_batch / penalized_likelihood (the several-series cases are
    MULTI_CASES): every rule of the table, then one case for every kernel the rules leave out."""
    out = []
    for L, W in SCAN_MEMBERS:                                   # every member at both ends of its range
        for T in member_lengths(L, W):
            out.append(_case("member", T, 1, 2, "ragged"))
    for T in (2, 3, 4, 5, 7):                                   # fin with one or two active lanes
        out += [_case("tiny", T, 1, 2, "dense"), _case("tiny", T, 1, 2, "last")]
    for T in BODY_T:                                            # every padded width on every FIT body
        for p in WIDTHS:
            for q in WIDTHS:
                out.append(_case("width", T, p, q, "scattered30"))
    for mask in ("dense", "paleo30", "scattered90", "first", "onlylast", "none"):
        out.append(_case("mask", 813, 3, 3, mask))
    for T in (130, 2049):
        out += [_case("absent", T, 3, 2, "scattered30", u=False), _case("absent", T, 3, 2, "scattered30", v=False),
                _case("absent", T, 3, 2, "scattered30", u=False, v=False)]
    out += [_case("serial", 120, 9, 2, "scattered30"), _case("serial", 120, 16, 16, "scattered30"),
            _case("serial", 8193, 1, 2, "ragged")]
    # the rules above reach each member at p = 1, q = 2 and each width on seven members: the remaining
    # (member, padded width) instantiations once each, at the member's interior length
    have = set((_member_of(c["T"]), _pad(c["p"]), _pad(c["q"])) for c in out if c["u"] and c["v"])
    for L, W in SCAN_MEMBERS:
        for p in PADDED:
            for q in PADDED:
                if ((L, W), p, q) not in have:
                    out.append(_case("fill", member_lengths(L, W)[1], p, q, "scattered30"))
    return out


def _pad(n):
    return 1 if n <= 1 else 2 if n <= 2 else 4 if n <= 4 else 8 if n <= 8 else 16


def _member_of(T):
    """the (L, W) of SCAN_MEMBERS whose range holds T (None beyond 8192)"""
    for L, W in SCAN_MEMBERS:
        lo, _, hi = member_lengths(L, W)
        if lo <= T <= hi:
            return L, W
    return None


def propagate_cases():
    out = [_case("propagate", T, p, p, "ragged") for T in (2, 3, 85, 813, 2049, 8193) for p in (1, 3, 7, 16)]
    out += [_case("propagate", 85, 3, 2, "ragged", u=False), _case("propagate", 85, 3, 2, "ragged", v=False),
            _case("propagate", 85, 3, 2, "ragged", u=False, v=False)]
    return out


def mstep_cases():
    out = [_case("mstep", 3, 1, 2, "dense")] + [_case("mstep", T, 1, 2, "ragged") for T in (85, 813, 2049)]
    out += [_case("mstep", 150, p, q, "scattered30") for p in WIDTHS for q in WIDTHS]
    out += [_case("mstep", 85, 3, 2, "scattered30", u=False), _case("mstep", 85, 3, 2, "scattered30", v=False),
            _case("mstep", 85, 3, 2, "scattered30", u=False, v=False)]
    out += [_case("mstep", 813, 3, 3, mask) for mask in ("dense", "scattered30", "paleo30")]
    return out


# several series in one call: (tag, T, p, q, shared inputs); cell_offsets [0, 2, 2, 5] puts two cells on series
# 0, none on series 1 and three on series 2.  T = 300 at (1, 2) runs two single-wave cells per workgroup (three
# cells: a workgroup whose waves hold different cells and a partly filled last one), T = 2100 one two-wave cell
# per workgroup, T = 1100 at (8, 8) the global image with four cells per workgroup, (9, 2) the serial smoother.
MULTI_OFFSETS = (0, 2, 2, 5)
MULTI_CASES = [(300, 1, 2, False), (300, 1, 2, True), (2100, 1, 2, False), (2100, 1, 2, True), (1100, 8, 8, False),
               (120, 9, 2, False)]


def apply_mask(y, mask):
    """y dense -> y with the case's missing values (NaN, and one +-Inf in the ragged mask)."""
    from ldsr_amd import synth
    y = y.copy()
    T = y.size
    if mask == "ragged":
        # NaN at t = 0 and t = T-1, a run of 5 inside, one +-Inf; a series too short for all of it keeps what
        # fits (T = 2, 3: y[0] only, so that a step stays observed)
        y[0] = np.nan
        if T >= 4:
            y[T - 1] = np.nan
        if T >= 16:
            y[T // 3:T // 3 + 5] = np.nan
        if T >= 8:
            y[2 * T // 3] = np.inf if T % 2 == 0 else -np.inf
    elif mask == "last":
        y[T - 1] = np.nan
    elif mask.startswith("scattered"):
        y[synth.uniform(4242, T, T) < int(mask[9:]) / 100.0] = np.nan
    elif mask == "paleo30":
        y[:T - 30] = np.nan
    elif mask == "first":
        y[1:] = np.nan
    elif mask == "onlylast":
        y[:T - 1] = np.nan
    elif mask == "none":
        y[:] = np.nan
    elif mask != "dense":
        raise ValueError(mask)
    return y


def case_thetas(p, q, n=4):
    """make_init's draws with Q, R, mu1 moved off their defaults (as the older FIT test does); row 1 has
    A = 0.999, row 2 has C < 0."""
    from ldsr_amd import synth
    th = synth.make_init_packed(p, q, n, seed=14)
    th[1, 0] = 0.999
    th[2, 1 + p] = -th[2, 1 + p]
    th[:, 2 + p + q] = 0.3 + th[:, 0]                   # Q
    th[:, 3 + p + q] = 0.05 + 0.5 * np.abs(th[:, 1 + p])   # R
    th[:, 4 + p + q] = 0.2                              # mu1
    return th


def case_inputs(c, series_id=55):
    """-> y (with the case's mask), u, v (None where absent), thetas [4, 6+p+q] of a case."""
    from ldsr_amd import synth
    y, u, v = synth.make_series(c["T"], c["p"], c["q"], series_id=series_id)
    u, v = (u if c["u"] else None), (v if c["v"] else None)
    p, q = (c["p"] if c["u"] else 1), (c["q"] if c["v"] else 1)
    return apply_mask(y, c["mask"]), u, v, case_thetas(p, q)


def nan_for_inf(y):
    """the oracle keeps the reference's is_na test in the filter: it is given NaN where y is +-Inf"""
    return np.where(np.isfinite(y), y, np.nan)


def gap(a, ld):
    """max |a - ld| / (1e-6 |ld| + 1e-9): a's distance from the longdouble model in units of the bar
    (NaN == NaN; a NaN on one side only is an infinite gap)."""
    a = np.asarray(a, dtype=np.longdouble)
    ld = np.asarray(ld, dtype=np.longdouble)
    both = np.isnan(a) & np.isnan(ld)
    with np.errstate(invalid="ignore"):
        g = np.abs(a - ld) / (RTOL * np.abs(ld) + ATOL)
    g = np.where(both, 0.0, np.where(np.isnan(g), np.inf, g))
    return float(np.max(g)) if g.size else 0.0


def smoother_refs(c):
    """-> inputs, the oracle's rows and the longdouble model of a smoother case.  Keys of both references:
    X, Y, V, J [4, T], lik (stdlik), lik0 (not), pl = lik0 - LAM ssq."""
    from oracle import oracle as O
    y, u, v, th = case_inputs(c)
    yo = nan_for_inf(y)
    rows = [O.kalman_smoother(yo, u, v, t) for t in th]
    orc = {k: np.stack([r[k] for r in rows]) for k in "XYVJ"}
    orc["lik"] = np.array([r["lik"] for r in rows])
    orc["lik0"] = np.array([O.kalman_smoother(yo, u, v, t, stdlik=False)["lik"] for t in th])
    orc["pl"] = orc["lik0"] - LAM * SM.ssq(th, orc["X"], u)
    ld = SM.smoother(th, y, u, v, stdlik=False, dtype=np.longdouble)
    ld["lik0"] = ld["lik"]
    with np.errstate(invalid="ignore", divide="ignore"):
        ld["lik"] = ld["lik0"] / np.longdouble(np.count_nonzero(np.isfinite(y)))
    ld["pl"] = ld["lik0"] - np.longdouble(LAM) * SM.ssq(th, ld["X"], u)
    return y, u, v, th, orc, ld


def worst_gap(got, ld, keys):
    return max(gap(got[k], ld[k]) for k in keys)


@pytest.fixture(scope="module")
def eng():
    import ldsr_amd
    from ldsr_amd import _lib
    assert _lib.lib().ldsr_device_count() >= 1, "no GPU visible"
    return ldsr_amd


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


SMOOTH_KEYS = ("X", "Y", "V", "J", "lik", "lik0", "pl")


def _run_smoother(eng, y, u, v, th, off=None):
    g = eng.smooth_batch(y, u, v, th, cell_offsets=off)
    g0 = eng.smooth_batch(y, u, v, th, cell_offsets=off, stdlik=False)
    out = {k: g[k] for k in "XYVJ"}
    out["lik"], out["lik0"] = g["lik"], g0["lik"]
    out["pl"] = eng.penalized_likelihood(y, u, v, th, LAM, cell_offsets=off)
    out["pl_lam0"] = eng.penalized_likelihood(y, u, v, th, 0.0, cell_offsets=off)
    for k in "XYVJ":                                            # (3) the switch touches lik alone
        assert _same(g[k], g0[k]), ("stdlik changes", k)
    assert _same(out["lik0"], out["pl_lam0"]), ("lik0 vs pl(lambda = 0)", out["lik0"], out["pl_lam0"])
    return out


@pytest.mark.parametrize("c", smoother_cases(), ids=lambda c: c["id"])
def test_smoother_and_penalized_likelihood(eng, c):
    y, u, v, th, orc, ld = smoother_refs(c)
    got = _run_smoother(eng, y, u, v, th)
    d, o = worst_gap(got, ld, SMOOTH_KEYS), worst_gap(orc, ld, SMOOTH_KEYS)
    print("GAP smoother %-44s device %.3e oracle %.3e" % (c["id"], d, o))
    for k in SMOOTH_KEYS:
        assert parity_close(got[k], orc[k], RTOL, ATOL), (c["id"], k)                      # (1)
    if c["mask"] == "none":
        assert np.all(np.isnan(got["lik"])) and np.all(got["lik0"] == 0.0), (got["lik"], got["lik0"])
    for k in SMOOTH_KEYS:
        assert gap(got[k], ld[k]) <= DEVICE_CAP, (c["id"], k, gap(got[k], ld[k]))           # (2)
    back = _run_smoother(eng, y, u, v, th[::-1].copy())                                     # (3)
    for k in got:
        assert _same(got[k], back[k][::-1]), (c["id"], "position in the batch changes", k)


def multi_inputs(T, p, q, shared):
    """S = 3 series (scattered, dense and ragged masks), their inputs (one u, v for all when shared) and the
    five thetas MULTI_OFFSETS deals out."""
    from ldsr_amd import synth
    ser = [synth.make_series(T, p, q, series_id=70 + s) for s in range(3)]
    Y = np.stack([apply_mask(ser[s][0], ("scattered30", "dense", "ragged")[s]) for s in range(3)])
    U = ser[0][1] if shared else np.stack([a[1] for a in ser])
    V = ser[0][2] if shared else np.stack([a[2] for a in ser])
    return Y, U, V, case_thetas(p, q, n=5)


def multi_refs(T, p, q, shared):
    """-> per cell (series, cell, y, u, v, theta, the oracle's row, the longdouble model's row)"""
    from oracle import oracle as O
    Y, U, V, th = multi_inputs(T, p, q, shared)
    out = []
    for s in range(3):
        for i in range(MULTI_OFFSETS[s], MULTI_OFFSETS[s + 1]):
            us, vs = (U, V) if shared else (U[s], V[s])
            yo = nan_for_inf(Y[s])
            r, r0 = O.kalman_smoother(yo, us, vs, th[i]), O.kalman_smoother(yo, us, vs, th[i], stdlik=False)
            orc = {k: r[k] for k in "XYVJ"}
            orc.update(lik=r["lik"], lik0=r0["lik"], pl=r0["lik"] - LAM * SM.ssq(th[i], r["X"], us)[0])
            ld = SM.smoother(th[i], Y[s], us, vs, stdlik=False, dtype=np.longdouble)
            ldr = {k: ld[k][0] for k in "XYVJ"}
            ldr.update(lik0=ld["lik"][0], lik=ld["lik"][0] / np.longdouble(np.count_nonzero(np.isfinite(Y[s]))),
                       pl=ld["lik"][0] - np.longdouble(LAM) * SM.ssq(th[i], ld["X"], us)[0])
            out.append((s, i, Y[s], us, vs, th[i], orc, ldr))
    return out


@pytest.mark.parametrize("T,p,q,shared", MULTI_CASES)
def test_several_series_in_one_call(eng, T, p, q, shared):
    """cell_offsets [0, 2, 2, 5] over S = 3 series, with own and with shared inputs: a series without cells,
    more cells than a workgroup holds, the cell * T store offset for cell > 0.  Every row is bit-equal to the
    same cell run alone, and is held to the oracle and the model."""
    Y, U, V, th = multi_inputs(T, p, q, shared)
    got = _run_smoother(eng, Y, U, V, th, off=list(MULTI_OFFSETS))
    worst_d = worst_o = 0.0
    for s, i, ys, us, vs, thi, orc, ldr in multi_refs(T, p, q, shared):
        alone = _run_smoother(eng, ys, us, vs, th[i:i + 1])
        for k in got:
            assert _same(got[k][i], alone[k][0]), ("series %d cell %d differs from a run alone" % (s, i), k)
        row = {k: got[k][i] for k in SMOOTH_KEYS}
        worst_d, worst_o = max(worst_d, worst_gap(row, ldr, SMOOTH_KEYS)), max(worst_o, worst_gap(orc, ldr, SMOOTH_KEYS))
        for k in SMOOTH_KEYS:
            assert parity_close(row[k], orc[k], RTOL, ATOL), (s, i, k)
            assert gap(row[k], ldr[k]) <= DEVICE_CAP, (s, i, k, gap(row[k], ldr[k]))
    print("GAP several  %-44s device %.3e oracle %.3e" % ("T%d-p%d-q%d-%s" % (T, p, q, "shared" if shared else "own"),
                                                          worst_d, worst_o))


PROP_KEYS = ("X", "Y", "V", "lik", "lik0")


def propagate_refs(c):
    from oracle import oracle as O
    y, u, v, th = case_inputs(c)
    yo = nan_for_inf(y)
    rows = [O.propagate(t, u, v, yo) for t in th]
    orc = {k: np.stack([r[k] for r in rows]) for k in "XYV"}
    orc["lik"] = np.array([r["lik"] for r in rows])
    orc["lik0"] = np.array([O.propagate(t, u, v, yo, stdlik=False)["lik"] for t in th])
    ld = SM.propagate(th, u, v, y, stdlik=False, dtype=np.longdouble)
    ld["lik0"] = ld["lik"]
    ld["lik"] = ld["lik0"] / np.longdouble(np.count_nonzero(np.isfinite(y)))
    return y, u, v, th, orc, ld


def _run_propagate(eng, y, u, v, th):
    g = eng.smooth_batch(y, u, v, th, mode="propagate")
    g0 = eng.smooth_batch(y, u, v, th, stdlik=False, mode="propagate")
    for k in "XYV":
        assert _same(g[k], g0[k]), ("stdlik changes", k)
    return {"X": g["X"], "Y": g["Y"], "V": g["V"], "lik": g["lik"], "lik0": g0["lik"]}


@pytest.mark.parametrize("c", propagate_cases(), ids=lambda c: c["id"])
def test_propagate(eng, c):
    y, u, v, th, orc, ld = propagate_refs(c)
    got = _run_propagate(eng, y, u, v, th)
    d, o = worst_gap(got, ld, PROP_KEYS), worst_gap(orc, ld, PROP_KEYS)
    print("GAP propagate %-43s device %.3e oracle %.3e" % (c["id"], d, o))
    for k in PROP_KEYS:
        assert parity_close(got[k], orc[k], RTOL, ATOL), (c["id"], k)
    for k in PROP_KEYS:
        assert gap(got[k], ld[k]) <= DEVICE_CAP, (c["id"], k, gap(got[k], ld[k]))
    back = _run_propagate(eng, y, u, v, th[::-1].copy())
    for k in got:
        assert _same(got[k], back[k][::-1]), (c["id"], "position in the batch changes", k)
    one = eng.propagate(th[3], u, v, y)                        # the reference's call shape: one theta
    assert _same(one["X"][0], got["X"][3]) and one["lik"] == got["lik"][3]


def mstep_refs(c):
    """The M-step of the ORACLE's smoother output at the case's thetas: only the M-step is under test."""
    from oracle import oracle as O
    y, u, v, th = case_inputs(c)
    yo = nan_for_inf(y)
    fits = [O.kalman_smoother(yo, u, v, t) for t in th]
    fit = {k: np.stack([f[k] for f in fits]) for k in "XVJ"}
    orc = np.stack([O.mstep(yo, u, v, f) for f in fits])
    ld = SM.mstep(y, u, v, fit, dtype=np.longdouble)
    return y, u, v, fit, orc, ld


def mstep_batch(eng, Y, U, V, off, fit):
    """ldsr_mstep_batch on the rows of fit -> theta [n, 6+p+q], status [n]"""
    from ldsr_amd import _lib, api
    Yc, Uc, Vc, S, T, p, q, shared = api._series(Y, U, V)
    X, Vv, J = (np.ascontiguousarray(fit[k], dtype=np.float64) for k in "XVJ")
    n = X.shape[0]
    th, st = np.empty((n, 6 + p + q)), np.empty(n, dtype=np.int32)
    _lib.check(_lib.lib().ldsr_mstep_batch(0, S, T, p, q, api._d(Yc), api._d(Uc), api._d(Vc), shared,
                                           api._i(np.ascontiguousarray(off, dtype=np.int32)), api._d(X), api._d(Vv),
                                           api._d(J), api._d(th), api._i(st)))
    return th, st


@pytest.mark.parametrize("c", mstep_cases(), ids=lambda c: c["id"])
def test_mstep(eng, c):
    y, u, v, fit, orc, ld = mstep_refs(c)
    p, q = (1 if u is None else c["p"]), (1 if v is None else c["q"])
    got, st = mstep_batch(eng, y, u, v, [0, 4], fit)
    assert np.all(st == 0) and np.all(np.isfinite(orc))
    print("GAP mstep    %-44s device %.3e oracle %.3e" % (c["id"], gap(got, ld), gap(orc, ld)))
    assert parity_close(got, orc, RTOL, ATOL), c["id"]
    assert gap(got, ld) <= DEVICE_CAP, (c["id"], gap(got, ld))
    back, _ = mstep_batch(eng, y, u, v, [0, 4], {k: fit[k][::-1] for k in fit})
    assert _same(got, back[::-1]), (c["id"], "position in the batch changes")
    one = eng.pack_theta(eng.Mstep(y, u, v, {k: fit[k][2] for k in fit}), p, q)   # the reference's call shape
    assert _same(one, got[2])


def mstep_two_series_refs():
    """S = 2 series at T = 150, p = 2, q = 3, five cells dealt [0, 3, 5], fed with the oracle's smoother output
    -> (Y, U, V, fit), per row (cell, series, y, u, v, the row's fit, the oracle's theta, the model's)"""
    from ldsr_amd import synth
    from oracle import oracle as O
    T, p, q = 150, 2, 3
    ser = [synth.make_series(T, p, q, series_id=80 + s) for s in range(2)]
    Y = np.stack([apply_mask(ser[0][0], "scattered30"), apply_mask(ser[1][0], "ragged")])
    U, V = np.stack([a[1] for a in ser]), np.stack([a[2] for a in ser])
    th = case_thetas(p, q, n=5)
    soc = [0, 0, 0, 1, 1]
    fits = [O.kalman_smoother(nan_for_inf(Y[s]), U[s], V[s], th[i]) for i, s in enumerate(soc)]
    fit = {k: np.stack([f[k] for f in fits]) for k in "XVJ"}
    rows = []
    for i, s in enumerate(soc):
        row = {k: fit[k][i:i + 1] for k in fit}
        rows.append((i, s, Y[s], U[s], V[s], row, O.mstep(nan_for_inf(Y[s]), U[s], V[s], fits[i]),
                     SM.mstep(Y[s], U[s], V[s], row, dtype=np.longdouble)[0]))
    return (Y, U, V, fit), rows


def test_mstep_batch_of_two_series(eng):
    """ldsr_mstep_batch with S = 2 and offsets [0, 3, 5]: every row bit-equal to the same row alone."""
    (Y, U, V, fit), rows = mstep_two_series_refs()
    got, st = mstep_batch(eng, Y, U, V, [0, 3, 5], fit)
    assert np.all(st == 0)
    worst_d = worst_o = 0.0
    for i, s, ys, us, vs, row, orc, ld in rows:
        alone, _ = mstep_batch(eng, ys, us, vs, [0, 1], row)
        assert _same(got[i], alone[0]), i
        worst_d, worst_o = max(worst_d, gap(got[i], ld)), max(worst_o, gap(orc, ld))
        assert parity_close(got[i], orc, RTOL, ATOL), i
        assert gap(got[i], ld) <= DEVICE_CAP, (i, gap(got[i], ld))
    print("GAP mstep    %-44s device %.3e oracle %.3e" % ("two-series-T150-p2-q3", worst_d, worst_o))
