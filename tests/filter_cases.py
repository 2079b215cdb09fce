"""The case table of the Kalman filter's tests (tests/test_filter_host.py, tests/test_gpu_filter.py) and the
longdouble model's answer to each case, computed once and shared.

A case is one call: S series of T steps, each with its own mask and its cells (thetas), (p, q) inputs of which
u or v may be absent, per-series or shared, and a number of lags.  Series come from synth.make_series, thetas
from synth.make_init_packed; the masks are made here.  At most 8 cells a case."""
import functools

import numpy as np

import filter_model as FM
from ldsr_amd import synth


def mask(kind, T, seed):
    """observed steps [T] (bool)"""
    m = np.ones(T, dtype=bool)
    if kind == "dense":
        pass
    elif kind == "none":
        m[:] = False
    elif kind == "last":
        m[:] = False
        m[T - 1] = True
    elif kind == "first":
        m[:] = False
        m[0] = True
    elif kind == "lead150":          # a long all-missing lead (T = 200)
        m[:150] = False
    elif kind == "scatter30":        # 30 % missing, scattered
        m = synth.uniform(977, seed, T) >= 0.3
    elif kind == "straddle":         # a hole across the chunk boundary 63 | 64 and one just before it
        m[63:65] = False
        m[58:61] = False
    else:
        raise ValueError(kind)
    return m


#        name                T    p   q   u      v      masks                              cells      shared lags
CASES = [
    ("T2",                   2,   1,  2,  True,  True,  ["dense"],                         [2],       0,     1),
    ("T3_all_lags",          3,   3,  3,  True,  True,  ["dense"],                         [2],       0,     2),
    ("T63_scatter",          63,  1,  2,  True,  True,  ["scatter30"],                     [3],       0,     8),
    ("T64_dense",            64,  3,  3,  True,  True,  ["dense"],                         [2],       0,     1),
    ("T65_dense",            65,  1,  2,  True,  True,  ["dense"],                         [3],       0,     8),
    ("T65_straddle",         65,  3,  3,  True,  True,  ["straddle"],                      [2],       0,     8),
    ("T127_wide_scatter",    127, 16, 16, True,  True,  ["scatter30"],                     [2],       0,     0),
    ("T128_no_u",            128, 1,  2,  False, True,  ["dense"],                         [2],       0,     8),
    ("T129_no_v_straddle",   129, 3,  3,  True,  False, ["straddle"],                      [2],       0,     1),
    ("T200_no_uv_lead",      200, 1,  1,  False, False, ["lead150"],                       [3],       0,     8),
    ("T200_wide_dense",      200, 16, 16, True,  True,  ["dense"],                         [2],       0,     8),
    ("T129_none_observed",   129, 1,  2,  True,  True,  ["none"],                          [2],       0,     8),
    ("T65_last_only",        65,  3,  3,  True,  True,  ["last"],                          [2],       0,     1),
    ("T128_first_only",      128, 1,  2,  True,  True,  ["first"],                         [2],       0,     0),
    ("T129_three_series",    129, 3,  3,  True,  True,  ["dense", "scatter30", "straddle"], [2, 3, 2], 0,     8),
    ("T65_shared_uv",        65,  1,  2,  True,  True,  ["dense", "scatter30", "last"],    [2, 2, 2], 1,     8),
    ("T200_ragged_empty",    200, 3,  3,  True,  True,  ["dense", "scatter30", "lead150"], [3, 0, 3], 1,     1),
    ("T127_wide_no_u_multi", 127, 16, 16, False, True,  ["scatter30", "dense"],            [1, 2],    0,     8),
]
NAMES = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: T, p, q, Y [S, T], u / v ([k, T] shared, [S, k, T] per series, None absent), theta [n, 6+p+q],
    off [S+1], shared, n_lags; series(s) -> (y, u, v) of series s as the models take them"""
    _, T, p, q, has_u, has_v, masks, cells, shared, n_lags = CASES[NAMES.index(name)]
    S = len(masks)
    base = 100 * NAMES.index(name)
    ys, us, vs = [], [], []
    for s, kind in enumerate(masks):
        y, u, v = synth.make_series(T, p, q, series_id=base + s)
        y = np.where(mask(kind, T, base + s), y, np.nan)
        ys.append(y), us.append(u), vs.append(v)
    Y = np.array(ys)
    if shared or S == 1:
        u, v = us[0], vs[0]
    else:
        u, v = np.array(us), np.array(vs)
    u, v = (u if has_u else None), (v if has_v else None)
    p, q = (p if has_u else 1), (q if has_v else 1)         # an absent input has one (ignored) slot in theta
    n = int(sum(cells))
    assert n <= 8
    theta = synth.make_init_packed(p, q, n, seed=11 + NAMES.index(name))
    theta[:, 4 + p + q] = 0.25 * np.arange(n) - 0.5         # mu1 and V1 off make_init's 0 and 1
    theta[:, 5 + p + q] = 0.5 + 0.5 * np.arange(n)
    off = np.concatenate([[0], np.cumsum(cells)]).astype(np.int32)
    c = {"name": name, "T": T, "p": p, "q": q, "S": S, "Y": Y, "u": u, "v": v, "theta": theta, "off": off,
         "shared": shared, "n_lags": n_lags, "n": n}

    def series(s):
        pick = lambda a: None if a is None else (a if a.ndim == 2 else a[s])      # noqa: E731
        return Y[s], pick(u), pick(v)

    c["series"] = series
    return c


def run_model(c, stdlik=True, dtype=np.longdouble, n_lags=None):
    """the model on every cell of the case -> dict of [n, ...] arrays in `dtype` (n_obs: [n] ints)"""
    theta = c["theta"]
    n_lags = c["n_lags"] if n_lags is None else n_lags
    parts = []
    for s in range(c["S"]):
        a, b = c["off"][s], c["off"][s + 1]
        if b > a:
            y, u, v = c["series"](s)
            r = FM.kalman_filter(theta[a:b], y, u, v, stdlik=stdlik, n_lags=n_lags, dtype=dtype)
            r["n_obs"] = np.full(b - a, r["n_obs"])
            parts.append(r)
    return {k: np.concatenate([r[k] for r in parts], axis=0) for k in parts[0]}


@functools.lru_cache(maxsize=None)
def reference(name, stdlik=True):
    """the longdouble model's answer to the case, computed once; callers leave it unchanged"""
    return run_model(case(name), stdlik=stdlik)


def close(a, ref, frac):
    """|a - ref| <= frac * (1e-6 |ref| + 1e-9) -- a fraction of the project's bar (conftest.parity_close) -- with
    NaN exactly where ref has NaN; compared in ref's precision.  -> (ok, worst ratio to the allowance)"""
    ref = np.asarray(ref)
    a = np.asarray(a).astype(ref.dtype)
    nan_a, nan_r = np.isnan(a), np.isnan(ref)
    if not np.array_equal(nan_a, nan_r):
        return False, np.inf
    with np.errstate(invalid="ignore"):
        ratio = np.abs(a - ref) / (frac * (1e-6 * np.abs(ref) + 1e-9))
    ratio = np.where(nan_r, 0, ratio)
    worst = float(np.max(ratio)) if ratio.size else 0.0
    return bool(worst <= 1.0), worst
