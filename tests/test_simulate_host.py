"""Stochastic replicates (LDS_rep / one_LDS_rep, the reference's R/stochastics.R), host side: R's
normal draws on the host (rrng), the uniform counts and offsets of the R-stream mode, argument
checks, and no host fallback.  Also the numpy twin of one_LDS_rep that tests/test_gpu_simulate.py
compares the GPU against: a line-by-line transcription of R/stochastics.R:20-45 fed with the same
uniforms."""
import ctypes as C
import math

import numpy as np
import pytest

from ldsr_amd import _lib, rrng, synth

_BIG = 134217728.0


# ---- the twin ------------------------------------------------------------------------------------
class Uniforms:
    """A uniform stream in R's consumption order: RUniform(k) for set.seed(k), or a fixed array."""

    def __init__(self, src):
        self.g = src if isinstance(src, rrng.RUniform) else None
        self.a = None if self.g else np.asarray(src, dtype=np.float64)
        self.used = 0

    def unif_rand(self, n):
        if self.g is not None:
            out = self.g.unif_rand(n)
        else:
            out = self.a[self.used:self.used + n]
            assert out.size == n, "uniform stream exhausted"
        self.used += n
        return out


def counter_uniforms(seed, model, rep, n):
    """Counter mode's uniforms of (model, rep): SplitMix64 of synth.py, mapped to (0, 1)."""
    with np.errstate(over="ignore"):
        stream = np.uint64((model << 32) + rep)
        base = synth._splitmix64(np.uint64(seed) ^ synth._splitmix64(stream))
        z = synth._splitmix64(base + np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    return ((z >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def _sd(var):
    with np.errstate(invalid="ignore"):
        return float(np.sqrt(np.float64(var)))


def twin_rnorm(src, n, sd):
    """R's rnorm(n, 0, sd) from a uniform stream (nmath rnorm.c + snorm.c INVERSION)."""
    if math.isnan(sd) or math.isinf(sd) or sd < 0:
        return np.full(n, np.nan)
    if sd == 0:
        return np.zeros(n)
    u = src.unif_rand(2 * n).reshape(n, 2)
    return sd * rrng.qnorm((np.floor(_BIG * u[:, 0]) + u[:, 1]) / _BIG)


def twin_one_rep(src, th, p, q, u, v, n, mu=0.0, exp_trans=True):
    """R/stochastics.R:20-45 for a packed theta; u / v are p x n' / q x n' or None."""
    A, B, Cc, D = th[0], th[1:1 + p], th[1 + p], th[2 + p:2 + p + q]
    Q, R, V1 = th[2 + p + q], th[3 + p + q], th[5 + p + q]
    X = np.zeros(n + 1)
    Y = np.zeros(n)
    X[0] = twin_rnorm(src, 1, _sd(V1))[0]
    qn = twin_rnorm(src, n, _sd(Q))
    rn = twin_rnorm(src, n, _sd(R))
    if u is None:
        for t in range(n):
            X[t + 1] = A * X[t] + qn[t]
            Y[t] = Cc * X[t] + rn[t]
    else:
        for t in range(n):
            X[t + 1] = A * X[t] + B @ u[:, t] + qn[t]
            Y[t] = Cc * X[t] + D @ v[:, t] + rn[t]
    with np.errstate(over="ignore", invalid="ignore"):
        Qs = np.exp(Y + mu) if exp_trans else Y + mu
    return X[:n], Y, Qs


def twin_count(th, p, q, n):
    """Uniforms one replicate consumes."""
    return sum(2 * k for k, var in ((1, th[5 + p + q]), (n, th[2 + p + q]), (n, th[3 + p + q]))
               if not (math.isnan(_sd(var)) or math.isinf(_sd(var)) or _sd(var) == 0))


# ---- tests ---------------------------------------------------------------------------------------
PUBLISHED = {1: [-0.6264538, 0.1836433, -0.8356286, 1.5952808, 0.3295078],
             42: [1.3709584, -0.5646982, 0.3631284, 0.6328626, 0.4042683],
             123: [-0.5604756, -0.2301775, 1.5587083, 0.0705084, 0.1292877]}


@pytest.mark.parametrize("seed", sorted(PUBLISHED))
def test_rnorm_reproduces_published_draws(seed):
    np.testing.assert_allclose(rrng.RUniform(seed).rnorm(5), PUBLISHED[seed], rtol=0, atol=5e-8)
    # the twin's normal path is the same rule
    np.testing.assert_allclose(twin_rnorm(Uniforms(rrng.RUniform(seed)), 5, 1.0), PUBLISHED[seed], rtol=0, atol=5e-8)


def test_qnorm_round_trips_through_erfc():
    tail = np.logspace(-15, math.log10(0.075), 700)
    p = np.concatenate([tail, np.linspace(0.075, 0.925, 701), 1.0 - tail])
    z = rrng.qnorm(p)
    back = np.array([0.5 * math.erfc(-zz / math.sqrt(2.0)) for zz in z])
    np.testing.assert_allclose(back, p, rtol=1e-13, atol=0)
    assert np.all(np.diff(z[np.argsort(p)]) >= 0) and rrng.qnorm(np.array([0.5]))[0] == 0.0


@pytest.mark.parametrize("sd,expect", [(0.0, 0.0), (np.nan, np.nan), (-1.0, np.nan), (np.inf, np.nan)])
def test_rnorm_sd_rules_consume_no_uniforms(sd, expect):
    g = rrng.RUniform(7)
    got = g.rnorm(4, 0.0, sd)
    np.testing.assert_array_equal(got, np.full(4, expect))
    assert g.unif_rand(1)[0] == rrng.RUniform(7).unif_rand(1)[0]      # the stream did not move
    src = Uniforms(rrng.RUniform(7))
    np.testing.assert_array_equal(twin_rnorm(src, 4, sd), np.full(4, expect))
    assert src.used == 0


def _thetas():
    base = np.array([0.6, 0.3, -0.2, 0.9, 0.1, 0.4, 0.5, 0.2, 0.0, 0.8])       # p = 2, q = 2
    rows = []
    for slot in (6, 7, 9):                  # Q, R, V1
        for val in (1.0, 0.0, np.nan, -1.0, np.inf):
            th = base.copy()
            th[slot] = val
            rows.append(th)
    return np.array(rows)


def test_draw_count_and_offsets_match_the_twin():
    L = _lib.lib()
    th = _thetas()
    n, reps, p, q = 37, 3, 2, 2
    off = np.empty(th.shape[0] + 1, dtype=np.int64)
    total = L.ldsr_simulate_draw_count(th.shape[0], n, p, q, th.ctypes.data_as(C.POINTER(C.c_double)), reps,
                                       off.ctypes.data_as(C.POINTER(C.c_longlong)))
    want = np.concatenate([[0], np.cumsum([reps * twin_count(t, p, q, n) for t in th])])
    assert total == want[-1] and np.array_equal(off, want)
    # ... and it is what the transcription of the reference actually consumes
    u = np.ones((p, n))
    for t in th:
        src = Uniforms(rrng.RUniform(3))
        for _ in range(reps):
            twin_one_rep(src, t, p, q, u, u, n)
        assert src.used == reps * twin_count(t, p, q, n)
    from ldsr_amd import sim
    assert sim.draw_count(th, n, reps, p, q)[0] == total


def test_argument_validation():
    L = _lib.lib()
    dp = C.POINTER(C.c_double)
    th = (C.c_double * 8)(0.5, 0.1, 0.7, 0.2, 1, 1, 0, 1)
    out = (C.c_double * 64)()

    def batch(n_models=1, T=4, p=1, q=1, theta=th, num_reps=2, first_rep=0):
        return L.ldsr_simulate_batch(0, n_models, T, p, q, None, None, 0, theta, None, num_reps, first_rep, 1, 5,
                                     None, out, None, None)

    for kw, msg in ((dict(T=0), b"T must be"), (dict(num_reps=0), b"num_reps"), (dict(theta=None), b"theta"),
                    (dict(p=0), b"p and q"), (dict(q=0), b"p and q"), (dict(n_models=0), b"n_models"),
                    (dict(first_rep=-1), b"first_rep")):
        assert batch(**kw) == 1 and msg in L.ldsr_last_error(), kw
    assert L.ldsr_simulate_draw_count(1, 0, 1, 1, th, 2, None) == -1
    assert L.ldsr_simulate_draw_count(1, 4, 1, 1, None, 2, None) == -1
    assert L.ldsr_simulate_draw_count(1, 4, 1, 1, th, 0, None) == -1
    assert L.ldsr_simulate_batch_device(0, None, 1, 0, 1, 1, None, None, 0, th, None, 2, 0, 1, 5, None, None,
                                        None, None, None) == 1
    # R-stream mode on the device entry needs the offsets
    assert L.ldsr_simulate_batch_device(0, None, 1, 4, 1, 1, None, None, 0, th, None, 2, 0, 1, 5, th, None,
                                        None, None, None) == 1
    assert b"d_offsets" in L.ldsr_last_error()
    # p, q beyond the EM kernels' 16 are fine here: only the validation runs on the host
    wide = np.zeros(6 + 20 + 24)
    wide[[46, 47, 49]] = 1.0                # Q, R, V1
    assert L.ldsr_simulate_draw_count(1, 5, 20, 24, wide.ctypes.data_as(dp), 1, None) == 2 * (1 + 5 + 5)


def test_python_surface_checks_its_arguments():
    import ldsr_amd
    th = {"A": 0.5, "B": [0.1, 0.2], "C": 0.7, "D": [0.3], "Q": 1.0, "R": 1.0, "mu1": 0.0, "V1": 1.0}
    with pytest.raises(ValueError, match="years"):
        ldsr_amd.LDS_rep(th, num_reps=2)
    with pytest.raises(ValueError, match="v is required"):
        ldsr_amd.LDS_rep(th, u=np.zeros((2, 5)), years=np.arange(5))
    with pytest.raises(ValueError, match="columns"):
        ldsr_amd.LDS_rep(th, u=np.zeros((2, 3)), v=np.zeros((1, 3)), years=np.arange(5))
    with pytest.raises(ValueError, match="p and q"):
        ldsr_amd.LDS_rep(np.zeros(9), years=np.arange(5))
    with pytest.raises(ValueError, match="uniforms"):
        ldsr_amd.simulate_batch(np.zeros(8), None, None, 5, 1, uniforms=np.zeros(3))


def test_no_host_fallback():
    """Without a GPU LDS_rep fails loudly; it never simulates on the host."""
    import ldsr_amd
    if _lib.lib().ldsr_device_count() > 0:
        pytest.skip("GPU present")
    th = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0])
    for kw in (dict(r_seed=1), dict(seed=3), {}):
        with pytest.raises(_lib.LdsrError):
            ldsr_amd.LDS_rep(th, years=np.arange(2), num_reps=1, exp_trans=False, **kw)
