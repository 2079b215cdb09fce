"""Stochastic replicates on the MI355X (simulate.hip through ldsr_simulate_batch[_device]) against the
numpy twin of the reference's one_LDS_rep (tests/test_simulate_host.py): R-stream mode (set.seed(k);
LDS_rep(...)), counter mode, the reference's branches, layouts and offsets, and the statistics of
the draws themselves."""
import numpy as np
import pytest

import ldsr_amd
from ldsr_amd import rrng
from test_simulate_host import Uniforms, counter_uniforms, twin_count, twin_one_rep

pytestmark = pytest.mark.gpu


def _close_x(got, want):
    """simX / simY: max |diff| <= 1e-11 max(1, max |x|) (the scan reassociates the recursion)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    scale = max(1.0, float(np.max(np.abs(want[ok]), initial=0.0)))
    assert float(np.max(np.abs(got[ok] - want[ok]), initial=0.0)) <= 1e-11 * scale


def _close_q(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def _twin_reps(src, th, p, q, u, v, n, reps, mu=0.0, exp_trans=True):
    out = [twin_one_rep(src, th, p, q, u, v, n, mu, exp_trans) for _ in range(reps)]
    return [np.array([o[k] for o in out]) for k in range(3)]


def test_published_draws_end_to_end():
    """A = B = C = D = 0, Q = R = V1 = 1, n = 2: simX = (x_1, q_1) and simY = r_1..r_2 are the 1st,
    2nd, 4th and 5th draws of set.seed(1); rnorm(5)."""
    th = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0])
    r = ldsr_amd.LDS_rep(th, years=[2001, 2002], num_reps=1, r_seed=1, exp_trans=False)
    np.testing.assert_allclose(r["simX"], [-0.6264538, 0.1836433], rtol=0, atol=5e-8)
    np.testing.assert_allclose(r["simY"], [1.5952808, 0.3295078], rtol=0, atol=5e-8)
    np.testing.assert_array_equal(r["simQ"], r["simY"])
    assert list(r["year"]) == [2001, 2002] and list(r["rep"]) == [1, 1]


@pytest.fixture(scope="module")
def np_fit(npcase):
    c = npcase(1200)                         # u = v = t(NPpc), 3 x 813
    init = ldsr_amd.make_init(3, 3, 20, seed=11)
    fit = ldsr_amd.LDS_EM_restart(c["y"], c["u"], c["v"], init, niter=1000, tol=1e-5)
    return c, fit["theta"]


@pytest.mark.parametrize("exp_trans", [True, False])
def test_vignette_call_matches_the_twin(np_fit, exp_trans):
    """set.seed(100); LDS_rep(lds$theta, u, v, years = 1200:2012, mu = mean(log(Qa))) -- 100 replicates."""
    c, theta = np_fit
    years = np.arange(1200, 2013)
    r = ldsr_amd.LDS_rep(theta, c["u"], c["v"], years=years, num_reps=100, mu=c["mu"], exp_trans=exp_trans,
                         r_seed=100)
    th = ldsr_amd.pack_theta(theta, 3, 3)
    X, Y, Q = _twin_reps(Uniforms(rrng.RUniform(100)), th, 3, 3, c["u"], c["v"], 813, 100, c["mu"], exp_trans)
    _close_x(r["simX"], X.ravel())
    _close_x(r["simY"], Y.ravel())
    _close_q(r["simQ"], Q.ravel())
    assert np.array_equal(r["rep"], np.repeat(np.arange(1, 101), 813))
    assert np.array_equal(r["year"], np.tile(years, 100))


def test_no_input_branch_drops_D_even_with_v():
    th = {"A": 0.8, "B": [0.5, -0.3], "C": 1.1, "D": [0.7], "Q": 0.4, "R": 0.2, "mu1": 5.0, "V1": 2.0}
    v = np.random.default_rng(1).normal(size=(1, 70))
    r = ldsr_amd.LDS_rep(th, None, v, years=np.arange(70), num_reps=3, r_seed=4, mu=0.5)
    pk = ldsr_amd.pack_theta(th, 2, 1)
    X, Y, Q = _twin_reps(Uniforms(rrng.RUniform(4)), pk, 2, 1, None, None, 70, 3, 0.5)
    _close_x(r["simX"], X.ravel())
    _close_x(r["simY"], Y.ravel())
    _close_q(r["simQ"], Q.ravel())


def _models(n_models, p, q, seed):
    g = np.random.default_rng(seed)
    th = np.empty((n_models, 6 + p + q))
    th[:, 0] = g.uniform(-0.9, 0.9, n_models)
    th[:, 1:1 + p] = g.normal(size=(n_models, p)) * 0.3
    th[:, 1 + p] = g.uniform(0.2, 1.5, n_models)
    th[:, 2 + p:2 + p + q] = g.normal(size=(n_models, q)) * 0.3
    th[:, 2 + p + q] = g.uniform(0.1, 1.0, n_models)
    th[:, 3 + p + q] = g.uniform(0.1, 1.0, n_models)
    th[:, 4 + p + q] = 3.0
    th[:, 5 + p + q] = g.uniform(0.5, 2.0, n_models)
    return th


def test_models_in_one_call_equal_calls_per_model_and_consecutive_LDS_rep():
    """Different thetas and mu, per-model inputs: one call == one call per model == consecutive
    LDS_rep calls after one set.seed (an RUniform whose stream continues)."""
    p, q, n, reps = 2, 3, 150, 4
    th = _models(3, p, q, 5)
    th[1, 2 + p + q] = 0.0                   # Q = 0: no q draws, the offsets shift
    th[2, 5 + p + q] = 0.0                   # V1 = 0
    g = np.random.default_rng(2)
    u, v = g.normal(size=(3, p, n + 7)), g.normal(size=(3, q, n + 7))
    mu = np.array([0.1, -0.4, 2.0])
    count, off = ldsr_amd.sim.draw_count(th, n, reps, p, q)
    uni = rrng.RUniform(9).unif_rand(count)
    one = ldsr_amd.simulate_batch(th, u, v, n, reps, mu=mu, uniforms=uni)
    src, rs = Uniforms(rrng.RUniform(9)), rrng.RUniform(9)
    for m in range(3):
        solo = ldsr_amd.simulate_batch(th[m], u[m], v[m], n, reps, mu=mu[m], uniforms=uni[off[m]:off[m + 1]])
        seq = ldsr_amd.LDS_rep(th[m], u[m], v[m], years=np.arange(n), num_reps=reps, mu=mu[m], r_seed=rs)
        X, Y, Q = _twin_reps(src, th[m], p, q, u[m], v[m], n, reps, mu[m])
        for k, want in (("simX", X), ("simY", Y), ("simQ", Q)):
            np.testing.assert_array_equal(one[k][m], solo[k][0])
            np.testing.assert_array_equal(one[k][m].ravel(), seq[k])
        _close_x(one["simX"][m], X)
        _close_x(one["simY"][m], Y)
        _close_q(one["simQ"][m], Q)
    assert src.used == count


@pytest.mark.parametrize("slot,val", [(6, 0.0), (7, 0.0), (9, 0.0), (7, np.nan), (6, -1.0), (9, np.inf)])
def test_zero_and_invalid_variances_shift_the_offsets(slot, val):
    """Q (slot 6), R (7) or V1 (9) of a p = 2, q = 2 theta set to 0 / NaN / negative / Inf: R draws
    nothing for them, so the next model's and replicate's draws move up."""
    p, q, n, reps = 2, 2, 90, 3
    th = _models(2, p, q, 8)
    th[0, slot] = val
    u = np.random.default_rng(3).normal(size=(p, n))
    count, off = ldsr_amd.sim.draw_count(th, n, reps, p, q)
    assert off[1] == reps * twin_count(th[0], p, q, n)
    r = ldsr_amd.simulate_batch(th, u, u, n, reps, uniforms=rrng.RUniform(21).unif_rand(count))
    src = Uniforms(rrng.RUniform(21))
    for m in range(2):
        X, Y, Q = _twin_reps(src, th[m], p, q, u, u, n, reps)
        _close_x(r["simX"][m], X)
        _close_x(r["simY"][m], Y)
        _close_q(r["simQ"][m], Q)


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 127, 128, 129, 813])
def test_series_lengths_around_the_chunk(T):
    p, q, reps = 3, 3, 5
    th = _models(2, p, q, T)
    g = np.random.default_rng(T)
    u, v = g.normal(size=(p, T)), g.normal(size=(q, T))
    count, _ = ldsr_amd.sim.draw_count(th, T, reps, p, q)
    r = ldsr_amd.simulate_batch(th, u, v, T, reps, mu=0.3, uniforms=rrng.RUniform(T).unif_rand(count))
    src = Uniforms(rrng.RUniform(T))
    for m in range(2):
        X, Y, Q = _twin_reps(src, th[m], p, q, u, v, T, reps, 0.3)
        _close_x(r["simX"][m], X)
        _close_x(r["simY"][m], Y)
        _close_q(r["simQ"][m], Q)


def test_wide_inputs_have_no_row_limit():
    p, q, n, reps = 20, 24, 200, 3
    th = _models(2, p, q, 4)
    g = np.random.default_rng(4)
    u, v = g.normal(size=(2, p, n)), g.normal(size=(q, n))       # per-model u, shared v
    count, _ = ldsr_amd.sim.draw_count(th, n, reps, p, q)
    r = ldsr_amd.simulate_batch(th, u, v, n, reps, uniforms=rrng.RUniform(6).unif_rand(count))
    src = Uniforms(rrng.RUniform(6))
    for m in range(2):
        X, Y, Q = _twin_reps(src, th[m], p, q, u[m], v, n, reps)
        _close_x(r["simX"][m], X)
        _close_x(r["simY"][m], Y)
        _close_q(r["simQ"][m], Q)


def test_shared_and_per_model_inputs_agree():
    p, q, n, reps = 2, 2, 100, 3
    th = _models(3, p, q, 12)
    u = np.random.default_rng(5).normal(size=(p, n))
    a = ldsr_amd.simulate_batch(th, u, u, n, reps, seed=77)
    b = ldsr_amd.simulate_batch(th, np.stack([u] * 3), np.stack([u] * 3), n, reps, seed=77)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])


def test_null_outputs_leave_the_others_identical():
    th = _models(2, 3, 3, 1)
    u = np.random.default_rng(6).normal(size=(3, 300))
    full = ldsr_amd.simulate_batch(th, u, u, 300, 7, seed=5, mu=1.0)
    for keep in (("simX",), ("simY",), ("simQ",), ("simX", "simQ")):
        part = ldsr_amd.simulate_batch(th, u, u, 300, 7, seed=5, mu=1.0, outputs=keep)
        assert set(part) == set(keep)
        for k in keep:
            np.testing.assert_array_equal(part[k], full[k])


def test_counter_mode_matches_the_twin_on_regenerated_uniforms():
    p, q, n, reps, seed, first = 3, 3, 813, 6, 123456789, 40
    th = _models(2, p, q, 9)
    g = np.random.default_rng(7)
    u, v = g.normal(size=(p, n)), g.normal(size=(q, n))
    r = ldsr_amd.simulate_batch(th, u, v, n, reps, mu=0.7, seed=seed, first_rep=first)
    for m in range(2):
        k = twin_count(th[m], p, q, n)
        out = [twin_one_rep(Uniforms(counter_uniforms(seed, m, first + j, k)), th[m], p, q, u, v, n, 0.7)
               for j in range(reps)]
        _close_x(r["simX"][m], [o[0] for o in out])
        _close_x(r["simY"][m], [o[1] for o in out])
        _close_q(r["simQ"][m], [o[2] for o in out])


def test_counter_mode_does_not_depend_on_the_split_of_replicates():
    th = _models(2, 3, 3, 10)
    u = np.random.default_rng(8).normal(size=(3, 813))
    whole = ldsr_amd.simulate_batch(th, u, u, 813, 200, seed=31)
    a = ldsr_amd.simulate_batch(th, u, u, 813, 100, seed=31, first_rep=0)
    b = ldsr_amd.simulate_batch(th, u, u, 813, 100, seed=31, first_rep=100)
    for k in whole:
        assert np.array_equal(whole[k], np.concatenate([a[k], b[k]], axis=1))
    one = ldsr_amd.one_LDS_rep(7, th[0], u, u, years=np.arange(813), seed=31)
    assert np.array_equal(one["simX"], whole["simX"][0, 6]) and set(one["rep"]) == {7}


def test_device_entry_equals_host_entry():
    import ctypes as C

    import torch
    from ldsr_amd import _lib
    p, q, n, reps = 3, 3, 813, 50
    th = _models(4, p, q, 14)
    u = np.random.default_rng(9).normal(size=(p, n))
    mu = np.array([0.0, 1.0, -1.0, 2.0])
    L = _lib.lib()
    dev = torch.device("cuda:0")
    d_th = torch.from_numpy(th).to(dev)
    d_u = torch.from_numpy(np.ascontiguousarray(u.T)).to(dev)
    d_mu = torch.from_numpy(mu).to(dev)
    count, off = ldsr_amd.sim.draw_count(th, n, reps, p, q)
    uni = rrng.RUniform(3).unif_rand(count)
    for mode in ("counter", "rstream"):
        outs = [torch.empty((4, reps, n), dtype=torch.float64, device=dev) for _ in range(3)]
        d_uni = torch.from_numpy(uni).to(dev) if mode == "rstream" else None
        d_off = torch.from_numpy(off[:-1].copy()).to(dev) if mode == "rstream" else None
        stream = torch.cuda.current_stream(dev)
        _lib.check(L.ldsr_simulate_batch_device(
            0, C.c_void_p(stream.cuda_stream), 4, n, p, q, d_u.data_ptr(), d_u.data_ptr(), 1, d_th.data_ptr(),
            d_mu.data_ptr(), reps, 0, 1, 99, None if d_uni is None else d_uni.data_ptr(),
            None if d_off is None else d_off.data_ptr(), *[o.data_ptr() for o in outs]))
        torch.cuda.synchronize(dev)
        host = ldsr_amd.simulate_batch(th, u, u, n, reps, mu=mu, seed=99,
                                       uniforms=uni if mode == "rstream" else None)
        for o, k in zip(outs, ("simX", "simY", "simQ")):
            assert np.array_equal(o.cpu().numpy(), host[k]), (mode, k)


def test_statistics_of_the_replicates():
    """20 000 counter-mode replicates of x_{t+1} = 0.7 x_t + q_t (B = D = 0, C = 1): at t = 500 the
    state has mean 0 and variance Q / (1 - A^2); the lag-1 autocorrelation is A; and the draws
    themselves (A = C = 0: y_t = r_t) are N(0, 1) by mean, variance and the 1 % / 99 % quantiles."""
    A, Q, n, reps = 0.7, 0.6, 600, 20000
    th = np.array([A, 0.0, 1.0, 0.0, Q, 0.3, 0.0, 1.0])
    r = ldsr_amd.simulate_batch(th, None, None, n, reps, seed=2024, exp_trans=False)
    x = r["simX"][0]
    var = Q / (1 - A * A)
    xs = x[:, 500]
    assert abs(xs.mean()) < 5 * np.sqrt(var / reps)
    assert abs(xs.var() - var) < 5 * var * np.sqrt(2.0 / reps)
    a, b = x[:, 500], x[:, 501]
    rho = np.corrcoef(a, b)[0, 1]
    assert abs(rho - A) < 5 * (1 - A * A) / np.sqrt(reps)
    th0 = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0])
    z = ldsr_amd.simulate_batch(th0, None, None, 50, reps, seed=7, exp_trans=False)["simY"][0].ravel()
    N = z.size
    assert abs(z.mean()) < 5 / np.sqrt(N)
    assert abs(z.var() - 1.0) < 5 * np.sqrt(2.0 / N)
    for prob, zq in ((0.01, -2.3263478740408408), (0.99, 2.3263478740408408)):
        se = np.sqrt(prob * (1 - prob) / N) / 0.026652           # density of N(0,1) at the 1 % quantile
        assert abs(np.quantile(z, prob) - zq) < 5 * se
