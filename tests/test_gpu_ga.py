"""LDS_GA on the GPU (run with -m gpu), all through the public Python entry.  The fitness is checked
against the CPU oracle (Kalman_smoother with stdlik = FALSE and the ssq of R/LDS_GA.R:34-39 in numpy,
bar: |d| <= 1e-6 |ref| + 1e-9); the generation step, the bookkeeping and the stop rule against the host
model of the specification (tests/ga_model.py) fed with the DEVICE's fitness values, so that a 1e-12
difference in a fitness cannot flip a rank."""
import numpy as np
import pytest

import ga_model as M
from conftest import parity_close

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-9


@pytest.fixture(scope="module")
def eng():
    import ldsr_amd
    from ldsr_amd import _lib
    assert _lib.lib().ldsr_device_count() >= 1, "no GPU visible"
    return ldsr_amd


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def _box(p, q, neg_var=False):
    """Bounds of a packed theta: A, C in [0.05, 0.95], B, D in [-1, 1], Q, R, V1 in [0.05, 2], mu1 in [-1, 1]."""
    lo = -0.3 if neg_var else 0.05
    lb = np.concatenate([[0.05], np.full(p, -1.0), [0.05], np.full(q, -1.0), [lo, lo, -1.0, 0.05]])
    ub = np.concatenate([[0.95], np.full(p, 1.0), [0.95], np.full(q, 1.0), [2.0, 2.0, 1.0, 2.0]])
    return lb, ub


def _oracle_fitness(O, y, u, v, pop, lam):
    p = u.shape[0]
    out = np.empty(pop.shape[:-1])
    for idx in np.ndindex(*out.shape):
        th = pop[idx]
        with np.errstate(all="ignore"):
            ks = O.kalman_smoother(y, u, v, th, stdlik=False)
            X = np.asarray(ks["X"]).reshape(-1)
            ssq = np.sum((X[1:] - th[0] * X[:-1] - th[1:1 + p] @ u[:, :-1]) ** 2)
            out[idx] = ks["lik"] - lam * ssq
    return out


_FITNESS_CASES = [(p, q, T, mask, False) for (p, q) in ((1, 1), (1, 2), (3, 3), (4, 8), (9, 2))      # p = 9: beyond the scan kernel
                  for T in (50, 813) for mask in ("dense", "paleo")]
_FITNESS_CASES.append((1, 2, 50, "dense", True))       # a box that admits negative variances: non-finite fitness


@pytest.mark.parametrize("p,q,T,mask,neg_var", _FITNESS_CASES)
def test_fitness_of_the_returned_population_matches_the_oracle(eng, O, p, q, T, mask, neg_var):
    """The case (4, 8, 50, paleo) has 5 observations for 8 columns of v: Svv is singular, the scan kernel
    (which whitens v by it) has no answer, and the GA runs that series' cells on the serial smoother."""
    from ldsr_amd import synth
    y, u, v = synth.make_series(T, p, q, series_id=3, mask=mask)
    lb, ub = _box(p, q, neg_var)
    lam = 0.7
    r = eng.ga_batch(y, u, v, lb, ub, lambda_=lam, num_islands=2, pop_per_island=24, maxiter=1 if neg_var else 3,
                     seed=17, return_population=True)
    pop, fit = r["population"][0], r["fitness"][0]
    assert np.all(pop >= lb) and np.all(pop <= ub)
    ref = _oracle_fitness(O, y, u, v, pop, lam)
    fin = np.isfinite(ref)
    print("fitness %s: %d of %d finite, max rel err %.3g" % (
        (p, q, T, mask), fin.sum(), fin.size, np.max(np.abs(fit[fin] - ref[fin]) / (np.abs(ref[fin]) + 1e-300), initial=0.0)))
    assert np.array_equal(np.isfinite(fit), fin)
    assert parity_close(fit[fin], ref[fin], RTOL, ATOL)
    assert fin.any() and (not fin.all() if neg_var else True)     # (each case tests what it is there for)


def _run(eng, y, u, v, lb, ub, maxiter, **kw):
    kw.setdefault("return_population", True)
    return eng.ga_batch(y, u, v, lb, ub, maxiter=maxiter, **kw)


def test_generations_and_bookkeeping_follow_the_specification(eng):
    """Runs to maxiter = 1 .. 12 with one seed give every generation's population and device fitness
    (a run to g + 1 continues the run to g).  The model's step from generation g must give the device's
    generation g + 1 -- g = 0, 1, 8, 9 (crosses a migration), 10 among them -- exactly for elites,
    migrants, mutated genes and uncrossed children, within 4 ulp of max(|lb|, |ub|) for crossed genes;
    and the model's bookkeeping on those fitness values gives the device's pl, theta, trace, n_gen."""
    from ldsr_amd import synth
    p, q, K, n, G, seed, lam = 1, 2, 3, 20, 12, 5, 1.0
    y, u, v = synth.make_series(200, p, q, series_id=7)
    lb, ub = _box(p, q)
    runs = [_run(eng, y, u, v, lb, ub, g + 1, lambda_=lam, num_islands=K, pop_per_island=n, seed=seed, run=100)
            for g in range(G)]
    assert np.array_equal(runs[0]["population"][0], M.initial_population(seed, 0, K, n, lb, ub))
    st = M.new_state(lb.size)
    trace = np.full(G, np.nan)
    tol = 4 * np.spacing(np.maximum(np.abs(lb), np.abs(ub)))
    for g in range(G):
        r = runs[g]
        pop, fit = r["population"][0], r["fitness"][0]
        st = M.bookkeeping(st, pop, fit, g, G, 100)
        trace[g] = st["best"]
        # the run that stopped here reports the model's bookkeeping
        assert r["n_gen"][0] == g + 1 and r["pl"][0] == st["best"]
        assert np.array_equal(r["theta"][0], st["theta"])
        assert np.array_equal(r["trace"][0], trace[:g + 1])
        if g + 1 < G:
            d = {}
            want = M.breed(pop, fit, g, seed, 0, lb, ub, detail=d)
            got = runs[g + 1]["population"][0]
            assert np.all(np.abs(got - want) <= tol), (g, np.max(np.abs(got - want)))
            exact = np.ones(want.shape, dtype=bool)
            child = d["kind"] == "child"
            exact[child & d["crossed"]] = False
            for k, i in zip(*np.nonzero(d["mutated_gene"] >= 0)):
                exact[k, i, d["mutated_gene"][k, i]] = True
            assert np.array_equal(got[exact], want[exact]), g
            assert np.any(d["kind"] == "migrant") == (g == 9)
            print("generation %d -> %d: max |device - model| = %.3g over %d crossed genes" % (
                g, g + 1, np.max(np.abs(got - want)), (~exact).sum()))
    assert np.all(np.diff(trace) >= 0)


def test_runs_are_deterministic_and_problems_independent(eng):
    from ldsr_amd import synth
    p, q, T, K, n = 1, 2, 120, 2, 16
    lb, ub = _box(p, q)
    y0, u, v = synth.make_series(T, p, q, series_id=1)
    Y = np.stack([y0, y0, y0])
    Y[1, 10:30] = np.nan
    Y[2, :60] = np.nan
    kw = dict(lambda_=1.0, num_islands=K, pop_per_island=n, run=100)
    keys = ("theta", "pl", "n_gen", "trace", "population", "fitness")
    a = _run(eng, Y, u, v, lb, ub, 25, seed=40, **kw)
    b = _run(eng, Y, u, v, lb, ub, 25, seed=40, **kw)
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for s in range(3):      # problem s under seed is problem 0 under seed + s
        one = _run(eng, Y[s], u, v, lb, ub, 25, seed=40 + s, **kw)
        for k in keys:
            assert np.array_equal(a[k][s], one[k][0], equal_nan=True), (s, k)
    assert not np.array_equal(a["population"][0], a["population"][1])

    # Problem 0 stops early by the run rule while problem 1 runs to maxiter = 40.  (The bounds are one
    # box per call, so the early stop comes from the data, not from lb == ub: problem 0's series has no
    # observation and the penalty is off, so no theta is better than another.)
    Y2 = np.stack([np.full(T, np.nan), y0])
    kw2 = dict(lambda_=0.0, num_islands=K, pop_per_island=n, run=6)
    two = _run(eng, Y2, u, v, lb, ub, 40, seed=9, **kw2)
    g0 = int(two["n_gen"][0])
    assert g0 in (6, 7) and g0 < 40
    short = _run(eng, Y2[0], u, v, lb, ub, g0, seed=9, **kw2)
    other = _run(eng, Y2[1], u, v, lb, ub, 40, seed=10, **kw2)
    for k in keys:
        if k == "trace":
            assert np.array_equal(two[k][0, :g0], short[k][0], equal_nan=True)
            assert np.all(np.isnan(two[k][0, g0:]))
        else:
            assert np.array_equal(two[k][0], short[k][0], equal_nan=True), k     # generations past its stop were no-ops
        assert np.array_equal(two[k][1], other[k][0], equal_nan=True), k


def test_stop_rule_with_a_degenerate_box(eng):
    """lb == ub at a theta of finite fitness: generation 0 sets the best, nothing can improve, the run
    stops after `run` more generations -- the n_gen of the host model -- well before maxiter."""
    from ldsr_amd import synth
    p, q = 1, 2
    y, u, v = synth.make_series(150, p, q, series_id=2)
    th = np.array([0.7, 0.2, 0.5, 0.1, -0.1, 0.4, 0.2, 0.0, 1.0])
    pl = eng.penalized_likelihood(y, u, v, th, 1.0)[0]
    assert np.isfinite(pl)
    for run in (7, 40):     # (40: the stop falls behind the first chunk of enqueued generations)
        r = _run(eng, y, u, v, th, th, 200, lambda_=1.0, num_islands=2, pop_per_island=10, run=run, seed=1)
        model = M.run_ga(lambda pop: np.full(pop.shape[:2], pl), 1, 0, 2, 10, th, th, 200, run=run)
        assert r["n_gen"][0] == model["n_gen"] == run + 1
        assert np.all(r["trace"][0, :run + 1] == pl) and np.all(np.isnan(r["trace"][0, run + 1:]))
        assert r["pl"][0] == pl and np.array_equal(r["theta"][0], th)
        assert np.all(r["population"][0] == th) and np.all(r["fitness"][0] == pl)


def test_elitism_keeps_a_suggested_em_winner(eng):
    from ldsr_amd import synth
    p, q, lam = 1, 2, 1.0
    y, u, v = synth.make_series(200, p, q, series_id=7)
    init = [eng.unpack_theta(t, p, q) for t in synth.make_init_packed(p, q, 16, seed=3)]
    em = eng.LDS_EM_restart(y, u, v, init, niter=200, tol=1e-5)
    th = eng.pack_theta(em["theta"], p, q)
    lb, ub = np.minimum(_box(p, q)[0], th - 0.5), np.maximum(_box(p, q)[1], th + 0.5)
    pl_em = eng.penalized_likelihood(y, u, v, th, lam)[0]
    r = _run(eng, y, u, v, lb, ub, 30, lambda_=lam, num_islands=4, pop_per_island=50, seed=77, suggestions=th[None])
    print("EM winner pl %.6f, GA seeded with it %.6f after %d generations" % (pl_em, r["pl"][0], r["n_gen"][0]))
    assert r["pl"][0] >= pl_em
    t = r["trace"][0, :r["n_gen"][0]]
    assert t[0] >= pl_em and np.all(np.diff(t) >= 0)
    assert np.all(r["population"] >= lb) and np.all(r["population"] <= ub)
    unseeded = _run(eng, y, u, v, lb, ub, 30, lambda_=lam, num_islands=4, pop_per_island=50, seed=77)
    assert np.all(np.diff(unseeded["trace"][0, :unseeded["n_gen"][0]]) >= 0)
    assert np.all(unseeded["population"] >= lb) and np.all(unseeded["population"] <= ub)


def test_lds_ga_returns_the_reference_list(eng):
    from ldsr_amd import synth
    p, q = 1, 2
    y, u, v = synth.make_series(200, p, q, series_id=7)
    lb, ub = _box(p, q)
    r = eng.LDS_GA(y, u, v, lambda_=1, ub=ub, lb=lb, num_islands=2, pop_per_island=20, niter=15, seed=4)
    assert sorted(r) == ["fit", "lik", "pl", "theta"]            # R/LDS_GA.R:78-81
    assert sorted(r["theta"]) == sorted(["A", "B", "C", "D", "Q", "R", "mu1", "V1"])
    ks = eng.Kalman_smoother(y, u, v, r["theta"])
    for k in "XYVJ":
        assert np.array_equal(r["fit"][k], ks[k])
    assert r["fit"]["lik"] == ks["lik"] == r["lik"]
    b = eng.ga_batch(y, u, v, lb, ub, num_islands=2, pop_per_island=20, maxiter=15, seed=4)
    assert r["pl"] == b["pl"][0] and np.array_equal(eng.pack_theta(r["theta"], p, q), b["theta"][0])
    assert r["pl"] == eng.penalized_likelihood(y, u, v, b["theta"][0], 1.0)[0]
