"""LDS_GA without a GPU: the entry exists on every layer, its argument errors surface before any device
call, nothing computes on the host -- and the host model of the specification (tests/ga_model.py, what
the GPU tests compare the device with) has the properties INTEGRATION.md states."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ga_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ga_entry_is_declared_exported_and_bound():
    import ldsr_amd
    from ldsr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ldsr_hip.h")).read()
    assert re.search(r"\bint\s+ldsr_ga_batch\s*\(", hdr)
    assert "ldsr_ga_batch" in _lib.SIGNATURES
    assert hasattr(C.CDLL(_lib.SO_PATH), "ldsr_ga_batch")
    assert callable(ldsr_amd.LDS_GA) and callable(ldsr_amd.ga_batch)
    # the operator constants are the header's, and the model's are the same
    for name, want in (("LDSR_GA_PCROSSOVER", M.PCROSSOVER), ("LDSR_GA_PMUTATION", M.PMUTATION),
                       ("LDSR_GA_MIGRATION_INTERVAL", M.MIGRATION_INTERVAL), ("LDSR_GA_MAX_POP", 1024),
                       ("LDSR_GA_ELITE_PCT", 5), ("LDSR_GA_MIGRATION_PCT", 10)):
        m = re.search(r"#define\s+%s\s+([0-9.]+)" % name, hdr)
        assert m and float(m.group(1)) == want, name


def _call(L, **kw):
    """ldsr_ga_batch on a tiny valid problem (T = 4, p = q = 1) with single arguments replaced."""
    P = 8
    a = dict(device=0, n_series=1, T=4, p=1, q=1, y=(C.c_double * 4)(0.1, -0.2, 0.3, 0.0), u=None, v=None,
             shared_uv=0, lb=(C.c_double * P)(*([0.1] * P)), ub=(C.c_double * P)(*([0.9] * P)), lam=1.0,
             K=2, n=8, maxiter=5, run=3, seed=1, sugg=None, n_sugg=0, theta=(C.c_double * P)(),
             pl=(C.c_double * 1)(), n_gen=(C.c_int * 1)())
    a.update(kw)
    return L.ldsr_ga_batch(a["device"], a["n_series"], a["T"], a["p"], a["q"], a["y"], a["u"], a["v"], a["shared_uv"],
                           a["lb"], a["ub"], a["lam"], a["K"], a["n"], a["maxiter"], a["run"], a["seed"], a["sugg"],
                           a["n_sugg"], a["theta"], a["pl"], a["n_gen"], None, None, None)


def test_ga_argument_errors_without_gpu():
    from ldsr_amd import _lib
    L = _lib.lib()
    P = 8
    EINVAL, EUNSUPPORTED = 1, 2

    def bounds(i, x):
        b = [0.5] * P
        b[i] = x
        return (C.c_double * P)(*b)

    cases = [
        (dict(lb=bounds(3, 0.95)), EINVAL, b"lb must be <= ub"),
        (dict(lb=bounds(0, float("-inf"))), EINVAL, b"finite"),
        (dict(ub=bounds(7, float("nan"))), EINVAL, b"finite"),
        (dict(lb=bounds(1, -1e308), ub=bounds(1, 1e308)), EINVAL, b"finite"),
        (dict(lb=None), EINVAL, b"lb and ub"),
        (dict(n=1), EINVAL, b"pop_per_island"),
        (dict(n=1025), EINVAL, b"pop_per_island"),
        (dict(K=0), EINVAL, b"num_islands"),
        (dict(maxiter=0), EINVAL, b"maxiter"),
        (dict(run=0), EINVAL, b"run"),
        (dict(n_series=0), EINVAL, b"n_series"),
        (dict(T=1), EINVAL, b"T must be"),
        (dict(p=0), EINVAL, b"p and q"),
        (dict(p=17), EUNSUPPORTED, b"not supported"),
        (dict(q=17), EUNSUPPORTED, b"not supported"),
        (dict(y=None), EINVAL, b"y"),
        (dict(n_sugg=9, sugg=(C.c_double * (9 * P))()), EINVAL, b"n_suggestions"),
        (dict(n_sugg=2), EINVAL, b"suggestions"),
        (dict(theta=None), EINVAL, b"theta_best"),
        (dict(lam=float("nan")), EINVAL, b"lambda"),
    ]
    for kw, code, msg in cases:
        rc = _call(L, **kw)
        assert rc == code, (kw.keys(), rc)
        assert msg in L.ldsr_last_error(), (kw.keys(), L.ldsr_last_error())


def test_ga_has_no_host_implementation():
    """A valid call without a GPU fails loudly (the rule of test_no_cpu_fallback)."""
    import ldsr_amd
    from ldsr_amd import _lib, synth
    if _lib.lib().ldsr_device_count() > 0:
        pytest.skip("GPU present")
    y, u, v = synth.make_series(50, 1, 2)
    lb, ub = np.full(9, 0.05), np.full(9, 0.95)
    with pytest.raises(_lib.LdsrError):
        ldsr_amd.ga_batch(y, u, v, lb, ub, maxiter=3)
    with pytest.raises(_lib.LdsrError):
        ldsr_amd.LDS_GA(y, u, v, ub=ub, lb=lb, niter=3, seed=1)
    with pytest.raises(ValueError):
        ldsr_amd.LDS_GA(y, u, v)                    # the reference stops without bounds too
    src = open(os.path.join(ROOT, "ldsr_amd", "ga.py")).read()
    assert "ga_model" not in src and "synth" not in src


def test_model_selection_closed_form_agrees_with_table_search():
    """P(rank r) sums to 1, the cumulative is r (2n - 1 - r) / (n (n - 1)), and the closed-form inverse
    with one step of fix-up is the table search, for every n at every boundary u = c_r and one ulp to
    either side (and at the ends of [0, 1))."""
    for n in range(2, 1025):
        pr = M.selection_probabilities(n)
        assert abs(pr.sum() - 1.0) < 1e-12 and pr[-1] == 0.0 and np.all(np.diff(pr) < 0)
        num = M.cumulative_numerators(n)
        N = n * (n - 1)
        assert num[-1] == N and np.all(np.abs(np.cumsum(pr) - num / N) < 1e-12)
        c = num[:-1] / float(N)
        u = np.concatenate([c, np.nextafter(c, 0.0), np.nextafter(c, 2.0), [0.0, np.nextafter(1.0, 0.0)]])
        u = u[(u >= 0.0) & (u < 1.0)]
        a, b = M.select_rank(u, n), M.select_rank_table(u, n)
        assert np.array_equal(a, b), (n, u[a != b][:4])
        assert a.min() >= 0 and a.max() <= max(n - 2, 0)
    # and the draws follow the probabilities
    n = 10
    r = M.select_rank(M.uniforms(5, 0, 0, 0, 200000), n)
    freq = np.bincount(r, minlength=n) / r.size
    assert np.all(np.abs(freq - M.selection_probabilities(n)) < 5e-3)


def test_model_order_puts_non_finite_last_and_breaks_ties_by_index():
    f = np.array([1.0, np.nan, 3.0, 3.0, -np.inf, np.inf, -2.0, 1.0])
    assert list(M.order(f)) == [2, 3, 0, 7, 6, 1, 4, 5]


def _toy(point):
    return lambda pop: -np.sum((pop - point) ** 2, axis=-1)


def test_model_one_generation_structure():
    """Children of in-bounds parents are in bounds, the e elites reappear unchanged, migration writes
    exactly the last m slots (of the NEXT island, from the best m of this one)."""
    K, n, P = 3, 40, 9
    lb = np.linspace(-1.0, 0.0, P)
    ub = lb + np.linspace(0.5, 2.0, P)
    e, m = M.n_elite(n), M.n_migrants(n)
    assert (e, m) == (2, 4) and (M.n_elite(100), M.n_migrants(100)) == (5, 10)
    assert (M.n_elite(2), M.n_migrants(2)) == (1, 1) and M.n_elite(10) == 1 and M.n_elite(50) == 3
    pop = M.initial_population(11, 0, K, n, lb, ub)
    assert np.all(pop >= lb) and np.all(pop <= ub)
    fit = _toy(0.5 * (lb + ub))(pop)
    for g in (0, 8, 9):
        d = {}
        nxt = M.breed(pop, fit, g, 11, 0, lb, ub, detail=d)
        assert np.all(nxt >= lb) and np.all(nxt <= ub)
        for k in range(K):
            o = M.order(fit[k])
            assert np.array_equal(nxt[k, :e], pop[k, o[:e]])
            assert list(d["kind"][k, :e]) == ["elite"] * e
        migrate = (g + 1) % M.MIGRATION_INTERVAL == 0
        assert np.any(d["kind"] == "migrant") == migrate
        if migrate:
            quiet = M.breed(pop, fit, g, 11, 0, lb, ub)
            other = M.breed(pop[:1], fit[:1], g, 11, 0, lb, ub)       # one island: no migration
            for k in range(K):
                o = M.order(fit[k])
                assert np.array_equal(nxt[(k + 1) % K, n - m:], pop[k, o[:m]])
                assert np.all(d["kind"][k, n - m:] == "migrant") and np.all(d["kind"][k, :n - m] != "migrant")
            # everything but the last m slots is what a single island would have bred
            assert np.array_equal(other[0, :n - m], nxt[0, :n - m]) and np.array_equal(quiet, nxt)
        # uncrossed, unmutated children are copies of a parent
        for k in range(K):
            for i in range(e, n):
                if d["kind"][k, i] == "child" and not d["crossed"][k, i] and d["mutated_gene"][k, i] < 0:
                    assert np.any(np.all(pop[k] == nxt[k, i], axis=1))
    # a degenerate box: nothing can move
    flat = M.initial_population(3, 0, 2, 8, lb, lb)
    assert np.all(flat == lb) and np.all(M.breed(flat, _toy(lb)(flat), 9, 3, 0, lb, lb) == lb)


def test_model_streams_are_counter_mode():
    """A run to maxiter = g + 1 continues the run to maxiter = g; problem s under seed is problem 0
    under seed + s; suggestions fill the first slots of island 0, clipped."""
    K, n, P = 2, 12, 8
    lb, ub = np.full(P, -1.0), np.full(P, 1.0)
    fit = _toy(np.full(P, 0.25))
    a = M.run_ga(fit, 7, 0, K, n, lb, ub, maxiter=12)
    b = M.run_ga(fit, 7, 0, K, n, lb, ub, maxiter=13)
    assert np.array_equal(a["trace"], b["trace"][:12]) and a["n_gen"] == 12 and b["n_gen"] == 13
    assert np.array_equal(M.breed(a["population"], a["fitness"], 11, 7, 0, lb, ub), b["population"])
    c = M.run_ga(fit, 7, 2, K, n, lb, ub, maxiter=12)
    d = M.run_ga(fit, 9, 0, K, n, lb, ub, maxiter=12)
    assert np.array_equal(c["population"], d["population"]) and not np.array_equal(a["population"], c["population"])
    sg = np.array([np.full(P, 0.25), np.full(P, 5.0)])
    p0 = M.initial_population(7, 0, K, n, lb, ub, sg)
    assert np.all(p0[0, 0] == 0.25) and np.all(p0[0, 1] == 1.0)
    assert np.array_equal(p0[0, 2:], M.initial_population(7, 0, K, n, lb, ub)[0, 2:])
    r = M.run_ga(fit, 7, 0, K, n, lb, ub, maxiter=5, suggestions=sg)
    assert r["pl"] == 0.0 and np.all(r["theta"] == 0.25)      # the exact optimum survives as an elite


def test_model_trace_is_monotone_and_the_run_rule_stops_it():
    K, n, P = 4, 30, 10
    lb, ub = np.full(P, 0.0), np.full(P, 1.0)
    r = M.run_ga(_toy(np.linspace(0.2, 0.8, P)), 3, 0, K, n, lb, ub, maxiter=400, run=5)
    t = r["trace"][:r["n_gen"]]
    assert np.all(np.diff(t) >= 0) and np.all(np.isnan(r["trace"][r["n_gen"]:]))
    assert 5 < r["n_gen"] < 400                              # stopped by the run rule ...
    assert np.all(t[-6:] == t[-1]) and t[-7] < t[-1]          # ... exactly 5 generations after the last gain
    assert r["pl"] == t[-1] and r["pl"] > _toy(np.linspace(0.2, 0.8, P))(r["population"]).min()
    assert np.array_equal(_toy(np.linspace(0.2, 0.8, P))(r["theta"][None])[0], r["pl"])
    # nothing can improve after generation 0: run + 1 generations
    flat = M.run_ga(_toy(lb), 3, 0, 2, 8, lb, lb, maxiter=50, run=7)
    assert flat["n_gen"] == 8 and np.all(flat["trace"][:8] == 0.0) and np.all(np.isnan(flat["trace"][8:]))
    # no finite fitness at all: the best stays -inf, theta NaN
    bad = M.run_ga(lambda pop: np.full(pop.shape[:2], np.nan), 3, 0, 2, 8, lb, ub, maxiter=50, run=4)
    assert bad["n_gen"] == 4 and bad["pl"] == -np.inf and np.all(np.isnan(bad["theta"]))
