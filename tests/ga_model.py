"""Host model of the island GA behind ldsr_ga_batch -- the specification of INTEGRATION.md ("The
island GA") in numpy, generation by generation.  A helper of the tests, not a test and not part of the
package: the product has no host implementation.  The fitness function is an argument:
fitness(pop [K, n, P]) -> [K, n].  Every random number is synth.uniform(seed + s, stream(k, g), .)."""
import numpy as np

from ldsr_amd import synth

PCROSSOVER = 0.8
PMUTATION = 0.1
MIGRATION_INTERVAL = 10
_M64 = (1 << 64) - 1


def n_elite(n):
    return max(1, (5 * n + 50) // 100)


def n_migrants(n):
    return max(1, 10 * n // 100)


def stream_word(k, g):
    """Stream of island k, generation g; g = -1 is the initial population."""
    return (k << 32) | (g + 1)


def draw_offsets(n, P):
    """Index ranges of a generation's stream: selection [n], crossover decision [n/2] (at n),
    crossover weights [n P] (pair j, gene c at j P + c), mutation decision [n], gene [n], value [n]."""
    return {"sel": 0, "cross": n, "weight": 2 * n, "mut": 2 * n + n * P, "gene": 3 * n + n * P,
            "value": 4 * n + n * P, "total": 5 * n + n * P}


def uniforms(seed, s, k, g, count):
    return synth.uniform((seed + s) & _M64, stream_word(k, g), count)


def clip(x, lb, ub):
    return np.fmin(np.fmax(x, lb), ub)


def in_box(u, lb, ub):
    return clip(lb + u * (ub - lb), lb, ub)


def selection_probabilities(n):
    r = np.arange(1, n + 1, dtype=np.float64)
    return (2.0 / n) * (1.0 - (r - 1.0) / (n - 1.0))


def cumulative_numerators(n):
    """c_r n (n - 1) = r (2 n - 1 - r), r = 1 .. n: integers."""
    r = np.arange(1, n + 1, dtype=np.int64)
    return r * (2 * n - 1 - r)


def select_rank(u, n):
    """0-based rank selected by the uniform(s) u: the smallest r with u n (n-1) < r (2n-1-r), by the
    closed-form root and one step of fix-up (what the device does)."""
    u = np.asarray(u, dtype=np.float64)
    b = float(2 * n - 1)
    w = u * float(n * (n - 1))
    r = np.floor((b - np.sqrt(b * b - 4.0 * w)) * 0.5).astype(np.int64) + 1
    r = np.clip(r, 1, n - 1)
    down = (r > 1) & (w < ((r - 1) * (2 * n - r)).astype(np.float64))
    up = ~down & (r < n - 1) & ~(w < (r * (2 * n - 1 - r)).astype(np.float64))
    return r - down + up - 1


def select_rank_table(u, n):
    """The same by searching the table of cumulative numerators."""
    w = np.asarray(u, dtype=np.float64) * float(n * (n - 1))
    return np.searchsorted(cumulative_numerators(n).astype(np.float64), w, side="right")


def order(f):
    """Indices of one island by fitness: finite ones first, descending, ties by lower index; the
    non-finite ones after them by index."""
    f = np.asarray(f, dtype=np.float64)
    idx = np.arange(f.size)
    fin = np.isfinite(f)
    key = np.where(fin, -f, 0.0)
    return np.lexsort((idx, key, ~fin))


def initial_population(seed, s, K, n, lb, ub, suggestions=None):
    P = lb.size
    pop = np.empty((K, n, P))
    for k in range(K):
        pop[k] = in_box(uniforms(seed, s, k, -1, n * P).reshape(n, P), lb, ub)
    if suggestions is not None and len(suggestions):
        sg = np.asarray(suggestions, dtype=np.float64).reshape(-1, P)
        pop[0, :sg.shape[0]] = clip(sg, lb, ub)
    return pop


def new_state(P):
    return {"best": -np.inf, "theta": np.full(P, np.nan), "stall": 0, "done": False, "n_gen": 0}


def bookkeeping(state, pop, fit, g, maxiter, run):
    """Step 3.  Returns the new state (a copy)."""
    st = dict(state, theta=state["theta"].copy())
    flat = fit.reshape(-1)
    fin = np.isfinite(flat)
    improved = False
    if fin.any():
        cand = np.where(fin, flat, -np.inf)
        bi = int(np.argmax(cand))          # first = lowest (island, index) on ties
        if flat[bi] > st["best"]:
            improved = True
            st["best"] = float(flat[bi])
            st["theta"] = pop.reshape(-1, pop.shape[-1])[bi].copy()
    st["stall"] = 0 if improved else st["stall"] + 1
    st["n_gen"] = g + 1
    st["done"] = g + 1 >= maxiter or st["stall"] >= run
    return st


def breed(pop, fit, g, seed, s, lb, ub, detail=None):
    """Steps 2 and 4-8: the next population [K, n, P] from generation g's and its fitness.  detail (a
    dict) receives per island what became of every slot: kind [K, n] ('elite', 'child', 'migrant'),
    crossed [K, n], mutated gene [K, n] (-1: none)."""
    K, n, P = pop.shape
    e, m = n_elite(n), n_migrants(n)
    off = draw_offsets(n, P)
    nxt = np.empty_like(pop)
    orders = [order(fit[k]) for k in range(K)]
    kind = np.full((K, n), "child", dtype=object)
    crossed_all = np.zeros((K, n), dtype=bool)
    mgene_all = np.full((K, n), -1)
    for k in range(K):
        U = uniforms(seed, s, k, g, off["total"])
        o = orders[k]
        nxt[k, :e] = pop[k, o[:e]]
        kind[k, :e] = "elite"
        for i in range(n - e):
            j = i >> 1
            x1 = pop[k, o[int(select_rank(U[off["sel"] + 2 * j], n))]]
            x2 = pop[k, o[int(select_rank(U[off["sel"] + 2 * j + 1], n))]]
            second = bool(i & 1)
            crossed = U[off["cross"] + j] < PCROSSOVER
            x = (x2 if second else x1).copy()
            if crossed:
                a = U[off["weight"] + j * P:off["weight"] + (j + 1) * P]
                wa, wb = (1.0 - a, a) if second else (a, 1.0 - a)
                x = clip(wa * x1 + wb * x2, lb, ub)
            if U[off["mut"] + i] < PMUTATION:
                c = min(int(U[off["gene"] + i] * float(P)), P - 1)
                x[c] = in_box(U[off["value"] + i], lb[c], ub[c])
                mgene_all[k, e + i] = c
            crossed_all[k, e + i] = crossed
            nxt[k, e + i] = x
    if K > 1 and (g + 1) % MIGRATION_INTERVAL == 0:
        for k in range(K):
            nxt[(k + 1) % K, n - m:] = pop[k, orders[k][:m]]
            kind[(k + 1) % K, n - m:] = "migrant"
    if detail is not None:
        detail.update(kind=kind, crossed=crossed_all, mutated_gene=mgene_all)
    return nxt


def run_ga(fitness, seed, s, K, n, lb, ub, maxiter, run=100, suggestions=None):
    """The whole run of problem s.  Returns dict: theta, pl, n_gen, trace [maxiter] (NaN beyond n_gen),
    population / fitness of the last evaluated generation."""
    lb = np.asarray(lb, dtype=np.float64)
    ub = np.asarray(ub, dtype=np.float64)
    pop = initial_population(seed, s, K, n, lb, ub, suggestions)
    st = new_state(lb.size)
    trace = np.full(maxiter, np.nan)
    g = 0
    while True:
        fit = np.asarray(fitness(pop), dtype=np.float64)
        st = bookkeeping(st, pop, fit, g, maxiter, run)
        trace[g] = st["best"]
        if st["done"]:
            break
        pop = breed(pop, fit, g, seed, s, lb, ub)
        g += 1
    return {"theta": st["theta"], "pl": st["best"], "n_gen": st["n_gen"], "trace": trace,
            "population": pop, "fitness": fit}
