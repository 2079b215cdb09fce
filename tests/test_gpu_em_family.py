"""Every compiled EM kernel of the scan family and of the pair family -- one case per non-FIT name of
ldsr_kernel_inventory() -- against the fp64 oracle AND against the extended-precision EM loop of
tests/smoother_model.py (em(), numpy.longdouble).  tests/test_em_model_host.py proves that the table and
UNREACHABLE together are the inventory without the FIT forms.

A case is derived by rule from the kernel's name (em_cases): one launch of 13 cells on one series at the
member's smallest interior length, with the `ragged` mask of the smoother table (steady members: once dense, once
ragged), make_init_packed rows (work-queue cases: four of them warm starts that stop after three or four
iterations; dense steady cases: two slow cells), niter = 6 at tol = 0 for static kernels and niter = 12 at
tol = 1e-5 for work-queue kernels, through the explicit algorithm of em_batch.

LEAD forms (em_pair_kernel<..., true>) run through AUTO: an all-missing lead, then a ragged tail.  The tail is a
multiple of 16 (em_plan.hip lead_tail), so at 16 lanes and for L = 4, 8, 16 every tail of a member fills its lanes
evenly: those members take their smallest tail, the others their smallest interior one.  The lead is the shortest
the plan accepts for the kernel.  Three ways to the launch (lead_case):
 * "child": a fresh child process with LDSR_FORCE_FILL=1, where the launch plan is the ldsr_em_plan_lead query;
   one child per (LPC, PP) group, one at a time, each with its own time limit (lead_runs);
 * "long": 32-lane members with tails <= 256 steps and padded p > 2 or q > 4, which the switch never selects
   because four cells per wave fit as well (or selects only behind a lead longer than this): T = 1536 without the switch, where 13 cells fill two cells per wave
   but not four (em_plan.hip fills());
 * "many": the same members with p <= 2, q <= 4 and the work queue: 4096 cells, tol > 0 and a lead below 1024
   steps fill two cells per wave (3569 cells on 256 CUs) but not four (7137).  The oracle checks every cell, the
   model the first 13.
The static 32-lane members with p <= 2, q <= 4 that no lead reaches are UNREACHABLE.

Per case:
 1. ldsr_last_em_kernel names the case's kernel;
 2. the project's bar against the oracle: identical status and n_iter, then theta, lik and the liks trace within
    1e-6 |ref| + 1e-9;
 3. the gap to the longdouble model is at most a TENTH of that bar (DEVICE_CAP, the smoother family's rule:
    a fraction of the project's own bar, not a measured figure).  tests/test_em_model_host.py proves without a GPU
    that on every case the oracle sits within a thousandth of the bar of the model, that oracle, float64 model and
    longdouble model stop at the same iterations, and that no stop decision is nearer to tol than four times
    the device's cap;
 4. return_liks on and off give the same bits, and the reversed batch gives the reversed outputs.

Each test prints `GAP <case id> device ... oracle ...` (profiles/r11_em_gaps.txt is that output of one run)."""
import ctypes as C
import functools

import numpy as np
import pytest

import smoother_model as SM
from conftest import parity_close
from test_gpu_smoother_family import (DEVICE_CAP, ORACLE_CAP, RTOL, ATOL, apply_mask, gap, member_lengths,
                                      nan_for_inf)

SCAN, PAIR, QUAD = 2, 3, 4            # LDSR_ALGO_SCAN, _PAIR (two cells per wave), _QUAD (four)
N_CELLS = 13
STATIC = (6, 0.0)                     # niter, tol of a static-schedule case
QUEUE = (12, 1e-5)                    # ... of a work-queue case
WARM_ROWS = (1, 4, 8, 11)             # work-queue cases: rows that start at the oracle's converged theta
SLOW_ROWS = ((3, 0.97, 0.03), (6, 0.80, 0.15))      # dense steady cases: row, A, C (test_gpu_pair.py's slow cells)
SEED_ORDER = tuple(range(12))             # a case that misses a condition of test_em_model_host.py takes the next one
SEEDS = {                             # case id -> position in SEED_ORDER, where it is not the first
    "em_pair_kernel<4, 1, 3, 32, true, true>": 1,
    "em_pair_kernel<4, 2, 3, 32, true, true>": 1,
    "em_pair_kernel<4, 4, 3, 32, true, true>": 1,
    "em_pair_kernel<4, 8, 3, 32, true, true>": 1,
    "em_pair_kernel<8, 2, 3, 32, true, true>": 1,
    "em_pair_kernel<8, 8, 3, 32, true, true>": 3,
    "em_pair_kernel<8, 1, 4, 32, true, true>": 2,
    "em_pair_kernel<8, 2, 4, 32, true, true>": 2,
    "em_pair_kernel<8, 4, 4, 32, true, true>": 1,
    "em_pair_kernel<8, 8, 4, 32, true, true>": 2,
    "em_pair_kernel<2, 2, 5, 32, true, true>": 1,
    "em_pair_kernel<2, 4, 5, 32, true, true>": 6,
    "em_pair_kernel<1, 2, 6, 32, true, true>": 1,
    "em_pair_kernel<2, 1, 6, 32, true, true>": 4,
    "em_pair_kernel<2, 2, 6, 32, true, true>": 5,
    "em_pair_kernel<2, 4, 6, 32, true, true>": 1,
    "em_pair_kernel<2, 4, 7, 32, true, true>": 1,
    "em_pair_kernel<1, 2, 8, 32, true, true>": 1,
    "em_pair_kernel<1, 1, 15, 32, true, true>": 1,
    "em_pair_kernel<1, 4, 15, 32, true, true>": 1,
    "em_pair_kernel<1, 2, 11, 16, true, true>": 1,
    "em_pair_kernel<1, 4, 11, 16, true, true>": 1,
    "em_pair_kernel<1, 2, 15, 16, true, true>": 1,
    "em_pair_kernel<1, 1, 16, 16, true, true>": 1,
}


N_MANY = 4096                         # cells of a "many" launch
LEAD_T_LONG = 1536                    # em_plan.hip fills(): from here a lead fills two cells per wave at any size

# Kernels no launch through the public entries and the documented switches runs: static LEAD forms at two cells
# per wave with tails <= 256 steps and p <= 2, q <= 4.  For them lead_quad() holds whenever lead_fits(.., 32)
# does up to T = 8192, and with tol = 0 fills(tail, 16) holds whenever fills(tail, 32) does (half as many
# workgroups against half the threshold), so the plan always takes four cells per wave.  (Their work-queue forms
# run in the "many" cases; p = 2 from L = 5 on is reached by leads too long for four cells per wave.)
UNREACHABLE = (
    "em_pair_kernel<1, 1, 3, 32, false, true>",
    "em_pair_kernel<1, 2, 3, 32, false, true>",
    "em_pair_kernel<1, 4, 3, 32, false, true>",
    "em_pair_kernel<2, 1, 3, 32, false, true>",
    "em_pair_kernel<2, 2, 3, 32, false, true>",
    "em_pair_kernel<2, 4, 3, 32, false, true>",
    "em_pair_kernel<1, 1, 4, 32, false, true>",
    "em_pair_kernel<1, 2, 4, 32, false, true>",
    "em_pair_kernel<1, 4, 4, 32, false, true>",
    "em_pair_kernel<2, 1, 4, 32, false, true>",
    "em_pair_kernel<2, 2, 4, 32, false, true>",
    "em_pair_kernel<2, 4, 4, 32, false, true>",
    "em_pair_kernel<1, 1, 5, 32, false, true>",
    "em_pair_kernel<1, 2, 5, 32, false, true>",
    "em_pair_kernel<1, 4, 5, 32, false, true>",
    "em_pair_kernel<1, 1, 6, 32, false, true>",
    "em_pair_kernel<1, 2, 6, 32, false, true>",
    "em_pair_kernel<1, 4, 6, 32, false, true>",
    "em_pair_kernel<1, 1, 7, 32, false, true>",
    "em_pair_kernel<1, 2, 7, 32, false, true>",
    "em_pair_kernel<1, 4, 7, 32, false, true>",
    "em_pair_kernel<1, 1, 8, 32, false, true>",
    "em_pair_kernel<1, 2, 8, 32, false, true>",
    "em_pair_kernel<1, 4, 8, 32, false, true>",
)


def inventory():
    from ldsr_amd import _lib
    L = _lib.lib()
    n = L.ldsr_kernel_inventory(None, 0)
    buf = C.create_string_buffer(n)
    L.ldsr_kernel_inventory(buf, n)
    return [k for k in buf.value.decode().split("\n") if k]


def parse(name):
    """"em_scan_kernel<PP, QQ, L, W, QUEUE, GIMG, FIT>" / "em_pair_kernel<PP, QQ, L, LPC, QUEUE, LEAD>" -> dict"""
    fam, args = name[:-1].split("<")
    a = args.split(", ")
    k = {"family": fam[3:7], "PP": int(a[0]), "QQ": int(a[1]), "L": int(a[2]), "n": int(a[3]), "queue": a[4] == "true"}
    if k["family"] == "scan":
        k["gimg"], k["fit"] = a[5] == "true", a[6] == "true"
    else:
        k["lead"] = a[5] == "true"
    return k


def pair_chunk(T, lpc, Ls):
    """pair_plan's chunk length (kernels_scan.hip): the first compiled L with T <= lpc L whose lanes come out
    even, 1 <= rp <= nl (nl = ceil(T / L) active lanes, the first rp of them with L steps, the others L - 1)"""
    for L in Ls:
        if T <= lpc * L:
            nl = -(-T // L)
            if 1 <= T - nl * (L - 1) <= nl:
                return L
    return 0


def pair_length(L, lpc, Ls):
    """the smallest interior T of a pair member: 64 < T (pair_plan refuses T <= 64, kernels_scan.hip), the plan
    maps it to L, L does not divide it, and rp is neither 1 nor nl.  pair_plan's code has no L (L - 1) <= T
    clause, only 1 <= rp <= nl and T <= LPC L: at 16 lanes T = 258 runs L = 17 (rp = 2) although 17 * 16 = 272.
    tests/test_em_model_host.py asserts T <= LPC L, and its plan query catches a drift from pair_plan."""
    for T in range(65, lpc * L + 1):
        nl = -(-T // L)
        if pair_chunk(T, lpc, Ls) == L and T % L and (T - nl * (L - 1)) not in (1, nl):
            return T
    raise AssertionError("no interior length for pair member (%d, %d)" % (L, lpc))


def pair_steady(L, lpc, PP, QQ):
    """em_pair_impl.h pair_steady(): the members whose fully observed cells take the steady body"""
    K = 1 + PP + QQ
    img = lpc * 2 * (L * (K // 2) + (K & 1) * ((L + 1) // 2))
    return lpc == 32 and L >= 24 and (img + 8 * 64 * (L - 1) + lpc * 2 * ((K + 1) // 2)) * 8 <= 160 * 1024


def _width(PP, L):
    """even L: the padded width itself; odd L: 3 for 4 and 5 for 8 (the identity padding)"""
    return PP if L % 2 == 0 or PP <= 2 else PP // 2 + 1


def _case(name, k, T, algo, mask, sched, tag=""):
    cid = name + tag
    return {"id": cid, "kernel": name, "T": T, "p": _width(k["PP"], k["L"]), "q": _width(k["QQ"], k["L"]),
            "algo": algo, "mask": mask, "niter": sched[0], "tol": sched[1], "n": N_CELLS, "mode": "direct",
            "steady": k["family"] == "pair" and pair_steady(k["L"], k["n"], k["PP"], k["QQ"]),
            "seed": SEED_ORDER[SEEDS.get(cid, 0)]}


def _plan_lead(T, p, q, sched, lead_steps):
    from ldsr_amd import _lib
    buf = C.create_string_buffer(160)
    a = _lib.lib().ldsr_em_plan_lead(T, p, q, sched[0], sched[1], 0, lead_steps, buf, 160)
    return buf.value.decode() if a > 0 else ""


def _first_lead(name, tail, p, q, sched):
    """the shortest lead (T - tail >= 191: the host entry counts the tail's missing first step too, 192) for
    which a device-filling AUTO launch runs `name`; 0 if there is none up to T = 8192.  The leads a kernel accepts
    form runs far longer than 16 steps: a stride of 16, then back to the run's first."""
    for lead in list(range(191, 208)) + list(range(208, 8192 - tail + 1, 16)):
        if _plan_lead(tail + lead, p, q, sched, lead + 1) == name:
            while lead > 191 and _plan_lead(tail + lead - 1, p, q, sched, lead) == name:
                lead -= 1
            return lead
    return 0


def lead_case(name, k, Ls, sched, tag=""):
    """-> the case of a LEAD name and schedule, or None (UNREACHABLE)"""
    lpc, L, p, q = k["n"], k["L"], _width(k["PP"], k["L"]), _width(k["QQ"], k["L"])
    tails = [t for t in range(80, lpc * 16 + 1, 16) if pair_chunk(t, lpc, Ls) == L]
    inner = [t for t in tails if t % L and (t - -(-t // L) * (L - 1)) not in (1, -(-t // L))]
    tail = (inner or tails)[0]
    c = _case(name, k, 0, 0, "lead+ragged", sched, tag)
    c.update(tail=tail, n=N_CELLS, group="%d-%d" % (lpc, k["PP"]))
    lead = _first_lead(name, tail, p, q, sched)
    long_ok = lpc == 32 and tail <= 256 and (k["PP"] > 2 or k["QQ"] > 4)
    if lead and not (long_ok and tail + lead > LEAD_T_LONG):      # (the shorter lead of the two ways)
        c.update(mode="child", T=tail + lead)
    elif long_ok:
        c.update(mode="long", T=LEAD_T_LONG)
    elif lpc == 32 and tail <= 256 and sched[1] > 0:
        c.update(mode="many", T=tail + 191, n=N_MANY)
    else:
        return None
    return c


@functools.lru_cache(maxsize=None)
def em_cases():
    """One case per name of the inventory that is neither a FIT form nor UNREACHABLE, in the inventory's
    order; a second one (dense) for the steady pair members, and a static call (tol = 0) for the scan members
    that exist as work-queue forms only."""
    names = inventory()
    pair_Ls = {lpc: sorted(set(k["L"] for k in map(parse, names) if k["family"] == "pair" and k["n"] == lpc))
               for lpc in (32, 16)}
    out = []
    for name in names:
        k = parse(name)
        if k["family"] == "pair" and k["lead"]:
            wide = k["PP"] > 4 or k["QQ"] > 4           # (work queue only: a tol = 0 call runs this kernel too)
            for sched, tag in ((QUEUE if k["queue"] else STATIC, ""),) + (((STATIC, " static call"),) if wide else ()):
                c = lead_case(name, k, pair_Ls[k["n"]], sched, tag)
                if c is not None:
                    out.append(c)
            continue
        if k["family"] == "scan":
            if k["fit"]:
                continue
            T = member_lengths(k["L"], k["n"])[1]
            out.append(_case(name, k, T, SCAN, "ragged", QUEUE if k["queue"] else STATIC))
            if k["gimg"]:                   # (no static form: a tol = 0 call runs this kernel too)
                out.append(_case(name, k, T, SCAN, "ragged", STATIC, " static call"))
        else:
            T = pair_length(k["L"], k["n"], pair_Ls[k["n"]])
            algo, sched = (PAIR if k["n"] == 32 else QUAD), (QUEUE if k["queue"] else STATIC)
            if pair_steady(k["L"], k["n"], k["PP"], k["QQ"]):
                out.append(_case(name, k, T, algo, "dense", sched, " dense"))
                out.append(_case(name, k, T, algo, "ragged", sched, " ragged"))
            else:
                out.append(_case(name, k, T, algo, "ragged", sched))
    return tuple(out)


@functools.lru_cache(maxsize=64)
def _series(T, p, q, sid):
    from ldsr_amd import synth
    return synth.make_series(T, p, q, series_id=sid)


@functools.lru_cache(maxsize=64)
def _warm(T, p, q, mask, tail, seed):
    """the oracle's converged thetas (niter = 400, tol = 1e-5) of the series, from the draws behind the cold rows"""
    from ldsr_amd import synth
    from oracle import oracle as O
    y, u, v = _masked(T, p, q, mask, tail, seed)
    draws = synth.make_init_packed(p, q, len(WARM_ROWS), seed=40 + seed, first=N_CELLS)
    return [O.lds_em(nan_for_inf(y), u, v, d, 400, 1e-5)["theta"] for d in draws]


def _masked(T, p, q, mask, tail, seed):
    y, u, v = _series(T, p, q, 200 + seed)
    if mask == "lead+ragged":                       # an all-missing lead, then a ragged tail
        y = np.concatenate([np.full(T - tail, np.nan), apply_mask(y[T - tail:], "ragged")])
    else:
        y = apply_mask(y, mask)
    return y, u, v


def case_inputs(c):
    """-> y (masked), u, v, theta0 [n, 6+p+q] of a case"""
    from ldsr_amd import synth
    p, q = c["p"], c["q"]
    y, u, v = _masked(c["T"], p, q, c["mask"], c.get("tail", 0), c["seed"])
    th0 = synth.make_init_packed(p, q, N_CELLS, seed=40 + c["seed"])
    if c["steady"] and c["mask"] == "dense":
        for r, a, cc in SLOW_ROWS:
            th0[r, 0], th0[r, 1 + p] = a, cc
    if c["tol"] > 0:
        for r, w in zip(WARM_ROWS, _warm(c["T"], p, q, c["mask"], c.get("tail", 0), c["seed"])):
            th0[r] = w
    if c["n"] > N_CELLS:                            # ("many": cold rows behind the case's 13)
        th0 = np.concatenate([th0, synth.make_init_packed(p, q, c["n"] - N_CELLS, seed=40 + c["seed"], first=100)])
    return y, u, v, th0


@functools.lru_cache(maxsize=8)
def em_refs(cid):
    """-> inputs, the oracle's result and the longdouble model's of a case.  The oracle's theta, lik, n_iter,
    status hold every cell, its liks [13, niter] (NaN behind n_iter) and the model's theta, lik, liks, n_iter,
    margin the first 13."""
    from oracle import oracle as O
    c = next(c for c in em_cases() if c["id"] == cid)
    y, u, v, th0 = case_inputs(c)
    yo = nan_for_inf(y)
    th, lik, nit, st = O.em_batch(yo[None], u.T[None].copy(), v.T[None].copy(), np.zeros(c["n"], np.int32), th0,
                                  c["niter"], c["tol"], n_threads=4)
    liks = np.full((N_CELLS, c["niter"]), np.nan)
    for i in range(N_CELLS):
        tr = O.lds_em(yo, u, v, th0[i], c["niter"], c["tol"])["liks"]
        assert tr.size == nit[i] and tr[-1] == lik[i], (cid, i)
        liks[i, :tr.size] = tr
    orc = {"theta": th, "lik": lik, "liks": liks, "n_iter": nit, "status": st}
    ld = SM.em(th0[:N_CELLS], y, u, v, c["niter"], c["tol"], dtype=np.longdouble)
    return y, u, v, th0, orc, ld


def first13(r):
    return {k: r[k][:N_CELLS] for k in r}


KEYS = ("theta", "lik", "liks")


def worst(got, ld):
    return max(gap(got[k][:N_CELLS], ld[k]) for k in KEYS)


def launch(c, y, u, v, th0):
    """the case's three launches -> {"got", "plain" (return_liks off), "back" (batch reversed), "kernel"}"""
    import ldsr_amd
    kw = dict(niter=c["niter"], tol=c["tol"], algo=c["algo"])
    got = ldsr_amd.em_batch(y, u, v, th0, return_liks=True, **kw)
    out = {"got": got, "kernel": _last_kernel()}
    out["plain"] = ldsr_amd.em_batch(y, u, v, th0, **kw)
    out["back"] = ldsr_amd.em_batch(y, u, v, th0[::-1].copy(), return_liks=True, **kw)
    return out


def run_group(group, path):
    """(in a child process) every "child" case of a group -> .npz of its launches' outputs and kernel names"""
    out = {}
    for i, c in enumerate(c for c in em_cases() if c["mode"] == "child" and c["group"] == group):
        r = launch(c, *case_inputs(c))
        out["%d_kernel" % i] = np.array(r["kernel"])
        for w in ("got", "plain", "back"):
            for k, a in r[w].items():
                out["%d_%s_%s" % (i, w, k)] = a
    np.savez(path, **out)


@pytest.fixture(scope="module")
def eng():
    import ldsr_amd
    from ldsr_amd import _lib
    assert _lib.lib().ldsr_device_count() >= 1, "no GPU visible"
    return ldsr_amd


class LeadRuns:
    """The children of the "child" cases: one per (LPC, PP) group, started when its first case asks, one at a
    time, with LDSR_FORCE_FILL=1 and a time limit sized to the group.  A child that ends on a signal or on its
    time limit fails every later request, and nothing further is started."""

    def __init__(self, tmp):
        self.tmp, self.done, self.dead = tmp, {}, None

    def get(self, c):
        import os
        import subprocess
        import sys
        g = c["group"]
        if self.dead:
            pytest.fail("no further child is started: " + self.dead)
        if g not in self.done:
            here = os.path.dirname(os.path.abspath(__file__))
            path = str(self.tmp / ("lead_%s.npz" % g))
            n = sum(1 for x in em_cases() if x["mode"] == "child" and x["group"] == g)
            code = "import sys; sys.path[:0] = [%r, %r]; import conftest, test_gpu_em_family as E; E.run_group(%r, %r)" % (
                os.path.dirname(here), here, g, path)
            try:
                p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, LDSR_FORCE_FILL="1"),
                                   timeout=60 + 2 * n)
            except subprocess.TimeoutExpired:
                self.dead = "the child of group %s ran into its time limit" % g
                pytest.fail(self.dead)
            if p.returncode != 0:
                self.dead = "the child of group %s ended with status %d" % (g, p.returncode)
                pytest.fail(self.dead)
            self.done[g] = np.load(path)
        d = self.done[g]
        i = [x["id"] for x in em_cases() if x["mode"] == "child" and x["group"] == g].index(c["id"])
        r = {"kernel": str(d["%d_kernel" % i])}
        for w in ("got", "plain", "back"):
            r[w] = {k[len("%d_%s_" % (i, w)):]: d[k] for k in d.files if k.startswith("%d_%s_" % (i, w))}
        return r


@pytest.fixture(scope="module")
def lead_runs(tmp_path_factory):
    return LeadRuns(tmp_path_factory.mktemp("lead"))


def _last_kernel():
    from ldsr_amd import _lib
    buf = C.create_string_buffer(160)
    assert _lib.lib().ldsr_last_em_kernel(0, buf, 160) == 0
    return buf.value.decode()


@pytest.mark.gpu
@pytest.mark.parametrize("c", em_cases(), ids=lambda c: c["id"])
def test_em_kernel(eng, lead_runs, c):
    y, u, v, th0, orc, ld = em_refs(c["id"])
    r = lead_runs.get(c) if c["mode"] == "child" else launch(c, y, u, v, th0)
    got, plain, back = r["got"], r["plain"], r["back"]
    assert r["kernel"] == c["kernel"]                                                      # (1)
    d, o = worst(got, ld), worst(orc, ld)
    print("GAP %-58s device %.3e oracle %.3e" % (c["id"], d, o))
    assert np.array_equal(got["status"], orc["status"]) and np.all(orc["status"] == 0), got["status"]    # (2)
    assert np.array_equal(got["n_iter"], orc["n_iter"]), (got["n_iter"], orc["n_iter"])
    for k in ("theta", "lik"):
        assert parity_close(got[k], orc[k], RTOL, ATOL), (c["id"], k)
    assert parity_close(got["liks"][:N_CELLS], orc["liks"], RTOL, ATOL), (c["id"], "liks")
    assert np.array_equal(np.isnan(got["liks"][:N_CELLS]), np.isnan(orc["liks"]))
    assert np.array_equal(got["n_iter"][:N_CELLS], ld["n_iter"])                           # (3)
    for k in KEYS:
        assert gap(got[k][:N_CELLS], ld[k]) <= DEVICE_CAP, (c["id"], k, gap(got[k][:N_CELLS], ld[k]))
    for k in ("theta", "lik", "n_iter", "status"):                                         # (4)
        assert np.array_equal(got[k], plain[k]), (c["id"], "return_liks changes", k)
        assert np.array_equal(got[k], back[k][::-1]), (c["id"], "position in the batch changes", k)
    assert np.array_equal(got["liks"], back["liks"][::-1], equal_nan=True), (c["id"], "position changes liks")
