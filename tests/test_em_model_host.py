"""The case table of tests/test_gpu_em_family.py, checked without a GPU:

 * COVERAGE: the plan query with a case's arguments names exactly the case's kernel, and the table's kernels are
   the inventory minus the FIT forms of the scan family minus UNREACHABLE -- a member added to em_members.h
   without a case fails here;
 * THE CAP CONDITION: on every case the oracle and the float64 model stop where the longdouble model stops, and
   the oracle's gap to the longdouble model, max |oracle - ld| / (1e-6 |ld| + 1e-9) over theta, lik and the
   trace, is at most ORACLE_CAP = 1/1000 of the bar.  That is what lets the GPU test hold a kernel to 1/10 of the
   bar against the model;
 * THE STOP MARGIN: on every case with tol > 0 no |dlik| a stop decision read is nearer to tol than
   4 DEVICE_CAP (1e-6 |lik| + 1e-9): a device trace inside its cap moves a difference of two liks by at most half
   of that, so it cannot change a stop decision.

A case that misses a condition takes the next seed of SEED_ORDER (test_gpu_em_family.SEEDS); a condition is never
widened."""
import ctypes as C

import numpy as np
import pytest

import smoother_model as SM
import test_gpu_em_family as E
from conftest import parity_close


def _plan(c, y):
    from ldsr_amd import _lib
    name = C.create_string_buffer(160)
    obs = np.isfinite(y)
    lead_steps = -1 if obs.all() else int(np.argmax(obs))      # what the host entry finds in y
    a = _lib.lib().ldsr_em_plan_lead(c["T"], c["p"], c["q"], c["niter"], c["tol"], c["algo"], lead_steps, name, 160)
    return a, name.value.decode()


def _interior(T, L):
    """both families deal T steps to nl = ceil(T / L) lanes, the first rp = T - nl (L - 1) of them with L steps
    (member_lengths of test_gpu_smoother_family.py, pair_plan): interior = L does not divide T, 1 < rp < nl"""
    nl = -(-T // L)
    return T % L != 0 and (T - nl * (L - 1)) not in (1, nl)


def test_case_table_runs_every_em_kernel():
    cases = E.em_cases()
    assert len(set(c["id"] for c in cases)) == len(cases)
    for c in cases:
        k = E.parse(c["kernel"])
        y = E._masked(c["T"], 1, 1, c["mask"], c.get("tail", 0), 0)[0]
        a, name = _plan(c, y)
        if c["mode"] in ("direct", "child"):                    # the plan query names the case's kernel
            assert name == c["kernel"] and a == (c["algo"] or (3 if k["n"] == 32 else 4)), c["id"]
        else:
            # "long", "many": the query assumes a launch that fills four cells per wave and names the 16-lane
            # sibling of the same tail; that the case's launch does not fill it is the rule of em_plan.hip fills()
            # restated in the module's docstring, and the GPU test reads ldsr_last_em_kernel
            s = E.parse(name)
            assert s["lead"] and s["n"] == 16 and (s["PP"], s["QQ"]) == (k["PP"], k["QQ"]) and k["n"] == 32, c["id"]
            assert c["tail"] <= 256 and (c["T"] >= 1536 if c["mode"] == "long" else
                                         (c["tol"] > 0 and c["T"] - c["tail"] < 1023 and c["T"] < 1536 and c["n"] == 4096))
            assert (k["PP"] > 2 or k["QQ"] > 4) == (c["mode"] == "long")
        if "tail" in c:                                         # LEAD: the lead the plan accepts, the member's tail
            assert c["algo"] == 0 and c["T"] - c["tail"] >= 191 and c["tail"] % 16 == 0 and c["T"] <= 8192
            assert _interior(c["tail"], k["L"]) or k["n"] == 16 or k["L"] in (4, 8, 16), c["id"]
            if c["mode"] == "child" and c["T"] - c["tail"] > 191:     # ... and no shorter lead
                c2 = dict(c, T=c["T"] - 1)
                assert _plan(c2, y[1:])[1] != c["kernel"], c["id"]
        else:
            assert _interior(c["T"], k["L"]) and c["T"] <= 8192, c["id"]
        Te = c.get("tail", c["T"])                              # the steps the sweeps work on
        assert Te <= (64 if k["family"] == "scan" else 1) * k["n"] * k["L"], c["id"]
        assert (c["niter"], c["tol"]) == (E.QUEUE if k["queue"] and "static call" not in c["id"] else E.STATIC)
        assert E._width(k["PP"], k["L"]) == c["p"] and E._width(k["QQ"], k["L"]) == c["q"]
        assert (c["p"] == k["PP"] and c["q"] == k["QQ"]) if k["L"] % 2 == 0 else (c["p"] in (1, 2, 3, 5) and c["q"] in (1, 2, 3, 5))
    inv = E.inventory()
    want = set(k for k in inv if not (k.startswith("em_scan_kernel<") and k.endswith(", true>")))
    ran = set(c["kernel"] for c in cases)
    assert not ran & set(E.UNREACHABLE) and len(set(E.UNREACHABLE)) == len(E.UNREACHABLE)
    assert sorted(want - ran - set(E.UNREACHABLE)) == []
    assert sorted((ran | set(E.UNREACHABLE)) - want) == []
    for name in E.UNREACHABLE:                                  # only LEAD forms at two cells per wave
        k = E.parse(name)
        assert k["family"] == "pair" and k["lead"] and k["n"] == 32, name
    # steady members: a dense and a ragged case each; queue-only members: a static call as well
    for name in ran:
        k, ids = E.parse(name), [c["id"] for c in cases if c["kernel"] == name]
        if k["family"] == "pair" and not k["lead"] and E.pair_steady(k["L"], k["n"], k["PP"], k["QQ"]):
            assert ids == [name + " dense", name + " ragged"]
        elif (k["family"] == "scan" and k["gimg"]) or (k["family"] == "pair" and (k["PP"] > 4 or k["QQ"] > 4)):
            assert ids == [name, name + " static call"]
        else:
            assert ids == [name]
    assert any(c["steady"] for c in cases)


@pytest.mark.parametrize("c", E.em_cases(), ids=lambda c: c["id"])
def test_em_model_against_oracle(c):
    y, u, v, th0, orc, ld = E.em_refs(c["id"])
    f64 = SM.em(th0[:E.N_CELLS], y, u, v, c["niter"], c["tol"])
    assert np.all(orc["status"] == 0) and np.all(np.isfinite(orc["theta"]))
    assert np.array_equal(orc["n_iter"][:E.N_CELLS], ld["n_iter"]) and np.array_equal(f64["n_iter"], ld["n_iter"]), c["id"]
    for k in E.KEYS:
        assert f64[k].dtype == np.float64 and ld[k].dtype == np.longdouble, k
        assert parity_close(f64[k], orc[k][:E.N_CELLS]), (c["id"], "float64 model", k)
    g = E.worst(orc, ld)
    print("GAP %-58s oracle %.3e float64 model %.3e margin/tol %.3g" % (
        c["id"], g, E.worst(f64, ld), np.min(ld["margin"]) / c["tol"] if c["tol"] > 0 else np.inf))
    assert g <= E.ORACLE_CAP, (c["id"], g)
    if c["tol"] > 0:
        big = np.nanmax(np.abs(np.asarray(ld["liks"], dtype=np.float64)), axis=1)      # the largest |lik| of the trace
        need = 4 * E.DEVICE_CAP * (E.RTOL * big + E.ATOL)
        assert np.all(ld["margin"] > need), (c["id"], ld["margin"], need)
        warm = ld["n_iter"][list(E.WARM_ROWS)]
        assert np.all((warm == 3) | (warm == 4)), (c["id"], warm)       # the warm starts pull the next cell early
        assert np.any(ld["n_iter"] == c["niter"]), c["id"]             # ... while cold rows run on
