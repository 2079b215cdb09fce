"""ldsr_filter_batch_device between tests/extents.py's guard bands and ldsr_filter_batch under the arenas' guard
mode (LDSR_ARENA_GUARD=1): the filter kernel reads and writes nothing outside its buffers, with every output
requested and with scalars only, and the workspace it asks for is the workspace it needs."""
import os
import subprocess
import sys

import numpy as np
import pytest

import extents as X
import filter_model as FM
import filter_runs as FR
from ldsr_amd import synth

pytestmark = pytest.mark.gpu

LDSR_EINVAL = 1
N_LAGS = 8


def ext_case(T, p, q, shared):
    """three series (dense; 30 % missing; a hole across step 63 | 64), cells 2 + 1 + 2"""
    ys, us, vs = [], [], []
    for s in range(3):
        y, u, v = synth.make_series(T, p, q, series_id=7000 + 10 * T + s)
        if s == 1:
            y = np.where(synth.uniform(5, s, T) >= 0.3, y, np.nan)
        if s == 2:
            y[62:66] = np.nan
        ys.append(y), us.append(u), vs.append(v)
    u, v = (us[0], vs[0]) if shared else (np.array(us), np.array(vs))
    theta = synth.make_init_packed(p, q, 5, seed=T + p)
    return {"name": "T%d-p%d-q%d-%s" % (T, p, q, "shared" if shared else "per-series"), "T": T, "p": p, "q": q, "S": 3,
            "Y": np.array(ys), "u": u, "v": v, "theta": theta, "off": np.array([0, 2, 3, 5], np.int32), "shared": shared,
            "n_lags": N_LAGS, "n": 5}


CASES = [ext_case(T, p, q, shared) for T in (65, 129) for (p, q) in ((3, 2), (16, 16)) for shared in (0, 1)]


@pytest.fixture(scope="module")
def eng():
    import ldsr_amd
    from ldsr_amd import _lib
    assert _lib.lib().ldsr_device_count() >= 1, "no GPU visible"
    return ldsr_amd


@pytest.mark.parametrize("c", CASES, ids=lambda c: c["name"])
def test_device_entry_under_guard_bands(eng, c):
    full = FR.device_run(c, guarded=True)                       # every output, both fill patterns
    small = FR.device_run(c, rows=(), guarded=True)             # scalars only
    X.same_bits(small, {k: full[k] for k in small}, "scalars only and every output")
    X.same_bits(full, FR.host_run(c), "the device entry under guard bands and the host entry")
    bare = FR.device_run(c, n_lags=0, rows=(), guarded=True)    # no lags: no strip of z in the workspace
    X.same_bits(bare, {k: full[k] for k in bare}, "no lags and %d lags" % N_LAGS)


@pytest.mark.parametrize("n_lags", [0, N_LAGS])
def test_exact_workspace_is_accepted_and_a_short_one_refused_with_nothing_written(eng, n_lags):
    from ldsr_amd import _lib
    from test_gpu_extents import TorchBlock
    c = CASES[0]
    inputs = FR.abi_inputs(c)
    wsb = FR.workspace_bytes(c, n_lags)
    assert wsb >= 4 * c["n"] + (8 * c["n"] * c["T"] if n_lags else 0)
    lay = FR.layout(c, inputs, FM.ROWS, n_lags, wsb)
    before = lay.image(0xFF, inputs)
    block = TorchBlock(before)
    assert FR.device_call(c, block, lay.off, wsb, 1, n_lags) == 0, _lib.lib().ldsr_last_error()
    lay.check(before, block.image(), 0xFF)
    short = FR.layout(c, inputs, FM.ROWS, n_lags, wsb - 256) if wsb > 256 else lay
    before = short.image(0xFF, inputs)
    block = TorchBlock(before)
    rc = FR.device_call(c, block, short.off, wsb - 256, 1, n_lags)
    msg = _lib.lib().ldsr_last_error().decode()
    assert rc == LDSR_EINVAL and msg == "workspace too small: need %d bytes" % wsb, (rc, msg)
    assert np.array_equal(block.image(), before)


def run_host_entry(path):
    """(in a child process) ldsr_filter_batch on two cases with every output, with scalars only and without lags;
    the outputs and the guard report go to `path`"""
    import ctypes as C
    from ldsr_amd import _lib
    out = {}
    for c in (CASES[0], CASES[-1]):
        for tag, kw in (("all", {}), ("scalars", {"rows": ()}), ("nolags", {"n_lags": 0, "rows": ("e", "S")})):
            for k, a in FR.host_run(c, **kw).items():
                out["%s:%s:%s" % (c["name"], tag, k)] = a
    buf = C.create_string_buffer(1 << 16)
    n = _lib.lib().ldsr_arena_guard_report(buf, len(buf))
    out["report"] = np.array([str(n), buf.value.decode()])
    np.savez(path, **out)


def _child(tmp, guard):
    """one child with its own time limit; it is started fresh, never an exec of this process"""
    here = os.path.dirname(os.path.abspath(__file__))
    path = str(tmp / ("filter_host_%d.npz" % guard))
    code = ("import sys; sys.path[:0] = [%r, %r]; import conftest, test_gpu_filter_extents as G; G.run_host_entry(%r)"
            % (os.path.dirname(here), here, path))
    env = {k: v for k, v in os.environ.items() if k != "LDSR_ARENA_GUARD"}
    if guard:
        env["LDSR_ARENA_GUARD"] = "1"
    p = subprocess.run([sys.executable, "-c", code], env=env, timeout=120)
    assert p.returncode == 0, "the %s child ended with status %d" % ("guarded" if guard else "plain", p.returncode)
    return dict(np.load(path))


def test_host_entry_under_the_arenas_guard_mode(eng, tmp_path):
    g = _child(tmp_path, 1)
    n, text = g.pop("report")
    assert int(n) == 0, text
    p = _child(tmp_path, 0)         # (started only after the guarded child ended well)
    assert int(p.pop("report")[0]) == 0
    assert set(g) == set(p) and len(g) >= 30
    X.same_bits(g, p, "LDSR_ARENA_GUARD=1 and the plain mode")
