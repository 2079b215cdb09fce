"""No kernel reads or writes outside its buffers (run with -m gpu).

Part 1, the device-pointer entries (ldsr_em_batch_device, ldsr_em_batch_device_lead, ldsr_simulate_batch_device):
every pointer argument of a call lies in ONE torch uint8 allocation laid out by tests/extents.py -- each buffer
exactly its documented size, 256-byte aligned, guard bands of max(64 KiB, one row) between them and at both
ends, the EM workspace exactly ldsr_em_workspace_bytes(...) bytes.  Bands, outputs and workspace are pre-filled;
each case runs under the patterns 0xFF and 0x55.  After the call:
 1. every guard byte holds its pattern, 2. every input holds what was uploaded, 3. the outputs have the same bits
 under both patterns (extents.guarded), 4. the outputs have the bits of the same call through the host-pointer
 entry (separate allocations; ldsr_last_em_kernel names the same kernel) and meet the suite's bar against the
 oracle (EM: parity_close) or the numpy twin (replicates: _close_x / _close_q of test_gpu_simulate.py).
One EM case per CLASS of kernel (em_extent_cases), at the class's smallest interior length; the per-member cases
are test_gpu_em_family.py's.  The workspace contract: for every EM case and each of tol in {0, 1e-5}, lead_steps
in {-1, 0, the case's}, algo in {AUTO, the case's}, the exact-size workspace is accepted (and the bands hold);
once, a workspace 256 bytes short is refused with LDSR_EINVAL before anything is written.
tests/test_extents_host.py proves without a GPU that the checker can fail.

Part 2, the host-pointer entries: their buffers are carved from an arena, so the library's guard mode
(LDSR_ARENA_GUARD=1, host_runtime.h) puts the bands there.  run_host_entries makes one small call of every
host entry; it runs in a fresh child with the mode on and in a second one without, one at a time, each under its
own time limit.  The guarded child's report is empty after every call, every output has the plain child's bits
(NaN positions included: a kernel that consumes arena bytes nobody wrote returns NaN under the 0xFF fill), and the
self-test reports exactly one violation."""
import ctypes as C
import functools

import numpy as np
import pytest

import extents as X
from conftest import parity_close
from test_gpu_em_family import (PAIR, QUAD, QUEUE, SCAN, SLOW_ROWS, STATIC, WARM_ROWS, inventory, pair_length,
                                pair_steady, parse)
from test_gpu_smoother_family import RTOL, ATOL, apply_mask, member_lengths, nan_for_inf

AUTO, SERIAL = 0, 1
LDSR_EINVAL = 1
OFF3 = (0, 0, 5, 6)                   # three series: one without cells, odd counts


# ---- the EM cases -------------------------------------------------------------------------------------------------
def plan_name(T, p, q, niter, tol, algo, lead):
    from ldsr_amd import _lib
    buf = C.create_string_buffer(160)
    a = _lib.lib().ldsr_em_plan_lead(T, p, q, niter, float(tol), algo, lead, buf, 160)
    return buf.value.decode() if a > 0 else ""


def _em(cls, T, p, q, n, algo, sched=STATIC, mask="ragged", off=None, shared=0, u=True, v=True, liks=True, lead=0,
        warm=False, slow=False, tag=""):
    off = tuple(off) if off else (0, n)
    c = {"cls": cls, "T": T, "p": p if u else 1, "q": q if v else 1, "off": off, "n": off[-1], "S": len(off) - 1,
         "algo": algo, "niter": sched[0], "tol": sched[1], "mask": mask, "shared": shared, "u": u, "v": v, "liks": liks,
         "lead": lead, "warm": warm, "slow": slow}
    c["id"] = "%s-T%d-p%d-q%d-n%s%s%s%s%s%s%s" % (
        cls, T, p, q, "+".join(str(b - a) for a, b in zip(off, off[1:])), "-queue" if sched[1] > 0 else "",
        "-shared" if shared else "",
        "" if u else "-nou", "" if v else "-nov", "" if liks else "-noliks", tag)
    return c


def _pair_T(lpc, algo, widths):
    """the smallest interior length of the family's generic members that every width of the class runs"""
    ks = [k for k in map(parse, inventory()) if k["family"] == "pair" and k["n"] == lpc and not k["lead"]]
    Ls = sorted(set(k["L"] for k in ks))
    for L in Ls:
        T = pair_length(L, lpc, Ls)
        names = [plan_name(T, p, q, 6, 0.0, algo, 0) for p, q in widths]
        if all(nm and parse(nm)["L"] == L and not pair_steady(L, lpc, parse(nm)["PP"], parse(nm)["QQ"]) for nm in names):
            return T
    raise AssertionError("no generic member of %d lanes runs every width" % lpc)


@functools.lru_cache(maxsize=None)
def em_extent_cases():
    out = []
    # serial: T = 2 (no inputs: two observations determine nothing more), T = 9 at p = q = 8, a wide input; 1 and 65
    # cells (scratch_stride rounds to 64)
    for n in (1, 65):
        out += [_em("serial", 2, 1, 1, n, SERIAL, mask="dense", u=False, v=False), _em("serial", 9, 8, 8, n, SERIAL, mask="dense", liks=n == 1),
                _em("serial", 40, 9, 2, n, SERIAL, mask="scattered30")]
    out += [_em("serial", 9, 3, 3, 0, SERIAL, off=OFF3), _em("serial", 9, 3, 3, 0, SERIAL, off=OFF3, shared=1, u=False)]
    # scan, one wave per cell: static and work queue
    T1 = member_lengths(2, 1)[1]
    out += [_em("scan1", T1, 1, 2, 13, SCAN), _em("scan1", T1, 3, 3, 0, SCAN, off=OFF3, liks=False),
            _em("scan1", T1, 3, 3, 0, SCAN, off=OFF3, shared=1, v=False),
            _em("scan1", T1, 1, 2, 13, SCAN, QUEUE, warm=True), _em("scan1", T1, 2, 5, 0, SCAN, QUEUE, off=OFF3, u=False, v=False)]
    # scan, several waves per cell on a global image; one long and wide shape (whichever member of the family runs it)
    out += [_em("scanG", 2049, 1, 2, 3, SCAN), _em("scanG", 4097, 1, 2, 3, SCAN, liks=False),
            _em("scan", 1281, 4, 5, 3, SCAN), _em("scanG", 2049, 3, 3, 0, SCAN, QUEUE, off=OFF3, shared=1)]
    # pair (32 lanes) and quad (16 lanes), generic body: one, two and three phantom partners; the identity padding
    widths = ((1, 1), (3, 3), (4, 4))
    for cls, lpc, algo in (("pair", 32, PAIR), ("quad", 16, QUAD)):
        T = _pair_T(lpc, algo, widths)
        for p, q in widths:
            for n in (1, 3, 5):
                out.append(_em(cls, T, p, q, n, algo, liks=n != 3))
        out += [_em(cls, T, 3, 3, 0, algo, off=OFF3), _em(cls, T, 3, 3, 0, algo, off=OFF3, shared=1, u=False),
                _em(cls, T, 2, 4, 0, algo, off=OFF3, shared=1, v=False, liks=False),
                # work-queue forms: fully observed, warm rows, so that cells stop at different iterations
                _em(cls + "Q", T, 1, 2, 13, algo, QUEUE, mask="dense", lead=-1, warm=True),
                _em(cls + "Q", T, 3, 3, 0, algo, QUEUE, mask="dense", lead=-1, off=OFF3, shared=1)]
    # steady pair body: dense, an odd cell count, two slow rows
    out.append(_em("steady", 737, 1, 2, 13, PAIR, mask="dense", slow=True))
    out.append(_em("steady", 737, 1, 2, 13, PAIR, QUEUE, mask="dense", lead=-1, warm=True, liks=False))
    # LEAD forms through AUTO, launches large enough that AUTO takes them; an odd cell count
    out += [_em("lead16", 1000, 1, 2, 8191, AUTO, mask="lead", lead=900, liks=False),        # lead of 888 steps
            _em("lead32", 1000, 1, 2, 8191, AUTO, mask="lead", lead=600),                    # ... of 600: no multiple of 16
            _em("lead32", 1008, 3, 3, 8191, AUTO, mask="lead", lead=608, liks=False)]        # ... of 608: a multiple
    assert len(set(c["id"] for c in out)) == len(out)
    return tuple(out)


def want_kernel(c, tol=None, lead=None, algo=None):
    return plan_name(c["T"], c["p"], c["q"], c["niter"], c["tol"] if tol is None else tol,
                     c["algo"] if algo is None else algo, c["lead"] if lead is None else lead)


def in_class(c, name):
    """does the kernel `name` belong to the case's class"""
    cls = c["cls"]
    if cls == "serial":
        return name.startswith("em_serial_kernel<")
    if not name.startswith("em_scan_kernel<") and not name.startswith("em_pair_kernel<"):
        return False
    k = parse(name)
    if cls in ("scan", "scan1", "scanG"):
        if k["family"] != "scan" or k["fit"]:
            return False
        if cls == "scan":
            return True
        return (k["n"] == 1 and not k["gimg"] and k["queue"] == (c["tol"] > 0)) if cls == "scan1" else (k["n"] > 1 or k["gimg"])
    if k["family"] != "pair":
        return False
    if cls.startswith("lead"):
        return k["lead"] and k["n"] == int(cls[4:])
    lpc = 16 if cls.startswith("quad") else 32
    steady = pair_steady(k["L"], k["n"], k["PP"], k["QQ"])
    return k["n"] == lpc and not k["lead"] and k["queue"] == (c["tol"] > 0) and steady == (cls == "steady")


@functools.lru_cache(maxsize=4)
def em_inputs(cid):
    """-> Y [S, T] (masked), U [nuv, T, p] or None, V likewise, theta0 [n, P] of a case (time-major, as uploaded)"""
    from ldsr_amd import synth
    from oracle import oracle as O
    c = next(c for c in em_extent_cases() if c["id"] == cid)
    T, p, q, S, n = c["T"], c["p"], c["q"], c["S"], c["n"]
    Y, U, V = np.empty((S, T)), np.empty((S, T, p)), np.empty((S, T, q))
    for s in range(S):
        y, u, v = synth.make_series(T, p, q, series_id=300 + s)
        if c["mask"] == "lead":         # missing up to the lead, observed right behind it, a hole in the tail
            y = y.copy()
            y[:c["lead"]] = np.nan
            y[c["lead"] + 25:c["lead"] + 30] = np.nan
        else:
            y = apply_mask(y, c["mask"])
        Y[s], U[s], V[s] = y, u.T, v.T
    if c["shared"]:
        U, V = U[:1].copy(), V[:1].copy()
    U, V = (U if c["u"] else None), (V if c["v"] else None)
    th0 = synth.make_init_packed(p, q, n, seed=71)
    if c["slow"]:
        for r, a, cc in SLOW_ROWS:
            th0[r, 0], th0[r, 1 + p] = a, cc
    if c["warm"]:                       # rows that start at the oracle's converged theta
        assert S == 1
        draws = synth.make_init_packed(p, q, len(WARM_ROWS), seed=71, first=n)
        for r, d in zip(WARM_ROWS, draws):
            th0[r] = O.lds_em(nan_for_inf(Y[0]), U[0].T if c["u"] else None, V[0].T if c["v"] else None, d, 400, 1e-5)["theta"]
    return Y, U, V, th0


def _per_series(A, c):
    """[nuv, T, k] -> [S, T, k] (or None)"""
    return None if A is None else np.ascontiguousarray(np.broadcast_to(A, (c["S"],) + A.shape[1:])) if c["shared"] else A


@functools.lru_cache(maxsize=4)
def em_oracle(cid):
    from oracle import oracle as O
    c = next(c for c in em_extent_cases() if c["id"] == cid)
    Y, U, V, th0 = em_inputs(cid)
    soc = np.repeat(np.arange(c["S"]), np.diff(c["off"])).astype(np.int32)
    Yo = nan_for_inf(Y)
    Uo, Vo = _per_series(U, c), _per_series(V, c)
    th, lik, nit, st = O.em_batch(Yo, Uo, Vo, soc, th0, c["niter"], c["tol"], n_threads=16)
    liks = None
    if c["liks"]:
        liks = np.full((c["n"], c["niter"]), np.nan)
        for i in range(c["n"]):
            s = soc[i]
            tr = O.lds_em(Yo[s], None if Uo is None else Uo[s].T, None if Vo is None else Vo[s].T, th0[i], c["niter"],
                          c["tol"])["liks"]
            liks[i, :tr.size] = tr
    return {"d_theta": th, "d_lik": lik, "d_n_iter": nit, "d_status": st, "d_liks": liks}


def em_layout(c, wsb):
    T, p, q, S, n, P = c["T"], c["p"], c["q"], c["S"], c["n"], 6 + c["p"] + c["q"]
    nuv = 1 if c["shared"] else S
    b = [X.Buf("d_y", 8 * S * T, 8 * T, X.IN)]
    if c["u"]:
        b.append(X.Buf("d_u", 8 * nuv * T * p, 8 * T * p, X.IN))
    if c["v"]:
        b.append(X.Buf("d_v", 8 * nuv * T * q, 8 * T * q, X.IN))
    b += [X.Buf("d_theta0", 8 * n * P, 8 * P, X.IN), X.Buf("d_theta", 8 * n * P, 8 * P, X.OUT, np.float64),
          X.Buf("d_lik", 8 * n, 8, X.OUT, np.float64), X.Buf("d_n_iter", 4 * n, 4, X.OUT, np.int32),
          X.Buf("ws", wsb, 256, X.WS), X.Buf("d_status", 4 * n, 4, X.OUT, np.int32)]
    if c["liks"]:
        b.append(X.Buf("d_liks", 8 * n * c["niter"], 8 * c["niter"], X.OUT, np.float64))
    return X.Layout(b)


def em_upload(c):
    Y, U, V, th0 = em_inputs(c["id"])
    d = {"d_y": Y, "d_theta0": th0}
    if c["u"]:
        d["d_u"] = U
    if c["v"]:
        d["d_v"] = V
    return d


class TorchBlock:
    """the block on the device: one uint8 allocation, its first byte 256-byte aligned"""

    def __init__(self, image):
        import torch
        self.raw = torch.empty(image.size + 256, dtype=torch.uint8, device="cuda:0")
        pad = (-self.raw.data_ptr()) % 256
        self.t = self.raw[pad:pad + image.size]
        self.t.copy_(torch.from_numpy(image))
        self.base = self.t.data_ptr()
        assert self.base % 256 == 0
        torch.cuda.synchronize()

    def image(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy()


def workspace_bytes(c, algo):
    from ldsr_amd import _lib
    return _lib.lib().ldsr_em_workspace_bytes(c["S"], c["T"], c["p"], c["q"], c["n"], algo)


def em_call(c, block, off, wsb, tol, lead, algo):
    """the case's call on the block -> rc (lead_steps = 0 goes through ldsr_em_batch_device)"""
    import torch
    from ldsr_amd import _lib
    L = _lib.lib()

    def at(name):
        return C.c_void_p(block.base + off[name]) if name in off else None
    offs = (C.c_int * (c["S"] + 1))(*c["off"])
    args = [0, C.c_void_p(torch.cuda.current_stream().cuda_stream), c["S"], c["T"], c["p"], c["q"], at("d_y"), at("d_u"),
            at("d_v"), c["shared"], offs, at("d_theta0"), c["niter"], float(tol), algo, at("d_theta"), at("d_lik"),
            at("d_n_iter"), at("d_status"), at("d_liks"), at("ws"), wsb]
    return L.ldsr_em_batch_device(*args) if lead == 0 else L.ldsr_em_batch_device_lead(*args, lead)


def last_kernel():
    from ldsr_amd import _lib
    buf = C.create_string_buffer(160)
    assert _lib.lib().ldsr_last_em_kernel(0, buf, 160) == 0
    return buf.value.decode()


def last_error():
    from ldsr_amd import _lib
    return _lib.lib().ldsr_last_error().decode()


@pytest.fixture(scope="module")
def eng():
    import ldsr_amd
    from ldsr_amd import _lib
    assert _lib.lib().ldsr_device_count() >= 1, "no GPU visible"
    return ldsr_amd


def em_host(eng, c):
    """the same call the plain way: the host-pointer entry, separate allocations -> outputs under the block's names"""
    Y, U, V, th0 = em_inputs(c["id"])

    def rt(A):      # [nuv, T, k] -> k x T (one series for all) or [S, k, T]
        if A is None:
            return None
        return A[0].T.copy() if c["shared"] or c["S"] == 1 else np.transpose(A, (0, 2, 1)).copy()
    r = eng.em_batch(Y if c["S"] > 1 else Y[0], rt(U), rt(V), th0, cell_offsets=list(c["off"]), niter=c["niter"],
                     tol=c["tol"], algo=c["algo"], return_liks=c["liks"])
    out = {"d_theta": r["theta"].reshape(-1), "d_lik": r["lik"], "d_n_iter": r["n_iter"], "d_status": r["status"]}
    if c["liks"]:
        out["d_liks"] = r["liks"].reshape(-1)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c", em_extent_cases(), ids=lambda c: c["id"])
def test_em_device_entry_under_guard_bands(eng, c):
    want = want_kernel(c)
    assert in_class(c, want), (c["cls"], want)
    wsb = workspace_bytes(c, c["algo"])
    assert wsb > 0 and wsb % 256 == 0
    ran = []

    def call(block, off):
        rc = em_call(c, block, off, wsb, c["tol"], c["lead"], c["algo"])
        assert rc == 0, last_error()
        ran.append(last_kernel())
    got = X.guarded(em_layout(c, wsb), em_upload(c), call, make_block=TorchBlock)       # (1), (2), (3)
    assert ran == [want, want], (ran, want)
    host = em_host(eng, c)                                                              # (4)
    assert last_kernel() == want, "the host entry plans another kernel"
    X.same_bits(got, host, "the device entry under guard bands and the host entry")
    ref = em_oracle(c["id"])
    assert np.array_equal(got["d_status"], ref["d_status"]), got["d_status"]
    assert np.array_equal(got["d_n_iter"], ref["d_n_iter"]), (got["d_n_iter"], ref["d_n_iter"])
    ok = ref["d_status"] == 0
    P = 6 + c["p"] + c["q"]
    assert parity_close(got["d_theta"].reshape(-1, P)[ok], ref["d_theta"][ok], RTOL, ATOL)
    assert parity_close(got["d_lik"][ok], ref["d_lik"][ok], RTOL, ATOL)
    if c["liks"]:
        gl = got["d_liks"].reshape(-1, c["niter"])
        assert parity_close(gl[ok], ref["d_liks"][ok], RTOL, ATOL)
        assert np.array_equal(np.isnan(gl[ok]), np.isnan(ref["d_liks"][ok]))
    assert np.all(ok), ref["d_status"]
    if c["warm"]:
        assert len(set(got["d_n_iter"].tolist())) > 1, "the case wants cells that stop at different iterations"


@pytest.mark.gpu
@pytest.mark.parametrize("c", em_extent_cases(), ids=lambda c: c["id"])
def test_exact_size_workspace_is_accepted(eng, c):
    """ldsr_em_workspace_bytes plans with niter = 2, the default tol, no lead and an assumed device; the call
    plans with its real arguments: whatever they are, the queried size suffices and the bands hold"""
    inputs = em_upload(c)
    combos = sorted(set((tol, lead, algo) for tol in (0.0, 1e-5) for lead in (-1, 0, c["lead"])
                        for algo in (AUTO, c["algo"])))
    for tol, lead, algo in combos:
        wsb = workspace_bytes(c, algo)
        assert wsb > 0
        lay = em_layout(c, wsb)
        before = lay.image(0xFF, inputs)
        block = TorchBlock(before)
        rc = em_call(c, block, lay.off, wsb, tol, lead, algo)
        assert rc == 0, "tol %g lead_steps %d algo %d: %s" % (tol, lead, algo, last_error())
        lay.check(before, block.image(), 0xFF)


@pytest.mark.gpu
def test_a_short_workspace_is_refused_before_anything_is_written(eng):
    c = next(c for c in em_extent_cases() if c["cls"] == "scan1")
    wsb = workspace_bytes(c, c["algo"])
    lay = em_layout(c, wsb - 256)
    before = lay.image(0xFF, em_upload(c))
    block = TorchBlock(before)
    rc = em_call(c, block, lay.off, wsb - 256, c["tol"], c["lead"], c["algo"])
    assert rc == LDSR_EINVAL and "workspace too small" in last_error(), (rc, last_error())
    assert np.array_equal(block.image(), before)


# ---- the replicate cases ------------------------------------------------------------------------------------------
SIM_T = (1, 2, 63, 64, 65, 129)
ALL3 = ("simX", "simY", "simQ")


def sim_extent_cases():
    out = []
    for i, T in enumerate(SIM_T):
        for mode in ("counter", "rstream"):
            out.append({"T": T, "mode": mode, "keep": ALL3, "shared": (i + (mode == "rstream")) % 2})
    for keep in (("simX",), ("simY",), ("simQ",), ("simX", "simQ")):       # test_null_outputs_leave_the_others_identical's
        for mode in ("counter", "rstream"):
            out.append({"T": 65, "mode": mode, "keep": keep, "shared": int(mode == "counter")})
    for c in out:
        c["id"] = "T%d-%s-%s-%s" % (c["T"], c["mode"], "shared" if c["shared"] else "permodel", "+".join(k[3:] for k in c["keep"]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("c", sim_extent_cases(), ids=lambda c: c["id"])
def test_simulate_device_entry_under_guard_bands(eng, c):
    import torch
    from ldsr_amd import _lib, rrng
    from test_gpu_simulate import _close_q, _close_x, _models
    from test_simulate_host import Uniforms, counter_uniforms, twin_count, twin_one_rep
    T, p, q, M, reps, seed, first, mu = c["T"], 3, 3, 2, 5, 4711, 3, np.array([0.3, -0.2])
    P = 6 + p + q
    th = _models(M, p, q, 100 + T)
    th[1, 2 + p + q] = 0.0                        # Q = 0: no q draws, the offsets shift
    g = np.random.default_rng(T)
    nuv = 1 if c["shared"] else M
    u, v = g.normal(size=(nuv, p, T)), g.normal(size=(nuv, q, T))
    count, off = eng.sim.draw_count(th, T, reps, p, q)
    uni = rrng.RUniform(T).unif_rand(count) if c["mode"] == "rstream" else None
    inputs = {"d_u": np.ascontiguousarray(np.transpose(u, (0, 2, 1))), "d_v": np.ascontiguousarray(np.transpose(v, (0, 2, 1))),
              "d_theta": th, "d_mu": mu}
    bufs = [X.Buf("d_u", 8 * nuv * T * p, 8 * T * p, X.IN), X.Buf("d_v", 8 * nuv * T * q, 8 * T * q, X.IN),
            X.Buf("d_theta", 8 * M * P, 8 * P, X.IN), X.Buf("d_mu", 8 * M, 8, X.IN)]
    if uni is not None:
        assert uni.size == count
        inputs.update(d_uniforms=uni, d_offsets=off[:M].copy())
        bufs += [X.Buf("d_uniforms", 8 * count, 8, X.IN), X.Buf("d_offsets", 8 * M, 8, X.IN)]
    bufs += [X.Buf("d_" + k, 8 * M * reps * T, 8 * T, X.OUT, np.float64) for k in c["keep"]]
    L = _lib.lib()

    def call(block, o):
        def at(name):
            return C.c_void_p(block.base + o[name]) if name in o else None
        _lib.check(L.ldsr_simulate_batch_device(
            0, C.c_void_p(torch.cuda.current_stream().cuda_stream), M, T, p, q, at("d_u"), at("d_v"), c["shared"],
            at("d_theta"), at("d_mu"), reps, first, 1, seed, at("d_uniforms"), at("d_offsets"), at("d_simX"),
            at("d_simY"), at("d_simQ")))
    got = X.guarded(X.Layout(bufs), inputs, call, make_block=TorchBlock)
    uu, vv = (u[0], v[0]) if c["shared"] else (u, v)
    host = eng.simulate_batch(th, uu, vv, T, reps, mu=mu, seed=seed, first_rep=first, uniforms=uni, outputs=c["keep"])
    X.same_bits(got, {"d_" + k: host[k].reshape(-1) for k in c["keep"]},
                "the device entry under guard bands and the host entry")
    src = Uniforms(rrng.RUniform(T)) if uni is not None else None
    for m in range(M):
        um, vm = (u[0], v[0]) if c["shared"] else (u[m], v[m])
        k = twin_count(th[m], p, q, T)
        rows = [twin_one_rep(src if src else Uniforms(counter_uniforms(seed, m, first + j, k)), th[m], p, q, um, vm, T,
                             mu[m]) for j in range(reps)]
        for i, name in enumerate(ALL3):
            if name in c["keep"]:
                (_close_q if name == "simQ" else _close_x)(got["d_" + name].reshape(M, reps, T)[m], np.array([r[i] for r in rows]))


# ---- part 2: the host-pointer entries under the arenas' guard mode -------------------------------------------------
def guard_report():
    from ldsr_amd import _lib
    buf = C.create_string_buffer(1 << 16)
    n = _lib.lib().ldsr_arena_guard_report(buf, len(buf))
    return n, buf.value.decode()


def run_host_entries(path):
    """(in a child process) one small call of every host-pointer entry -> .npz of every output, and after every call
    the guard report's count and text ("report:<call>"); last, the self-test's return code and report"""
    import ldsr_amd as E
    from ldsr_amd import _lib, synth
    from ldsr_amd.bfgs import bfgs_batch, bfgs_update_batch, pl_grad, ssq_train, start_points
    from ldsr_amd.ga import ga_batch
    from ldsr_amd.pcr import pcr_batch
    from test_gpu_bfgs import _mask, _thetas
    out = {}

    def keep(call, r):
        def put(k, a):
            if isinstance(a, dict):
                for kk, aa in a.items():
                    put(k + "." + kk, aa)
            elif isinstance(a, (list, tuple)):
                for i, aa in enumerate(a):
                    put("%s.%d" % (k, i), aa)
            elif a is not None:
                out["%s:%s" % (call, k)] = np.asarray(a)
        put("r", r)
        n, text = guard_report()
        out["report:" + call] = np.array([str(n), text])

    def series(T, p, q, S, mask):
        ys, us, vs = zip(*(synth.make_series(T, p, q, series_id=500 + s) for s in range(S)))
        return np.stack([apply_mask(y, mask) for y in ys]), np.stack(us), np.stack(vs)

    # the smoother family: a FIT scan shape, serial shapes, a singular series
    fits = [("fit65", 65, 3, 3, (0, 0, 4, 5), "ragged"), ("fit3", 3, 1, 2, (0, 2, 3), "dense"),
            ("fit40p9", 40, 9, 2, (0, 2, 3), "scattered30")]
    for tag, T, p, q, off, mask in fits:
        Y, U, V = series(T, p, q, len(off) - 1, mask)
        th = synth.make_init_packed(p, q, off[-1], seed=5)
        sm = E.smooth_batch(Y, U, V, th, cell_offsets=off)
        keep(tag + ".smooth", sm)
        keep(tag + ".smooth_nostd", E.smooth_batch(Y, U, V, th, cell_offsets=off, stdlik=False))
        keep(tag + ".propagate", E.smooth_batch(Y, U, V, th, cell_offsets=off, mode="propagate"))
        keep(tag + ".penlik", E.penalized_likelihood(Y, U, V, th, 0.4, cell_offsets=off))
        L = _lib.lib()
        tho, st = np.empty_like(th), np.empty(off[-1], dtype=np.int32)
        o = np.ascontiguousarray(off, dtype=np.int32)
        Ut, Vt = (np.ascontiguousarray(np.transpose(a, (0, 2, 1))) for a in (U, V))
        _lib.check(L.ldsr_mstep_batch(0, len(off) - 1, T, p, q, E.api._d(Y), E.api._d(Ut), E.api._d(Vt), 0, E.api._i(o),
                                      E.api._d(sm["X"]), E.api._d(sm["V"]), E.api._d(sm["J"]), E.api._d(tho), E.api._i(st)))
        keep(tag + ".mstep", {"theta": tho, "status": st})
    y1, u1, v1 = synth.make_series(65, 3, 3, series_id=68)
    y1 = _mask(y1, "last")
    ths = _thetas(3, 3, (0.0, 0.5, -0.9, 0.999))
    keep("singular.smooth", E.smooth_batch(y1, u1, v1, ths))
    keep("singular.penlik", E.penalized_likelihood(y1, u1, v1, ths, 0.25))
    keep("singular.propagate", E.smooth_batch(y1, u1, v1, ths, mode="propagate"))

    # the EM entries: T = 130, odd cell counts
    Y, U, V = series(130, 1, 2, 3, "ragged")
    off = (0, 5, 8, 11)
    th0 = synth.make_init_packed(1, 2, 11, seed=9)
    thg = th0.copy()
    thg[5:8, 0] = np.nan                          # NaN likelihoods in every restart of series 1: no selectable winner
    u0, v0 = U[0], V[0]
    for tol, niter in ((0.0, 6), (1e-5, 12)):
        tag = "tol%g" % tol
        keep("em." + tag, E.em_batch(Y, U, V, th0, cell_offsets=off, niter=niter, tol=tol, return_liks=True))
        keep("em_noliks." + tag, E.em_batch(Y, u0, v0, th0, cell_offsets=off, niter=niter, tol=tol))
        keep("em_multi." + tag, E.em_batch(Y, U, V, th0, cell_offsets=off, niter=niter, tol=tol, devices=[0, 0, 0],
                                           return_liks=True))
        keep("grid." + tag, E.em_restart_grid(Y, u0, v0, thg, cell_offsets=off, niter=niter, tol=tol))
        keep("grid_noall." + tag, E.em_restart_grid(Y, U, V, th0, cell_offsets=off, niter=niter, tol=tol, return_all=False))
        keep("grid_multi." + tag, E.em_restart_grid(Y, U, V, thg, cell_offsets=off, niter=niter, tol=tol, devices=[0, 0, 0]))
    _, U3, V3 = series(130, 3, 3, 3, "ragged")
    keep("groups", E.ensemble_restart(Y, [(u0, v0), (U3[0], V3[0])],
                                      [th0, synth.make_init_packed(3, 3, 11, seed=10)], niter=6, tol=0.0,
                                      cell_offsets=off))

    # the GA: two islands of 8, three generations, one suggestion, two series
    Y2, U2, V2 = series(65, 1, 2, 2, "ragged")
    lb = np.array([0.0, -1.0, 0.0, -1.0, -1.0, 0.05, 0.05, -1.0, 0.1])
    ub = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.5, 1.5, 1.0, 1.5])
    sug = np.stack([synth.make_init_packed(1, 2, 1, seed=3)] * 2)
    keep("ga", ga_batch(Y2, U2[0], V2[0], lb, ub, lambda_=0.4, num_islands=2, pop_per_island=8, maxiter=3, run=3, seed=5,
                        suggestions=sug, return_population=True))

    # the L-BFGS learners and their gradients: three starts over two series, maxit = 3
    for T in (65, 113):
        Yb, Ub, Vb = series(T, 1, 2, 2, "scattered30")
        offb = (0, 1, 3)
        par0 = start_points(lb, ub, 3, seed=T)
        tag = "T%d" % T
        for grad in (False, True):
            keep("ssq.%s.grad%d" % (tag, grad), ssq_train(Yb, Ub[0], Vb[0], par0, cell_offsets=offb, grad=grad))
            keep("plg.%s.grad%d" % (tag, grad), pl_grad(Yb, Ub[0], Vb[0], par0, 0.4, cell_offsets=offb, grad=grad))
        for smooth in (False, True):
            keep("bfgs.%s.smooth%d" % (tag, smooth), bfgs_batch(Yb, Ub[0], Vb[0], par0, lb, ub, cell_offsets=offb, maxit=3,
                                                               smooth=smooth))
        keep("bfgs_noall." + tag, bfgs_batch(Yb, Ub, Vb, par0, lb, ub, cell_offsets=offb, maxit=3, return_all=False))
        keep("bfgs_update." + tag, bfgs_update_batch(Yb, Ub[0], Vb[0], par0, lb, ub, lam=0.4, cell_offsets=offb, maxit=3))

    # replicates: both modes, one NULL output
    ths = np.stack([_thetas(3, 3, (0.5,))[0], _thetas(3, 3, (-0.3,))[0]])
    ths[:, 11] = 0.7
    g = np.random.default_rng(65)
    us, vs = g.normal(size=(3, 65)), g.normal(size=(2, 3, 65))
    count, _ = E.sim.draw_count(ths, 65, 5, 3, 3)
    keep("sim.counter", E.simulate_batch(ths, us, vs, 65, 5, mu=0.3, seed=12, outputs=("simX", "simQ")))
    keep("sim.rstream", E.simulate_batch(ths, us, vs, 65, 5, mu=0.3, uniforms=E.rrng.RUniform(3).unif_rand(count),
                                         outputs=("simY", "simQ")))

    # PCR: three folds at (13, 3); members of 16 and 1 columns at n = 46; the first shape on the raised LDS limit;
    # predictions at N = 813 rows
    def pcr(tag, n, ks, folds, N=None):
        g = np.random.default_rng(n)
        members = [g.normal(size=(n, k)) for k in ks]
        y = g.normal(size=n)
        y[n // 2] = np.nan
        held = (g.uniform(size=(folds, n)) < 0.2).astype(np.uint8) if folds > 1 else np.zeros((1, n), np.uint8)
        pm = None if N is None else [g.normal(size=(N, k)) for k in ks]
        keep(tag, pcr_batch(members, y, held, pred_members=pm, lev=True))
    pcr("pcr.13x3", 13, (3,), 3)
    pcr("pcr.46", 46, (16, 1), 2)
    pcr("pcr.452x16", 452, (16,), 1)
    pcr("pcr.pred813", 46, (3, 1), 2, N=813)

    rc = _lib.lib().ldsr_arena_guard_selftest(0)
    n, text = guard_report()
    out["selftest"] = np.array([str(rc), str(n), text])
    np.savez(path, **out)


class HostRuns:
    """The two children of part 2, started when first asked for, one at a time, each under its own time limit (a
    few dozen millisecond-scale calls and the library's load: a bound against hangs).  A child that ends on a signal
    or on its limit fails every later request, and nothing further is started."""
    LIMIT = 120

    def __init__(self, tmp):
        self.tmp, self.done, self.dead = tmp, {}, None

    def get(self, guard):
        import os
        import subprocess
        import sys
        if self.dead:
            pytest.fail("no further child is started: " + self.dead)
        if guard not in self.done:
            here = os.path.dirname(os.path.abspath(__file__))
            path = str(self.tmp / ("host_entries_%d.npz" % guard))
            code = "import sys; sys.path[:0] = [%r, %r]; import conftest, test_gpu_extents as G; G.run_host_entries(%r)" % (
                os.path.dirname(here), here, path)
            env = {k: v for k, v in os.environ.items() if k != "LDSR_ARENA_GUARD"}
            if guard:
                env["LDSR_ARENA_GUARD"] = "1"
            try:
                p = subprocess.run([sys.executable, "-c", code], env=env, timeout=self.LIMIT)
            except subprocess.TimeoutExpired:
                self.dead = "the %s child ran into its time limit" % ("guarded" if guard else "plain")
                pytest.fail(self.dead)
            if p.returncode != 0:
                self.dead = "the %s child ended with status %d" % ("guarded" if guard else "plain", p.returncode)
                pytest.fail(self.dead)
            self.done[guard] = dict(np.load(path))
        return self.done[guard]


@pytest.fixture(scope="module")
def host_runs(tmp_path_factory):
    return HostRuns(tmp_path_factory.mktemp("extents"))


@pytest.mark.gpu
def test_guard_mode_reports_nothing_for_any_host_entry(host_runs):
    d = host_runs.get(1)
    reports = {k: v for k, v in d.items() if k.startswith("report:")}
    assert len(reports) >= 50, sorted(reports)
    bad = ["%s: %s" % (k[7:], v[1]) for k, v in sorted(reports.items()) if int(v[0]) != 0]
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_guard_mode_self_test_reports_exactly_one_violation(host_runs):
    rc, n, text = host_runs.get(1)["selftest"]
    assert int(rc) == 0 and int(n) == 1, (rc, n, text)
    assert "ldsr_arena_guard_selftest: band behind carve 0 " in text and "1 byte(s) changed, first at band offset 3, last at 3" in text, text
    rc, n, text = host_runs.get(0)["selftest"]          # off: no bands, the hook says so
    assert int(rc) == LDSR_EINVAL and int(n) == 0, (rc, n, text)


@pytest.mark.gpu
def test_guard_mode_changes_no_output_bit(host_runs):
    g, p = host_runs.get(1), host_runs.get(0)
    assert set(g) == set(p)
    outs = [k for k in g if not k.startswith("report:") and k != "selftest"]
    assert len(outs) > 200
    for k in sorted(outs):
        a, b = g[k], p[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k
        if a.dtype.kind == "f":
            assert np.array_equal(np.isnan(a), np.isnan(b)), k
    for k, v in p.items():
        if k.startswith("report:"):
            assert int(v[0]) == 0, k
