"""LDS_BFGS_with_update without a GPU: its two entries exist on every layer, their argument errors surface
before any device call, nothing computes on the host, and the pre-launch extent check of the new kernels
 names the field of a parameter struct that does not fit the call's block."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EHIP, EINTERNAL = 1, 2, 3, 5


def test_entries_are_declared_exported_and_bound():
    import ldsr_amd
    from ldsr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ldsr_hip.h")).read()
    so = C.CDLL(_lib.SO_PATH)
    for name in ("ldsr_pl_grad_batch", "ldsr_bfgs_update_batch"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES and hasattr(so, name), name
    assert len(_lib.SIGNATURES["ldsr_bfgs_update_batch"][1]) == len(_lib.SIGNATURES["ldsr_bfgs_batch"][1])
    assert callable(ldsr_amd.LDS_BFGS_with_update) and callable(ldsr_amd.bfgs_update_batch)
    assert callable(ldsr_amd.pl_grad)
    m = re.search(r"#define\s+LDSR_EINTERNAL\s+(\d+)", hdr)
    assert m and int(m.group(1)) == EINTERNAL


def _call(L, **kw):
    """ldsr_bfgs_update_batch on a tiny valid problem (T = 4, p = q = 1, 2 restarts) with single arguments replaced."""
    P = 8
    a = dict(device=0, n_series=1, T=4, p=1, q=1, y=(C.c_double * 4)(0.1, -0.2, 0.3, 0.0), u=None, v=None,
             shared_uv=0, off=(C.c_int * 2)(0, 2), par0=(C.c_double * (2 * P))(*([0.5] * (2 * P))),
             lb=(C.c_double * P)(*([0.1] * P)), ub=(C.c_double * P)(*([0.9] * P)), lam=1.0, maxit=10, lmm=5,
             factr=1e7, pgtol=0.0, select_max=1, winner=(C.c_int * 1)(), theta_w=(C.c_double * P)(),
             value_w=(C.c_double * 1)())
    a.update(kw)
    return L.ldsr_bfgs_update_batch(a["device"], a["n_series"], a["T"], a["p"], a["q"], a["y"], a["u"], a["v"],
                                    a["shared_uv"], a["off"], a["par0"], a["lb"], a["ub"], a["lam"], a["maxit"],
                                    a["lmm"], a["factr"], a["pgtol"], a["select_max"], None, None, None, None, None,
                                    a["winner"], a["theta_w"], a["value_w"], None, None, None, None, None)


def test_argument_errors_without_gpu():
    from ldsr_amd import _lib
    L = _lib.lib()
    P = 8

    def bounds(i, x):
        b = [0.5] * P
        b[i] = x
        return (C.c_double * P)(*b)

    cases = [
        (dict(lam=float("nan")), EINVAL, b"lambda must be finite"),
        (dict(lam=float("inf")), EINVAL, b"lambda must be finite"),
        (dict(lb=bounds(3, 0.95)), EINVAL, b"lb must be <= ub in every variable"),
        (dict(ub=bounds(7, float("nan"))), EINVAL, b"finite"),
        (dict(lb=None), EINVAL, b"lb and ub"),
        (dict(maxit=0), EINVAL, b"maxit must be >= 1"),
        (dict(lmm=0), EINVAL, b"lmm must be in 1 .. 8"),
        (dict(lmm=9), EINVAL, b"lmm must be in 1 .. 8"),
        (dict(factr=-1.0), EINVAL, b"factr"),
        (dict(pgtol=-1e-3), EINVAL, b"pgtol"),
        (dict(off=(C.c_int * 2)(1, 2)), EINVAL, b"cell_offsets[0]"),
        (dict(T=1), EINVAL, b"T must be"),
        (dict(p=17), EUNSUPPORTED, b"not supported"),
        (dict(y=None), EINVAL, b"y"),
        (dict(par0=None), EINVAL, b"par0 must not be NULL"),
        (dict(winner=None), EINVAL, b"winner, theta_w and value_w must not be NULL"),
        (dict(theta_w=None), EINVAL, b"winner, theta_w and value_w must not be NULL"),
        (dict(value_w=None), EINVAL, b"winner, theta_w and value_w must not be NULL"),
    ]
    for kw, code, msg in cases:
        rc = _call(L, **kw)
        assert rc == code, (kw.keys(), rc)
        assert msg in L.ldsr_last_error(), (kw.keys(), L.ldsr_last_error())
    # ... and of the objective's entry
    y, th, f = (C.c_double * 4)(0.1, -0.2, 0.3, 0.0), (C.c_double * P)(*([0.5] * P)), (C.c_double * 1)()
    off = (C.c_int * 2)(0, 1)
    for kw, code, msg in ((dict(T=1), EINVAL, b"T must be"), (dict(q=17), EUNSUPPORTED, b"not supported"),
                          (dict(theta=None), EINVAL, b"theta and pl must not be NULL"),
                          (dict(pl=None), EINVAL, b"theta and pl must not be NULL"),
                          (dict(lam=float("nan")), EINVAL, b"lambda must be finite"),
                          (dict(off=(C.c_int * 2)(1, 1)), EINVAL, b"cell_offsets[0]")):
        a = dict(T=4, p=1, q=1, theta=th, pl=f, off=off, lam=1.0)
        a.update(kw)
        assert L.ldsr_pl_grad_batch(0, 1, a["T"], a["p"], a["q"], y, None, None, 0, a["off"], a["theta"], a["lam"],
                                    a["pl"], None) == code, kw.keys()
        assert msg in L.ldsr_last_error(), (kw.keys(), L.ldsr_last_error())


def test_without_bounds_is_a_value_error():
    import ldsr_amd
    from ldsr_amd import synth
    src = open(os.path.join(ROOT, "ldsr_amd", "bfgs.py")).read()
    assert "plgrad_model" not in src and "bfgs_model" not in src and "oracle" not in src
    with pytest.raises(ValueError):
        ldsr_amd.LDS_BFGS_with_update(*synth.make_series(50, 1, 2))      # the reference stops without bounds too
    with pytest.raises(ValueError):
        ldsr_amd.LDS_BFGS_with_update(*synth.make_series(50, 1, 2), ub=np.full(9, 0.95))


def test_no_host_implementation():
    """A valid call without a GPU fails loudly (the rule of test_no_cpu_fallback)."""
    import ldsr_amd
    from ldsr_amd import _lib, synth
    if _lib.lib().ldsr_device_count() > 0:
        pytest.skip("a GPU is present: the calls below succeed")
    y, u, v = synth.make_series(50, 1, 2)
    lb, ub = np.full(9, 0.05), np.full(9, 0.95)
    with pytest.raises(_lib.LdsrError):
        ldsr_amd.pl_grad(y, u, v, np.full(9, 0.5), 1.0)
    with pytest.raises(_lib.LdsrError):
        ldsr_amd.bfgs_update_batch(y, u, v, np.full((3, 9), 0.5), lb, ub)
    with pytest.raises(_lib.LdsrError):
        ldsr_amd.LDS_BFGS_with_update(y, u, v, ub=ub, lb=lb, num_restarts=3, seed=1)
    L = _lib.lib()
    assert _call(L) == EHIP
    yy, th, f = (C.c_double * 4)(0.1, -0.2, 0.3, 0.0), (C.c_double * 8)(*([0.5] * 8)), (C.c_double * 1)()
    assert L.ldsr_pl_grad_batch(0, 1, 4, 1, 1, yy, None, None, 0, (C.c_int * 2)(0, 1), th, 1.0, f, None) == EHIP


# (kernel, n_series, T, p, q, has_u, has_v, shared_uv, cell_offsets, with_grad): T = 2 is the first device call of
# the GPU tests; then several series with an empty one, wide inputs, and more cells than waves
_SHAPES = [(0, 1, 2, 1, 1, 1, 1, 0, [0, 1], 0), (0, 1, 2, 1, 1, 1, 1, 0, [0, 1], 1), (1, 1, 2, 1, 1, 0, 0, 0, [0, 1], 1),
           (0, 3, 65, 3, 2, 1, 0, 1, [0, 0, 5, 7], 1), (1, 3, 65, 3, 2, 0, 1, 0, [0, 3, 5, 5], 1),
           (0, 2, 813, 16, 16, 1, 1, 0, [0, 100, 200], 1), (1, 1, 1639, 3, 3, 1, 1, 1, [0, 2500], 1)]


@pytest.mark.parametrize("shape", _SHAPES)
def test_extent_check_passes_the_entries_own_layout_and_names_what_does_not_fit(shape):
    from ldsr_amd import _lib
    L = _lib.lib()
    kernel, S, T, p, q, hu, hv, shared, off, with_grad = shape
    off = (C.c_int * len(off))(*off)

    def check(strip_short=0, out_shift=0):
        rc = L.ldsr_plg_extent_check(kernel, S, T, p, q, hu, hv, shared, off, with_grad, strip_short, out_shift)
        return rc, L.ldsr_last_error()

    assert check()[0] == 0
    rc, msg = check(strip_short=8)                      # the strip one double short
    assert rc == EINTERNAL and b"of strip," in msg and b"not launched" in msg, msg
    name = b"par" if kernel == 1 else b"grad"
    if kernel == 1 or with_grad:
        rc, msg = check(out_shift=1 << 30)              # the extent leaves the block
        assert rc == EINTERNAL and b"of " + name + b"," in msg, msg
        rc, msg = check(out_shift=-(1 << 30))
        assert rc == EINTERNAL and b"of " + name + b"," in msg, msg
    else:
        assert check(out_shift=1 << 30)[0] == 0         # (no grad: nothing to move)
