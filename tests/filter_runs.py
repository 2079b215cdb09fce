"""Running a case of tests/filter_cases.py on the device, through either entry of the C ABI (the helpers of
tests/test_gpu_filter.py and tests/test_gpu_filter_extents.py).  Both give the same dict: the requested rows
[n, T], lik [n], zstat [n, 2], status [n] and, with lags, acf [n, n_lags]."""
import ctypes as C

import numpy as np

import extents as X
import filter_model as FM

ROWS = FM.ROWS


def host_run(c, stdlik=True, n_lags=None, rows=ROWS, theta=None, device=0):
    """ldsr_filter_batch through ldsr_amd.filter_batch"""
    import ldsr_amd
    n_lags = c["n_lags"] if n_lags is None else n_lags
    th = c["theta"] if theta is None else theta
    r = ldsr_amd.filter_batch(c["Y"] if c["S"] > 1 else c["Y"][0], c["u"], c["v"], th, cell_offsets=list(c["off"]),
                              stdlik=stdlik, n_lags=n_lags, rows=rows, device=device)
    out = {k: r[k] for k in rows}
    out.update(lik=r["lik"], zstat=np.stack([r["zmean"], r["zvar"]], axis=1), status=r["status"])
    if n_lags > 0:
        out["acf"] = r["acf"]
    return out


def abi_inputs(c, theta=None):
    """the bytes the ABI takes: y [S][T], u / v time-major [S or 1][T][k] (absent: not in the dict), theta"""
    def tm(a):
        a = a[None] if a.ndim == 2 else a
        return np.ascontiguousarray(np.transpose(a, (0, 2, 1)))
    d = {"d_y": np.ascontiguousarray(c["Y"]), "d_theta": np.ascontiguousarray(c["theta"] if theta is None else theta)}
    if c["u"] is not None:
        d["d_u"] = tm(c["u"])
    if c["v"] is not None:
        d["d_v"] = tm(c["v"])
    return d


def shared_flag(c):
    return 1 if (c["S"] > 1 and all(a is None or a.ndim == 2 for a in (c["u"], c["v"]))) else 0


def workspace_bytes(c, n_lags):
    from ldsr_amd import _lib
    return _lib.lib().ldsr_filter_workspace_bytes(c["S"], c["T"], c["p"], c["q"], c["n"], n_lags)


def layout(c, inputs, rows, n_lags, wsb):
    n, T = c["n"], c["T"]
    bufs = [X.Buf(k, a.nbytes, a.shape[-1] * 8 * (T if k in ("d_u", "d_v") else 1), X.IN) for k, a in inputs.items()]
    bufs += [X.Buf(k, 8 * n * T, 8 * T, X.OUT, np.float64) for k in rows]
    bufs += [X.Buf("lik", 8 * n, 8, X.OUT, np.float64), X.Buf("zstat", 16 * n, 16, X.OUT, np.float64)]
    if n_lags > 0:
        bufs.append(X.Buf("acf", 8 * n * n_lags, 8 * n_lags, X.OUT, np.float64))
    bufs += [X.Buf("status", 4 * n, 4, X.OUT, np.int32), X.Buf("ws", wsb, 8 * T, X.WS)]
    return X.Layout(bufs)


def device_call(c, block, off, wsb, stdlik, n_lags):
    """ldsr_filter_batch_device on the block's buffers (a buffer that is not in `off` is passed as NULL) -> rc"""
    import torch
    from ldsr_amd import _lib

    def at(name):
        return C.c_void_p(block.base + off[name]) if name in off else None
    offs = (C.c_int * (c["S"] + 1))(*c["off"])
    return _lib.lib().ldsr_filter_batch_device(
        0, C.c_void_p(torch.cuda.current_stream().cuda_stream), c["S"], c["T"], c["p"], c["q"], at("d_y"), at("d_u"),
        at("d_v"), shared_flag(c), offs, at("d_theta"), int(stdlik), n_lags, *[at(k) for k in ROWS], at("lik"),
        at("zstat"), at("acf"), at("status"), at("ws"), wsb)


def shape_outputs(c, out, n_lags):
    n, T = c["n"], c["T"]
    r = {k: (v.reshape(n, T) if k in ROWS else v) for k, v in out.items()}
    r["zstat"] = r["zstat"].reshape(n, 2)
    if n_lags > 0:
        r["acf"] = r["acf"].reshape(n, n_lags)
    return r


def device_run(c, stdlik=True, n_lags=None, rows=ROWS, theta=None, guarded=False):
    """ldsr_filter_batch_device on torch memory; guarded: under extents.py's bands, once per fill pattern"""
    from ldsr_amd import _lib
    from test_gpu_extents import TorchBlock
    n_lags = c["n_lags"] if n_lags is None else n_lags
    inputs = abi_inputs(c, theta)
    wsb = workspace_bytes(c, n_lags)
    assert wsb > 0 and wsb % 256 == 0
    lay = layout(c, inputs, rows, n_lags, wsb)

    def call(block, off):
        rc = device_call(c, block, off, wsb, stdlik, n_lags)
        assert rc == 0, _lib.lib().ldsr_last_error().decode()
    if guarded:
        return shape_outputs(c, X.guarded(lay, inputs, call, make_block=TorchBlock), n_lags)
    block = TorchBlock(lay.image(0xFF, inputs))
    call(block, lay.off)
    return shape_outputs(c, lay.outputs(block.image()), n_lags)
