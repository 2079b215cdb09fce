"""The host/device functions of ldsr_amd/csrc/plgrad.h without a GPU: tests/plgrad_host/main.cpp, a stand-alone
program that includes plgrad.h only, is built with the address and undefined-behaviour sanitizers and run on
its own.  It walks the addressing of the kernels (both lane-to-step mappings cover every step once, every strip
offset lies inside the strip, the wave count times the strip is what the host reserves) and evaluates pl and
its gradient serially with the per-step functions the kernels call; the results must be the host model's
(tests/plgrad_model.py) on every case of test_plgrad_host.vg_cases(), under the project's own bars."""
import os
import subprocess

import numpy as np
import pytest

import plgrad_model as M
from conftest import parity_close
from test_plgrad_host import grad_close, vg_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def _fmt(a):
    return " ".join(repr(float(x)) for x in np.asarray(a, dtype=np.float64).reshape(-1))


def write_cases(path, cases):
    """the input file of main.cpp (its header comment has the format); u, v go time-major as in the C ABI"""
    rows = [(y, u, v, th, lam) for _, y, u, v, thetas, lam in cases for th in thetas]
    with open(path, "w") as f:
        f.write("%d\n" % len(rows))
        for y, u, v, th, lam in rows:
            p, q = (1 if u is None else u.shape[0]), (1 if v is None else v.shape[0])
            f.write("%d %d %d %d %d %r\n" % (y.size, p, q, u is not None, v is not None, float(lam)))
            f.write(_fmt(y) + "\n")
            if u is not None:
                f.write(_fmt(u.T) + "\n")
            if v is not None:
                f.write(_fmt(v.T) + "\n")
            f.write(_fmt(th) + "\n")
    return rows


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("plgrad_host")
    exe = str(d / "plgrad_host")
    r = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Xarch_host",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "ldsr_amd", "csrc"),
                        os.path.join(ROOT, "tests", "plgrad_host", "main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe, d


def _run(exe, *args):
    env = dict(os.environ)      # (the program carries its sanitizer runtime itself)
    env["ASAN_OPTIONS"] = "detect_leaks=1:halt_on_error=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def test_addressing_walk_is_clean(program):
    exe, _ = program
    assert _run(exe) == ""


def test_step_functions_give_the_models_value_and_gradient(program):
    exe, d = program
    path = str(d / "cases.txt")
    rows = write_cases(path, vg_cases())
    out = _run(exe, path).strip().split("\n")
    assert len(out) == len(rows)
    for line, (y, u, v, th, lam) in zip(out, rows):
        got = np.array([float(x) for x in line.split()])
        f, g = M.pl_grad(th, y, u, v, lam)
        assert got.size == 1 + th.size
        assert np.isfinite(got[0]) and parity_close(got[0], f), (y.size, th[0], got[0], f)
        assert grad_close(got[1:], g, scale=1), (y.size, th[0], got[1:], g)
        p, q = (1 if u is None else u.shape[0]), (1 if v is None else v.shape[0])
        zero = ([1] if u is None else []) + ([2 + p] if v is None else [])
        assert np.all(got[1:][zero] == 0.0)
