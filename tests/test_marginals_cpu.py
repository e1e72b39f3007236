"""tsgo_marginals at the boundary, without a device: declared, bound, exported, and safe on a NULL handle."""
import ctypes as C
import os
import re
import subprocess

import pytest

from toyslam_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_in_the_header_and_listed_in_the_bindings():
    h = open(os.path.join(ROOT, "include", "tsgo.h")).read()
    assert re.search(r"\bint\s+tsgo_marginals\s*\(", h)
    assert "tsgo_marginal_stats" in h
    assert "tsgo_marginals" in _lib.DEVICE_SYMBOLS
    names = [f for f, _t in _lib.tsgo_marginal_stats._fields_]
    assert names == ["columns", "batches", "batch_width", "pcg_iters_max", "pcg_iters_total", "preconditioner", "fallbacks", "ms_total", "ms_solve"]


def test_the_library_exports_it():
    so = build.build_hip()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT tsgo_marginals\b", out)


def test_null_handle_returns_an_error():
    L = _lib.hip_lib()
    cov = (C.c_double * 9)()
    ids = (C.c_uint32 * 1)(0)
    st = _lib.tsgo_marginal_stats()
    assert L.tsgo_marginals(None, C.cast(ids, C.c_void_p), 1, 0.0, C.cast(cov, C.c_void_p), C.byref(st)) < 0
    assert b"null" in L.tsgo_last_error()


def test_the_wrapper_has_the_method():
    from toyslam_amd.optimizer import HipOptimizer
    assert callable(getattr(HipOptimizer, "marginals", None))
