"""Kernarg preload moves where the kernels' arguments arrive, not what they compute: libtsgo_hip.so (built with the preload option,
csrc/tsgo_kernels.h "Argument heads") against libtsgo_hip_plain.so (the same sources without it, toyslam_amd/build.py: build_hip_plain),
one handle on each in one process, bit for bit.  The graphs are those of tests/precond_cases.py — one per branch of
Engine::launch_vcycle_v — and one with priors and a robust kernel set on every edge class."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import precond_cases as pc
from toyslam_amd import _lib, build
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu

CASES = dict(pc.CASES)
CASES["priors_robust"] = dict(graph=lambda: pc._mixed(True), env={}, kw=dict(odom_jacobian="analytic"),
                              robust=dict(all=("cauchy", 1.0), lm=("huber", 0.8), pose_prior=("geman_mcclure", 2.0)))


@pytest.fixture(scope="module")
def plain_lib():
    """libtsgo_hip_plain.so loaded by path, next to the product library (the way tests/research/bench_with_lib.py picks another build)."""
    if not os.path.exists(build.HIP_PLAIN_SO):
        pytest.fail("%s is missing — run __graft_entry__.build()" % build.HIP_PLAIN_SO)
    lib = C.CDLL(build.HIP_PLAIN_SO)
    _lib._declare_host(lib)
    _lib._declare_device(lib)
    return lib


def _run(monkeypatch, lib, case):
    with monkeypatch.context() as m:
        for k in pc.KNOBS:
            m.delenv(k, raising=False)
        for k, v in case["env"].items():
            m.setenv(k, v)
        if lib is not None:
            m.setattr(_lib, "hip_lib", lambda: lib)
        o = HipOptimizer(pcg_rel_tol=1e-10, **case["kw"])
        try:
            assert o.lib is (lib if lib is not None else _lib.hip_lib())
            if case.get("robust"):
                o.set_robust(**case["robust"])
            o.set_graph(case["graph"]())
            step = o.solve_step()
            opt = o.optimize(3)
            return step, opt, o.vertices()
        finally:
            o.close()


@pytest.mark.parametrize("name", list(CASES))
def test_preload_and_plain_builds_agree_bit_for_bit(name, plain_lib, monkeypatch):
    case = CASES[name]
    step_a, opt_a, v_a = _run(monkeypatch, None, case)
    step_b, opt_b, v_b = _run(monkeypatch, plain_lib, case)
    assert step_a["cg_iters"] > 0 and np.isfinite(step_a["delta"]).all() and np.abs(step_a["delta"]).max() > 0
    np.testing.assert_array_equal(step_a["delta"], step_b["delta"])
    np.testing.assert_array_equal(np.float64(step_a["chi2"]), np.float64(step_b["chi2"]))
    assert step_a["cg_iters"] == step_b["cg_iters"]
    assert opt_a["iters"] == opt_b["iters"] and opt_a["stop"] == opt_b["stop"]
    np.testing.assert_array_equal(opt_a["chi2"], opt_b["chi2"])
    np.testing.assert_array_equal(opt_a["cg_iters"], opt_b["cg_iters"])
    np.testing.assert_array_equal(v_a, v_b)
