"""tsgo_set_edge_information / tsgo_get_edge_information (include/tsgo.h) without a GPU: the bindings through every layer, the C++
wrapper's demo compiled, and the two facts about the outlier scenario (tests/robust.py) that the device tests rely on, pinned on the
numpy restatement alone so that tests/test_gpu_edge_info.py cannot pass vacuously."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import edge_info, robust
from toyslam_amd import _lib, build
from toyslam_amd.optimizer import HipOptimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tsgo_set_edge_information", "tsgo_get_edge_information")


# ---- 1. bindings ----------------------------------------------------------------------------------------------------------------------
def test_every_layer_declares_the_two_entry_points():
    text = open(os.path.join(ROOT, "include", "tsgo.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.DEVICE_SYMBOLS and name not in _lib.HOST_SYMBOLS
    for method in ("set_edge_information", "edge_information", "disable_edges"):
        assert callable(getattr(HipOptimizer, method, None)), method
    s = _lib.tsgo_edge_info_stats
    assert [n for n, _t in s._fields_] == ["edges_listed", "edges_by_class", "maps_built", "reserved", "ms_total", "ms_host", "ms_device"]
    assert (s.edges_listed.offset, s.edges_by_class.offset, s.maps_built.offset, s.reserved.offset, s.ms_total.offset, C.sizeof(s)) == (0, 8, 48, 52, 56, 80)
    hpp = open(os.path.join(ROOT, "include", "tsgo.hpp")).read()
    assert "SetEdgeInformation(const std::vector<int64_t>& edges, const std::vector<double>& inf, tsgo_edge_info_stats* stats = nullptr)" in hpp
    assert re.search(r"std::vector<double> EdgeInformation\(\)", hpp)


def test_the_built_libraries_export_them_and_refuse_a_null_handle():
    assert os.path.exists(build.HIP_SO), "libtsgo_hip.so is not built (run __graft_entry__.build())"
    libs = [_lib.hip_lib()] + ([_lib.hip_testing_lib()] if os.path.exists(build.HIP_TESTING_SO) else [])
    for lib in libs:
        for name in NAMES:
            assert hasattr(lib, name), name
        w = np.ones(3)
        assert lib.tsgo_set_edge_information(None, 1, None, w.ctypes.data, None) < 0 and b"tsgo_set_edge_information" in lib.tsgo_last_error()
        assert lib.tsgo_get_edge_information(None, w.ctypes.data, 1) < 0 and b"tsgo_get_edge_information" in lib.tsgo_last_error()


def test_the_cpp_demo_compiles_against_the_wrapper(tmp_path):
    lib_dir = os.path.join(ROOT, "toyslam_amd")
    if not os.path.exists(os.path.join(lib_dir, "libtsgo_hip.so")):
        pytest.fail("toyslam_amd/libtsgo_hip.so is not built (run __graft_entry__.build())")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "edge_information_demo.cpp"), "-o", str(tmp_path / "edge_information_demo"),
                           "-L" + lib_dir, "-ltsgo_hip", "-Wl,-rpath," + lib_dir])


# ---- 2. the restatement facts the device tests rely on ---------------------------------------------------------------------------------
def test_the_report_after_the_cauchy_run_flags_exactly_the_false_closures():
    """dense_lm under SCENARIO["robust"] for SCENARIO["iterations"], then the report there: w < 0.01 on the 13 appended false closures
    (indices 263 .. 275) and nowhere else, with a wide margin on both sides (0.734 against 4.25e-5)."""
    at, w = edge_info.scenario_after_cauchy()
    false = edge_info.scenario_false_edges()
    flagged = np.where(w < edge_info.FLAG_BELOW)[0]
    true = np.setdiff1d(np.arange(len(w)), false)
    print("flagged %s; smallest true-edge weight %.4f, largest false-edge weight %.3e" % (flagged.tolist(), w[true].min(), w[false].max()))
    np.testing.assert_array_equal(false, np.arange(263, 276))
    np.testing.assert_array_equal(flagged, false)
    assert w[true].min() >= 0.73 and w[false].max() <= 4.3e-5


def test_zero_information_on_the_flagged_edges_is_the_clean_graph_bit_for_bit():
    """From the estimates of the Cauchy run: the scenario with e_inf = 0 on the 13 false closures and the clean scenario (which does not
    hold them) take the same dense_lm run under the default setting, bitwise: zero information adds exact zeros."""
    at, w = edge_info.scenario_after_cauchy()
    flagged = np.where(w < edge_info.FLAG_BELOW)[0]
    sc = robust.SCENARIO
    off = robust.dense_lm(edge_info.edited(at, np.zeros((len(flagged), 3)), flagged), None, sc["iterations"], lambda0=sc["lambda0"])
    clean = robust.scenario_clean(); clean.v_pos[:] = at.v_pos
    ref = robust.dense_lm(clean, None, sc["iterations"], lambda0=sc["lambda0"])
    from tests import util
    diff = util.max_vertex_diff(off["v_pos"], ref["v_pos"], at.v_type)
    print("max vertex difference %r, final chi2 %r (edges at zero) and %r (edges absent), %d trials, %s" % (diff, off["chi2"][-1], ref["chi2"][-1], off["iters"], off["stop"]))
    assert diff == 0.0 and np.array_equal(off["v_pos"], ref["v_pos"])
    assert off["chi2"][-1] == ref["chi2"][-1]      # (earlier entries may differ in the last bit: numpy sums 276 and 263 terms in other pairs)
    np.testing.assert_allclose(off["chi2"], ref["chi2"], rtol=1e-15)
    assert (off["iters"], off["stop"]) == (ref["iters"], ref["stop"])
    # the value the issue records (up to the last bits of another machine's dense solves)
    assert abs(off["chi2"][-1] - 6.283568458239522) <= 1e-9 * 6.283568458239522
