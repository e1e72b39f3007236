"""tsgo_set_fixed / tsgo_get_fixed / tsgo_set_estimates (include/tsgo.h) without a GPU: the bindings through every layer, the helpers of
tests/vertex_edit.py against the dense numpy restatement (so that tests/test_gpu_vertex_edit.py cannot pass vacuously: the graph a fresh
handle is given there really is the original with k * 1e6 on the block of every re-fixed vertex), and the C++ wrapper's demo compiled and
run."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import edge_cases, robust, vertex_edit
from toyslam_amd import _lib, build
from toyslam_amd.optimizer import HipOptimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tsgo_set_fixed", "tsgo_get_fixed", "tsgo_set_estimates")
GAUGE = 1e6      # per occurrence in the fixed list (include/tsgo.h)


# ---- 1. bindings ----------------------------------------------------------------------------------------------------------------------
def test_every_layer_declares_the_three_entry_points():
    text = open(os.path.join(ROOT, "include", "tsgo.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.DEVICE_SYMBOLS and name not in _lib.HOST_SYMBOLS
    for method in ("set_fixed", "release", "fixed_counts", "set_vertices"):
        assert callable(getattr(HipOptimizer, method, None)), method
    s = _lib.tsgo_vertex_edit_stats
    assert [n for n, _t in s._fields_] == ["listed", "poses", "landmarks", "fixed_now", "released", "ms_total", "ms_host", "ms_device"]
    assert (s.listed.offset, s.fixed_now.offset, s.ms_total.offset, s.ms_device.offset, C.sizeof(s)) == (0, 24, 40, 56, 64)
    hpp = open(os.path.join(ROOT, "include", "tsgo.hpp")).read()
    for decl in ("void SetFixed(const std::vector<uint32_t>& ids,", "void Release(const std::vector<uint32_t>& ids,",
                 "std::vector<int32_t> FixedCounts(size_t n_vertices)", "void SetEstimates(const std::vector<uint32_t>& ids, const std::vector<double>& xyt,"):
        assert decl in hpp, decl


def test_the_built_libraries_export_them_and_refuse_a_null_handle():
    assert os.path.exists(build.HIP_SO), "libtsgo_hip.so is not built (run __graft_entry__.build())"
    libs = [_lib.hip_lib()] + ([_lib.hip_testing_lib()] if os.path.exists(build.HIP_TESTING_SO) else [])
    for lib in libs:
        for name in NAMES:
            assert hasattr(lib, name), name
        ids = np.zeros(1, np.uint32); cnt = np.ones(1, np.int32); pos = np.zeros(3)
        assert lib.tsgo_set_fixed(None, 1, ids.ctypes.data, cnt.ctypes.data, None) < 0 and b"tsgo_set_fixed" in lib.tsgo_last_error()
        assert lib.tsgo_get_fixed(None, cnt.ctypes.data, 1) < 0 and b"tsgo_get_fixed" in lib.tsgo_last_error()
        assert lib.tsgo_set_estimates(None, 1, ids.ctypes.data, pos.ctypes.data, None) < 0 and b"tsgo_set_estimates" in lib.tsgo_last_error()


# ---- 2. the helpers against the dense restatement ---------------------------------------------------------------------------------------
def test_refixed_is_the_dense_system_with_k_times_1e6_on_the_block():
    g = edge_cases.fixed_landmark_and_duplicate_fixed_ids()
    lm = g.v_id[g.v_type == 1]
    np.testing.assert_array_equal(g.fixed, [0, 0, lm[3], lm[3], lm[3], 7])
    before = vertex_edit.counts(g)
    assert before.sum() == 6 and sorted(before[before > 0]) == [1, 2, 3]
    ids = np.array([lm[3], 0, 11, lm[8], 7], np.uint32)      # release the landmark, 2 -> 1, fix a pose twice, fix a landmark, keep 7 at 1
    cnt = np.array([0, 1, 2, 1, 1])
    h = vertex_edit.refixed(g, ids, cnt)
    at = {int(v): k for k, v in enumerate(g.v_id)}
    want = before.copy()
    for i, k in zip(ids, cnt):
        want[at[int(i)]] = k
    np.testing.assert_array_equal(vertex_edit.counts(h), want)
    # canonical: vertex order, each id count times
    np.testing.assert_array_equal(h.fixed, np.repeat(g.v_id, want))
    assert h.fixed.dtype == np.uint32 and np.array_equal(g.fixed, [0, 0, lm[3], lm[3], lm[3], 7])      # g itself is untouched
    for name in ("v_id", "v_type", "v_pos", "e_type", "e_ids", "e_meas", "e_inf"):
        np.testing.assert_array_equal(getattr(h, name), getattr(g, name))
    H0, b0, chi0, off = robust.dense_system(g)
    H1, b1, chi1, off1 = robust.dense_system(h)
    np.testing.assert_array_equal(off, off1)
    expect = np.zeros(len(b0))
    for v in range(len(g.v_id)):
        expect[off[v]:off[v + 1]] = GAUGE * (float(want[v]) - float(before[v]))
    assert np.count_nonzero(expect) == 2 * 2 + 3 * 2      # two landmarks (one -3, one +1), two poses (-1, +2)
    # the terms are integers times 1e6 added to O(1e3) sums: the difference is exact to an ulp of the largest, 2.3e-10 at 2e6
    assert np.abs((H1 - H0) - np.diag(expect)).max() <= 1e-9
    np.testing.assert_array_equal(b0, b1)
    assert chi0 == chi1
    # the scalar form, and the round trip back to g's own counts
    np.testing.assert_array_equal(vertex_edit.counts(vertex_edit.refixed(g, [11, 12], 1)), before + np.isin(g.v_id, [11, 12]))
    back = vertex_edit.refixed(h, ids, [3, 2, 0, 0, 1])
    np.testing.assert_array_equal(vertex_edit.counts(back), before)
    np.testing.assert_array_equal(np.sort(back.fixed), np.sort(g.fixed))
    assert len(vertex_edit.refixed(g, [0, lm[3], 7], 0).fixed) == 0


def test_moved_replaces_the_listed_rows_and_nothing_else():
    g = edge_cases.shuffled_vertices_and_edges()[0]
    poses, lms = g.v_id[g.v_type == 0], g.v_id[g.v_type == 1]
    ids = np.r_[poses[[3, 0, 17]], lms[[5, 2]]]
    pos = np.arange(15, dtype=np.float64).reshape(5, 3) / 7.0
    h = vertex_edit.moved(g, ids, pos)
    at = {int(v): k for k, v in enumerate(g.v_id)}
    rows = [at[int(i)] for i in ids]
    np.testing.assert_array_equal(h.v_pos[rows[:3]], pos[:3])
    np.testing.assert_array_equal(h.v_pos[rows[3:], :2], pos[3:, :2])
    assert np.all(h.v_pos[rows[3:], 2] == 0)
    rest = np.setdiff1d(np.arange(len(g.v_id)), rows)
    np.testing.assert_array_equal(h.v_pos[rest], g.v_pos[rest])
    np.testing.assert_array_equal(h.fixed, g.fixed)
    assert robust.chi2_at(h) != robust.chi2_at(g)
    np.testing.assert_array_equal(vertex_edit.moved(h, None, g.v_pos).v_pos, g.v_pos)


# ---- 3. the C++ wrapper ---------------------------------------------------------------------------------------------------------------
def test_the_cpp_demo_compiles_and_fails_loudly_without_a_device(tmp_path):
    import torch
    lib_dir = os.path.join(ROOT, "toyslam_amd")
    if not os.path.exists(os.path.join(lib_dir, "libtsgo_hip.so")):
        pytest.fail("toyslam_amd/libtsgo_hip.so is not built (run __graft_entry__.build())")
    exe = str(tmp_path / "vertex_edit_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "vertex_edit_demo.cpp"), "-o", exe, "-L" + lib_dir, "-ltsgo_hip", "-Wl,-rpath," + lib_dir])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    if torch.cuda.is_available() or torch.cuda.device_count() > 0:
        assert p.returncode == 0, p.stderr      # a GPU is visible: the demo runs through
        assert "listed 2, released 1, fixed now 1; count of pose 0: 0, of pose 11: 1" in p.stdout, p.stdout
    else:
        assert p.returncode == 1
        assert "no CPU fallback" in p.stderr
