"""The per-edge residual report (tsgo_edge_report, include/tsgo.h) on the host side: the numpy restatement (tests/edge_report.py) against
the references that exist already, the device's per-slot arithmetic (tsgo_math.h: the edge functions and edge_record) compiled for the
host against the restatement, and the outlier scenario the GPU test runs, qualified on the dense reference alone."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import edge_report, robust
from tests.test_robust_cpu import scenario_references
from toyslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {0: "none", 1: ("huber", 1.5), 2: ("cauchy", 1.5), 3: ("geman_mcclure", 1.5), -1: ("huber", 1.5)}      # -1: the compile-time default


@functools.lru_cache(maxsize=None)
def _graph():
    return robust.c1_five_classes(True, True)


# ---- 1. the restatement against robust.py ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["mixed", "default"])
def test_the_restatement_sums_to_the_existing_chi2(setting):
    g = _graph()
    s = robust.MIXED if setting == "mixed" else None
    rec, summ = edge_report.report(g, s)
    assert set(np.unique(g.e_type)) == {0, 1, 2, 3, 4} and rec.shape == (len(g.e_type), 6)
    want = float(robust.chi2_at(g, s))
    per_class = robust.class_chi2(g, s)
    print("chi2 %.9f against %.9f" % (summ["chi2"], want), {c: (summ[c]["rho_sum"], per_class[c]) for c in robust.CLASSES})
    assert abs(rec[:, 4].sum() - want) <= 1e-12 * want and abs(summ["chi2"] - want) <= 1e-12 * want
    for c in robust.CLASSES:
        assert abs(summ[c]["rho_sum"] - per_class[c]) <= 1e-12 * per_class[c], c
        assert summ[c]["edges"] == int((g.e_type == robust.CLASSES.index(c)).sum()) > 0
    assert np.all(rec[:, 5] > 0) and np.all(rec[:, 5] <= 1) and np.all(rec[:, 4] <= rec[:, 3] * (1 + 1e-15))
    assert np.all(rec[np.isin(g.e_type, edge_report.TWO_COMPONENTS), 2] == 0)


def test_the_bindings_declare_the_report():
    assert "tsgo_edge_report" in _lib.DEVICE_SYMBOLS
    import ctypes as C
    c, s = _lib.tsgo_edge_class_summary, _lib.tsgo_edge_report_stats
    assert [n for n, _t in c._fields_] == list(edge_report.FIELDS) and C.sizeof(c) == 48
    assert (s.cls.offset, s.chi2.offset, s.ms_total.offset, C.sizeof(s)) == (0, 240, 248, 256)


# ---- 2. the device arithmetic on the host ---------------------------------------------------------------------------------------------
def device_inputs(g):
    """Per edge the 17 numbers tests/cpp/edge_report_dump.cpp reads: the edge's inputs in the form the device tables hold them."""
    order = np.argsort(g.v_id, kind="stable")
    i1 = order[np.searchsorted(g.v_id[order], g.e_ids[:, 0])]
    i2 = order[np.searchsorted(g.v_id[order], g.e_ids[:, 1])]
    out = np.zeros((len(g.e_type), 17))

    def pose(i):
        x = g.v_pos[i]
        return [x[0], x[1], np.cos(x[2]), np.sin(x[2])]
    for k, t in enumerate(g.e_type):
        m, w = g.e_meas[k], g.e_inf[k]
        if t == 0:
            v = pose(i1[k]) + pose(i2[k]) + list(np.linalg.inv(m.reshape(3, 3))[:2].reshape(-1)) + list(w)
        elif t == 1:
            assert g.v_type[i1[k]] == 0 and g.v_type[i2[k]] == 1
            v = pose(i1[k]) + list(g.v_pos[i2[k], :2]) + [m[0] * np.cos(m[1]), m[0] * np.sin(m[1]), w[0], w[1]]
        elif t == 2:
            v = pose(i1[k]) + pose(i2[k]) + [m[0] * np.cos(m[1]), m[0] * np.sin(m[1]), m[2] * np.cos(m[3]), m[2] * np.sin(m[3]), w[0], w[1]]
        elif t == 3:
            v = [m[0], m[1], np.cos(m[2]), np.sin(m[2]), w[0], w[1], w[2]] + pose(i1[k])
        else:
            v = [m[0], m[1], w[0], w[1]] + list(g.v_pos[i1[k], :2])
        out[k, :len(v)] = v
    return out


@pytest.fixture(scope="module")
def host_records(tmp_path_factory):
    """{kind: (E, 12)}: what edge_report_dump printed for every edge of the five-class graph under each kernel; compiled and run once."""
    d = tmp_path_factory.mktemp("edge_report")
    exe = str(d / "edge_report_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "toyslam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "edge_report_dump.cpp"), "-o", exe])
    g = _graph()
    inputs = device_inputs(g)
    lines = []
    for kind, kernel in KINDS.items():
        delta = 0.0 if kernel == "none" else kernel[1]
        for t, v in zip(g.e_type, inputs):
            lines.append("%d %d %r %s\n" % (t, kind, delta, " ".join(repr(float(x)) for x in v)))
    path = d / "edges.txt"
    path.write_text("".join(lines))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, check=True).stdout.split("\n")
    vals = np.array([[float.fromhex(x) for x in ln.split()] for ln in out if ln])
    assert vals.shape == (len(lines), 12)
    E = len(g.e_type)
    return {kind: vals[n * E:(n + 1) * E] for n, kind in enumerate(KINDS)}


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_edge_record_on_the_host_matches_the_restatement(host_records, kind):
    """All five classes under each kernel.  f64: e 1e-12 x the coordinate scale, s and rho 1e-11 of the class's largest s, w 1e-11.  The f32
    instantiation (what a precision = 32 handle runs) against the f64 restatement: 1e-4 on the same scales."""
    g = _graph()
    ref = edge_report.records(g, robust.everywhere(KINDS[kind]))
    got = host_records[kind]
    edge_report.assert_records(got[:, :6], ref, g, 1e-12, 1e-11, 1e-11, "host f64, kind %d" % kind)
    edge_report.assert_records(got[:, 6:], ref, g, 1e-4, 1e-4, 1e-4, "host f32, kind %d" % kind)
    if kind == -1:
        np.testing.assert_array_equal(got, host_records[1])      # HuberDefault is Robust{HUBER, 1.5} bit for bit


# ---- 3. the outlier scenario ----------------------------------------------------------------------------------------------------------
def test_the_weights_separate_the_false_closures_under_cauchy_and_not_under_the_default():
    g, _clean, default, cauchy = scenario_references()
    n_false = len(g.e_type) - len(robust.scenario_clean().e_type)
    E = len(g.e_type)
    assert n_false == 13
    at = g.copy(); at.v_pos[:] = cauchy["v_pos"]
    rec, summ = edge_report.report(at, robust.SCENARIO["robust"])
    low = np.where(rec[:, 5] < 0.5)[0]
    print("cauchy on ODOM: false closures w %.2e .. %.2e, s >= %.3e; true edges w >= %.3f, s <= %.3f"
          % (rec[-n_false:, 5].min(), rec[-n_false:, 5].max(), rec[-n_false:, 3].min(), rec[:-n_false, 5].min(), rec[:-n_false, 3].max()))
    np.testing.assert_array_equal(low, np.arange(E - n_false, E))
    assert summ["odom"]["s_max_edge"] >= E - n_false and summ["odom"]["downweighted"] >= n_false
    at.v_pos[:] = default["v_pos"]
    rec0, _ = edge_report.report(at, None)
    print("default: false closures w >= %.3f, true edges w >= %.3f" % (rec0[-n_false:, 5].min(), rec0[:-n_false, 5].min()))
    assert not np.any(rec0[-n_false:, 5] < 0.5)
