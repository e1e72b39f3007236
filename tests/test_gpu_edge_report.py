"""The per-edge residual report (tsgo_edge_report, include/tsgo.h) on the device (`-m gpu`) against the numpy restatement
(tests/edge_report.py): records under every robust kernel and every OJ / PRI / RK instantiation, every edge written once and in input
order, the per-class summary with its arg-max tie rule, the state rule, structure reuse, the outlier scenario end to end, the f32 mode
and the error cases.  Graphs: the 150-pose c1 golden widened to all five edge classes (robust.c1_five_classes) and the outlier scenario
qualified in tests/test_edge_report_cpu.py.

Bounds (f64): e 1e-12 x max(1, largest |vertex coordinate|) — rounding in e scales with the coordinates it subtracts; s and rho 1e-11 of
the class's largest s, the project's bound for a single chi^2; w 1e-11.  f32: 1e-4 on the same scales."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import edge_report, lm_rules, robust
from tests.test_gpu_robust import SETTINGS, VARIANTS
from tests.test_robust_cpu import scenario_references
from toyslam_amd import _lib
from toyslam_amd.graph import GraphArrays
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu

F64 = (1e-12, 1e-11, 1e-11)
F32 = (1e-4, 1e-4, 1e-4)


@functools.lru_cache(maxsize=None)
def _graph(vlm=True, with_priors=True):
    return robust.c1_five_classes(vlm, with_priors)


@functools.lru_cache(maxsize=None)
def _ref(vlm, with_priors, name):
    return edge_report.report(_graph(vlm, with_priors), SETTINGS[name])


def _handle(setting=None, **kw):
    kw.setdefault("pcg_rel_tol", 1e-12)
    o = HipOptimizer(**kw)
    if setting is not None:
        o.set_robust(**setting)
    return o


def _device(g, setting=None, **kw):
    o = _handle(setting, **kw)
    try:
        o.set_graph(g)
        rec, summ = o.edge_report()
    finally:
        o.close()
    return rec["all"], summ


def _assert_summary(got, ref, what=""):
    for c in robust.CLASSES:
        a, b = got[c], ref[c]
        print(what, c, a, b)
        assert (a["edges"], a["downweighted"], a["s_max_edge"]) == (b["edges"], b["downweighted"], b["s_max_edge"]), (what, c)
        for f in ("s_sum", "rho_sum", "s_max"):
            assert abs(a[f] - b[f]) <= 1e-11 * abs(b[f]), (what, c, f)
    assert abs(got["chi2"] - ref["chi2"]) <= 1e-11 * ref["chi2"], what


def _permuted(g, perm):
    return GraphArrays(g.v_id, g.v_type, g.v_pos.copy(), g.e_type[perm], g.e_ids[perm], g.e_meas[perm], g.e_inf[perm], g.fixed)


# ---- 1 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_records_match_the_restatement(name):
    for (vlm, pri), lanes, jac in VARIANTS:
        g = _graph(vlm, pri)
        rec, summ = _device(g, SETTINGS[name], lanes_per_pose=lanes, lanes_per_lm=lanes, odom_jacobian=jac)
        ref, ref_summ = _ref(vlm, pri, name)
        what = "%s vlm %d priors %d lanes %d %s" % (name, vlm, pri, lanes, jac)
        edge_report.assert_records(rec, ref, g, *F64, what=what)
        assert [summ[c]["edges"] for c in robust.CLASSES] == [ref_summ[c]["edges"] for c in robust.CLASSES], what


def test_the_default_setting_runs_the_compile_time_huber():
    """No set_robust at all: the RK = 0 instantiations."""
    for (vlm, pri), lanes, jac in VARIANTS:
        g = _graph(vlm, pri)
        rec, summ = _device(g, None, lanes_per_pose=lanes, lanes_per_lm=lanes, odom_jacobian=jac)
        ref, ref_summ = edge_report.report(g, None)
        edge_report.assert_records(rec, ref, g, *F64, what="default vlm %d priors %d lanes %d %s" % (vlm, pri, lanes, jac))
        _assert_summary(summ, ref_summ, "default")


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------
def test_every_edge_is_written_and_nothing_behind_the_last():
    g = _graph()
    E = len(g.e_type)
    guard = 8
    buf = np.full(6 * E + guard, np.nan)
    sentinel = np.full(guard, -12345.678)
    buf[6 * E:] = sentinel
    o = _handle(robust.MIXED)
    try:
        o.set_graph(g)
        _lib.check(o.lib, o.lib.tsgo_edge_report(o.h, buf.ctypes.data, E, None), "tsgo_edge_report")      # stats may be NULL
    finally:
        o.close()
    assert np.all(np.isfinite(buf[:6 * E]))
    np.testing.assert_array_equal(buf[6 * E:].view(np.uint64), sentinel.view(np.uint64))
    edge_report.assert_records(buf[:6 * E].reshape(E, 6), _ref(True, True, "mixed")[0], g, *F64, what="NaN-filled buffer")


# ---- 3 --------------------------------------------------------------------------------------------------------------------------------
def test_the_report_follows_a_permutation_of_the_edge_list():
    g = _graph()
    E = len(g.e_type)
    perm = np.random.default_rng(17).permutation(E)
    rec, summ = _device(g, robust.MIXED)
    rec_p, summ_p = _device(_permuted(g, perm), robust.MIXED)
    edge_report.assert_records(rec_p, rec[perm], _permuted(g, perm), *F64, what="permuted against the device's own report, permuted")
    edge_report.assert_records(rec_p, _ref(True, True, "mixed")[0][perm], _permuted(g, perm), *F64, what="permuted against the restatement")
    inv = np.argsort(perm)
    for c in robust.CLASSES:
        assert summ_p[c]["s_max_edge"] == inv[summ[c]["s_max_edge"]], c
        assert summ_p[c]["edges"] == summ[c]["edges"] and summ_p[c]["downweighted"] == summ[c]["downweighted"]


# ---- 4 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "cauchy_0.5", "none_1.5"])
def test_the_summary_matches_and_the_summary_only_call_returns_the_same(name):
    g = _graph()
    o = _handle(SETTINGS[name])
    try:
        o.set_graph(g)
        none, only = o.edge_report(records=False)
        rec, full = o.edge_report()
        _d, _g, chi = o.linearize()
        us, nbytes = o.time_kernel(8, reps=3)
        _rec2, again = o.edge_report()
    finally:
        o.close()
    assert none is None and rec is not None
    _assert_summary(full, _ref(True, True, name)[1], name)
    assert only == full                                            # field for field, bit for bit: the same pass without its stores
    assert again == full                                           # (the timing probe leaves the estimates where they were)
    print("chi2: report %.9f, linearize %.9f; summary-only pass %.1f us, %.0f bytes" % (full["chi2"], chi, us, nbytes))
    assert abs(full["chi2"] - chi) <= 1e-11 * chi
    assert us > 0 and nbytes > 0


# ---- 5 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["odom", "lm", "virtual", "pose_prior", "lm_prior"])
@pytest.mark.parametrize("where", ["appended", "prepended"])
def test_equal_maxima_report_the_lowest_index(cls, where):
    """The class's worst edge (by the restatement) a second time, behind every other edge or in front of them: two candidates with the same s
    bit for bit, in different slots (lanes, waves or workgroups); the lower input index is the one reported."""
    g = _graph()
    E = len(g.e_type)
    worst = _ref(True, True, "mixed")[1][cls]["s_max_edge"]
    order = np.r_[np.arange(E), worst] if where == "appended" else np.r_[worst, np.arange(E)]
    g2 = _permuted(g, order)
    want = worst if where == "appended" else 0
    other = E if where == "appended" else worst + 1
    for lanes in (1, 8):
        rec, summ = _device(g2, robust.MIXED, lanes_per_pose=lanes, lanes_per_lm=lanes)
        assert rec[want, 3] == rec[other, 3] == summ[cls]["s_max"], (cls, where, lanes)
        assert summ[cls]["s_max_edge"] == want, (cls, where, lanes, summ[cls])
        assert summ[cls]["edges"] == _ref(True, True, "mixed")[1][cls]["edges"] + 1


# ---- 6 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rules", ["cpp", "lm"])
def test_the_report_changes_nothing_the_optimizer_reads(rules):
    g = _graph()
    kw = dict(rules="lm", odom_jacobian="analytic") if rules == "lm" else {}
    out = []
    for with_report in (False, True):
        o = _handle(robust.MIXED, **kw)
        try:
            o.set_graph(g)
            if with_report:
                o.edge_report(); o.edge_report(records=False)
            r = o.optimize(5)
            if with_report:
                o.edge_report()
            out.append((r, o.vertices()))
        finally:
            o.close()
    (ra, va), (rb, vb) = out
    np.testing.assert_array_equal(va, vb)
    np.testing.assert_array_equal(ra["chi2"], rb["chi2"]); np.testing.assert_array_equal(ra["cg_iters"], rb["cg_iters"])
    assert (ra["iters"], ra["stop"]) == (rb["iters"], rb["stop"])


# ---- 7 --------------------------------------------------------------------------------------------------------------------------------
def test_the_maps_survive_a_reused_structure_and_are_rebuilt_for_a_new_one():
    g = _graph()
    moved = lm_rules.perturbed(g, seed=1, sigma_xy=0.05, sigma_th=0.01)
    other = _permuted(_graph(False, True), np.random.default_rng(3).permutation(len(_graph(False, True).e_type)))
    o = _handle(robust.MIXED)
    try:
        o.set_graph(g)
        rec, _ = o.edge_report()
        edge_report.assert_records(rec["all"], _ref(True, True, "mixed")[0], g, *F64, what="first graph")
        for graph, reused in ((moved, True), (other, False)):
            o.set_graph(graph)
            rec, summ = o.edge_report()
            ref, ref_summ = edge_report.report(graph, robust.MIXED)
            edge_report.assert_records(rec["all"], ref, graph, *F64, what="reused %d" % reused)
            _assert_summary(summ, ref_summ, "reused %d" % reused)
            assert bool(o.optimize(1)["structure_reused"]) == reused
        assert np.abs(edge_report.records(moved, robust.MIXED)[:, 3] - _ref(True, True, "mixed")[0][:, 3]).max() > 1e-3      # (the estimates did move)
    finally:
        o.close()


# ---- 8 --------------------------------------------------------------------------------------------------------------------------------
def test_the_scenario_end_to_end_names_the_false_closures():
    g, _clean, _default, _cauchy = scenario_references()
    sc = robust.SCENARIO
    E = len(g.e_type)
    n_false = E - len(robust.scenario_clean().e_type)
    o = _handle(sc["robust"], rules="lm", odom_jacobian="analytic", lm_lambda0=sc["lambda0"])
    try:
        o.set_graph(g)
        r = o.optimize(sc["iterations"])
        rec, summ = o.edge_report()
        v = o.vertices()
    finally:
        o.close()
    at = g.copy(); at.v_pos[:] = v
    ref, ref_summ = edge_report.report(at, sc["robust"])
    low = np.where(rec["w"] < 0.5)[0]
    print("%d trials, %s; w of the false closures %.2e .. %.2e, of the true edges >= %.3f; down-weighted ODOM edges %d (restatement %d)"
          % (r["iters"], r["stop"], rec["w"][-n_false:].min(), rec["w"][-n_false:].max(), rec["w"][:-n_false].min(), summ["odom"]["downweighted"], ref_summ["odom"]["downweighted"]))
    assert n_false == 13
    np.testing.assert_array_equal(low, np.arange(E - n_false, E))
    assert summ["odom"]["downweighted"] == ref_summ["odom"]["downweighted"]
    edge_report.assert_records(rec["all"], ref, at, *F64, what="scenario, at the device's end point")


# ---- 9 --------------------------------------------------------------------------------------------------------------------------------
def test_precision_32_records():
    for (vlm, pri), lanes, jac in VARIANTS[:2]:
        g = _graph(vlm, pri)
        rec, summ = _device(g, robust.MIXED, precision=32, pcg_rel_tol=1e-5, lanes_per_pose=lanes, lanes_per_lm=lanes, odom_jacobian=jac)
        ref, ref_summ = _ref(vlm, pri, "mixed")
        edge_report.assert_records(rec, ref, g, *F32, what="f32 mixed lanes %d %s" % (lanes, jac))
        assert [summ[c]["edges"] for c in robust.CLASSES] == [ref_summ[c]["edges"] for c in robust.CLASSES]
        assert abs(summ["chi2"] - ref_summ["chi2"]) <= 1e-4 * ref_summ["chi2"]


# ---- 10 -------------------------------------------------------------------------------------------------------------------------------
def test_errors_are_refused_with_a_message_and_change_nothing():
    g = _graph()
    E = len(g.e_type)
    o = _handle(robust.MIXED)
    lib = o.lib
    st = _lib.tsgo_edge_report_stats()
    buf = np.zeros(6 * E)

    def refused(rc, *words):
        msg = lib.tsgo_last_error().decode()
        assert rc < 0 and "tsgo_edge_report" in msg and all(w in msg for w in words), (rc, msg)
    try:
        refused(lib.tsgo_edge_report(None, buf.ctypes.data, E, C.byref(st)), "null handle")
        refused(lib.tsgo_edge_report(o.h, buf.ctypes.data, E, C.byref(st)), "no graph set")
        o.set_graph(g)
        before = o.edge_report()
        refused(lib.tsgo_edge_report(o.h, None, 0, None), "both NULL")
        refused(lib.tsgo_edge_report(o.h, buf.ctypes.data, E - 1, C.byref(st)), "cap_edges", str(E))
        refused(lib.tsgo_edge_report(o.h, buf.ctypes.data, 0, None), "cap_edges")
        assert not buf.any()                                                      # a refused call writes nothing
        after = o.edge_report()
        np.testing.assert_array_equal(before[0]["all"], after[0]["all"])
        assert before[1] == after[1]
        assert lib.tsgo_edge_report(o.h, None, 0, C.byref(st)) == 0                # summary only: the capacity is not looked at
    finally:
        o.close()
    shard = HipOptimizer(world=2, rank=0, testing=True)
    try:
        rc = shard.lib.tsgo_edge_report(shard.h, None, 0, C.byref(st))
        msg = shard.lib.tsgo_last_error().decode()
        assert rc < 0 and "tsgo_edge_report: edge-sharded handles (world > 1) are not supported" in msg, msg
        with pytest.raises(RuntimeError, match="world > 1"):
            shard.edge_report(records=False)
    finally:
        shard.close()
