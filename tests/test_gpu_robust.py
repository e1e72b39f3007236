"""Selectable robust kernels per edge class (tsgo_set_robust, include/tsgo.h) on the device (`-m gpu`): the default path bit for bit, the
linearisation, one solve, the rules = 0 and rules = 2 loops, marginals and the f32 mode against the numpy restatement (tests/robust.py),
and what the setting does across set_graph and between optimize calls.  Graphs: the 150-pose c1 golden widened to all five edge
classes (robust.c1_five_classes) and the outlier scenario qualified in tests/test_robust_cpu.py.

Tolerances are the project's own for the same quantities (tests/test_gpu_priors.py, tests/test_gpu_lm_rules.py): blocks and gradient
1e-12 of the largest entry, a single chi^2 1e-11 relative, chi^2 traces 1e-9, vertices 1e-8, covariances 1e-8 of the largest entry."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import lm_rules, robust, util
from tests.test_robust_cpu import scenario_references
from toyslam_amd import _lib
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu

SETTINGS = {"%s_%s" % (k, d): robust.everywhere("none" if k == "none" else (k, d)) for k in ("none", "huber", "cauchy", "geman_mcclure") for d in (1.5, 0.5)}
SETTINGS["mixed"] = robust.MIXED
# (graph: vlm, priors), lanes per pose / landmark, ODOM Jacobians: every RK = 1 instantiation of the OJ and PRI axes, at 1 and at 8 lanes
VARIANTS = [((True, True), 1, "constant"), ((True, True), 8, "analytic"), ((False, False), 8, "constant"), ((False, True), 1, "constant"),
            ((True, False), 0, "analytic"), ((False, False), 1, "analytic")]


@functools.lru_cache(maxsize=None)
def _graph(vlm, with_priors):
    return robust.c1_five_classes(vlm, with_priors)


@functools.lru_cache(maxsize=None)
def _ref_lin(vlm, with_priors, name, jacobian):
    with lm_rules._Jacobians(jacobian):
        return robust.linearisation(_graph(vlm, with_priors), SETTINGS[name])


def _handle(setting=None, **kw):
    kw.setdefault("pcg_rel_tol", 1e-12)
    o = HipOptimizer(**kw)
    if setting is not None:
        o.set_robust(**setting)
    return o


def _assert_lin(got, ref, tol, chi_tol, what):
    (d, g, c), (d0, g0, c0) = got, ref
    # a block against its own largest entry (the fixed vertex's carries the 1e6 gauge term), the gradient against its largest entry
    ed = (np.abs(d - d0).max(1) / np.abs(d0).max(1)).max(); eg = np.abs(g - g0).max() / np.abs(g0).max(); ec = abs(c - c0) / c0
    print("%s: blocks %.2e of the block's largest entry, gradient %.2e of the largest entry, chi2 %.2e relative (chi2 %.6f)" % (what, ed, eg, ec, c0))
    assert ed <= tol and eg <= tol and ec <= chi_tol, what


# ---- 1 --------------------------------------------------------------------------------------------------------------------------------
def test_the_default_given_explicitly_changes_no_bit():
    g = _graph(True, True)
    out = []
    for explicit in (False, True):
        o = _handle(dict(all=("huber", 1.5)) if explicit else None)
        try:
            assert o.robust == robust.DEFAULT
            o.set_graph(g)
            out.append((o.linearize(), o.optimize(5), o.vertices()))
        finally:
            o.close()
    (la, ra, va), (lb, rb, vb) = out
    for a, b in zip(la, lb):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ra["chi2"], rb["chi2"]); np.testing.assert_array_equal(ra["cg_iters"], rb["cg_iters"])
    np.testing.assert_array_equal(va, vb)


# ---- 2 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_linearisation_matches_the_restatement(name):
    for (vlm, pri), lanes, jac in VARIANTS:
        o = _handle(SETTINGS[name], lanes_per_pose=lanes, lanes_per_lm=lanes, odom_jacobian=jac)
        try:
            o.set_graph(_graph(vlm, pri))
            got = o.linearize()
        finally:
            o.close()
        _assert_lin(got, _ref_lin(vlm, pri, name, jac), 1e-12, 1e-11, "%s vlm %d priors %d lanes %d %s" % (name, vlm, pri, lanes, jac))


def test_the_mixed_setting_differs_from_huber_in_every_class():
    g = _graph(True, True)
    mixed, huber = robust.class_chi2(g, robust.MIXED), robust.class_chi2(g, None)
    print(mixed, huber)
    for c in robust.CLASSES:
        assert abs(mixed[c] - huber[c]) > 1e-3 * huber[c] > 0, c
    o = _handle(robust.MIXED)
    try:
        o.set_graph(g)
        assert o.robust == robust.full(robust.MIXED)
        _d, _g, chi = o.linearize()
    finally:
        o.close()
    assert abs(chi - sum(mixed.values())) <= 1e-11 * chi


# ---- 3 --------------------------------------------------------------------------------------------------------------------------------
def test_solve_step_under_the_mixed_setting_solves_the_dense_system():
    g = _graph(True, True)
    H, b, chi, _off = robust.dense_system(g, robust.MIXED)
    o = _handle(robust.MIXED)
    try:
        o.set_graph(g); s = o.solve_step()
    finally:
        o.close()
    mask = np.arange(3)[None, :] < np.where(g.v_type == 0, 3, 2)[:, None]
    res = np.linalg.norm(H @ s["delta"][mask] - b) / np.linalg.norm(b)
    print("||H delta - b|| / ||b|| = %.2e, %d PCG iterations" % (res, s["cg_iters"]))
    assert res < 1e-9 and abs(s["chi2"] - chi) <= 1e-11 * chi


# ---- 4 --------------------------------------------------------------------------------------------------------------------------------
def test_rules_0_under_cauchy_matches_the_dense_gauss_newton_loop():
    g = _graph(True, True)
    setting = robust.everywhere(("cauchy", 1.0))
    ref = robust.dense_gn(g, setting, 10)
    o = _handle(setting)
    try:
        o.set_graph(g); r = o.optimize(10); v = o.vertices()
    finally:
        o.close()
    assert (r["iters"], r["stop"]) == (ref["iters"], ref["stop"])
    print("chi2 trace rel %.2e, vertices %.2e" % (np.abs(r["chi2"] / ref["chi2"] - 1).max(), util.max_vertex_diff(v, ref["v_pos"], g.v_type)))
    np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=1e-9)
    assert util.max_vertex_diff(v, ref["v_pos"], g.v_type) < 1e-8


# ---- 5, 6 -----------------------------------------------------------------------------------------------------------------------------
def _lm_run(g, setting, iterations, lambda0):
    o = _handle(setting, rules="lm", odom_jacobian="analytic", lm_lambda0=lambda0)
    try:
        o.set_graph(g); r = o.optimize(iterations); v = o.vertices()
    finally:
        o.close()
    return r, v


def _accepted(r):
    return (r["lm_gain"] > 0) & (r["lm_pred"] > 0)


def _assert_lm_parity(r, v, ref, g, what):
    tol = np.array([lm_rules.rho_tolerance(c, p) for c, p in zip(ref["chi2"], ref["pred"])])
    assert (r["iters"], r["stop"], r["rejected"]) == (ref["iters"], ref["stop"], ref["rejected"]), what
    np.testing.assert_array_equal(_accepted(r), ref["accepted"])
    print("%s: %d trials, %d rejected, %s; chi2 rel %.2e, chi2_trial rel %.2e, pred rel %.2e, rho / tol %.2e, vertices %.2e"
          % (what, r["iters"], r["rejected"], r["stop"], np.abs(r["chi2"] / ref["chi2"] - 1).max(), np.abs(r["lm_chi2_trial"] / ref["chi2_trial"] - 1).max(),
             np.abs(r["lm_pred"] / ref["pred"] - 1).max(), (np.abs(r["lm_gain"] - ref["rho"]) / tol).max(), util.max_vertex_diff(v, ref["v_pos"], g.v_type)))
    np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=1e-9)
    np.testing.assert_allclose(r["lm_chi2_trial"], ref["chi2_trial"], rtol=1e-9)
    np.testing.assert_allclose(r["lm_pred"], ref["pred"], rtol=1e-8)
    assert np.all(np.abs(r["lm_gain"] - ref["rho"]) <= tol)
    assert np.all(np.diff(r["chi2"]) <= 1e-12 * r["chi2"][:-1])                       # chi^2 never rises
    acc = np.where(_accepted(r))[0]
    acc = acc[acc + 1 < r["iters"]]
    assert len(acc) >= 2
    np.testing.assert_allclose(r["lm_chi2_trial"][acc], r["chi2"][acc + 1], rtol=1e-12)      # k_chi2 reports what the next linearisation reports


@pytest.mark.parametrize("setting", ["cauchy_on_odom", "default"])
def test_rules_2_on_the_outlier_scenario_matches_the_dense_loop_to_its_end(setting):
    g, _clean, default, cauchy = scenario_references()
    sc = robust.SCENARIO
    ref, s = (cauchy, sc["robust"]) if setting == "cauchy_on_odom" else (default, None)
    r, v = _lm_run(g, s, sc["iterations"], sc["lambda0"])
    _assert_lm_parity(r, v, ref, g, setting)
    assert util.max_vertex_diff(v, ref["v_pos"], g.v_type) < 1e-8


def test_rules_2_with_all_five_classes_keeps_the_chi2_pass_and_the_linearisation_together():
    """Priors present as well: k_chi2_lm_prior and the PRI = 1 instantiations of k_chi2 / k_lin_pose under the mixed setting."""
    g = _graph(True, True)
    ref = robust.dense_lm(g, robust.MIXED, 8)
    r, v = _lm_run(g, robust.MIXED, 8, 1e-3)
    _assert_lm_parity(r, v, ref, g, "mixed, five classes")


# ---- 7 --------------------------------------------------------------------------------------------------------------------------------
def test_marginals_use_the_handles_kernels():
    g = _graph(True, True)
    ids = g.v_id[np.r_[0:4, 150:154]]
    o = _handle(robust.MIXED)
    try:
        o.set_graph(g); o.optimize(3); v = o.vertices()
        cov, _st = o.marginals(ids, rel_tol=1e-12)
        jc, _off, _ = o.joint_marginals(ids, rel_tol=1e-12)
    finally:
        o.close()
    cur = g.copy(); cur.v_pos[:] = v
    H, _b, _chi, offs = robust.dense_system(cur, robust.MIXED)
    Hi = np.linalg.inv(H)
    H0 = robust.dense_system(cur, None)[0]
    at = {int(x): i for i, x in enumerate(g.v_id)}
    rows = np.concatenate([np.arange(offs[at[int(i)]], offs[at[int(i)] + 1]) for i in ids])
    ref = Hi[np.ix_(rows, rows)]
    assert np.abs(np.linalg.inv(H0)[np.ix_(rows, rows)] - ref).max() > 1e-3 * np.abs(ref).max()      # (the default's covariance is another one)
    print("joint %.2e of the largest entry" % (np.abs(jc - ref).max() / np.abs(ref).max()))
    assert np.abs(jc - ref).max() <= 1e-8 * np.abs(ref).max()
    for k, i in enumerate(ids):
        a = at[int(i)]; n = offs[a + 1] - offs[a]
        blk = Hi[offs[a]:offs[a + 1], offs[a]:offs[a + 1]]
        assert np.abs(cov[k, :n, :n] - blk).max() <= 1e-8 * np.abs(blk).max(), k


# ---- 8 --------------------------------------------------------------------------------------------------------------------------------
def test_precision_32_linearisation_under_the_mixed_setting():
    """The f32 bounds of the same quantities: 1e-4 (tests/test_gpu_priors.py, f32 case), chi^2 1e-5 (tests/test_gpu_parity.py)."""
    for (vlm, pri), lanes, jac in VARIANTS[:2]:
        o = _handle(robust.MIXED, precision=32, pcg_rel_tol=1e-5, lanes_per_pose=lanes, lanes_per_lm=lanes, odom_jacobian=jac)
        try:
            o.set_graph(_graph(vlm, pri))
            got = o.linearize()
        finally:
            o.close()
        _assert_lin(got, _ref_lin(vlm, pri, "mixed", jac), 1e-4, 1e-5, "f32 mixed lanes %d %s" % (lanes, jac))


# ---- 9 --------------------------------------------------------------------------------------------------------------------------------
def test_the_setting_survives_set_graph():
    g = _graph(True, True)
    moved = lm_rules.perturbed(g, seed=1, sigma_xy=0.05, sigma_th=0.01)
    other = _graph(False, True)
    o = _handle(robust.MIXED)
    try:
        o.set_graph(g); o.optimize(1)
        for graph, reused in ((moved, True), (other, False)):
            o.set_graph(graph)
            assert o.robust == robust.full(robust.MIXED)
            _d, _g, chi = o.linearize()
            assert bool(o.optimize(1)["structure_reused"]) == reused
            ref = float(robust.chi2_at(graph, robust.MIXED))
            assert abs(chi - ref) <= 1e-11 * ref, reused
            assert abs(float(robust.chi2_at(graph, None)) - ref) > 1e-3 * ref
    finally:
        o.close()


def test_a_change_between_two_optimize_calls_takes_effect():
    g = _graph(True, True)
    wide, narrow = robust.everywhere(("cauchy", 3.0)), robust.everywhere(("cauchy", 0.5))
    o = _handle(wide)
    try:
        o.set_graph(g); r1 = o.optimize(3); v = o.vertices()
        o.set_robust(**narrow)
        r2 = o.optimize(3)
        o.set_robust(lm="none")                      # one class: the others keep what they have
        assert o.robust == dict(narrow, lm="none")
    finally:
        o.close()
    cur = g.copy(); cur.v_pos[:] = v
    first, want, old = r2["chi2"][0], float(robust.chi2_at(cur, narrow)), float(robust.chi2_at(cur, wide))
    print("first chi2 of the second call %.6f, restatement at those estimates: narrow %.6f, wide %.6f" % (first, want, old))
    assert abs(r1["chi2"][0] - float(robust.chi2_at(g, wide))) <= 1e-11 * r1["chi2"][0]
    assert abs(first - want) <= 1e-11 * want and abs(old - want) > 1e-2 * want


def test_bad_settings_are_refused_with_a_message():
    o = _handle()
    lib = o.lib
    try:
        def attempt(**kw):
            r = _lib.tsgo_robust()
            lib.tsgo_default_robust(C.byref(r))
            for k, v in kw.get("kernel", {}).items():
                r.kernel[k] = v
            for k, v in kw.get("delta", {}).items():
                r.delta[k] = v
            return lib.tsgo_set_robust(o.h, C.byref(r)), lib.tsgo_last_error().decode()
        r = _lib.tsgo_robust(); lib.tsgo_default_robust(C.byref(r))
        assert lib.tsgo_set_robust(None, C.byref(r)) < 0 and "null" in lib.tsgo_last_error().decode()
        assert lib.tsgo_set_robust(o.h, None) < 0 and "null" in lib.tsgo_last_error().decode()
        assert lib.tsgo_get_robust(o.h, None) < 0
        for bad in (4, -1, 99):
            rc, msg = attempt(kernel={2: bad})
            assert rc < 0 and "unknown robust kernel" in msg and "virtual landmark" in msg, msg
        for bad in (float("nan"), float("inf"), 0.0, -1.0, 9e-7, 1.1e6):
            rc, msg = attempt(kernel={0: 2}, delta={0: bad})
            assert rc < 0 and "delta" in msg and "ODOM" in msg, (bad, msg)
        assert o.robust == robust.DEFAULT                                       # a refused call changes nothing
        assert attempt(kernel={1: 0}, delta={1: float("nan")})[0] == 0          # NONE ignores its width
        assert attempt(kernel={0: 3}, delta={0: 1e-6})[0] == 0 and attempt(kernel={0: 3}, delta={0: 1e6})[0] == 0
        with pytest.raises(ValueError):
            o.set_robust(odom="cauchy")
        with pytest.raises(ValueError):
            o.set_robust(odom=("tukey", 1.0))
    finally:
        o.close()
    shard = HipOptimizer(world=2, rank=0, testing=True)
    try:
        with pytest.raises(RuntimeError, match="world > 1"):
            shard.set_robust(odom=("cauchy", 1.0))
        shard.set_robust(all=("huber", 1.5))                                     # the default is not a setting
        assert shard.robust == robust.DEFAULT
    finally:
        shard.close()
