"""Powell's dogleg trust-region loop (tsgo_config.rules = 3, rules="dogleg") on the device (`-m gpu`): the trajectory trial by trial against
the dense restatement of the loop (tests/dogleg.py), what a rejected trial costs (no solve) and leaves behind (nothing), g'Hg and the dots
at a size no dense system reaches, the loop-closure pose graph, determinism, the radius stop, the parameters' errors, one GNC round and
the server.  The cases are qualified on the reference alone in tests/test_dogleg_cpu.py.  Tolerances: those of tests/test_gpu_lm_rules.py
for the same quantities."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import dogleg, gnc, independent, lm_rules, util
from toyslam_amd import _lib, remote, synth
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu

TRACES = ("dl_gg", "dl_gHg", "dl_gd", "dl_dd", "dl_step_norm", "dl_radius")


def _run(g, iterations, **kw):
    kw.setdefault("pcg_rel_tol", 1e-12)
    kw.setdefault("odom_jacobian", "analytic")
    o = HipOptimizer(rules="dogleg", **kw)
    try:
        o.set_graph(g); r = o.optimize(iterations); v = o.vertices()
    finally:
        o.close()
    return r, v


def _dl(kw):
    return {"dl_" + k: v for k, v in kw.items()}


def _accepted(r):
    return (r["lm_gain"] > 0) & (r["lm_pred"] > 0)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(graph, dense loop, parameters, trial cap, Jacobians) of a case; computed once, never modified."""
    return dogleg.reference(case)


def _assert_parity(case, **kw):
    g, ref, params, n, jac = _reference(case)
    r, v = _run(g, n, odom_jacobian=jac, **_dl(params), **kw)
    tol = np.array([lm_rules.rho_tolerance(c, p) for c, p in zip(ref["chi2"], ref["pred"])])
    print(case, kw, "trials", r["iters"], "rejected", r["rejected"], "stop", r["stop"], "solves", r["solves"], "kinds", r["dl_kind"], "pcg", r["cg_iters"])
    assert (r["iters"], r["stop"], r["rejected"], r["solves"]) == (ref["iters"], ref["stop"], ref["rejected"], ref["solves"])
    np.testing.assert_array_equal(_accepted(r), ref["accepted"])
    np.testing.assert_array_equal(r["dl_kind"], ref["kind"])
    np.testing.assert_array_equal(r["dl_solved"], ref["solved"])
    print("  chi2 rel", np.abs(r["chi2"] / ref["chi2"] - 1).max(), " chi2_trial rel", np.abs(r["lm_chi2_trial"] / ref["chi2_trial"] - 1).max(),
          " pred rel", np.abs(r["lm_pred"] / ref["pred"] - 1).max(), " gain abs / tol", (np.abs(r["lm_gain"] - ref["rho"]) / tol).max(),
          " vertices", util.max_vertex_diff(v, ref["v_pos"], g.v_type))
    print("  " + "  ".join("%s rel %.2e" % (k, np.abs(r[k] / ref[k[3:]] - 1).max()) for k in TRACES))
    np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=1e-9)
    np.testing.assert_allclose(r["lm_chi2_trial"], ref["chi2_trial"], rtol=1e-9)
    np.testing.assert_allclose(r["lm_pred"], ref["pred"], rtol=1e-8)
    for k in TRACES:
        np.testing.assert_allclose(r[k], ref[k[3:]], rtol=1e-8, err_msg=k)
    assert np.all(np.abs(r["lm_gain"] - ref["rho"]) <= tol)
    own, last = dogleg.radius_trace(params.get("radius0", dogleg.DEFAULTS["radius0"]), r["lm_gain"], r["lm_pred"], r["dl_kind"], r["dl_step_norm"])
    np.testing.assert_allclose(r["dl_radius"], own, rtol=1e-12)
    np.testing.assert_allclose(r["dl_radius_last"], last, rtol=1e-12)
    assert not np.any(r["lm_lambda"]) and r["lambda_last"] == 0
    # a trial that reused a solve ran no PCG iteration
    assert np.all(r["cg_iters"][r["dl_solved"] == 0] == 0) and np.all(r["cg_iters"][r["dl_solved"] == 1] > 0) and r["cg_total"] == r["cg_iters"].sum()
    assert util.max_vertex_diff(v, ref["v_pos"], g.v_type) < 1e-8
    return r


@pytest.mark.parametrize("precond", ["amg", "jacobi"])
@pytest.mark.parametrize("case", ["A", "B"])
def test_trajectory_matches_the_dense_loop(case, precond):
    _assert_parity(case, preconditioner=precond)


@pytest.mark.parametrize("case", ["C", "D_plain", "D_vlm", "D_priors", "c1_plain"])
def test_rejections_general_slots_priors_and_convergence(case):
    g = _reference(case)[0]
    if case.startswith("D_"):
        assert (g.v_type == 0).sum() > 2 * 256 and (g.v_type == 1).sum() > 2 * 256          # more than two workgroups of poses and of landmarks
    _assert_parity(case)


def test_a_rejection_is_free_and_leaves_no_trace():
    """Case C, three trials, all rejected: one linearisation and one solve served all three, the estimates are bit for bit what set_graph put
    there, and the handle's next run is the run of a fresh handle (every call starts at radius0): the same decisions, the traces to the parity
    tolerance (the handle's hierarchy has aged by one linearisation, so its PCG solves may stop an iteration apart)."""
    g, ref, params, n, jac = _reference("C")
    o = HipOptimizer(rules="dogleg", odom_jacobian=jac, pcg_rel_tol=1e-12)
    try:
        o.set_graph(g); v0 = o.vertices()
        first = o.optimize(n); v1 = o.vertices()
        r = o.optimize(7); v = o.vertices()
    finally:
        o.close()
    assert (first["iters"], first["rejected"], first["stop"], first["solves"]) == (3, 3, "cap", 1) and not _accepted(first).any()
    assert np.all(first["lm_chi2_trial"] > first["chi2"])
    assert list(first["dl_solved"]) == [1, 0, 0] and not np.any(first["cg_iters"][1:]) and first["cg_total"] == first["cg_iters"][0] > 0
    np.testing.assert_array_equal(v1, v0)
    rf, vf = _run(g, 7, odom_jacobian=jac)
    assert r["chi2"][0] == first["chi2"][0] == rf["chi2"][0]                 # the same point, linearised again
    np.testing.assert_array_equal(_accepted(r), _accepted(rf))
    np.testing.assert_array_equal(r["dl_kind"], rf["dl_kind"])
    np.testing.assert_array_equal(r["dl_solved"], rf["dl_solved"])
    assert r["dl_radius"][0] == dogleg.DEFAULTS["radius0"]
    for k in ("chi2", "lm_chi2_trial", "lm_pred"):
        np.testing.assert_allclose(r[k], rf[k], rtol=1e-9)
    assert util.max_vertex_diff(v, vf, g.v_type) < 1e-8


def test_ghg_and_the_dots_at_20k_poses():
    """Many workgroups per table; radius 1 keeps the step away from Gauss-Newton, so that g'Hg enters pred."""
    g = synth.make(20000, 8, seed=2)
    o = HipOptimizer(rules="dogleg", odom_jacobian="analytic", pcg_rel_tol=1e-12, dl_radius0=1.0)
    try:
        o.set_graph(g); r = o.optimize(1); v = o.vertices()
    finally:
        o.close()
    assert r["iters"] == 1 and r["solves"] == 1 and r["dl_kind"][0] in (1, 2)
    after = g.copy(); after.v_pos[:] = v
    oracle.set_odom_jacobian("analytic")
    try:
        lin = independent.Linearisation(g)
        b = lin.gradient()
        b[np.isin(g.v_id, g.fixed)] = 0
        Hb = lin.apply_H(b)
        chi_after = independent.Linearisation(after).chi2
    finally:
        oracle.set_odom_jacobian("constant")
    mask = np.arange(3)[None, :] < np.where(g.v_type == 0, 3, 2)[:, None]
    gg, gHg = float((b[mask] ** 2).sum()), float((b[mask] * Hb[mask]).sum())
    print("kind %d, g'g %.9e (device) %.9e (numpy), g'Hg %.9e (device) %.9e (numpy), chi2 %.6f -> %.6f (device) %.6f (numpy), gain %.4f"
          % (r["dl_kind"][0], r["dl_gg"][0], gg, r["dl_gHg"][0], gHg, r["chi2"][0], r["lm_chi2_trial"][0], chi_after, r["lm_gain"][0]))
    assert abs(r["chi2"][0] - lin.chi2) <= 1e-11 * lin.chi2
    assert abs(r["dl_gg"][0] - gg) <= 1e-8 * gg
    assert abs(r["dl_gHg"][0] - gHg) <= 1e-8 * gHg
    assert abs(r["lm_chi2_trial"][0] - chi_after) <= 1e-11 * chi_after
    assert abs(r["dl_step_norm"][0] - 1.0) <= 1e-8          # a step to the boundary


def test_loop_closure_pose_graph_descends_and_reuses_solves():
    r, _v = _run(lm_rules.loop_closure_pose_graph(), 30, odom_jacobian="constant")
    acc = _accepted(r)
    kept = np.r_[r["chi2"][0], r["lm_chi2_trial"][acc]]
    print("constant Jacobians: %d trials, %d rejected, %d solves, stop %s, chi2 %.3f -> %.3f" % (r["iters"], r["rejected"], r["solves"], r["stop"], kept[0], kept[-1]))
    assert r["rejected"] >= 1 and acc.sum() >= 1 and r["solves"] < r["iters"]
    assert r["solves"] == int(r["dl_solved"].sum()) and r["iters"] - r["solves"] == int((r["cg_iters"] == 0).sum())
    # (a linearisation's chi^2 and the chi^2-only pass's of the same point agree to 1e-12 relative, not to the bit)
    assert np.all(np.diff(kept) <= 1e-12 * kept[:-1]) and np.all(np.diff(r["chi2"]) <= 1e-12 * r["chi2"][:-1])
    assert kept[-1] < r["chi2"][0]


def test_two_handles_give_identical_bits():
    g, _ref, params, n, jac = _reference("A")
    a, va = _run(g, n, odom_jacobian=jac, **_dl(params))
    b, vb = _run(g, n, odom_jacobian=jac, **_dl(params))
    for k in ("chi2", "lm_chi2_trial", "lm_pred", "lm_gain", "cg_iters", "dl_kind", "dl_solved") + TRACES:
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(va, vb)


def test_radius_stop():
    """Case C with radius_min just above the radius its second rejection leaves."""
    g, ref, _params, _n, jac = _reference("C")
    left = 0.25 * ref["step_norm"][1]
    assert left == ref["radius"][2] < ref["radius"][1]
    r, _v = _run(g, 10, odom_jacobian=jac, dl_radius_min=1.01 * left)
    assert (r["iters"], r["stop"], r["rejected"], r["solves"]) == (2, "radius", 2, 1)
    assert r["dl_radius_last"] < 1.01 * left


def test_other_rules_leave_an_all_zero_trace():
    g = util.c1_arrays()
    for rules, kw in (("cpp", {}), ("python", {}), ("lm", dict(odom_jacobian="analytic"))):
        o = HipOptimizer(rules=rules, **kw)
        try:
            o.set_graph(g); r = o.optimize(3)
            tr = _lib.tsgo_dogleg_trace()
            _lib.check(o.lib, o.lib.tsgo_get_dogleg_trace(o.h, C.byref(tr)), "tsgo_get_dogleg_trace")
        finally:
            o.close()
        assert bytes(tr) == bytes(C.sizeof(tr))
        assert r["solves"] == 0 and r["dl_radius_last"] == 0
        for k in ("dl_kind", "dl_solved") + TRACES:
            assert len(r[k]) == r["iters"] and not np.any(r[k])


def test_unsupported_combinations_fail_at_creation():
    with pytest.raises(RuntimeError, match="precision = 64"):
        HipOptimizer(rules="dogleg", precision=32)
    with pytest.raises(RuntimeError, match="world > 1"):
        HipOptimizer(rules="dogleg", world=2, rank=0)


def test_set_dogleg_errors_leave_the_handle_unchanged():
    o = HipOptimizer(rules="dogleg", dl_radius0=50.0, dl_chi2_rel_tol=1e-7)
    try:
        want = dict(radius0=50.0, radius_min=1e-9, radius_max=1e9, chi2_rel_tol=1e-7)
        assert o.dogleg == want
        bad = [dict(radius0=float("nan")), dict(radius_max=float("inf")), dict(radius_min=0.0), dict(radius_min=-1.0), dict(radius_min=60.0),
               dict(radius_max=40.0), dict(chi2_rel_tol=-1e-9), dict(chi2_rel_tol=float("nan"))]
        for kw in bad:
            with pytest.raises(RuntimeError, match="tsgo_set_dogleg"):
                o.set_dogleg(**kw)
            assert o.dogleg == want, kw
        assert o.lib.tsgo_set_dogleg(o.h, None) < 0 and b"tsgo_set_dogleg" in o.lib.tsgo_last_error()
        p = _lib.tsgo_dogleg_params()
        assert o.lib.tsgo_set_dogleg(None, C.byref(p)) < 0 and o.lib.tsgo_get_dogleg(o.h, None) < 0 and o.lib.tsgo_get_dogleg_trace(o.h, None) < 0
        assert o.dogleg == want
        o.set_dogleg(radius_min=50.0, radius_max=50.0)      # the bounds may meet
        # the parameters belong to the handle: they survive set_graph
        o.set_graph(util.c1_arrays())
        assert o.dogleg == dict(want, radius_min=50.0, radius_max=50.0)
    finally:
        o.close()


def test_time_kernel_9_is_the_ghg_pass_of_a_dogleg_handle():
    g = _reference("D_priors")[0]
    o = HipOptimizer(rules="dogleg", odom_jacobian="analytic")
    try:
        o.set_graph(g)
        us9, b9 = o.time_kernel(9, reps=3)
        us7, b7 = o.time_kernel(7, reps=3)          # the chi^2-only pass it is compared with runs on this handle too
        r = o.optimize(2)                           # the probe leaves a consistent state behind
    finally:
        o.close()
    print("g'Hg pass %.1f us, %.0f bytes; chi^2-only pass %.1f us, %.0f bytes" % (us9, b9, us7, b7))
    assert us9 > 0 and us7 > 0 and b9 > b7 > 0          # the same tables, plus the gradient of both ends of every edge
    assert r["iters"] == 2 and r["solves"] >= 1
    o = HipOptimizer(rules="lm", odom_jacobian="analytic")
    try:
        o.set_graph(g)
        with pytest.raises(RuntimeError, match="rules = 3"):
            o.time_kernel(9, reps=3)
    finally:
        o.close()


def test_one_gnc_round_under_dogleg_rules():
    g, mask = gnc.c1_case()
    o = HipOptimizer(rules="dogleg", odom_jacobian="analytic", pcg_rel_tol=1e-12)
    try:
        o.set_robust(all="none"); o.set_graph(g)
        r = o.gnc(subject=mask, inner_iterations=4, rounds_max=1)
    finally:
        o.close()
    print("gnc under dogleg: rounds", r["rounds"], "stop", r["stop"], "inner", r["inner_iters"], r["inner_stop"], "chi2_inner", r["chi2_inner"])
    assert r["rounds"] == 1 and 1 <= r["inner_iters"][0] <= 4
    assert r["inner_stop"][0] in ("cap", "converged", "radius") and np.isfinite(r["chi2_inner"][0])


def test_server_with_dogleg_rules():
    """The reply carries f32 (the reference's wire format): the server's vertices are compared with the in-process run's rounded to f32,
    to the 1e-8 the two f64 results must agree to."""
    from tests.test_server_gpu import _start, _stop
    g = util.c1_arrays()
    _r, v = _run(g, 20, dl_radius0=500.0)
    # HOST PORT ITERATIONS PIPELINE SOLVER | PRECISION PCG_TOL DEVICE ENGINES RULES ODOM_JACOBIAN
    port, proc = _start(20, "64", "1e-12", "0", "1", "dogleg:500", "analytic")
    try:
        c = remote.GraphClient("127.0.0.1", port)
        c.connect()
        out = c.optimize(g)
        c.close()
    finally:
        _stop(proc)
    banner = proc.stdout.read()
    assert "dogleg" in banner and "radius from 500" in banner
    wire = v.astype(np.float32).astype(np.float64)
    assert util.max_vertex_diff(out.v_pos, wire, g.v_type) < 1e-8
