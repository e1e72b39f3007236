"""Levenberg-Marquardt with step acceptance (tsgo_config.rules = 2, rules="lm") on the device (`-m gpu`): the trajectory trial by trial
against the dense restatement of the loop (tests/lm_rules.py), the chi^2-only pass and the predicted decrease at a size no dense system
reaches, what a rejected step leaves behind (nothing), the loop-closure pose graph the fixed-step rules give up on, determinism, the
refused configurations and the server.  The inputs are qualified on the reference alone in tests/test_lm_rules_cpu.py."""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import independent, lm_rules, util
from toyslam_amd import remote, synth
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu


def _run(g, iterations, **kw):
    kw.setdefault("pcg_rel_tol", 1e-12)
    kw.setdefault("odom_jacobian", "analytic")
    o = HipOptimizer(rules="lm", **kw)
    try:
        o.set_graph(g); r = o.optimize(iterations); v = o.vertices()
    finally:
        o.close()
    return r, v


def _accepted(r):
    return (r["lm_gain"] > 0) & (r["lm_pred"] > 0)


@functools.lru_cache(maxsize=None)
def _reference(case):
    """(graph, dense loop, lambda0, trial cap) of a parity case; computed once, never modified."""
    if case == "c1_plain":
        g, lam0, n = lm_rules.c1_plain(), 1e-3, 30
    elif case == "c1_perturbed":
        g, lam0, n = lm_rules.c1_perturbed(), lm_rules.C1_PERTURBED["lambda0"], lm_rules.C1_PERTURBED["iterations"]
    else:
        g, lam0, n = lm_rules.synth_600(case[len("synth_"):]), 1e-3, 6
    return g, lm_rules.dense_lm(g, n, lambda0=lam0), lam0, n


def _assert_parity(case, **kw):
    g, ref, lam0, n = _reference(case)
    r, v = _run(g, n, lm_lambda0=lam0, **kw)
    tol = np.array([lm_rules.rho_tolerance(c, p) for c, p in zip(ref["chi2"], ref["pred"])])
    print(case, kw, "trials", r["iters"], "rejected", r["rejected"], "stop", r["stop"], "pcg", r["cg_iters"])
    print("  chi2       rel", np.abs(r["chi2"] / ref["chi2"][:len(r["chi2"])] - 1).max() if r["iters"] == ref["iters"] else "length differs")
    assert np.all(np.abs(ref["rho"]) > 10 * tol)                  # no decision of the reference sits near the boundary
    assert (r["iters"], r["stop"], r["rejected"]) == (ref["iters"], ref["stop"], ref["rejected"])
    np.testing.assert_array_equal(_accepted(r), ref["accepted"])
    print("  chi2_trial rel", np.abs(r["lm_chi2_trial"] / ref["chi2_trial"] - 1).max(), " pred rel", np.abs(r["lm_pred"] / ref["pred"] - 1).max(),
          " rho abs / tol", (np.abs(r["lm_gain"] - ref["rho"]) / tol).max(), " vertices", util.max_vertex_diff(v, ref["v_pos"], g.v_type))
    np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=1e-9)
    np.testing.assert_allclose(r["lm_chi2_trial"], ref["chi2_trial"], rtol=1e-9)
    np.testing.assert_allclose(r["lm_pred"], ref["pred"], rtol=1e-8)
    assert np.all(np.abs(r["lm_gain"] - ref["rho"]) <= tol)
    np.testing.assert_allclose(r["lm_lambda"], lm_rules.lambda_trace(lam0, r["lm_gain"], r["lm_pred"]), rtol=1e-12)
    assert r["lambda_last"] == r["lm_lambda"][-1]
    assert util.max_vertex_diff(v, ref["v_pos"], g.v_type) < 1e-8
    return r


@pytest.mark.parametrize("precond", ["amg", "jacobi"])
@pytest.mark.parametrize("case", ["c1_plain", "c1_perturbed"])
def test_trajectory_matches_the_dense_loop(case, precond):
    r = _assert_parity(case, preconditioner=precond)
    if case == "c1_perturbed":
        assert r["rejected"] >= 1 and int(_accepted(r).sum()) >= 3


@pytest.mark.parametrize("variant", ["plain", "vlm", "priors"])
def test_several_workgroups_general_slots_and_priors(variant):
    g = _reference("synth_" + variant)[0]
    assert {"vlm": (g.e_type == 2).sum() > 20, "priors": (g.e_type >= 3).sum() > 100 and len(g.fixed) == 0}.get(variant, True)
    assert (g.v_type == 0).sum() > 2 * 256 and (g.v_type == 1).sum() > 2 * 256          # more than two workgroups of poses and of landmarks
    _assert_parity("synth_" + variant)


def test_chi2_pass_and_predicted_decrease_at_20k_poses():
    g = synth.make(20000, 8, seed=2)
    lam = 1e-3
    o = HipOptimizer(rules="lm", odom_jacobian="analytic", pcg_rel_tol=1e-12, lm_lambda0=lam)
    try:
        o.set_graph(g); r = o.optimize(1); v = o.vertices(); r2 = o.optimize(1)
    finally:
        o.close()
    assert r["iters"] == 1 and _accepted(r)[0] and r["rejected"] == 0
    after = g.copy(); after.v_pos[:] = v
    oracle.set_odom_jacobian("analytic")
    try:
        before_lin = independent.Linearisation(g)
        b = before_lin.gradient()
        chi_after = independent.Linearisation(after).chi2
    finally:
        oracle.set_odom_jacobian("constant")
    b[np.isin(g.v_id, g.fixed)] = 0
    d = v - g.v_pos
    d[:, 2] = np.where(g.v_type == 0, util.angle_diff(v[:, 2], g.v_pos[:, 2]), 0.0)
    mask = np.arange(3)[None, :] < np.where(g.v_type == 0, 3, 2)[:, None]
    pred = float((b[mask] * d[mask]).sum() + lam * (d[mask] ** 2).sum())
    print("chi2 before %.6f, at the trial point %.6f (device) %.6f (numpy); pred %.6f (device) %.6f (numpy); next call's first chi2 %.6f"
          % (r["chi2"][0], r["lm_chi2_trial"][0], chi_after, r["lm_pred"][0], pred, r2["chi2"][0]))
    assert abs(r["chi2"][0] - before_lin.chi2) <= 1e-11 * before_lin.chi2
    assert abs(r["lm_chi2_trial"][0] - chi_after) <= 1e-11 * chi_after
    assert abs(r["lm_pred"][0] - pred) <= 1e-8 * abs(pred)
    assert abs(r2["chi2"][0] - r["lm_chi2_trial"][0]) <= 1e-12 * r["lm_chi2_trial"][0]          # same arithmetic, same association


def _loop_runs(iterations, lam0, **kw):
    return _run(lm_rules.loop_closure_pose_graph(), iterations, odom_jacobian="constant", lm_lambda0=lam0, **kw)


def test_a_rejected_step_leaves_no_trace():
    """One trial, rejected: the estimates are bit for bit what set_graph put there.  Every tsgo_optimize call starts at lm_lambda0 with nu = 2,
    so the damping a rejection leaves for the NEXT call is lm_lambda0 again: the handle's next run must be the run of a fresh handle with the
    same lambda0 — the same decisions, the traces to the parity tolerance (the handle's hierarchy has aged by the rejected
    trial's linearisation, so its PCG solves may stop an iteration apart)."""
    g = lm_rules.loop_closure_pose_graph()
    lam0 = lm_rules.LOOP_LAMBDA0
    o = HipOptimizer(rules="lm", odom_jacobian="constant", pcg_rel_tol=1e-12, lm_lambda0=lam0)
    try:
        o.set_graph(g); v0 = o.vertices()
        first = o.optimize(1); v1 = o.vertices()
        r = o.optimize(7); v = o.vertices()
    finally:
        o.close()
    assert (first["iters"], first["rejected"], first["stop"]) == (1, 1, "cap") and not _accepted(first)[0]
    assert first["lm_chi2_trial"][0] > first["chi2"][0]
    np.testing.assert_array_equal(v1, v0)
    rf, vf = _loop_runs(7, lam0)
    assert r["chi2"][0] == first["chi2"][0] == rf["chi2"][0]                 # the same point, linearised again
    np.testing.assert_array_equal(_accepted(r), _accepted(rf))
    np.testing.assert_array_equal(r["lm_lambda"][:2], [lam0, 2 * lam0])
    np.testing.assert_allclose(r["lm_lambda"], lm_rules.lambda_trace(lam0, r["lm_gain"], r["lm_pred"]), rtol=1e-12)
    for k in ("chi2", "lm_chi2_trial", "lm_pred"):
        np.testing.assert_allclose(r[k], rf[k], rtol=1e-9)
    assert util.max_vertex_diff(v, vf, g.v_type) < 1e-8


def test_loop_closure_pose_graph_descends_where_the_fixed_step_gives_up():
    g = lm_rules.loop_closure_pose_graph()
    o = HipOptimizer(rules="cpp", pcg_rel_tol=1e-12)
    try:
        o.set_graph(g); r0 = o.optimize(30)
    finally:
        o.close()
    assert r0["stop"] == "worse"
    r, _v = _loop_runs(30, 1e-3)
    acc = _accepted(r)
    kept = np.r_[r["chi2"][0], r["lm_chi2_trial"][acc]]
    print("constant Jacobians: %d trials, %d rejected, stop %s, chi2 %.3f -> %.3f" % (r["iters"], r["rejected"], r["stop"], kept[0], kept[-1]))
    assert r["rejected"] >= 1 and acc.sum() >= 1
    # (a linearisation's chi^2 and the chi^2-only pass's of the same point agree to 1e-12 relative, not to the bit)
    assert np.all(np.diff(kept) <= 1e-12 * kept[:-1]) and np.all(np.diff(r["chi2"]) <= 1e-12 * r["chi2"][:-1])
    assert kept[-1] < r["chi2"][0]


def test_two_handles_give_identical_bits():
    g, _ref, lam0, n = _reference("c1_perturbed")
    a, va = _run(g, n, lm_lambda0=lam0)
    b, vb = _run(g, n, lm_lambda0=lam0)
    for k in ("chi2", "lm_chi2_trial", "lm_pred", "lm_gain", "lm_lambda", "cg_iters"):
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(va, vb)


def test_other_rules_report_no_lm_fields():
    g = util.c1_arrays()
    for rules in ("cpp", "python"):
        o = HipOptimizer(rules=rules)
        try:
            o.set_graph(g); r = o.optimize(3)
        finally:
            o.close()
        assert r["rejected"] == 0
        for k in ("lm_lambda", "lm_gain", "lm_pred", "lm_chi2_trial"):
            assert not np.any(r[k])


def test_unsupported_combinations_fail_at_creation():
    with pytest.raises(RuntimeError, match="precision = 64"):
        HipOptimizer(rules="lm", precision=32)
    with pytest.raises(RuntimeError, match="world > 1"):
        HipOptimizer(rules="lm", world=2, rank=0)


def test_server_with_lm_rules():
    """The reply carries f32 (the reference's wire format): the server's vertices are compared with the in-process run's rounded to f32,
    to the 1e-8 the two f64 results must agree to."""
    from tests.test_server_gpu import _start, _stop
    g = util.c1_arrays()
    _r, v = _run(g, 20)
    # HOST PORT ITERATIONS PIPELINE SOLVER | PRECISION PCG_TOL DEVICE ENGINES RULES ODOM_JACOBIAN
    port, proc = _start(20, "64", "1e-12", "0", "1", "lm", "analytic")
    try:
        c = remote.GraphClient("127.0.0.1", port)
        c.connect()
        out = c.optimize(g)
        c.close()
    finally:
        _stop(proc)
    banner = proc.stdout.read()
    assert "Levenberg-Marquardt" in banner
    wire = v.astype(np.float32).astype(np.float64)
    assert util.max_vertex_diff(out.v_pos, wire, g.v_type) < 1e-8
