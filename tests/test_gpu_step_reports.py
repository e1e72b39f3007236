"""Step reports and the fused k_save_update against the path they replace (TSGO_STEP_DRAINS=1: copy + synchronise, k_save_x and
k_pose_update as two launches), on fresh handles.  Neither touches a number or moves a decision, so everything a caller can see must be
BITWISE equal: the chi^2 trace, the PCG iteration counts, the stop reason, the iterations run, the last delta norm and the vertices (under
rules = 2 and 3 the per-trial traces as well, under rules = 3 the dogleg trace).  Only the device times (ms_*) may differ between the two.
The reference side also sets TSGO_PACE_SPLIT=0, whole-iteration pacing: split pacing of the paced solve was built, measured and taken out
again (profiles/r12_step_chain.txt), so today that is the only pacing and nothing reads the variable."""
import numpy as np
import pytest

from tests import dogleg, edge_cases, lm_rules
from toyslam_amd import synth
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu

KEYS = ("chi2", "cg_iters", "stop", "iters", "delta_norm", "rejected", "lm_lambda", "lm_gain", "lm_pred", "lm_chi2_trial",
        "dl_kind", "dl_solved", "dl_radius", "dl_step_norm", "dl_gg", "dl_gHg", "dl_gd", "dl_dd", "solves", "dl_radius_last")


def _run(monkeypatch, old_way, graphs, calls, paced=False, **kw):
    """One fresh handle: every graph of `graphs` in turn, `calls` optimize calls on each.  Returns per graph (results ..., vertices)."""
    for name, value in (("TSGO_STEP_DRAINS", "1"), ("TSGO_PACE_SPLIT", "0")):
        if old_way:
            monkeypatch.setenv(name, value)
        else:
            monkeypatch.delenv(name, raising=False)
    if paced:
        monkeypatch.setenv("TSGO_FORCE_PACED", "1")
    else:
        monkeypatch.delenv("TSGO_FORCE_PACED", raising=False)
    o = HipOptimizer(testing=True, **kw)
    out = []
    try:
        for g in graphs:
            o.set_graph(g)
            out.append([o.optimize(n) for n in calls] + [o.vertices()])
    finally:
        o.close()
    return out


def _same(new, old):
    assert len(new) == len(old)
    for a, b in zip(new, old):
        for ra, rb in zip(a[:-1], b[:-1]):
            for k in KEYS:
                np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
        np.testing.assert_array_equal(a[-1], b[-1])


def _both(monkeypatch, graphs, calls, both_ways=False, **kw):
    new, old = _run(monkeypatch, False, graphs, calls, **kw), _run(monkeypatch, True, graphs, calls, **kw)
    _same(new, old)
    return (new, old) if both_ways else new


@pytest.fixture(scope="module")
def g2000():
    return synth.make(2000, 10, loop_closures=10, seed=17)


@pytest.fixture(scope="module")
def g300():
    return synth.make(300, 10, loop_closures=4, seed=5)


@pytest.mark.parametrize("use_graphs,paced", [(0, False), (0, True), (1, False), (2, False), (2, True)])
def test_rules_0_twelve_iterations(monkeypatch, g2000, use_graphs, paced):
    """Bursts, replay (captured at the second call) and the paced path (TSGO_FORCE_PACED: the chi^2 report leaves ahead of k_pose_finalize)."""
    r = _both(monkeypatch, [g2000], (12, 3), paced=paced, use_graphs=use_graphs)
    assert r[0][0]["iters"] == 12 and (r[0][0]["cg_iters"] > 0).all()
    if use_graphs == 1:
        assert r[0][1]["graph_replay"]


@pytest.mark.parametrize("rules,paced", [("python", False), ("python", True), ("lm", False), ("lm", True)])
def test_rules_1_and_2_four_iterations(monkeypatch, g2000, rules, paced):
    kw = dict(odom_jacobian="analytic") if rules == "lm" else {}
    r = _both(monkeypatch, [g2000], (4,), paced=paced, use_graphs=0, rules=rules, **kw)
    assert r[0][0]["iters"] == 4


@pytest.mark.parametrize("paced", [False, True])
def test_rules_2_with_a_rejection(monkeypatch, paced):
    """c1 from a badly perturbed start: tests/test_lm_rules_cpu.py qualifies the case as rejecting at least one trial on the reference, so the
    restore and the relinearisation at the restored point run both ways."""
    p = lm_rules.C1_PERTURBED
    r = _both(monkeypatch, [lm_rules.c1_perturbed()], (p["iterations"],), paced=paced, use_graphs=0, rules="lm", odom_jacobian="analytic", lm_lambda0=p["lambda0"])
    assert r[0][0]["rejected"] >= 1


@pytest.mark.parametrize("paced", [False, True])
@pytest.mark.parametrize("case", ["B", "C", "D_priors"])
def test_rules_3_trials(monkeypatch, case, paced):
    """The dogleg loop both ways (the cases are qualified on the reference alone in tests/test_dogleg_cpu.py): B, boundary and dogleg steps;
    C, one solve serving three rejected trials (the timing of a trial that reused a solve, the trial's report with the closing event behind
    it); D_priors, the landmark priors' partials behind the g'Hg partials.  The device times are not compared between the two ways: each
    way's must be finite, and positive wherever a phase ran."""
    make, params, trials, jac = dogleg.CASES[case]
    new, old = _both(monkeypatch, [make()], (trials,), both_ways=True, paced=paced, use_graphs=0, rules="dogleg", odom_jacobian=jac,
                     **{"dl_" + k: v for k, v in params.items()})
    r = new[0][0]
    assert r["iters"] >= 1 and r["solves"] >= 1
    if case == "C":
        assert r["rejected"] == 3 and r["solves"] == 1 and list(r["dl_solved"]) == [1, 0, 0]
    if case in ("B", "C"):
        for way in (new, old):
            ms = [way[0][0][k] for k in ("ms_linearize", "ms_solve", "ms_update")]
            print(case, "paced" if paced else "burst", "report" if way is new else "drain", "ms_linearize %.4f ms_solve %.4f ms_update %.4f" % tuple(ms))
            assert all(np.isfinite(m) and m >= 0 for m in ms), ms
            assert ms[0] > 0 and ms[1] > 0 and ms[2] > 0, ms


@pytest.mark.parametrize("paced", [False, True])
def test_penalty_rule_fires_on_the_same_iteration(monkeypatch, paced):
    """A pose graph with loop closures: the reference's constants drive it into "Error is getting worse"."""
    r = _both(monkeypatch, [edge_cases.pose_graph_without_landmarks()], (50,), paced=paced, use_graphs=0, pcg_rel_tol=1e-12)
    assert r[0][0]["stop"] == "worse"


@pytest.mark.parametrize("paced", [False, True])
def test_iteration_cap_of_the_solver_takes_no_step(monkeypatch, g2000, paced):
    r = _both(monkeypatch, [g2000], (5,), paced=paced, use_graphs=0, pcg_max_iters=3)
    assert r[0][0]["stop"] == "solver_failed" and r[0][0]["iters"] == 1


def test_first_gate_reports_done(monkeypatch, g300):
    """A second optimize(1) on a converged graph at a loose tolerance: the warm start already meets the rule (k_warm_scale sets `done`),
    the first gate reports a finished solve of 0 iterations."""
    r = _both(monkeypatch, [g300], (30, 1), paced=True, use_graphs=0, pcg_rel_tol=3e-2)
    assert r[0][1]["cg_iters"][0] == 0, (r[0][0]["cg_iters"], r[0][1]["cg_iters"])


def test_report_buffer_follows_the_largest_graph(monkeypatch, g2000, g300):
    """2 000, then 6 000 (the pinned buffer is reallocated), then 300 poses (it is kept) on one handle."""
    _both(monkeypatch, [g2000, synth.make(6000, 10, loop_closures=10, seed=3), g300], (3,), use_graphs=0)


def test_block_jacobi(monkeypatch, g300):
    r = _both(monkeypatch, [g300], (2, 2), preconditioner="jacobi")
    assert r[0][0]["iters"] == 2
