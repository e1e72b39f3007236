"""Max-mixture edges without a GPU: the defaults through libtsgo_host.so, the argmin rules of the restatement tests/mixture.py, the null-twin
helper, and the two closure-or-nothing scenario runs as conditions on the restatement itself.

What the restatement gives on robust.scenario() (240 poses, 24 true and 13 false closures, a null twin of each, inner robust.dense_lm under
"none" with 5 trials, lambda0 1e-3):
  start "cauchy" (the Cauchy run of robust.SCENARIO, mean pose error 0.2205 to the clean optimum), kappa 1e-6: 2 passes, changed 37, 0,
    stop "stable"; 13 of 13 false closures and 0 of 24 true closures on the null; mean pose error 0.01601; smallest gap in a group 41.4;
  start "perturbed" (the scenario's own estimates), kappa 1e-8: 3 passes, changed 37, 1, 0, stop "stable"; 13 of 13 false and 5 of 24
    true closures on the null (6 after the first pass); mean pose error 0.263; smallest gap 8.33.
The device test (tests/test_gpu_mixture.py) relies on the gap >= 1 to compare selections exactly."""
import ctypes as C

import numpy as np
import pytest

from tests import mixture, robust
from toyslam_amd import _lib, graph


def test_defaults_through_the_host_library():
    p = _lib.tsgo_mixture_params(-1, -1, -1, -1)
    _lib.host_lib().tsgo_default_mixture(C.byref(p))
    assert (p.rounds_max, p.inner_iterations, p.keep_selection, p.reserved) == (32, 5, 1, 0)
    _lib.host_lib().tsgo_default_mixture(None)      # a NULL is ignored
    assert _lib.TSGO_MIX_MAX_ROUNDS == 128 and _lib.TSGO_MIX_MAX_MEMBERS == 64 and _lib.MIX_STOP == {0: "stable", 1: "rounds", 2: "solver"}
    st = _lib.tsgo_mixture_stats()
    assert len(st.n_changed) == len(st.cost_sum) == _lib.TSGO_MIX_MAX_ROUNDS + 1      # a stable stop adds one pass


def test_ties_go_to_the_lowest_position_and_non_finite_costs_count_as_infinite():
    off = np.array([0, 3, 5, 8, 9, 12])
    cost = np.array([2.0, 1.0, 1.0,   np.inf, np.nan,   np.nan, -np.inf, 7.0,   np.nan,   3.0, 3.0, 3.0])
    sel, win = mixture.select(cost, off)
    assert sel.tolist() == [1, 0, 2, 0, 0]      # the first of two minima; all infinite: 0; NaN and -inf are +inf; a group of one; a triple tie
    assert win.tolist() == [1.0, np.inf, 7.0, np.inf, 3.0]
    assert mixture.gaps(cost, off).tolist()[0] == 0.0 and mixture.gaps(cost, off)[3] == np.inf


def test_a_constant_on_every_log_weight_of_a_group_changes_nothing_and_a_log_weight_from_the_gap_flips_that_group():
    g, groups, _true, _false = mixture.scenario("perturbed")
    off, member = mixture.flat(groups)
    base = g.e_inf.copy()
    k = mixture.constants(g.e_type, base, member)
    np.testing.assert_allclose(k[0], -np.log(base[member[0]]).sum(), rtol=1e-15)
    cost = mixture.gnc.s_base(g, base, g.v_pos)[member] + k
    sel, _ = mixture.select(cost, off)
    lw = np.zeros(len(member))
    lw[off[3]:off[4]] = 17.25; lw[off[9]:off[10]] = -4.0
    shifted = mixture.gnc.s_base(g, base, g.v_pos)[member] + mixture.constants(g.e_type, base, member, lw)
    np.testing.assert_array_equal(mixture.select(shifted, off)[0], sel)
    # group 5: the loser needs more than gap / 2 of log-weight to win (c = s + k - 2 log_weight)
    gap = mixture.gaps(cost, off)[5]
    loser = off[5] + 1 - sel[5]
    for factor, flips in ((0.49, False), (0.51, True)):
        lw = np.zeros(len(member)); lw[loser] = factor * gap
        got, _ = mixture.select(mixture.gnc.s_base(g, base, g.v_pos)[member] + mixture.constants(g.e_type, base, member, lw), off)
        want = sel.copy()
        if flips:
            want[5] = 1 - sel[5]
        np.testing.assert_array_equal(got, want)


def test_the_null_twin_helper_appends_twins_and_returns_the_groups():
    g = robust.scenario()
    edges = [len(g.e_type) - 1, 250, 7]
    tw, groups = graph.with_null_twins(g, edges, 1e-6)
    ref, ref_groups = mixture.null_twins(g, edges, 1e-6)
    assert groups == ref_groups == [[len(g.e_type) - 1, len(g.e_type)], [250, len(g.e_type) + 1], [7, len(g.e_type) + 2]]
    for name in ("v_id", "v_type", "v_pos", "e_type", "e_ids", "e_meas", "e_inf", "fixed"):
        np.testing.assert_array_equal(getattr(tw, name), getattr(ref, name), err_msg=name)
    np.testing.assert_array_equal(tw.e_inf[-3:], g.e_inf[edges] * 1e-6)
    np.testing.assert_array_equal(tw.e_inf[:len(g.e_type)], g.e_inf)
    for bad in (dict(edges=[1, 1], kappa=1e-6), dict(edges=[len(g.e_type)], kappa=1e-6), dict(edges=[0], kappa=0.0), dict(edges=[0], kappa=float("nan"))):
        with pytest.raises(ValueError):
            graph.with_null_twins(g, **bad)


@pytest.mark.parametrize("start", ["cauchy", "perturbed"])
def test_the_scenario_runs_put_every_false_closure_on_the_null_and_stop_stable(start):
    from tests.test_robust_cpu import scenario_references
    g, groups, true, false = mixture.scenario(start)
    assert len(true) == 24 and len(false) == 13 and len(groups) == 37 and all(len(m) == 2 for m in groups)
    r = mixture.scenario_run(start)
    _g, clean, _default, cauchy = scenario_references()
    err = robust.mean_pose_error(r["v_pos"], clean["v_pos"], g.v_type)
    err_start = robust.mean_pose_error(g.v_pos, clean["v_pos"], g.v_type)
    on_null = r["selected"] == 1
    print("%s: %d passes, %d rounds, %s; changed %s; false on the null %d of %d, true on the null %d of %d; mean pose error %.5f (start %.5f); "
          "smallest gap per pass %s; inner trials %s" % (start, r["passes"], r["rounds"], r["stop"], r["n_changed"], on_null[false].sum(), len(false),
                                                        on_null[true].sum(), len(true), err, err_start, r["gap_min"], r["inner_iters"]))
    assert r["stop"] == "stable" and r["passes"] == r["rounds"] + 1 and r["n_changed"][0] == 37 and r["n_changed"][-1] == 0
    assert on_null[false].all()
    # the device test compares selections exactly: no group of any pass is near a tie
    assert np.all(r["gap_min"] >= 1.0)
    if start == "cauchy":
        assert not on_null[true].any()
        assert err < robust.mean_pose_error(cauchy["v_pos"], clean["v_pos"], g.v_type) == err_start
    else:
        assert on_null[true].sum() <= 6
    # what the tables hold at the end: base for the winners, 0 for the losers, the chain untouched
    off, member = mixture.flat(groups)
    win = member[off[:-1] + r["selected"]]
    lose = np.setdiff1d(member, win)
    assert np.array_equal(r["e_inf"][win], g.e_inf[win]) and np.all(r["e_inf"][lose] == 0)
    rest = np.setdiff1d(np.arange(len(g.e_type)), member)
    np.testing.assert_array_equal(r["e_inf"][rest], g.e_inf[rest])


def test_rounds_max_stops_a_run_that_has_not_settled_with_the_last_selection_scattered():
    g, groups, _true, _false = mixture.scenario("perturbed")
    full = mixture.scenario_run("perturbed")
    r = mixture.max_mixture(g, groups, inner=mixture.SCENARIO_INNER, rounds_max=1, lambda0=robust.SCENARIO["lambda0"])
    assert (r["stop"], r["rounds"], r["passes"]) == ("rounds", 1, 2)
    np.testing.assert_array_equal(r["n_changed"], full["n_changed"][:2])
    off, member = mixture.flat(groups)
    np.testing.assert_array_equal(r["e_inf"], mixture.switched(g.e_inf, off, member, r["selected"]))
