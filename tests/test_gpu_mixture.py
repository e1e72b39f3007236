"""tsgo_max_mixture on the device (`-m gpu`): groups of alternative edges, one switched on per group.

Oracles.  The costs: the device's OWN edge_report s (taken before the call under "none": the same edge functions, the same estimates) plus
k from numpy (mixture.constants of the handle's edge_information()), to 1e-12 (|s| + |k|): a few ulps of three logarithms from two libms
and one addition.  The selection: the strict argmin of those, exactly (the test first asserts that no group is near a tie).  The scatter:
edge_information() must be base for the winners and 0 for the losers bit for bit, and a FRESH handle given that graph through set_graph
must linearise bit for bit the same (the oracle of tests/test_gpu_gnc.py::_assert_tables).  The loop: the numpy restatement
tests/mixture.py on robust.dense_lm; tests/test_mixture_cpu.py shows that every group of every pass has a cost gap >= 1 there, so passes,
changes and selections are compared exactly.

Final vertices against the restatement.  PCG at 1e-10 against a dense solve, compounded over the rounds, has no derivable bound, so the
bound is 10 x the largest difference measured on an MI355X over the two scenario runs and nothing above 1e-6 is accepted.  Measured: the
Cauchy start (1 round, 4 Levenberg-Marquardt trials) 1.499e-12, the perturbed start (2 rounds, 4 and 3 trials) 1.146e-11; VERTEX_BOUND =
10 x the larger = 1.146e-10.  The inner runs took the restatement's numbers of trials and stopped as it did.

The world > 1 refusal is the first argument check after the precision's; it is tried here on a testing handle created with world = 2 and
no communicator, as tests/test_gpu_gnc.py does."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import edge_cases, edge_info, mixture, robust, util
from toyslam_amd import _lib
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu

MEASURED_CAUCHY, MEASURED_PERTURBED = 1.499e-12, 1.146e-11      # largest vertex difference against the restatement, see the module docstring
VERTEX_BOUND = 10 * max(MEASURED_CAUCHY, MEASURED_PERTURBED)

GRAPHS = {"five": dict(vlm=True, with_priors=True), "priors": dict(vlm=False, with_priors=True), "plain": dict(vlm=False, with_priors=False)}


# ---- 1. select only ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name, seed=31):
    """(graph with the members' information perturbed, groups): groups of 1, 2 and 3 members in every class the graph holds, one of 64 LM
    edges, input edge 0 and the last input edge among the members, one group of several priors on one vertex; about half of the edges of
    every class stay outside."""
    g = robust.c1_five_classes(**GRAPHS[name]).copy()
    rng = np.random.default_rng(seed)
    E = len(g.e_type)
    free = np.ones(E, bool)
    groups = []

    def take(edges):
        groups.append([int(e) for e in edges]); free[list(edges)] = False

    take([0] + [int(e) for e in rng.choice(np.where((mixture.axes(g.e_type) == mixture.axes(g.e_type[:1])[0]) & (np.arange(E) > 0) & (np.arange(E) < E - 1))[0], 2, replace=False)])
    same_dof = np.where((mixture.axes(g.e_type) == mixture.axes(g.e_type[-1:])[0]) & free & (np.arange(E) < E - 1))[0]
    take([int(rng.choice(same_dof)), E - 1])
    if GRAPHS[name]["with_priors"]:
        v = next(v for v in np.unique(g.e_ids[g.e_type == 3, 0]) if np.sum((g.e_type == 3) & (g.e_ids[:, 0] == v) & free) > 1)
        take(np.where((g.e_type == 3) & (g.e_ids[:, 0] == v) & free)[0])
    take(rng.choice(np.where((g.e_type == 1) & free)[0], _lib.TSGO_MIX_MAX_MEMBERS, replace=False))
    for t in range(5):
        pool = rng.permutation(np.where((g.e_type == t) & free)[0])
        pool = pool[:len(pool) // 2]
        at, k = 0, 0
        while at + 3 <= len(pool):
            n = (1, 2, 3)[k % 3]
            take(pool[at:at + n]); at += n; k += 1
    groups = [groups[i] for i in rng.permutation(len(groups))]
    member = np.concatenate([np.asarray(m) for m in groups])
    g.e_inf[member] *= rng.uniform(0.5, 2.0, size=(len(member), 3))
    return g, groups


@functools.lru_cache(maxsize=None)
def _select_only(name, lanes, jacobian):
    g, groups = _case(name)
    off, member = mixture.flat(groups)
    kw = dict(lanes_per_pose=lanes, lanes_per_lm=lanes, odom_jacobian=jacobian)
    what = "%s, lanes %d, %s" % (name, lanes, jacobian)
    o = HipOptimizer(**kw)
    try:
        o.set_robust(all="none"); o.set_graph(g)
        rec, _summary = o.edge_report()
        s = rec["s"].copy()
        base, lin, v = o.edge_information(), o.linearize(), o.vertices()
        np.testing.assert_array_equal(base, edge_info.held(g))
        k = mixture.constants(g.e_type, base, member)
        want = s[member] + k
        sel, win = mixture.select(want, off)
        assert np.all(mixture.gaps(want, off) > 1e-9 * (1 + np.abs(win))), what      # no group near a tie: the argmin is compared exactly
        results = []
        for keep in (False, True):
            r = o.max_mixture(groups, inner_iterations=0, rounds_max=1, keep_selection=keep)
            cost = np.concatenate(r["cost"])
            err = np.abs(cost - want) / (np.abs(s[member]) + np.abs(k))
            print("%s, keep_selection %d: %d groups, %d members %s; cost against s + k %.3e; cost_sum rel %.3e; passes %d, %s, changed %s; %.3f ms in the kernels" % (
                what, keep, len(groups), len(member), r["members_by_class"], err.max(), abs(r["cost_sum"][0] / win.sum() - 1), r["passes"], r["stop"], r["n_changed"], r["ms_select"]))
            assert np.all(err <= 1e-12), what
            np.testing.assert_array_equal(r["selected"], sel, err_msg=what)
            np.testing.assert_array_equal(r["selected_edge"], member[off[:-1] + sel], err_msg=what)
            # one round scatters; the pass behind it finds nothing to change
            assert (r["rounds"], r["passes"], r["stop"]) == (1, 2, "stable") and r["n_changed"].tolist() == [len(groups), 0], (what, r)
            np.testing.assert_allclose(r["cost_sum"], [win.sum()] * 2, rtol=1e-12, err_msg=what)
            assert r["cost_sum"][0] == r["cost_sum"][1]
            assert r["members_by_class"] == {c: int((g.e_type[member] == t).sum()) for t, c in enumerate(robust.CLASSES)}
            assert len(r["inner_iters"]) == 1 and r["inner_iters"][0] == 0 and r["cg_total"] == 0
            np.testing.assert_array_equal(o.vertices(), v, err_msg=what)      # nothing moved the estimates
            held = o.edge_information()
            if not keep:
                np.testing.assert_array_equal(held, base, err_msg=what)
                edge_info.assert_same_linearisation(o.linearize(), lin, what + ", keep_selection = 0")
            else:
                graph = edge_info.edited(g, mixture.switched(g.e_inf, off, member, sel))
                np.testing.assert_array_equal(held, mixture.switched(base, off, member, sel), err_msg=what)
                np.testing.assert_array_equal(held, edge_info.held(graph), err_msg=what)
                rest = np.setdiff1d(np.arange(len(g.e_type)), member)
                np.testing.assert_array_equal(held[rest], base[rest], err_msg=what)
                f = HipOptimizer(**kw)
                try:
                    f.set_robust(all="none"); f.set_graph(graph)
                    edge_info.assert_same_linearisation(o.linearize(), f.linearize(), what + ", a fresh handle")
                finally:
                    f.close()
            results.append(cost)
        np.testing.assert_array_equal(results[0], results[1])      # the same call from the same state: the same bits
    finally:
        o.close()
    return results[1]


@pytest.mark.parametrize("jacobian", ["constant", "analytic"])
@pytest.mark.parametrize("lanes", [1, 8])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_select_only_costs_selection_tables_and_a_fresh_handle(name, lanes, jacobian):
    g, groups = _case(name)
    off, member = mixture.flat(groups)
    sizes = np.diff(off)
    assert {1, 2, 3, _lib.TSGO_MIX_MAX_MEMBERS} <= set(sizes.tolist()) and 0 in member and len(g.e_type) - 1 in member and len(np.unique(member)) == len(member)
    for t in np.unique(g.e_type):
        assert {1, 2, 3} <= {len(m) for m in groups if g.e_type[m[0]] == t}, t
        assert np.sum(g.e_type[np.setdiff1d(np.arange(len(g.e_type)), member)] == t) >= 3, t
    if GRAPHS[name]["with_priors"]:
        assert any(len(m) > 1 and np.all(g.e_type[m] == 3) and len(set(g.e_ids[m, 0])) == 1 for m in groups)      # several priors on one vertex
    assert set(np.unique(g.e_type).tolist()) == ({0, 1, 2, 3, 4} if name == "five" else {0, 1, 3, 4} if name == "priors" else {0, 1})
    _select_only(name, lanes, jacobian)


@pytest.mark.parametrize("jacobian", ["constant", "analytic"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_costs_do_not_depend_on_the_lanes_per_vertex(name, jacobian):
    np.testing.assert_array_equal(_select_only(name, 1, jacobian), _select_only(name, 8, jacobian))


# ---- 2. ties, log-weights, the edge cases of the scatter --------------------------------------------------------------------------------
def test_duplicate_edges_tie_to_position_0_and_a_log_weight_breaks_the_tie():
    g = edge_cases.self_loop_and_duplicate_edges()
    E = len(g.e_type)
    assert g.e_ids[E - 3, 0] == g.e_ids[E - 3, 1] and all(np.array_equal(getattr(g, a)[E - 1], getattr(g, a)[E - 2]) for a in ("e_ids", "e_meas", "e_inf", "e_type"))
    first = int(np.where(g.e_type == 1)[0][0])      # the third observation of that landmark from that pose, another measurement
    assert np.array_equal(g.e_ids[first], g.e_ids[E - 1])
    chain = int(np.where(g.e_type == 0)[0][4])
    # three LM observations of one landmark from one pose in one group; the self loop (two slots of one pose) against a chain edge
    groups, lw = [[E - 1, first, E - 2], [E - 3, chain]], [[0.0, 0.0, 0.0], [0.0, -1e9]]
    off, member = mixture.flat(groups)
    o, f = HipOptimizer(), HipOptimizer()
    try:
        o.set_robust(all="none"); o.set_graph(g)
        base = o.edge_information()
        r = o.max_mixture([[E - 2, E - 1]], inner_iterations=0, rounds_max=1, keep_selection=False)
        assert r["cost"][0][0] == r["cost"][0][1] and r["selected"].tolist() == [0] and r["selected_edge"].tolist() == [E - 2]
        np.testing.assert_array_equal(o.edge_information(), base)
        r = o.max_mixture([[E - 2, E - 1]], log_weight=[[0.0, 1e-3]], inner_iterations=0, rounds_max=1, keep_selection=False)
        assert r["cost"][0][1] < r["cost"][0][0] and r["selected"].tolist() == [1]
        r = o.max_mixture(groups, log_weight=lw, inner_iterations=0, rounds_max=1)
        print("costs %s, selected %s" % (r["cost"], r["selected"]))
        assert r["cost"][0][0] == r["cost"][0][2] and r["selected"][0] in (0, 1) and r["selected"][1] == 0 and r["stop"] == "stable"
        sel = r["selected"].astype(np.int64)
        np.testing.assert_array_equal(o.edge_information(), mixture.switched(base, off, member, sel))
        f.set_robust(all="none"); f.set_graph(edge_info.edited(g, mixture.switched(g.e_inf, off, member, sel)))
        edge_info.assert_same_linearisation(o.linearize(), f.linearize(), "LM triple and self loop")
    finally:
        o.close(); f.close()


# ---- 3. the loop against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", ["cauchy", "perturbed"])
def test_the_scenario_end_to_end_follows_the_restatement(start):
    """rules = "lm", analytic Jacobians, robust none, a null twin per closure.  Measured on an MI355X: passes, changes, selections and inner
    trials as the restatement; final vertices 1.499e-12 ("cauchy") and 1.146e-11 ("perturbed") from it (the bound is VERTEX_BOUND = 1.146e-10,
    see the module docstring)."""
    g, groups, true, false = mixture.scenario(start)
    ref = mixture.scenario_run(start)
    o = HipOptimizer(rules="lm", odom_jacobian="analytic", lm_lambda0=robust.SCENARIO["lambda0"])
    try:
        o.set_robust(all="none"); o.set_graph(g)
        base = o.edge_information()
        r = o.max_mixture(groups, inner_iterations=mixture.SCENARIO_INNER)
        v, held = o.vertices(), o.edge_information()
    finally:
        o.close()
    diff = util.max_vertex_diff(v, ref["v_pos"], g.v_type)
    print("%s: %d passes (%d), %d rounds, %s; changed %s; cost_sum rel %.2e; inner trials %s (%s), stops %s (%s); final vertices against the restatement %.3e; "
          "selection %.3f ms of %.1f" % (start, r["passes"], ref["passes"], r["rounds"], r["stop"], r["n_changed"],
                                        np.abs(r["cost_sum"] / ref["cost_sum"] - 1).max() if r["passes"] == ref["passes"] else np.nan, r["inner_iters"], ref["inner_iters"],
                                        r["inner_stop"], ref["inner_stop"], diff, r["ms_select"], r["ms_total"]))
    assert (r["passes"], r["rounds"], r["stop"]) == (ref["passes"], ref["rounds"], ref["stop"]) == (ref["passes"], ref["passes"] - 1, "stable")
    np.testing.assert_array_equal(r["n_changed"], ref["n_changed"])
    np.testing.assert_array_equal(r["selected"], ref["selected"])
    np.testing.assert_array_equal(r["selected_edge"], ref["selected_edge"])
    assert np.all(r["selected"][false] == 1)
    np.testing.assert_allclose(r["cost_sum"][0], ref["cost_sum"][0], rtol=1e-9)      # pass 0: the same start (through the host's cos / sin: the bound of tests/test_gpu_init_guess.py)
    np.testing.assert_array_equal(r["inner_iters"], ref["inner_iters"])
    assert r["inner_stop"] == ref["inner_stop"]
    off, member = mixture.flat(groups)
    np.testing.assert_array_equal(held, mixture.switched(base, off, member, ref["selected"]))      # keep_selection: the losers are off, exactly
    assert VERTEX_BOUND <= 1e-6
    assert diff <= VERTEX_BOUND


# ---- 4. state ---------------------------------------------------------------------------------------------------------------------------
def test_settings_edits_and_the_history_survive_and_the_call_is_deterministic():
    g, groups = _case("five")
    chain = np.where(g.e_type == 0)[0][:40]
    lm0 = g.v_id[g.v_type == 1][:2]
    kw = dict(pcg_rel_tol=1e-12, odom_jacobian="analytic")
    a, b = HipOptimizer(**kw), HipOptimizer(**kw)
    try:
        for o in (a, b):
            o.set_robust(**robust.MIXED); o.set_graph(g)
            o.exempt_edges(chain); o.set_fixed(lm0, 2)
            o.optimize(2)
        held, counts, per_edge = a.edge_information(), a.fixed_counts(), a.edge_robust[1].copy()
        # select and scatter only, then the base back: what follows is what follows an edit that wrote the same bits (the hierarchy is rebuilt,
        # the warm start's history and every setting stay)
        a.max_mixture(groups, inner_iterations=0, rounds_max=1, keep_selection=False)
        b.set_edge_information(b.edge_information())
        ra, rb = a.optimize(3), b.optimize(3)
        np.testing.assert_array_equal(ra["chi2"], rb["chi2"]); np.testing.assert_array_equal(ra["cg_iters"], rb["cg_iters"])
        np.testing.assert_array_equal(a.vertices(), b.vertices())
        # the same call twice from the same state (keep_selection = 0 puts the information back, set_vertices the estimates): the same bits
        start = a.vertices()
        runs = []
        for _ in range(2):
            a.set_vertices(start)
            r = a.max_mixture(groups, inner_iterations=2, rounds_max=2, keep_selection=False)
            assert r["rounds"] >= 1 and np.all(r["inner_iters"] >= 1)
            assert a.robust == robust.full(robust.MIXED)
            np.testing.assert_array_equal(a.edge_robust[1], per_edge)
            np.testing.assert_array_equal(a.fixed_counts(), counts)
            np.testing.assert_array_equal(a.edge_information(), held)
            assert util.max_vertex_diff(a.vertices(), start, g.v_type) > 1e-6
            runs.append((np.concatenate(r["cost"]), r["selected"], r["n_changed"], r["cost_sum"], r["chi2_inner"], a.vertices()))
        for x, y in zip(*runs):
            np.testing.assert_array_equal(x, y)
        # a later set_graph drops the selection
        kept = a.max_mixture(groups, inner_iterations=0, rounds_max=1)
        assert (a.edge_information() == 0).all(axis=1).sum() == sum(len(m) - 1 for m in groups) and kept["stop"] == "stable"
        a.set_graph(g)
        np.testing.assert_array_equal(a.edge_information(), edge_info.held(g))
    finally:
        a.close(); b.close()


def test_a_handle_that_selected_and_restored_optimises_bit_for_bit_as_one_that_never_did():
    g, groups = _case("five")
    kw = dict(rules="lm", odom_jacobian="analytic")
    a, b = HipOptimizer(**kw), HipOptimizer(**kw)
    try:
        for o in (a, b):
            o.set_robust(all="none"); o.set_graph(g)
        a.max_mixture(groups, inner_iterations=0, keep_selection=False)
        ra, rb = a.optimize(4), b.optimize(4)
        np.testing.assert_array_equal(ra["chi2"], rb["chi2"]); np.testing.assert_array_equal(ra["cg_iters"], rb["cg_iters"])
        np.testing.assert_array_equal(a.vertices(), b.vertices())
    finally:
        a.close(); b.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_argument_and_leaves_the_handle_as_it_was():
    g, groups = _case("five")
    E = len(g.e_type)
    off, member = mixture.flat(groups)
    o = HipOptimizer()
    lib = o.lib
    i64 = lambda x: np.ascontiguousarray(x, np.int64)      # noqa: E731

    def call(handle=None, params="default", n_groups=None, off_=off, member_=member, lw=None, sel=None, cap_groups=0, cost=None, cap_members=0, **fields):
        p = _lib.tsgo_mixture_params()
        lib.tsgo_default_mixture(C.byref(p))
        p.inner_iterations = 0
        for k, val in fields.items():
            setattr(p, k, val)
        off_, member_ = (None if off_ is None else i64(off_)), (None if member_ is None else i64(member_))
        rc = lib.tsgo_max_mixture(o.h if handle is None else handle, None if params is None else C.byref(p), (len(off_) - 1) if n_groups is None else n_groups,
                                  None if off_ is None else off_.ctypes.data, None if member_ is None else member_.ctypes.data, None if lw is None else lw.ctypes.data,
                                  None if sel is None else sel.ctypes.data, cap_groups, None if cost is None else cost.ctypes.data, cap_members, None)
        return rc, lib.tsgo_last_error().decode()

    try:
        rc, msg = call()
        assert rc < 0 and "no graph" in msg
        zero = edge_info.edited(g, [[0.0, 0.0, 0.0], [3.0, 0.0, 1.0]], [groups[0][0], groups[1][0]])      # two members without information on a used axis
        o.set_robust(all="none"); o.set_graph(zero)
        for m0 in (groups[0][0], groups[1][0]):
            rc, msg = call(off_=[0, 1], member_=[m0])
            assert rc < 0 and "tsgo_max_mixture" in msg and "information" in msg and "member_edge" in msg, msg
        o.set_graph(g)
        before, held, v = o.linearize(), o.edge_information(), o.vertices()
        nan, inf = float("nan"), float("inf")
        odom, lm = int(np.where(g.e_type == 0)[0][3]), int(np.where(g.e_type == 1)[0][3])
        big = np.where(g.e_type == 1)[0][:_lib.TSGO_MIX_MAX_MEMBERS + 1]
        lw_nan = np.zeros(len(member)); lw_nan[5] = nan
        lw_inf = np.zeros(len(member)); lw_inf[-1] = inf
        bad = {
            "params NULL": (dict(params=None), "params"),
            "n_groups negative": (dict(n_groups=-1), "n_groups"),
            "group_off NULL": (dict(off_=None, n_groups=len(groups)), "group_off"),
            "member_edge NULL": (dict(member_=None), "member_edge"),
            "group_off[0] not 0": (dict(off_=np.r_[1, off[1:]]), "group_off[0]"),
            "an empty group": (dict(off_=[0, 2, 2, 4], member_=member[:4]), "group_off"),
            "a decreasing group_off": (dict(off_=[0, 3, 2, 4], member_=member[:4]), "group_off"),
            "a group above the cap": (dict(off_=[0, len(big)], member_=big), "TSGO_MIX_MAX_MEMBERS"),
            "an edge index below 0": (dict(off_=[0, 2], member_=[-1, lm]), "member_edge"),
            "an edge index past the graph": (dict(off_=[0, 2], member_=[lm, E]), "member_edge"),
            "an edge twice in one group": (dict(off_=[0, 3], member_=[lm, lm + 1, lm]), "listed twice"),
            "an edge in two groups": (dict(off_=[0, 1, 3], member_=[odom, lm, odom]), "listed twice"),
            "members of different dof": (dict(off_=[0, 2], member_=[odom, lm]), "degrees of freedom"),
            "log_weight NaN": (dict(lw=lw_nan), "log_weight"),
            "log_weight infinite": (dict(lw=lw_inf), "log_weight"),
            "rounds_max 0": (dict(rounds_max=0), "rounds_max"),
            "rounds_max above the cap": (dict(rounds_max=_lib.TSGO_MIX_MAX_ROUNDS + 1), "rounds_max"),
            "inner_iterations negative": (dict(inner_iterations=-1), "inner_iterations"),
            "keep_selection 2": (dict(keep_selection=2), "keep_selection"),
            "cap_groups too small": (dict(sel=np.zeros(len(groups), np.int32), cap_groups=len(groups) - 1), "cap_groups"),
            "cap_members too small": (dict(cost=np.zeros(len(member)), cap_members=len(member) - 1), "cap_members"),
        }
        for what, (kwargs, names) in bad.items():
            rc, msg = call(**kwargs)
            assert rc < 0 and "tsgo_max_mixture" in msg and names in msg and len(msg) > 20, (what, rc, msg)
            edge_info.assert_same_linearisation(o.linearize(), before, what)
            np.testing.assert_array_equal(o.edge_information(), held, err_msg=what)
            np.testing.assert_array_equal(o.vertices(), v, err_msg=what)
        assert call(handle=C.c_void_p())[0] < 0
        assert call(n_groups=0)[0] == 0      # no group: 0, nothing done
        np.testing.assert_array_equal(o.edge_information(), held)
        with pytest.raises(ValueError):
            o.max_mixture(groups, log_weight=[[0.0]])
        # the handle is usable: one good call, then an optimize
        r = o.max_mixture(groups, inner_iterations=1, rounds_max=2)
        assert r["rounds"] >= 1 and np.isfinite(r["chi2_inner"]).all() and o.optimize(1)["iters"] == 1
    finally:
        o.close()
    f32 = HipOptimizer(precision=32)
    try:
        f32.set_graph(g)
        with pytest.raises(RuntimeError, match="precision"):
            f32.max_mixture(groups)
        assert f32.optimize(1)["iters"] == 1
    finally:
        f32.close()
    shard = HipOptimizer(world=2, rank=0, testing=True)
    try:
        p = _lib.tsgo_mixture_params(); shard.lib.tsgo_default_mixture(C.byref(p))
        o64 = i64(off); m64 = i64(member)
        assert shard.lib.tsgo_max_mixture(shard.h, C.byref(p), len(groups), o64.ctypes.data, m64.ctypes.data, None, None, 0, None, 0, None) < 0
        assert "world > 1" in shard.lib.tsgo_last_error().decode()
    finally:
        shard.close()
