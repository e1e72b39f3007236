"""tsgo_set_fixed / tsgo_get_fixed / tsgo_set_estimates on the device (`-m gpu`).  The oracle is a second, FRESH handle B: handle A gets
set_graph(g) and the edit, B set_graph(g') with g' = vertex_edit.refixed(g, ...) (the canonical fixed list) or vertex_edit.moved(g, ...);
both start from the same host estimates, so the same kernels see the same inputs and tsgo_linearize must agree bit for bit in diag, grad
and chi^2 — the rule of tests/test_gpu_edge_info.py.  tests/test_vertex_edit_cpu.py pins the two helpers on the dense restatement.

Bounds that are not bitwise are that file's, the project's own for the same comparison: chi^2 traces against a fresh handle 1e-9,
vertices 1e-8, marginals 1e-8 of the largest entry.  rules="lm" needs precision 64 (tsgo_create refuses it otherwise), so of the four
(precision, lanes, jacobian) combinations the Levenberg-Marquardt comparison runs on the two f64 ones."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import edge_cases, edge_info, init_guess, lm_rules, robust, util, vertex_edit
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu

same = vertex_edit.assert_same_linearisation


@functools.lru_cache(maxsize=None)
def _c1():
    return robust.c1_five_classes()


@functools.lru_cache(maxsize=None)
def _c1_edit():
    """(ids, count) of the five-class edit: the original fixed vertex released; three poses fixed, one of which carries several priors
    and one twice; two landmarks fixed."""
    g = _c1()
    prior_pose, n = np.unique(g.e_ids[g.e_type == 3, 0], return_counts=True)
    multi = int(prior_pose[n > 1][0])
    lm = g.v_id[g.v_type == 1]
    assert list(g.fixed) == [0] and multi not in (0, 41, 149)
    return np.array([lm[17], 149, 0, multi, lm[200], 41], np.uint32), np.array([1, 1, 0, 1, 1, 2], np.int32)


def _pair(g, want, edit, what, **kw):
    """A: set_graph(g), edit(A).  B, fresh: set_graph(want).  Bitwise linearisation and the counts; returns (A, B, what edit returned)."""
    a, b = HipOptimizer(**kw), HipOptimizer(**kw)
    try:
        a.set_graph(g)
        st = edit(a)
        b.set_graph(want)
        same(a.linearize(), b.linearize(), what)
        np.testing.assert_array_equal(a.fixed_counts(), vertex_edit.counts(want), err_msg=what)
        np.testing.assert_array_equal(b.fixed_counts(), vertex_edit.counts(want), err_msg=what)
    except Exception:
        a.close(); b.close()
        raise
    return a, b, st


def _fixed_against_fresh(g, ids, count, what, **kw):
    a, b, st = _pair(g, vertex_edit.refixed(g, ids, count), lambda o: o.set_fixed(ids, count), what, **kw)
    a.close(); b.close()
    return st


def _trace_close(r, rb, va, vb, v_type, what):
    print("%s: chi2 %s against %s, vertices %.2e" % (what, r["chi2"], rb["chi2"], util.max_vertex_diff(va, vb, v_type)))
    assert len(r["chi2"]) == len(rb["chi2"]) and r["stop"] == rb["stop"], what
    np.testing.assert_allclose(r["chi2"], rb["chi2"], rtol=1e-9, err_msg=what)
    assert util.max_vertex_diff(va, vb, v_type) < 1e-8, what


# ---- the fixed set --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision, lanes, jacobian", [(64, 1, "constant"), (64, 8, "analytic"), (32, 1, "analytic"), (32, 8, "constant")])
def test_five_classes_release_the_anchor_fix_poses_and_landmarks(precision, lanes, jacobian):
    g = _c1()
    assert all((g.e_type == t).sum() >= 3 for t in range(5))
    ids, count = _c1_edit()
    want = vertex_edit.refixed(g, ids, count)
    assert len(want.fixed) == 6 and 0 not in want.fixed
    kw = dict(precision=precision, lanes_per_pose=lanes, lanes_per_lm=lanes, odom_jacobian=jacobian)
    runs = [dict(kw, rules="cpp")] + ([dict(kw, rules="lm", odom_jacobian="analytic", pcg_rel_tol=1e-12)] if precision == 64 else [])
    for k in runs:
        what = "five classes, %s" % k
        a, b, st = _pair(g, want, lambda o: o.set_fixed(ids, count), what, **k)
        try:
            assert (st["listed"], st["poses"], st["landmarks"], st["fixed_now"], st["released"]) == (6, 4, 2, 5, 1), st
            v = a.vertices()
            np.testing.assert_array_equal(v, b.vertices())      # the edit wrote no estimate
            r, rb = a.optimize(5), b.optimize(5)
            _trace_close(r, rb, a.vertices(), b.vertices(), g.v_type, what)
            assert r["iters"] >= 1 and not np.array_equal(a.vertices(), v)
        finally:
            a.close(); b.close()


def test_fixed_landmark_duplicate_ids_shuffled_and_sparse_ids():
    g = edge_cases.fixed_landmark_and_duplicate_fixed_ids()
    lm = g.v_id[g.v_type == 1]
    o = HipOptimizer()
    try:
        o.set_graph(g)
        c = o.fixed_counts()      # right after a plain set_graph: the duplicates
    finally:
        o.close()
    at = {int(v): k for k, v in enumerate(g.v_id)}
    np.testing.assert_array_equal(c, vertex_edit.counts(g))
    assert (c[at[0]], c[at[int(lm[3])]], c[at[7]], c.sum()) == (2, 3, 1, 6)
    st = _fixed_against_fresh(g, [lm[3], 0], [0, 1], "release the fixed landmark, a duplicate from 2 to 1")
    assert (st["listed"], st["poses"], st["landmarks"], st["fixed_now"], st["released"]) == (2, 1, 1, 2, 1), st
    _fixed_against_fresh(g, [7, lm[3], lm[5]], [3, 1, 2], "other multiplicities")
    for graph, what in ((edge_cases.shuffled_vertices_and_edges()[0], "shuffled"), (edge_cases.sparse_large_ids(), "sparse large ids")):
        poses, lms = graph.v_id[graph.v_type == 0], graph.v_id[graph.v_type == 1]
        assert len(graph.fixed) == 1
        ids = np.r_[graph.fixed, poses[[5, 31, 59]], lms[[0, 63]]]
        assert len(set(ids.tolist())) == 6
        st = _fixed_against_fresh(graph, ids, [0, 1, 2, 1, 1, 4], what)
        assert (st["fixed_now"], st["released"]) == (5, 1), st


def test_a_list_one_longer_than_a_block_and_the_dense_form():
    g = lm_rules.synth_600()
    V = len(g.v_id)
    assert V % 256 != 0 and V > 512
    rng = np.random.default_rng(4)
    rows = rng.choice(V, 257, replace=False)
    assert 60 < (g.v_type[rows] == 0).sum() < 200      # poses and landmarks mixed
    count = rng.integers(0, 3, size=257)
    st = _fixed_against_fresh(g, g.v_id[rows], count, "257 vertices", odom_jacobian="analytic")
    assert st["listed"] == 257 and st["poses"] == (g.v_type[rows] == 0).sum() and st["fixed_now"] == (vertex_edit.counts(vertex_edit.refixed(g, g.v_id[rows], count)) > 0).sum()
    # estimates: the same list, then every vertex
    pos = g.v_pos[rows] + rng.normal(scale=0.05, size=(257, 3))
    for ids, p, what in ((g.v_id[rows], pos, "257 estimates"), (None, g.v_pos + rng.normal(scale=0.05, size=g.v_pos.shape), "dense, %d vertices" % V)):
        a, b, st = _pair(g, vertex_edit.moved(g, ids, p), lambda o: o.set_vertices(p, ids), what)
        a.close(); b.close()
        assert st["listed"] == len(p) and st["poses"] + st["landmarks"] == len(p) and st["fixed_now"] == 1, (what, st)


def test_fix_then_release_gives_the_unedited_bits_and_a_repeat_changes_nothing():
    g = _c1()
    ids, count = _c1_edit()
    a, b = HipOptimizer(), HipOptimizer()
    try:
        a.set_graph(g); b.set_graph(g)
        ref = b.linearize()
        a.set_fixed(ids, count)
        once = a.linearize()
        assert not np.array_equal(once[0], ref[0])
        st = a.set_fixed(ids, count)      # the same call again
        assert st["released"] == 0 and st["fixed_now"] == 5
        same(a.linearize(), once, "the same call twice")
        back = vertex_edit.counts(g)[[int(np.where(g.v_id == i)[0][0]) for i in ids]]
        st = a.set_fixed(ids, back)
        assert st["released"] == 5 and st["fixed_now"] == 1
        same(a.linearize(), ref, "fixed, then released back")
        np.testing.assert_array_equal(a.fixed_counts(), vertex_edit.counts(g))
        a.release([])      # n == 0
        assert a.lib.tsgo_set_fixed(a.h, 0, None, None, None) == 0
        same(a.linearize(), ref, "n == 0")
    finally:
        a.close(); b.close()


# ---- lifetime -------------------------------------------------------------------------------------------------------------------------
def test_the_next_set_graph_installs_its_own_list_and_edits_made_before_stay():
    g = _c1()
    ids, count = _c1_edit()
    a, b = HipOptimizer(), HipOptimizer()
    try:
        a.set_graph(g)
        a.set_fixed(ids, count)
        a.set_graph(g)      # the original graph: same_as compares the list of the previous set_graph, a refill
        b.set_graph(g)
        same(a.linearize(), b.linearize(), "a refill after set_fixed")
        np.testing.assert_array_equal(a.fixed_counts(), vertex_edit.counts(g))
        r = a.optimize(1)
        assert r["structure_reused"]
        cov, _st = a.marginals([0, 149], rel_tol=1e-12)      # the host mirror is the request's again: pose 0 anchors
        assert 0 < cov[0, 0, 0] < 1.0001e-6 < cov[1, 0, 0]
    finally:
        a.close(); b.close()
    # a weight edit and an exemption made BEFORE set_fixed are still in force after it
    edges, vals = edge_info.every_class(g, seed=1)
    chain = np.where(g.e_type == 0)[0][:40]
    want = vertex_edit.refixed(edge_info.edited(g, vals, edges), ids, count)
    a, b = HipOptimizer(), HipOptimizer()
    try:
        a.set_robust(**robust.MIXED); b.set_robust(**robust.MIXED)
        a.set_graph(g)
        a.set_edge_information(vals, edges)
        a.exempt_edges(chain)
        a.set_fixed(ids, count)
        b.set_graph(want)
        b.exempt_edges(chain)
        same(a.linearize(), b.linearize(), "weight edit and exemption before set_fixed")
        np.testing.assert_array_equal(a.edge_information(), edge_info.held(want))
        np.testing.assert_array_equal(a.edge_robust[1], b.edge_robust[1])
        assert a.robust == robust.full(robust.MIXED)
    finally:
        a.close(); b.close()


# ---- readers of the gauge -------------------------------------------------------------------------------------------------------------
def test_moving_the_anchor_marginals_samples_and_init_estimates():
    g = _c1()
    lm = g.v_id[g.v_type == 1]
    ids, count = [0, 149], [0, 1]
    want = vertex_edit.refixed(g, ids, count)
    np.testing.assert_array_equal(want.fixed, [149])
    query = [149, 0, 75, lm[3], lm[300]]
    kw = dict(pcg_rel_tol=1e-12)
    a, b, _st = _pair(g, want, lambda o: o.set_fixed(ids, count), "anchor moved to the last pose", **kw)
    try:
        cov, _s = a.marginals(query, rel_tol=1e-12)
        ref, _s = b.marginals(query, rel_tol=1e-12)
        err = np.abs(cov - ref).max() / np.abs(ref).max()
        print("marginals after the anchor moved: %.2e of the largest entry; the anchor's diagonal %s, pose 0's %s" % (err, np.diag(cov[0]), np.diag(cov[1])))
        assert np.abs(ref).max() > 0 and err <= 1e-8
        assert np.all(np.diag(cov[0]) > 1e-7) and np.all(np.diag(cov[0]) < 1.0001e-6)      # 1 / (1e6 + its own information)
        assert np.all(np.diag(cov[1]) > 1.0001e-6)                                          # pose 0 is free now: above what a gauge term allows
        sa, sb = a.sample_marginals(8, seed=7, samples=True), b.sample_marginals(8, seed=7, samples=True)
        np.testing.assert_array_equal(sa["samples"], sb["samples"])
        np.testing.assert_array_equal(sa["cov"], sb["cov"])
    finally:
        a.close(); b.close()
    t, _mask = init_guess.two_fixed()
    np.testing.assert_array_equal(t.fixed, [29, 0, 29])
    ids, count = [29, 0, 7, 22], [0, 0, 1, 2]
    want = vertex_edit.refixed(t, ids, count)
    np.testing.assert_array_equal(want.fixed, [7, 22, 22])
    a, b, _st = _pair(t, want, lambda o: o.set_fixed(ids, count), "two_fixed, other sources", **kw)
    try:
        sa, sb = a.init_estimates(), b.init_estimates()
        assert all(sa[k] == sb[k] for k in init_guess.STAT_KEYS) and sa["roots_fixed"] == 2, (sa, sb)
        va = a.vertices()
        np.testing.assert_array_equal(va, b.vertices())
        np.testing.assert_array_equal(va[[7, 22], :2], t.v_pos[[7, 22], :2])      # the new sources kept their estimates
        assert not np.array_equal(va[[0, 29]], t.v_pos[[0, 29]])                   # the old ones hang on the tree now
    finally:
        a.close(); b.close()


def test_release_everything_then_fix_one_again():
    """On c1 WITHOUT its priors: a pose prior with three positive weights anchors H as a fixed vertex does (mb_anchored), so on
    robust.c1_five_classes() itself a handle without fixed vertices — edited or fresh — answers tsgo_marginals; that is checked first."""
    g = _c1()
    a, b, _st = _pair(g, vertex_edit.refixed(g, [0], 0), lambda o: o.release([0]), "released, anchored by a pose prior", pcg_rel_tol=1e-12)
    try:
        cov, ref = a.marginals([0, 149], rel_tol=1e-12)[0], b.marginals([0, 149], rel_tol=1e-12)[0]
        assert np.abs(ref).max() > 0 and np.abs(cov - ref).max() <= 1e-8 * np.abs(ref).max()
    finally:
        a.close(); b.close()
    g = robust.c1_five_classes(with_priors=False)
    none = vertex_edit.refixed(g, [0], 0)
    assert len(none.fixed) == 0 and list(g.fixed) == [0]
    a, b, st = _pair(g, none, lambda o: o.release([0]), "every fixed vertex released", pcg_rel_tol=1e-12)
    try:
        assert (st["fixed_now"], st["released"]) == (0, 1)
        for o in (a, b):
            with pytest.raises(RuntimeError, match="need a fixed vertex"):
                o.marginals([0, 149])
        r = a.optimize(3)
        assert r["iters"] >= 1 and np.all(np.isfinite(r["chi2"])) and np.all(np.isfinite(a.vertices()))
        assert a.set_fixed([75])["fixed_now"] == 1
        cov, _s = a.marginals([75, 0], rel_tol=1e-12)
        assert np.all(np.isfinite(cov)) and np.all(np.diag(cov[0]) < 1.0001e-6) and np.all(np.diag(cov[1]) > 1.0001e-6)
    finally:
        a.close(); b.close()


# ---- estimates ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [64, 32])
def test_listed_estimates_against_a_fresh_handle_and_the_read_back(precision):
    g = _c1()
    rng = np.random.default_rng(9)
    poses, lms = g.v_id[g.v_type == 0], g.v_id[g.v_type == 1]
    ids = np.r_[rng.choice(poses[1:], 6, replace=False), [0], rng.choice(lms, 5, replace=False)]      # vertex 0 is fixed
    ids = rng.permutation(ids).astype(np.uint32)
    at = {int(v): k for k, v in enumerate(g.v_id)}
    rows = np.array([at[int(i)] for i in ids])
    pos = g.v_pos[rows] + rng.normal(scale=0.2, size=(12, 3))
    pos[:, 2] = rng.uniform(-1.5, 1.5, size=12)
    want = vertex_edit.moved(g, ids, pos)
    kw = dict(precision=precision, odom_jacobian="analytic")
    o = HipOptimizer(**kw)
    try:
        o.set_graph(g); v0 = o.vertices()
    finally:
        o.close()
    a, b, st = _pair(g, want, lambda o: o.set_vertices(pos, ids), "7 poses and 5 landmarks", **kw)
    try:
        assert (st["listed"], st["poses"], st["landmarks"], st["fixed_now"], st["released"]) == (12, 7, 5, 1, 0), st
        v = a.vertices()
        np.testing.assert_array_equal(v, b.vertices())
    finally:
        a.close(); b.close()
    rest = np.setdiff1d(np.arange(len(g.v_id)), rows)
    np.testing.assert_array_equal(v[rest], v0[rest])      # unchanged bits elsewhere
    held = want.v_pos[rows].astype(np.float32).astype(np.float64) if precision == 32 else want.v_pos[rows]
    np.testing.assert_array_equal(v[rows, :2], held[:, :2])
    is_pose = g.v_type[rows] == 0
    if precision == 64:
        assert np.abs(v[rows, 2] - want.v_pos[rows, 2])[is_pose].max() <= 1e-15
    else:      # the handle holds (float)cos, (float)sin: the angle is good to f32
        assert np.abs(v[rows, 2] - want.v_pos[rows, 2])[is_pose].max() <= 2e-7
    assert np.all(v[rows, 2][~is_pose] == 0)


@pytest.mark.parametrize("graph", ["c1", "synth_600"])
def test_all_estimates_back_to_the_start_after_optimising_with_a_replay_in_play(graph):
    g = _c1() if graph == "c1" else lm_rules.synth_600()
    kw = dict(pcg_rel_tol=1e-12, odom_jacobian="analytic", use_graphs=1, warm_requests=True)
    a, b = HipOptimizer(**kw), HipOptimizer(**kw)
    try:
        a.set_graph(g)
        a.optimize(5); live = a.optimize(5)      # the second call on these tables captures the PCG iterations, and replays them
        assert live["graph_replay"] and not np.array_equal(a.vertices(), g.v_pos)
        st = a.set_vertices(g.v_pos)
        assert st["listed"] == len(g.v_id)
        b.set_graph(g)
        same(a.linearize(), b.linearize(), "every estimate back at the start")
        np.testing.assert_array_equal(a.vertices(), b.vertices())
        r, rb = a.optimize(10), b.optimize(10)
        assert r["graph_replay"] and not r["history_carried"]
        _trace_close(r, rb, a.vertices(), b.vertices(), g.v_type, "%s: the next optimize" % graph)
    finally:
        a.close(); b.close()


def test_a_sparse_estimate_edit_after_optimising_keeps_the_other_bits():
    g = lm_rules.synth_600()
    kw = dict(pcg_rel_tol=1e-12, odom_jacobian="analytic")
    a, b = HipOptimizer(**kw), HipOptimizer(**kw)
    try:
        a.set_graph(g); a.optimize(3)
        v = a.vertices()
        ids = g.v_id[[3, 700, 11]]
        pos = v[[3, 700, 11]] + 0.25
        a.set_vertices(pos, ids)
        v1 = a.vertices()
        rest = np.setdiff1d(np.arange(len(g.v_id)), [3, 700, 11])
        np.testing.assert_array_equal(v1[rest], v[rest])
        np.testing.assert_array_equal(v1[[3, 700, 11], :2], pos[:, :2])
        # a fresh handle at the same host estimates: chi^2 of the linearisation to the bound of a trace (the poses went through atan2)
        h = g.copy(); h.v_pos[:] = v1
        b.set_graph(h)
        ca, cb = a.linearize()[2], b.linearize()[2]
        print("chi2 after a sparse edit %r against a fresh handle at vertices() %r" % (ca, cb))
        assert abs(ca - cb) <= 1e-9 * cb
        r, rb = a.optimize(3), b.optimize(3)
        _trace_close(r, rb, a.vertices(), b.vertices(), g.v_type, "after a sparse estimate edit")
    finally:
        a.close(); b.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_every_error_returns_a_code_and_a_message_and_leaves_the_handle_as_it_was():
    g = _c1()
    V = len(g.v_id)
    lm0 = int(g.v_id[g.v_type == 1][0])
    unknown = int(g.v_id.max()) + 5
    o = HipOptimizer()
    lib = o.lib

    def ptr(a, dt):
        return None if a is None else np.ascontiguousarray(a, dt)

    def fixed_call(n, ids, count, handle=None):
        i, c = ptr(ids, np.uint32), ptr(count, np.int32)
        rc = lib.tsgo_set_fixed(o.h if handle is None else handle, n, None if i is None else i.ctypes.data, None if c is None else c.ctypes.data, None)
        return rc, lib.tsgo_last_error().decode()

    def est_call(n, ids, pos, handle=None):
        i, p = ptr(ids, np.uint32), ptr(pos, np.float64)
        rc = lib.tsgo_set_estimates(o.h if handle is None else handle, n, None if i is None else i.ctypes.data, None if p is None else p.ctypes.data, None)
        return rc, lib.tsgo_last_error().decode()

    try:
        out = np.zeros(V, np.int32)
        for rc, msg in (fixed_call(1, [0], [1]), est_call(1, [0], [[0.0, 0.0, 0.0]])):
            assert rc < 0 and "no graph" in msg
        assert lib.tsgo_get_fixed(o.h, out.ctypes.data, V) < 0 and "no graph" in lib.tsgo_last_error().decode()
        o.set_graph(g)
        o.set_fixed([41, lm0], [2, 1])      # the buffer exists, one edit is in place
        o.set_vertices([[1.0, 2.0, 0.5]], [7])
        before, counts, verts = o.linearize(), o.fixed_counts(), o.vertices()
        nan, inf = float("nan"), float("inf")
        zeros = np.zeros((V, 3))
        bad_fixed = {
            "n < 0": (-1, [0], [1]),
            "ids NULL": (2, None, [1, 1]),
            "unknown id": (2, [5, unknown], [1, 1]),
            "an id twice": (3, [5, 9, 5], [1, 1, 1]),
            "more ids than vertices": (V + 1, np.r_[g.v_id, 0], np.ones(V + 1)),
            "count -1": (2, [5, 9], [1, -1]),
            "count 65536": (1, [lm0], [65536]),
        }
        bad_est = {
            "n < 0": (-1, [0], zeros[:1]),
            "v_pos NULL": (1, [0], None),
            "ids NULL with n != n_vertices": (V - 1, None, zeros[:V - 1]),
            "ids NULL with n = 0": (0, None, None),
            "unknown id": (1, [unknown], zeros[:1]),
            "an id twice": (2, [lm0, lm0], zeros[:2]),
            "NaN x of a pose": (2, [3, 4], [[0.0, 0.0, 0.0], [nan, 0.0, 0.0]]),
            "infinite theta of a pose": (1, [3], [[0.0, 0.0, inf]]),
            "NaN y of a landmark": (1, [lm0], [[0.0, nan, 0.0]]),
            "NaN, dense": (V, None, np.where(np.arange(V)[:, None] == V // 2, nan, zeros)),
        }
        for call, name, cases in ((fixed_call, "tsgo_set_fixed", bad_fixed), (est_call, "tsgo_set_estimates", bad_est)):
            for what, args in cases.items():
                rc, msg = call(*args)
                assert rc < 0 and name in msg and len(msg) > 30, (what, rc, msg)
                same(o.linearize(), before, what)
                np.testing.assert_array_equal(o.fixed_counts(), counts, err_msg=what)
                np.testing.assert_array_equal(o.vertices(), verts, err_msg=what)
        assert fixed_call(1, [lm0], [65535])[0] == 0 and o.fixed_counts()[np.where(g.v_id == lm0)[0][0]] == 65535
        assert est_call(1, [lm0], [[1.0, 1.0, nan]])[0] == 0      # the third entry of a landmark is not used
        assert est_call(0, [0], None)[0] == 0                      # a list of length 0 changes nothing
        assert fixed_call(1, [0], [1], handle=C.c_void_p())[0] < 0 and est_call(1, [0], zeros[:1], handle=C.c_void_p())[0] < 0
        assert lib.tsgo_get_fixed(o.h, out.ctypes.data, V - 1) < 0 and "cap_vertices" in lib.tsgo_last_error().decode()
        assert lib.tsgo_get_fixed(o.h, None, V) < 0
        assert lib.tsgo_get_fixed(None, out.ctypes.data, V) < 0
        with pytest.raises(ValueError):
            o.set_fixed([1, 2, 3], [1, 1])
        with pytest.raises(ValueError):
            o.set_vertices(zeros[:2], [1, 2, 3])
    finally:
        o.close()
    shard = HipOptimizer(world=2, rank=0, testing=True)
    try:
        i = np.zeros(1, np.uint32); c = np.ones(1, np.int32); p = np.zeros(3)
        for rc in (shard.lib.tsgo_set_fixed(shard.h, 1, i.ctypes.data, c.ctypes.data, None), shard.lib.tsgo_get_fixed(shard.h, c.ctypes.data, 1),
                   shard.lib.tsgo_set_estimates(shard.h, 1, i.ctypes.data, p.ctypes.data, None)):
            assert rc < 0
        assert "world > 1" in shard.lib.tsgo_last_error().decode()
    finally:
        shard.close()
