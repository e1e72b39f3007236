"""tsgo_gate_edges on the device: candidates of all five edge types against the numpy restatement (tests/gate.py: dense inverse of the
oracle's H) on config 1, an identity of odometry chains that needs no oracle, tsgo_joint_marginals, the shapes where the read-out can go
wrong, its properties, the state rule, the error cases and the use case (true loop closures pass the gate, false ones do not).

Bounds (the issue's).  innov: |S - S_ref| <= 1e-8 |J|_inf^2 max|Sigma_ref pair block| + 1e-12 max|S_ref| — the 1e-8 that
test_gpu_joint_marginals._check_blockwise grants Sigma at rel_tol = 1e-12, pushed through J . J^T.  d2: 4 cond(S_ref) (that bound / max|S_ref|)
d2_ref + 1e-12, the perturbation bound of a solve with S with a factor 2 for the residual scale; logdet: dof times the same relative bound.
Worst observed ratios to these bounds (config 1, MI355X): DESIGN.md section 15."""
import ctypes as C

import numpy as np
import pytest

from tests import edge_report, gate, util
from tests.test_gpu_marginals import _chain, _run
from toyslam_amd import _lib
from toyslam_amd.graph import GraphArrays
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu

TOL = 1e-12


def _c1_handle(preconditioner="amg", odom_jacobian="constant", **kw):
    g = util.c1_arrays()
    o = HipOptimizer(pcg_rel_tol=1e-12, preconditioner=preconditioner, odom_jacobian=odom_jacobian, **kw)
    o.set_graph(g)
    o.optimize(5)
    return g, o


def _odom_meas(rng):
    th = rng.uniform(-np.pi, np.pi)
    return [np.cos(th), -np.sin(th), rng.uniform(-5, 5), np.sin(th), np.cos(th), rng.uniform(-5, 5), 0, 0, 1]


def _inf(rng):
    return rng.uniform(1.0, 400.0, 3)


def _lm_meas(rng):
    return [rng.uniform(0.5, 10), rng.uniform(-np.pi, np.pi), 0, 0, 0, 0, 0, 0, 0]


def _vlm_meas(rng):
    return [rng.uniform(0.5, 10), rng.uniform(-np.pi, np.pi), rng.uniform(0.5, 10), rng.uniform(-np.pi, np.pi), 0, 0, 0, 0, 0]


def _prior(g, vid, rng):
    x = g.v_pos[np.flatnonzero(g.v_id == vid)[0]]
    pose = g.v_type[np.flatnonzero(g.v_id == vid)[0]] == 0
    return [x[0] + rng.normal(0, 0.5), x[1] + rng.normal(0, 0.5), (x[2] + rng.uniform(-0.5, 0.5)) if pose else 0.0, 0, 0, 0, 0, 0, 0]


def _c1_candidates(g, seed=0):
    """The candidate set of the dense-inverse test: (candidates, the graph edges the first 40 re-present).  About 60 distinct vertices."""
    rng = np.random.default_rng(seed)
    pose = g.v_id[g.v_type == 0]; lm = g.v_id[g.v_type == 1]
    od = np.flatnonzero(g.e_type == 0)[10:30]                                  # 20 consecutive ODOM edges: poses 10 .. 30
    track = pose[10:31]
    lme = rng.choice(np.flatnonzero((g.e_type == 1) & np.isin(g.e_ids[:, 0], track)), 20, replace=False)
    pool_p = np.concatenate([track, pose[60:150:10]])                          # 30 poses
    seen = np.unique(g.e_ids[lme, 1])
    pool_l = np.concatenate([seen, rng.choice(np.setdiff1d(lm, seen), 30 - len(seen), replace=False)])      # 30 landmarks
    again = np.concatenate([od, lme])
    t, ids, meas, inf = [], [], [], []

    def add(ty, a, b, m):
        t.append(ty); ids.append([a, b]); meas.append(m); inf.append(_inf(rng))
    for _ in range(20):
        a, b = rng.choice(pool_p, 2, replace=False); add(0, a, b, _odom_meas(rng))
    for _ in range(20):
        add(1, rng.choice(pool_p), rng.choice(pool_l), _lm_meas(rng))
    for _ in range(10):
        a, b = rng.choice(pool_p, 2, replace=False); add(2, a, b, _vlm_meas(rng))
    for _ in range(5):
        a = rng.choice(pool_p); add(3, a, a, _prior(g, a, rng))
    for _ in range(5):
        a = rng.choice(pool_l); add(4, a, a, _prior(g, a, rng))
    add(0, g.fixed[0], pool_p[3], _odom_meas(rng))                              # touches the fixed vertex
    hub = pool_p[5]                                                             # one pose shared by 30 candidates
    others = np.setdiff1d(pool_p, [hub])
    for k, b in enumerate(rng.choice(others, 15, replace=False)):
        if k % 3 == 0:
            add(2, hub, b, _vlm_meas(rng))
        elif k % 3 == 1:
            add(0, b, hub, _odom_meas(rng))
        else:
            add(0, hub, b, _odom_meas(rng))
    for b in rng.choice(pool_l, 15, replace=False):
        add(1, hub, b, _lm_meas(rng))
    c = gate.concat([gate.edges_of(g, again), gate.candidates(t, ids, meas, inf)])
    assert len(c.e_type) == 131
    return c, again


def _distinct(g, c):
    ids = np.unique(c.e_ids)
    ty = g.v_type[gate._positions(g, ids)]
    return int((ty == 0).sum()), int((ty == 1).sum())


def _check_stats(g, c, st, preconditioner="amg"):
    n_pose, n_lm = _distinct(g, c)
    s = st["solve"]
    assert st["candidates"] == len(c.e_type) and st["vertices"] == n_pose + n_lm and st["not_pd"] == 0
    assert s["columns"] == 3 * n_pose + 2 * n_lm
    assert s["fallbacks"] == 0 and s["batches"] == -(-s["columns"] // s["batch_width"])
    assert s["preconditioner"] == (1 if preconditioner == "amg" else 0)
    assert st["ms_total"] > 0 and 0 < st["ms_readout"] < st["ms_total"]


def _check_against(res, ref, g, what):
    """Every candidate against the restatement at the bounds of the module docstring; returns the worst ratios to them."""
    K = len(ref["d2"])
    assert (res["status"] == 0).all() and np.array_equal(res["dof"], ref["dof"])
    scale = edge_report.coordinate_scale(g)
    worst = dict(e=float(np.abs(res["e"] - ref["e"]).max() / (1e-12 * scale)), innov=0.0, d2=0.0, logdet=0.0)
    bad = []
    for k in range(K):
        smax = np.abs(ref["innov"][k]).max()
        b_s = 1e-8 * ref["jnorm"][k] ** 2 * ref["sigmax"][k] + 1e-12 * smax
        rel = 4 * ref["cond"][k] * b_s / smax
        r = (np.abs(res["innov"][k] - ref["innov"][k]).max() / b_s, abs(res["d2"][k] - ref["d2"][k]) / (rel * ref["d2"][k] + 1e-12),
             abs(res["logdet"][k] - ref["logdet"][k]) / (ref["dof"][k] * rel))
        for name, v in zip(("innov", "d2", "logdet"), r):
            worst[name] = max(worst[name], float(v))
        if max(r) > 1:
            bad.append((k, r))
    s_scale = max(1.0, float(ref["s"].max()))
    worst["s"] = float(np.abs(res["s"] - ref["s"]).max() / (1e-11 * s_scale))      # (tests/edge_report.assert_records: 1e-11 of the largest s)
    print("%s: worst ratio to its bound: e %.3g, s %.3g, innov %.3g, d2 %.3g, logdet %.3g" % (what, worst["e"], worst["s"], worst["innov"], worst["d2"], worst["logdet"]))
    assert worst["e"] <= 1 and worst["s"] <= 1, (what, worst)
    assert not bad, (what, bad[:5])
    return worst


# ---- 4. against the dense inverse ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preconditioner", ["amg", "jacobi"])
@pytest.mark.parametrize("odom_jacobian", ["constant", "analytic"])
def test_c1_against_dense_inverse(preconditioner, odom_jacobian):
    g, o = _c1_handle(preconditioner, odom_jacobian)
    try:
        v = o.vertices()
        c, again = _c1_candidates(g)
        res, st = o.gate_edges(c.e_type, c.e_ids, c.e_meas, c.e_inf, rel_tol=TOL, innovation=True)
        rep = o.edge_report()[0]["all"]
        assert np.array_equal(o.vertices(), v)
    finally:
        o.close()
    _check_stats(g, c, st, preconditioner)
    assert st["vertices"] <= 80
    # the re-presented graph edges: the residual and s of tsgo_edge_report (the same device functions)
    n = len(again)
    assert np.abs(res["e"][:n] - rep[again, 0:3]).max() <= 1e-12 * edge_report.coordinate_scale(g)
    assert np.abs(res["s"][:n] - rep[again, 3]).max() <= 1e-12 * max(1.0, rep[again, 3].max())
    ref = gate.gate(GraphArrays(g.v_id, g.v_type, v, g.e_type, g.e_ids, g.e_meas, g.e_inf, g.fixed), v, c, analytic=odom_jacobian == "analytic")
    _check_against(res, ref, g, "c1 %s %s" % (preconditioner, odom_jacobian))
    assert ref["d2"].max() > 100 and ref["d2"].min() < 10                    # both sides of any gate occur


# ---- 5. an identity that needs no oracle -------------------------------------------------------------------------------------------
def test_chain_edge_represented_has_the_sum_of_the_two_edge_covariances():
    """Odometry chain, first pose fixed, analytic Jacobians, zero residuals: H = Jt^T Omega Jt with Jt square (gauge rows included), so
    J_k Sigma J_k^T = Omega_k^-1 for every edge k: re-presented with information Omega_c it has S = diag(1 / Omega_k) + diag(1 / Omega_c)."""
    n = 60
    g = _chain(n)
    rng = np.random.default_rng(7)
    v = g.v_pos.copy()
    v[1:, 2] = rng.uniform(-1.0, 1.0, n - 1)                                    # rotations are not the identity
    meas = np.array([gate.relative_pose_meas(v[i], v[j]) for i, j in g.e_ids])
    inf = rng.uniform(20.0, 400.0, size=(n - 1, 3))
    g = GraphArrays(g.v_id, g.v_type, v, g.e_type, g.e_ids, meas, inf, g.fixed)
    inf_c = rng.uniform(20.0, 400.0, size=(n - 1, 3))
    o = HipOptimizer(pcg_rel_tol=1e-12, odom_jacobian="analytic")
    try:
        o.set_graph(g)
        res, st = o.gate_edges(g.e_type, g.e_ids, g.e_meas, inf_c, rel_tol=TOL, innovation=True)
    finally:
        o.close()
    assert st["solve"]["columns"] == 3 * n and st["vertices"] == n
    assert (res["status"] == 0).all()
    e_tol = 1e-12 * edge_report.coordinate_scale(g)
    assert np.abs(res["e"]).max() <= e_tol
    assert res["d2"].max() <= 3 * e_tol ** 2 * 200.0                            # |e|^2 |S^-1|, S >= (1 / 400 + 1 / 400) I
    for k in range(n - 1):
        ref = np.diag(1.0 / inf[k]) + np.diag(1.0 / inf_c[k])
        assert np.abs(res["innov"][k] - ref).max() <= 1e-8 * np.abs(ref).max(), (k, res["innov"][k], ref)


# ---- 6. the same solve, another read-out -------------------------------------------------------------------------------------------
def test_innovation_from_joint_marginals_agrees():
    g, o = _c1_handle()
    try:
        v = o.vertices()
        c, _ = _c1_candidates(g, seed=4)
        c = gate.take(c, [0, 25, 41, 47, 62, 68, 81, 85, 90, 93, 96, 99, 100, 104, 120])      # all five types
        assert set(c.e_type.tolist()) == {0, 1, 2, 3, 4}
        res, _st = o.gate_edges(c, rel_tol=TOL, innovation=True)
        ids = np.unique(c.e_ids)
        cov, off, _ = o.joint_marginals(ids, rel_tol=TOL)
    finally:
        o.close()
    _e, A, B = gate.linearise(g, v, c)
    at = {int(i): k for k, i in enumerate(ids)}
    for k in range(len(c.e_type)):
        dof = int(gate.DOF[c.e_type[k]])
        a, b = at[int(c.e_ids[k, 0])], at[int(c.e_ids[k, 1])]
        rows = np.arange(off[a], off[a + 1])
        J = A[k, :dof, :len(rows)]
        if c.e_type[k] <= 2:
            rb = np.arange(off[b], off[b + 1])
            J = np.hstack([J, B[k, :dof, :len(rb)]]); rows = np.concatenate([rows, rb])
        S = J @ cov[np.ix_(rows, rows)] @ J.T + np.diag(1.0 / c.e_inf[k, :dof])
        assert np.abs(res["innov"][k, :dof, :dof] - S).max() <= 1e-9 * np.abs(S).max(), (k, int(c.e_type[k]))


# ---- 7. shapes where the read-out can go wrong -------------------------------------------------------------------------------------
def _columns(g, c):
    """First column of every distinct vertex, in order of first appearance (3 a pose, 2 a landmark): the layout the header promises."""
    col, n = {}, 0
    for vid in c.e_ids.reshape(-1):
        if int(vid) not in col:
            col[int(vid)] = n
            n += 3 if g.v_type[np.flatnonzero(g.v_id == vid)[0]] == 0 else 2
    return col, n


def test_read_out_shapes():
    g, o = _c1_handle()
    rng = np.random.default_rng(21)
    pose = g.v_id[g.v_type == 0]; lm = g.v_id[g.v_type == 1]
    deg = np.bincount(g.e_ids[g.e_type == 1, 1], minlength=int(g.v_id.max()) + 1)
    single = int(np.flatnonzero(deg == 1)[0]); busiest = int(deg.argmax())
    assert deg[busiest] >= 20
    try:
        v = o.vertices()
        at_v = GraphArrays(g.v_id, g.v_type, v, g.e_type, g.e_ids, g.e_meas, g.e_inf, g.fixed)
        Hinv = gate.dense_inverse(at_v, v, False)

        def run(c, what):
            res, st = o.gate_edges(c, rel_tol=TOL, innovation=True)
            _check_stats(g, c, st)
            assert st["solve"]["batch_width"] == 16
            _check_against(res, gate.gate(at_v, v, c, False, Hinv), g, what)
            return res, st

        # columns: poses 20 .. 24 fill 0 .. 14, pose 25 straddles the first two batches (15 | 16, 17), the landmark of the fourth candidate
        # lies in the second batch while its pose lies in the first, and the last batch is partial
        p = pose[20:26]
        c = gate.candidates([0, 0, 0, 1, 0], [[p[0], p[1]], [p[2], p[3]], [p[4], p[5]], [p[0], lm[7]], [p[1], pose[40]]],
                            [_odom_meas(rng), _odom_meas(rng), _odom_meas(rng), _lm_meas(rng), _odom_meas(rng)], [_inf(rng) for _ in range(5)])
        col, n = _columns(g, c)
        assert col[int(p[5])] == 15 and col[int(lm[7])] == 18 and col[int(p[0])] == 0 and n == 23
        _res, st = run(c, "straddle / two batches / partial batch")
        assert st["solve"]["columns"] == 23 and st["solve"]["batches"] == 2

        one = gate.candidates([1], [[pose[33], single]], [_lm_meas(rng)], [_inf(rng)])
        _res, st = run(one, "K = 1")
        assert st["candidates"] == 1 and st["solve"]["columns"] == 5 and st["solve"]["batches"] == 1

        res, _st = run(gate.take(c, [0, 3, 0, 3, 0]), "duplicates")
        for a, b in ((0, 2), (0, 4), (1, 3)):
            for f in ("e", "s", "d2", "logdet", "innov"):
                assert np.array_equal(res[f][a], res[f][b]), (a, b, f)

        m = _vlm_meas(rng); w = _inf(rng)
        both = gate.candidates([2, 2], [[pose[50], pose[90]], [pose[90], pose[50]]], [m, [m[2], m[3], m[0], m[1], 0, 0, 0, 0, 0]], [w, w])
        res, _st = run(both, "a virtual landmark candidate and its reverse")
        assert np.abs(res["e"][0] + res["e"][1]).max() <= 1e-12 * edge_report.coordinate_scale(g)
        assert abs(res["d2"][0] - res["d2"][1]) <= 1e-9 * res["d2"][0]

        few = gate.candidates([1, 4, 1, 4, 1], [[pose[100], single], [single, single], [pose[3], busiest], [busiest, busiest], [pose[140], busiest]],
                              [_lm_meas(rng), _prior(g, single, rng), _lm_meas(rng), _prior(g, busiest, rng), _lm_meas(rng)], [_inf(rng) for _ in range(5)])
        run(few, "a landmark with one observation and the one with the most")
    finally:
        o.close()


def test_width_one_agrees_with_width_sixteen(monkeypatch):
    g = util.c1_arrays()
    c = gate.take(_c1_candidates(g, seed=2)[0], [0, 21, 40, 61, 80, 90, 95, 100])
    out = {}
    for w in ("16", "1"):
        monkeypatch.setenv("TSGO_MARGINAL_WIDTH", w)
        o = HipOptimizer(pcg_rel_tol=1e-12, testing=True)
        try:
            o.set_graph(g)
            o.optimize(5)
            out[w] = o.gate_edges(c, rel_tol=TOL, innovation=True)
        finally:
            o.close()
    (r16, s16), (r1, s1) = out["16"], out["1"]
    assert s16["solve"]["batch_width"] == 16 and s1["solve"]["batch_width"] == 1 and s1["solve"]["batches"] == s1["solve"]["columns"] == s16["solve"]["columns"]
    assert np.array_equal(r1["e"], r16["e"]) and np.array_equal(r1["s"], r16["s"])
    for f in ("innov", "d2", "logdet"):
        assert np.abs(r1[f] - r16[f]).max() <= 1e-9 * np.abs(r16[f]).max(), f


# ---- 8. properties -----------------------------------------------------------------------------------------------------------------
def test_properties_determinism_permutation_symmetry_and_no_innovation():
    g, o = _c1_handle()
    try:
        c, _ = _c1_candidates(g, seed=1)
        r1, st = o.gate_edges(c, rel_tol=TOL, innovation=True)
        r2, _ = o.gate_edges(c, rel_tol=TOL, innovation=True)
        r3, _ = o.gate_edges(c, rel_tol=TOL)
        perm = np.random.default_rng(5).permutation(len(c.e_type))
        rp, _ = o.gate_edges(gate.take(c, perm), rel_tol=TOL, innovation=True)
    finally:
        o.close()
    assert st["solve"]["batches"] > 1
    for f in ("e", "s", "d2", "dof", "logdet", "status", "innov"):
        assert np.array_equal(r1[f], r2[f]), f                                  # a repeated call gives the same bits
        if f != "innov":
            assert np.array_equal(r1[f], r3[f]), f                              # ... and so does one without innov_out
    assert "innov" not in r3
    assert np.array_equal(r1["innov"], r1["innov"].transpose(0, 2, 1))          # exactly symmetric
    two = r1["dof"] == 2
    assert not r1["innov"][two][:, 2, :].any() and not r1["innov"][two][:, :, 2].any() and not r1["e"][two, 2].any()
    for f in ("e", "s", "d2", "logdet", "innov"):
        a, b = rp[f], r1[f][perm]
        scale = np.abs(b).reshape(len(perm), -1).max(axis=1).reshape((-1,) + (1,) * (b.ndim - 1))
        assert (np.abs(a - b) <= 1e-9 * np.maximum(scale, 1e-300)).all(), f
    assert np.array_equal(rp["dof"], r1["dof"][perm])


# ---- 9. the state rule -------------------------------------------------------------------------------------------------------------
def test_no_side_effects_on_the_solver():
    g = util.c1_arrays()
    c = gate.take(_c1_candidates(g)[0], np.arange(0, 131, 4))

    def a(o, m):
        o.set_graph(g)
        if m:
            o.gate_edges(c)
        r = o.optimize(10)
        return o.vertices(), r["chi2"], r["cg_iters"]
    for x, y in zip(_run(lambda o: a(o, False)), _run(lambda o: a(o, True))):
        assert np.array_equal(x, y)

    def b(o, m):
        o.set_graph(g)
        o.optimize(5)
        if m:
            v0 = o.vertices()
            o.gate_edges(c, innovation=True)
            assert np.array_equal(o.vertices(), v0)
        r = o.optimize(5)
        return r["stop"], r["iters"], r["chi2"], r["cg_iters"], o.vertices()
    x, y = _run(lambda o: b(o, False)), _run(lambda o: b(o, True))
    assert x[0] == y[0] and x[1] == y[1]
    for p, q in zip(x[2:], y[2:]):
        assert np.array_equal(p, q)


# ---- 10. errors --------------------------------------------------------------------------------------------------------------------
def _raw(o, c, n=None, rec="own", handle="own"):
    K = len(c.e_type)
    buf = np.full(8 * max(K, 1), -7.0)
    t = np.ascontiguousarray(c.e_type, np.uint32); ids = np.ascontiguousarray(c.e_ids, np.uint32)
    m = np.ascontiguousarray(c.e_meas, np.float64); w = np.ascontiguousarray(c.e_inf, np.float64)
    rc = o.lib.tsgo_gate_edges(o.h if handle == "own" else None, K if n is None else n, t.ctypes.data, ids.ctypes.data, m.ctypes.data, w.ctypes.data, 0.0,
                               buf.ctypes.data if rec == "own" else None, None, None)
    return rc, o.lib.tsgo_last_error().decode(), buf


def test_errors_leave_the_handle_usable():
    g = util.c1_arrays()
    rng = np.random.default_rng(8)
    pose = g.v_id[g.v_type == 0]; lm = g.v_id[g.v_type == 1]
    p, q, l = int(pose[3]), int(pose[9]), int(lm[0])
    good = gate.candidates([0, 1, 2, 3, 4], [[p, q], [p, l], [q, p], [p, p], [l, l]],
                           [_odom_meas(rng), _lm_meas(rng), _vlm_meas(rng), _prior(g, p, rng), _prior(g, l, rng)], [_inf(rng) for _ in range(5)])

    def variant(k, **kw):
        c = gate.take(good, np.arange(5))
        for f, val in kw.items():
            getattr(c, f)[k] = val
        return c

    def refused(o, c, *words, **kw):
        rc, msg, buf = _raw(o, c, **kw)
        assert rc < 0 and "tsgo_gate_edges" in msg and all(x in msg for x in words), (rc, msg)
        assert (buf == -7.0).all()                                             # a refused call writes nothing

    o = HipOptimizer()
    try:
        refused(o, good, "null handle", handle=None)
        refused(o, good, "no graph")
        o.set_graph(g)
        refused(o, variant(1, e_ids=[p, 987654]), "unknown vertex id 987654")
        refused(o, variant(2, e_type=7), "candidate 2", "unknown edge type 7")
        refused(o, variant(1, e_ids=[l, p]), "candidate 1", "Se2 vertex to a Point2")       # LM: a pose, then a landmark
        refused(o, variant(0, e_ids=[p, l]), "candidate 0", "two Se2")
        refused(o, variant(2, e_ids=[l, p]), "candidate 2", "two Se2")
        refused(o, variant(3, e_ids=[l, l]), "candidate 3", "Se2 vertex")
        refused(o, variant(4, e_ids=[p, p]), "candidate 4", "Point2 vertex")
        refused(o, variant(0, e_ids=[p, p]), "candidate 0", "to itself")
        refused(o, variant(2, e_ids=[q, q]), "candidate 2", "to itself")
        refused(o, variant(3, e_ids=[p, q]), "candidate 3", "same vertex id twice")
        refused(o, variant(4, e_ids=[l, int(lm[1])]), "candidate 4", "same vertex id twice")
        for bad in (0.0, -1.0, np.nan, np.inf):
            refused(o, variant(0, e_inf=[4.0, 4.0, bad]), "candidate 0", "information entry 2")
            refused(o, variant(1, e_inf=[bad, 4.0, 0.0]), "candidate 1", "information entry 0")
            refused(o, variant(4, e_inf=[4.0, bad, 0.0]), "candidate 4", "information entry 1")
        refused(o, variant(0, e_meas=np.zeros(9)), "candidate 0", "singular measurement")
        refused(o, good, "n = -1", n=-1)
        refused(o, good, "outside", n=(1 << 20) + 1)
        refused(o, good, "bad argument", rec=None)
        rc, _msg, buf = _raw(o, good, n=0)
        assert rc == 0 and (buf == -7.0).all()                                 # n == 0 returns 0 and solves nothing
        res, st = o.gate_edges(gate.candidates([], [], [], []))
        assert st["candidates"] == 0 and st["solve"]["columns"] == 0 and len(res["d2"]) == 0
        # the third information entry of a 2-dof type is not read
        res, st = o.gate_edges(variant(1, e_inf=[4.0, 4.0, -1.0]), innovation=True)
        assert (res["status"] == 0).all() and np.isfinite(res["d2"]).all() and st["not_pd"] == 0 and st["vertices"] == 3
        free = GraphArrays(g.v_id, g.v_type, g.v_pos, g.e_type, g.e_ids, g.e_meas, g.e_inf, np.zeros(0, np.uint32))
        o.set_graph(free)
        refused(o, good, "fixed vertex")
        o.set_graph(g)
        assert np.isfinite(o.gate_edges(good)[0]["d2"]).all()
        assert o.optimize(2)["iters"] == 2
    finally:
        o.close()
    o = HipOptimizer(precision=32)
    try:
        o.set_graph(g)
        refused(o, good, "precision")
        assert o.optimize(2)["iters"] == 2
    finally:
        o.close()
    shard = HipOptimizer(world=2, rank=0, testing=True)
    try:
        refused(shard, good, "world > 1")
        with pytest.raises(RuntimeError, match="world > 1"):
            shard.gate_edges(good)
    finally:
        shard.close()


# ---- 11. the use case --------------------------------------------------------------------------------------------------------------
def test_the_gate_separates_true_from_false_loop_closures():
    base, cand, is_true = gate.scenario_split()
    o = HipOptimizer(pcg_rel_tol=1e-12, rules="lm", odom_jacobian="analytic")
    try:
        o.set_graph(base)
        r = o.optimize(30)
        v = o.vertices()
        res, st = o.gate_edges(cand, rel_tol=TOL)
    finally:
        o.close()
    assert r["stop"] == "converged"
    ref = gate.gate(base, v, cand, analytic=True)
    accept, accept_ref = res["d2"] < gate.CHI2_99[3], ref["d2"] < gate.CHI2_99[3]
    print("device d2: true %.3g .. %.3g, false %.3g .. %.3g" % (res["d2"][is_true].min(), res["d2"][is_true].max(), res["d2"][~is_true].min(), res["d2"][~is_true].max()))
    assert np.array_equal(accept, accept_ref) and np.array_equal(accept, is_true)
    assert accept.sum() == 12 and (~accept).sum() == 13
    assert (np.abs(res["d2"] - ref["d2"]) <= 1e-4 * ref["d2"]).all()
    assert st["not_pd"] == 0 and (res["status"] == 0).all()
