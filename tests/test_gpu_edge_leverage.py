"""tsgo_edge_leverage on the device against the numpy restatement of tests/leverage.py: the records from the device's own samples (the
sharp test), from the dense samples, the stats, the closed form of a landmark's only observation, the bitwise properties, the statistics
at K = 512, the state rule and every refusal.

Measured on the first device run (the largest value over every case of the test named; each bound is 10 x that, under the cap the test
states):
  MEASURED_SHARP   test_records_from_the_devices_own_samples: |C - C_ref| over the largest |C| of the edge's class, and |h - h_ref| over
                   (the largest weight of the class) x (that |C|) — h = sum_j a_j C_jj carries the weight's unit.  Only the summation
                   order and the recomputed J differ; y = delta_v - delta_u is the difference of two large correlated numbers, so the
                   figure is not derivable.
  MEASURED_DENSE   test_records_from_the_dense_samples: the same two ratios against the restatement's dense samples — the sample error
                   6.3e-10 of tests/test_gpu_sample_marginals.py amplified by |delta| / |y|.
  MEASURED_TRACE   test_stats: stats.trace against (1 / K) sum_k delta_k^T H delta_k of the device's samples, relative.
  MEASURED_CLOSED  test_a_landmarks_only_observation_in_closed_form: K h against sum_k (n0^2 + n1^2), relative.
  MEASURED_ORDER   test_width_and_lanes_agree: width 1 against 16 and lanes 1 against 8, the ratios of the sharp test."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import leverage, posterior, util
from toyslam_amd import _lib
from toyslam_amd.graph import GraphArrays
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu

MEASURED_SHARP = 8.134e-15      # C 7.600e-16, h 8.134e-15 (block-Jacobi, analytic Jacobians, lanes 8, the five-class graph)
MEASURED_DENSE = 8.516e-11      # C 8.516e-11, h 3.117e-11 (block-Jacobi, analytic Jacobians, the five-class graph; multigrid stays below 7.7e-11)
MEASURED_TRACE = 3.552e-15      # (c1, multigrid, constant Jacobians, lanes 1)
MEASURED_CLOSED = 1.252e-15     # (63 edges of c1)
MEASURED_ORDER = 5.001e-15      # width 1 against 16: 4.167e-16, lanes 1 against 8: 5.001e-15
SHARP_TOL = min(10 * MEASURED_SHARP, 1e-8)
DENSE_TOL = min(10 * MEASURED_DENSE, 1e-5)
TRACE_TOL = min(10 * MEASURED_TRACE, 1e-6)
CLOSED_TOL = min(10 * MEASURED_CLOSED, 1e-6)
ORDER_TOL = min(10 * MEASURED_ORDER, 1e-11)
K_SMALL = 21      # 16 + 5 at width 16, 8 + 8 + 5 under block-Jacobi

CASES = [(p, j, lanes) for p in ("amg", "jacobi") for j in ("constant", "analytic") for lanes in (1, 8)] + [("amg", "analytic", "per-edge")]
EXEMPT = ["none"]      # the palette of the per-edge case: a few edges of types 0 - 2 leave their class's kernel


def _handle(preconditioner="amg", odom_jacobian="constant", lanes=0, **kw):
    return HipOptimizer(preconditioner=preconditioner, odom_jacobian=odom_jacobian, lanes_per_pose=lanes, lanes_per_lm=lanes, **kw)


@functools.lru_cache(maxsize=None)
def _five():
    return posterior.five_class_graph()[0]


def _exempt_entry(g):
    return ((np.arange(len(g.e_type)) % 7 == 0) & (g.e_type <= 2)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _five_reference(jacobian, per_edge):
    """(restatement, dense system, dense samples) of the five-class graph at its own estimates (no device step is taken on it)."""
    g = _five()
    R = leverage.Restatement(g, posterior.ROBUST, jacobian, *((EXEMPT, _exempt_entry(g)) if per_edge else ()))
    S = R.system()
    return R, S, S.samples(posterior.SEED, K_SMALL)[0]


@functools.lru_cache(maxsize=None)
def _case(preconditioner, odom_jacobian, lanes):
    """One device run per case, shared by tests 1 - 3: a list of (name, restatement, dense system, dense samples, sample_marginals result,
    edge_leverage result)."""
    per_edge = lanes == "per-edge"
    c1, five = util.c1_arrays(), _five()
    out = []
    o = _handle(preconditioner, odom_jacobian, 0 if per_edge else lanes)
    try:
        if not per_edge:
            o.set_graph(c1)
            o.optimize(5)
            v = o.vertices()
            s1 = o.sample_marginals(K_SMALL, seed=posterior.SEED, samples=True)
            l1 = o.edge_leverage(K_SMALL, seed=posterior.SEED)
            assert np.array_equal(o.vertices(), v)
            R = leverage.Restatement(posterior.at(c1, v), None, odom_jacobian)
            S = R.system()
            out.append(("c1", R, S, S.samples(posterior.SEED, K_SMALL)[0], s1, l1))
        o.set_robust(**posterior.ROBUST)
        o.set_graph(five)
        if per_edge:
            assert o.set_edge_robust(EXEMPT, _exempt_entry(five))["active"]
        s5 = o.sample_marginals(K_SMALL, seed=posterior.SEED, samples=True)
        l5 = o.edge_leverage(K_SMALL, seed=posterior.SEED)
        out.append(("five classes",) + _five_reference(odom_jacobian, per_edge) + (s5, l5))
    finally:
        o.close()
    return out


def _errors(R, rec, ref):
    """(worst C error, worst h error) in the units of the module docstring; dof_a must be equal."""
    t = R.g.e_type
    scale = leverage.class_scale(ref, t)
    amax = np.zeros(len(t))
    for c in range(5):
        if (t == c).any():
            amax[t == c] = R.a[t == c].max()
    assert np.array_equal(rec[:, 7], ref[:, 7])
    return float((np.abs(rec[:, :6] - ref[:, :6]).max(axis=1) / scale).max()), float((np.abs(rec[:, 6] - ref[:, 6]) / (amax * scale)).max())


# ---- 1. the sharp test: the device's own samples through the restatement -------------------------------------------------------------
@pytest.mark.parametrize("preconditioner,odom_jacobian,lanes", CASES)
def test_records_from_the_devices_own_samples(preconditioner, odom_jacobian, lanes):
    for name, R, _S, _d, smp, lev in _case(preconditioner, odom_jacobian, lanes):
        rec = lev["all"]
        ec, eh = _errors(R, rec, R.records(smp["samples"]))
        print("sharp: %s C %.3e h %.3e (%s, %s, %s)" % (name, ec, eh, preconditioner, odom_jacobian, lanes))
        assert ec <= SHARP_TOL and eh <= SHARP_TOL, (name, ec, eh)
        # the views of the Python wrapper
        E = len(R.g.e_type)
        assert lev["cov"].shape == (E, 3, 3) and np.array_equal(lev["cov"], lev["cov"].transpose(0, 2, 1))
        assert np.array_equal(lev["cov"][:, 0, 1], rec[:, 1]) and np.array_equal(lev["cov"][:, 1, 2], rec[:, 4]) and np.array_equal(lev["cov"][:, 2, 2], rec[:, 5])
        assert np.array_equal(lev["h"], rec[:, 6]) and np.array_equal(lev["dof"], rec[:, 7]) and np.array_equal(lev["redundancy"], rec[:, 7] - rec[:, 6])
        assert not rec[leverage.DOF[R.g.e_type] == 2][:, [2, 4, 5]].any()
        zero = np.flatnonzero(~R.a.any(axis=1))
        assert (rec[zero, 6] == 0).all() and (rec[zero, 7] == 0).all() and (rec[zero, 0] > 0).all()
        assert len(zero) == (1 if name == "five classes" else 0)


# ---- 2. against the dense samples ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preconditioner,odom_jacobian,lanes", CASES)
def test_records_from_the_dense_samples(preconditioner, odom_jacobian, lanes):
    for name, R, _S, dense, _smp, lev in _case(preconditioner, odom_jacobian, lanes):
        ec, eh = _errors(R, lev["all"], R.records(dense))
        print("dense: %s C %.3e h %.3e (%s, %s, %s)" % (name, ec, eh, preconditioner, odom_jacobian, lanes))
        assert ec <= DENSE_TOL and eh <= DENSE_TOL, (name, ec, eh)


# ---- 3. the stats --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preconditioner,odom_jacobian,lanes", CASES)
def test_stats(preconditioner, odom_jacobian, lanes):
    width = 16 if preconditioner == "amg" else 8
    for name, R, S, _d, smp, lev in _case(preconditioner, odom_jacobian, lanes):
        st, rec, g = lev["stats"], lev["all"], R.g
        assert st["samples"] == K_SMALL and st["solve"]["columns"] == K_SMALL and st["solve"]["batch_width"] == width
        assert st["solve"]["batches"] == (2 if width == 16 else 3) and st["solve"]["fallbacks"] == 0
        assert st["ms_noise"] > 0 and st["ms_readout"] > 0 and st["ms_total"] >= st["solve"]["ms_solve"]
        edges, h_sum, dof_sum = leverage.fold(rec, g.e_type)
        assert np.array_equal(st["edges"], edges) and np.array_equal(st["dof_sum"], dof_sum)
        assert (np.abs(st["h_sum"] - h_sum) <= 1e-13 * np.abs(h_sum)).all()
        t = sum(h_sum.tolist(), 0.0) + st["h_gauge"]      # the classes in order, the gauge term last
        assert abs(st["trace"] - t) <= 1e-13 * abs(t)
        hg = R.h_gauge(smp["samples"])
        assert abs(st["h_gauge"] - hg) <= 1e-12 * hg
        assert st["unknowns"] == 3 * int((g.v_type == 0).sum()) + 2 * int((g.v_type == 1).sum()) == S.H.shape[0]
        x = S.packed(smp["samples"])
        q = float(np.einsum("kn,nm,km->k", x, S.H, x).mean())
        err = abs(st["trace"] - q) / q
        print("trace: %s %.6f against mean delta^T H delta %.6f: %.3e (%s, %s, %s)" % (name, st["trace"], q, err, preconditioner, odom_jacobian, lanes))
        assert err <= TRACE_TOL, (name, err)


# ---- 4. closed form: the only observation of a landmark ------------------------------------------------------------------------------
def test_a_landmarks_only_observation_in_closed_form():
    """The landmark absorbs the edge's whole perturbation: sqrt(a_j) y_j = n_j, the edge's own noise, so K h = sum_k (n0^2 + n1^2).  No
    solve is restated."""
    g = util.c1_arrays()
    single = posterior.single_observation_landmarks(g)
    assert not np.isin(single, g.fixed).any() and not (g.e_type >= 3).any()      # free, without a prior
    edges = np.flatnonzero((g.e_type == 1) & np.isin(g.e_ids[:, 1], single))
    assert len(edges) == len(single) > 0
    o = _handle()
    try:
        o.set_graph(g)
        lev = o.edge_leverage(K_SMALL, seed=posterior.SEED)
    finally:
        o.close()
    noise = _lib.host_lib().tsgo_sample_noise
    nrm = (C.c_double * 4)()
    worst = 0.0
    for e in edges:
        want = 0.0
        for k in range(K_SMALL):
            noise(posterior.SEED, 0, int(e), k, None, nrm)
            want += nrm[0] ** 2 + nrm[1] ** 2
        worst = max(worst, abs(K_SMALL * lev["h"][e] - want) / want)
    print("closed form: %d edges, worst relative difference %.3e" % (len(edges), worst))
    assert worst <= CLOSED_TOL
    assert (lev["dof"][edges] == 2).all()


# ---- 5. bitwise properties -----------------------------------------------------------------------------------------------------------
def test_repeat_and_seed():
    g = _five()
    o = _handle()
    try:
        o.set_robust(**posterior.ROBUST)
        o.set_graph(g)
        a = o.edge_leverage(K_SMALL, seed=posterior.SEED)
        b = o.edge_leverage(K_SMALL, seed=posterior.SEED)
        other = o.edge_leverage(K_SMALL, seed=posterior.SEED + 1)
    finally:
        o.close()
    assert np.array_equal(a["all"], b["all"])
    for f in ("edges", "h_sum", "dof_sum"):
        assert np.array_equal(a["stats"][f], b["stats"][f])
    assert a["stats"]["trace"] == b["stats"]["trace"] and a["stats"]["h_gauge"] == b["stats"]["h_gauge"]
    assert (a["all"][:, [0, 1, 3]] != other["all"][:, [0, 1, 3]]).all()      # every record moves (its 2x2 corner is there in every class)
    assert np.array_equal(a["all"][:, 7], other["all"][:, 7])


def test_width_and_lanes_agree(monkeypatch):
    g = _five()
    out = {}
    for name, width, lanes in (("w16", "16", 0), ("w1", "1", 0), ("l1", "16", 1), ("l8", "16", 8)):
        monkeypatch.setenv("TSGO_MARGINAL_WIDTH", width)
        o = _handle(lanes=lanes, testing=True)
        try:
            o.set_robust(**posterior.ROBUST)
            o.set_graph(g)
            out[name] = o.edge_leverage(5, seed=posterior.SEED)
        finally:
            o.close()
    assert out["w16"]["stats"]["solve"]["batch_width"] == 16 and out["w1"]["stats"]["solve"]["batch_width"] == 1
    assert out["w1"]["stats"]["solve"]["batches"] == 5
    R = _five_reference("constant", False)[0]
    e_w = max(_errors(R, out["w1"]["all"], out["w16"]["all"]))
    e_l = max(_errors(R, out["l1"]["all"], out["l8"]["all"]))
    print("summation order: width 1 against 16 %.3e  lanes 1 against 8 %.3e" % (e_w, e_l))
    assert e_w <= ORDER_TOL and e_l <= ORDER_TOL, (e_w, e_l)


# ---- 6. statistics -------------------------------------------------------------------------------------------------------------------
def test_statistics_at_512_samples():
    """c1 at its start, analytic Jacobians, multigrid: the graph, seed and K tests/test_edge_leverage_cpu.py qualifies."""
    from tests.test_edge_leverage_cpu import _c1
    g = util.c1_arrays()
    K = posterior.K_STAT
    o = _handle("amg", "analytic")
    try:
        o.set_graph(g)
        lev = o.edge_leverage(K, seed=posterior.SEED_STAT)
    finally:
        o.close()
    st = lev["stats"]
    assert st["solve"]["batches"] == K // 16 and st["solve"]["fallbacks"] == 0
    R, S, Sigma = _c1("analytic")
    ratio = R.weighted_rows(lev["all"]) / R.weighted_rows(R.exact(Sigma))
    bound = posterior.BOUND * np.sqrt(2.0 / K)
    n = S.H.shape[0]
    print("%d rows, a_j C_jj over its exact value in [%.4f, %.4f], bound 1 +- %.4f; trace %.3f (n = %d), h_gauge %.4f" %
          (len(ratio), ratio.min(), ratio.max(), bound, st["trace"], n, st["h_gauge"]))
    assert len(ratio) == int((R.a > 0).sum()) and np.abs(ratio - 1).max() <= bound
    assert n == 1134 and st["unknowns"] == n and abs(st["trace"] - n) <= 12.63      # 6 sqrt(2 n / K)
    assert abs(st["h_gauge"] - 3) <= posterior.BOUND * 3 * np.sqrt(2.0 / (3 * K))
    single = posterior.single_observation_landmarks(g)
    only = np.flatnonzero((g.e_type == 1) & np.isin(g.e_ids[:, 1], single))
    assert (lev["redundancy"][only] < 0).any() and (lev["redundancy"][only] > 0).any()      # h = dof exactly there: the sampled value is not clamped


# ---- 7. state rule -------------------------------------------------------------------------------------------------------------------
def test_no_side_effects_on_the_solver():
    g = util.c1_arrays()

    def fresh(call):      # from a handle that has not solved yet: bit for bit
        o = _handle()
        try:
            o.set_graph(g)
            lin = None
            if call:
                before = o.linearize()
                o.edge_leverage(5, seed=1)
                lin = o.linearize()
                for x, y in zip(before, lin):
                    assert np.array_equal(x, y)
            else:
                o.linearize(); lin = o.linearize()
            r = o.optimize(10)
            return (o.vertices(), r["chi2"], r["cg_iters"]) + tuple(np.asarray(x) for x in lin)
        finally:
            o.close()
    for x, y in zip(fresh(False), fresh(True)):
        assert np.array_equal(x, y)

    def run(call):
        o = _handle()
        try:
            o.set_graph(g)
            first = o.optimize(5)
            if call:
                v0 = o.vertices()
                o.edge_leverage(K_SMALL, seed=posterior.SEED)
                assert np.array_equal(o.vertices(), v0)
            r = o.optimize(5)
            return first, r, o.vertices()
        finally:
            o.close()
    (fa, ra, va), (fb, rb, vb) = run(False), run(True)
    assert np.array_equal(fa["chi2"], fb["chi2"]) and np.array_equal(fa["cg_iters"], fb["cg_iters"])
    assert ra["stop"] == rb["stop"] and ra["iters"] == rb["iters"]
    assert np.array_equal(ra["cg_iters"], rb["cg_iters"])
    # (the bounds tests/test_gpu_sample_marginals.py puts on the same run after its call: a handle with a solver history)
    assert np.abs(ra["chi2"] - rb["chi2"]).max() <= 1e-9 * np.abs(ra["chi2"]).max()
    assert util.max_vertex_diff(va, vb, g.v_type) <= 1e-9


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    g = util.c1_arrays()
    E = len(g.e_type)
    o = _handle()
    try:
        with pytest.raises(RuntimeError, match="no graph"):
            o.edge_leverage(4)
        o.set_graph(g)
        for k in (0, -3, 65537):
            with pytest.raises(RuntimeError, match="n_samples"):
                o.edge_leverage(k)
        rec = np.zeros((E, 8))
        raw = lambda *a: o.lib.tsgo_edge_leverage(o.h, *a)
        assert raw(4, 0, 0.0, None, E, None) < 0 and b"rec_out" in o.lib.tsgo_last_error()
        assert raw(4, 0, 0.0, rec.ctypes.data, E - 1, None) < 0 and b"cap_edges" in o.lib.tsgo_last_error()
        assert o.lib.tsgo_edge_leverage(None, 4, 0, 0.0, rec.ctypes.data, E, None) < 0 and b"null handle" in o.lib.tsgo_last_error()
        assert not rec.any()
        assert raw(4, 0, 0.0, rec.ctypes.data, E, None) == 0      # stats may be NULL, the exact capacity passes
        assert np.isfinite(rec).all() and (rec[:, 0] > 0).all()
        free = GraphArrays(g.v_id, g.v_type, g.v_pos, g.e_type, g.e_ids, g.e_meas, g.e_inf, np.zeros(0, np.uint32))
        o.set_graph(free)
        with pytest.raises(RuntimeError, match="fixed vertex"):
            o.edge_leverage(4)
        o.set_graph(g)
        assert o.optimize(2)["iters"] == 2
        assert o.edge_leverage(1)["stats"]["samples"] == 1
    finally:
        o.close()
    o = _handle(precision=32)
    try:
        o.set_graph(g)
        with pytest.raises(RuntimeError, match="precision"):
            o.edge_leverage(4)
        assert o.optimize(2)["iters"] == 2
    finally:
        o.close()
    shard = HipOptimizer(world=2, rank=0, testing=True)
    try:
        with pytest.raises(RuntimeError, match="world > 1"):
            shard.edge_leverage(4)
    finally:
        shard.close()
