"""tsgo_sample_marginals on the device against the dense restatement of tests/posterior.py: the samples themselves, cov_out against
the same call's samples, the bitwise properties, the statistics at K = 512, the state rule and every refusal."""
import functools

import numpy as np
import pytest

from tests import posterior, util
from toyslam_amd.graph import GraphArrays
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu

# max over samples of max |delta_dev - delta_dense| / max |delta_dense|.  Not derivable (PCG at 1e-10 in the D-norm against a dense solve
# of a matrix with cond(H) ~ 1e8), so measured on the first device run against the restatement: the largest value over every case of
# test_samples_against_the_dense_restatement was MEASURED_SAMPLE_ERROR (block-Jacobi, analytic Jacobians, the five-class graph; the
# multigrid cases stay below 2.5e-10, width 1 against 16 gave 3.4e-16 and lanes 1 against 8 2.7e-14); the bound is 10 x that, and
# nothing above 1e-6 is accepted.
MEASURED_SAMPLE_ERROR = 6.269e-10
SAMPLE_TOL = min(10 * MEASURED_SAMPLE_ERROR, 1e-6)
K_SMALL = 21      # 16 + 5 at width 16, 8 + 8 + 5 under block-Jacobi


def _mask(g):
    return np.arange(3)[None, :] < np.where(g.v_type == 0, 3, 2)[:, None]


def _sample_error(dev, ref):
    return max(float(np.abs(dev[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in range(len(ref)))


@functools.lru_cache(maxsize=None)
def _five():
    return posterior.five_class_graph()[0]


@functools.lru_cache(maxsize=None)
def _five_reference(jacobian):
    """The dense samples of the five-class graph at its own estimates (no device step is taken on it)."""
    return posterior.System(_five(), posterior.ROBUST, jacobian).samples(posterior.SEED, K_SMALL)[0]


def _handle(preconditioner="amg", odom_jacobian="constant", lanes=0, **kw):
    return HipOptimizer(preconditioner=preconditioner, odom_jacobian=odom_jacobian, lanes_per_pose=lanes, lanes_per_lm=lanes, **kw)


# ---- 1. samples against the dense restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 8])
@pytest.mark.parametrize("odom_jacobian", ["constant", "analytic"])
@pytest.mark.parametrize("preconditioner", ["amg", "jacobi"])
def test_samples_against_the_dense_restatement(preconditioner, odom_jacobian, lanes):
    c1 = util.c1_arrays()
    o = _handle(preconditioner, odom_jacobian, lanes)
    try:
        o.set_graph(c1)
        o.optimize(5)
        v = o.vertices()
        r1 = o.sample_marginals(K_SMALL, seed=posterior.SEED, samples=True)
        assert np.array_equal(o.vertices(), v)
        o.set_robust(**posterior.ROBUST)
        o.set_graph(_five())
        r5 = o.sample_marginals(K_SMALL, seed=posterior.SEED, samples=True)
    finally:
        o.close()
    width = 16 if preconditioner == "amg" else 8
    for r in (r1, r5):
        st = r["stats"]
        assert st["samples"] == K_SMALL and st["solve"]["columns"] == K_SMALL and st["solve"]["batch_width"] == width
        assert st["solve"]["batches"] == (2 if width == 16 else 3) and st["solve"]["fallbacks"] == 0
        assert st["solve"]["preconditioner"] == (1 if preconditioner == "amg" else 0)
        assert st["ms_noise"] > 0 and st["ms_readout"] > 0 and st["ms_total"] >= st["solve"]["ms_solve"]
    ref1 = posterior.System(posterior.at(c1, v), None, odom_jacobian).samples(posterior.SEED, K_SMALL)[0]
    e1, e5 = _sample_error(r1["samples"], ref1), _sample_error(r5["samples"], _five_reference(odom_jacobian))
    print("sample error: c1 %.3e  five classes %.3e  (%s, %s, lanes %d)" % (e1, e5, preconditioner, odom_jacobian, lanes))
    assert e1 <= SAMPLE_TOL and e5 <= SAMPLE_TOL, (e1, e5)
    lm = c1.v_type == 1
    assert np.all(r1["samples"][:, lm, 2] == 0) and np.all(r5["samples"][:, _five().v_type == 1, 2] == 0)


# ---- 2. cov_out is the second moment of the same call's samples ----------------------------------------------------------------------
@pytest.mark.parametrize("which", ["c1", "five"])
def test_cov_is_the_second_moment_of_the_samples(which):
    g = util.c1_arrays() if which == "c1" else _five()
    o = _handle()
    try:
        if which == "five":
            o.set_robust(**posterior.ROBUST)
        o.set_graph(g)
        r = o.sample_marginals(K_SMALL, seed=posterior.SEED, samples=True)
    finally:
        o.close()
    cov, d = r["cov"], r["samples"]
    want = np.einsum("kvi,kvj->vij", d, d) / K_SMALL
    scale = np.abs(want).max(axis=(1, 2), keepdims=True)
    assert (np.abs(cov - want) <= 1e-13 * scale).all(), float((np.abs(cov - want) / scale).max())
    assert np.array_equal(cov, cov.transpose(0, 2, 1))
    lm = g.v_type == 1
    assert np.all(cov[lm][:, 2, :] == 0) and np.all(cov[lm][:, :, 2] == 0)
    assert (np.diagonal(cov, axis1=1, axis2=2)[_mask(g)] > 0).all()


# ---- 3. bitwise properties -----------------------------------------------------------------------------------------------------------
def test_repeat_prefix_and_seed():
    g = _five()
    o = _handle()
    try:
        o.set_robust(**posterior.ROBUST)
        o.set_graph(g)
        a = o.sample_marginals(K_SMALL, seed=posterior.SEED, samples=True)
        b = o.sample_marginals(K_SMALL, seed=posterior.SEED, samples=True)
        five = o.sample_marginals(5, seed=posterior.SEED, samples=True)
        other = o.sample_marginals(K_SMALL, seed=posterior.SEED + 1, samples=True)
        nosamples = o.sample_marginals(K_SMALL, seed=posterior.SEED)
    finally:
        o.close()
    assert np.array_equal(a["samples"], b["samples"]) and np.array_equal(a["cov"], b["cov"])
    assert np.array_equal(a["samples"][:5], five["samples"])
    assert nosamples["samples"] is None and np.array_equal(nosamples["cov"], a["cov"])
    m = _mask(g)
    assert (a["samples"][:, m] != other["samples"][:, m]).all()


def test_width_and_lanes_agree(monkeypatch):
    g = _five()
    out = {}
    for name, width, lanes in (("w16", "16", 0), ("w1", "1", 0), ("l1", "16", 1), ("l8", "16", 8)):
        monkeypatch.setenv("TSGO_MARGINAL_WIDTH", width)
        o = _handle(lanes=lanes, testing=True)
        try:
            o.set_robust(**posterior.ROBUST)
            o.set_graph(g)
            out[name] = o.sample_marginals(5, seed=posterior.SEED, samples=True)
        finally:
            o.close()
    assert out["w16"]["stats"]["solve"]["batch_width"] == 16 and out["w1"]["stats"]["solve"]["batch_width"] == 1
    assert out["w1"]["stats"]["solve"]["batches"] == 5
    e_w = _sample_error(out["w1"]["samples"], out["w16"]["samples"])
    e_l = _sample_error(out["l1"]["samples"], out["l8"]["samples"])
    print("sample error: width 1 against 16 %.3e  lanes 1 against 8 %.3e" % (e_w, e_l))
    assert e_w <= SAMPLE_TOL and e_l <= SAMPLE_TOL, (e_w, e_l)


# ---- 4. statistics ---------------------------------------------------------------------------------------------------------------------
def test_statistics_at_512_samples():
    """c1 at its start, analytic Jacobians, multigrid: the graph, seed and K tests/test_sample_marginals_cpu.py qualifies."""
    g = util.c1_arrays()
    K = posterior.K_STAT
    o = _handle("amg", "analytic")
    try:
        o.set_graph(g)
        r = o.sample_marginals(K, seed=posterior.SEED_STAT, samples=True)
    finally:
        o.close()
    assert r["stats"]["solve"]["batches"] == K // 16 and r["stats"]["solve"]["fallbacks"] == 0
    S = posterior.System(g, None, "analytic")
    m = _mask(g)
    ratio = np.diagonal(r["cov"], axis1=1, axis2=2)[m] / S.inverse_diagonal()[m]
    bound = posterior.BOUND * np.sqrt(2.0 / K)
    print("variance ratio in [%.4f, %.4f], bound 1 +- %.4f" % (ratio.min(), ratio.max(), bound))
    assert np.abs(ratio - 1).max() <= bound
    x = S.packed(r["samples"])
    q, n = float(np.einsum("kn,nm,km->k", x, S.H, x).mean()), S.H.shape[0]
    print("mean delta^T H delta %.3f, n = %d, bound +- %.3f" % (q, n, posterior.BOUND * np.sqrt(2.0 * n / K)))
    assert abs(q - n) <= posterior.BOUND * np.sqrt(2.0 * n / K)      # (a forgotten gauge or prior term shows here)


# ---- 5. state rule -------------------------------------------------------------------------------------------------------------------
def test_no_side_effects_on_the_solver():
    g = util.c1_arrays()
    ids = g.v_id[::11]

    def run(sample):
        o = _handle()
        try:
            o.set_graph(g)
            first = o.optimize(5)
            m0 = v0 = m1 = None
            if sample:
                v0 = o.vertices()
                m0 = o.marginals(ids)[0]
                o.sample_marginals(K_SMALL, seed=posterior.SEED, samples=True)
                m1 = o.marginals(ids)[0]
                assert np.array_equal(o.vertices(), v0)
            r = o.optimize(5)
            return first, r, o.vertices(), m0, m1
        finally:
            o.close()
    (fa, ra, va, _x, _y), (fb, rb, vb, m0, m1) = run(False), run(True)
    assert np.array_equal(m0, m1)
    assert np.array_equal(fa["chi2"], fb["chi2"]) and np.array_equal(fa["cg_iters"], fb["cg_iters"])
    assert ra["stop"] == rb["stop"] and ra["iters"] == rb["iters"]
    assert np.array_equal(ra["cg_iters"], rb["cg_iters"])
    assert np.abs(ra["chi2"] - rb["chi2"]).max() <= 1e-9 * np.abs(ra["chi2"]).max()
    assert util.max_vertex_diff(va, vb, g.v_type) <= 1e-9

    def fresh(sample):      # from a handle that has not solved yet: bit for bit
        o = _handle()
        try:
            o.set_graph(g)
            if sample:
                o.sample_marginals(5, seed=1)
            r = o.optimize(10)
            return o.vertices(), r["chi2"], r["cg_iters"]
        finally:
            o.close()
    for x, y in zip(fresh(False), fresh(True)):
        assert np.array_equal(x, y)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    g = util.c1_arrays()
    V = len(g.v_id)
    o = _handle()
    try:
        with pytest.raises(RuntimeError, match="no graph"):
            o.sample_marginals(4)
        o.set_graph(g)
        for k in (0, -3, 65537):
            with pytest.raises(RuntimeError, match="n_samples"):
                o.sample_marginals(k)
        cov = np.zeros((V, 9)); smp = np.zeros((4, V, 3))
        raw = lambda *a: o.lib.tsgo_sample_marginals(o.h, *a)
        assert raw(4, 0, 0.0, None, V, None, 0, None) < 0 and b"cov_out" in o.lib.tsgo_last_error()
        assert raw(4, 0, 0.0, cov.ctypes.data, V - 1, None, 0, None) < 0 and b"cap_vertices" in o.lib.tsgo_last_error()
        assert raw(4, 0, 0.0, cov.ctypes.data, V, smp.ctypes.data, smp.size - 1, None) < 0 and b"samples_cap" in o.lib.tsgo_last_error()
        assert o.lib.tsgo_sample_marginals(None, 4, 0, 0.0, cov.ctypes.data, V, None, 0, None) < 0 and b"null handle" in o.lib.tsgo_last_error()
        assert not cov.any() and not smp.any()
        assert raw(4, 0, 0.0, cov.ctypes.data, V, smp.ctypes.data, smp.size, None) == 0      # stats may be NULL, exact capacities pass
        assert np.isfinite(cov).all() and cov.any() and smp.any()
        free = GraphArrays(g.v_id, g.v_type, g.v_pos, g.e_type, g.e_ids, g.e_meas, g.e_inf, np.zeros(0, np.uint32))
        o.set_graph(free)
        with pytest.raises(RuntimeError, match="fixed vertex"):
            o.sample_marginals(4)
        o.set_graph(g)
        assert o.optimize(2)["iters"] == 2
        assert o.sample_marginals(1)["stats"]["samples"] == 1
    finally:
        o.close()
    o = _handle(precision=32)
    try:
        o.set_graph(g)
        with pytest.raises(RuntimeError, match="precision"):
            o.sample_marginals(4)
        assert o.optimize(2)["iters"] == 2
    finally:
        o.close()
    shard = HipOptimizer(world=2, rank=0, testing=True)
    try:
        with pytest.raises(RuntimeError, match="world > 1"):
            shard.sample_marginals(4)
    finally:
        shard.close()
