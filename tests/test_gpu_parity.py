"""Parity of the HIP path (through the C ABI) against the CPU oracle.  Needs an MI355X: `-m gpu`.

Tolerances: north_star asks for 1e-6 on final chi^2 (relative) and on pose deltas (absolute); the f64
path is held to much tighter bounds here, written next to each check."""
import numpy as np
import pytest

from oracle import oracle
from tests import edge_cases, util
from toyslam_amd import synth
from toyslam_amd.graph import GraphArrays
from toyslam_amd.optimizer import HipOptimizer, free_local_group, local_group

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["amg", "jacobi"])
def opt(request):
    """Both preconditioners go through every parity check: the multigrid V-cycle (default) and the
    block-Jacobi fallback."""
    o = HipOptimizer(pcg_rel_tol=1e-12, preconditioner=request.param)
    yield o
    o.close()


def test_c1_linearisation_blocks_gradient_chi2(opt):
    g = util.c1_arrays()
    d_ref, err, diag_ref, grad_ref = util.dense_solution(g)
    opt.set_graph(g)
    diag, grad, chi2 = opt.linearize()
    assert abs(chi2 - err) <= 1e-12 * err                      # f64, different summation order only
    np.testing.assert_allclose(grad, grad_ref, rtol=0, atol=1e-10 * np.abs(grad_ref).max())
    np.testing.assert_allclose(diag, diag_ref, rtol=0, atol=1e-10 * np.abs(diag_ref).max())


def test_c1_one_solve_matches_dense_qr_class_solve(opt):
    g = util.c1_arrays()
    d_ref, err, _, _ = util.dense_solution(g)
    opt.set_graph(g)
    r = opt.solve_step()
    assert np.abs(r["delta"] - d_ref).max() <= 1e-9 * np.abs(d_ref).max()
    assert 0 < r["cg_iters"] < 500
    # the probe must not move the vertices
    assert util.max_vertex_diff(opt.vertices(), g.v_pos, g.v_type) < 1e-15


def test_c1_full_run_matches_cpu_eigen_rules(opt):
    """50-iteration cap, reference stop rules: same chi^2 trajectory, same stop, same vertices."""
    g = util.c1_arrays()
    ref = oracle.optimize(util.to_oracle(g), 50, mode="cpp", solver="chol")
    opt.set_graph(g)
    r = opt.optimize(50)
    assert r["stop"] == ref["stop"] == "plateau"
    assert r["iters"] == ref["iters"]
    np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=1e-9)            # north_star: 1e-6
    assert util.max_vertex_diff(opt.vertices(), ref["v_pos"], g.v_type) < 1e-8  # north_star: 1e-6
    assert abs(r["delta_norm"] - ref["delta_norm"]) < 1e-8


@pytest.mark.parametrize("name", ["tiny_a", "tiny_b", "tiny_c"])
def test_tiny_graphs(opt, name):
    g = util.tiny_arrays(name)
    d_ref, err, diag_ref, grad_ref = util.dense_solution(g)
    opt.set_graph(g)
    diag, grad, chi2 = opt.linearize()
    assert abs(chi2 - err) <= 1e-13 * max(1.0, err)
    np.testing.assert_allclose(grad, grad_ref, atol=1e-11 * max(1.0, np.abs(grad_ref).max()))
    np.testing.assert_allclose(diag, diag_ref, atol=1e-9 * np.abs(diag_ref).max())
    r = opt.solve_step()
    assert np.abs(r["delta"] - d_ref).max() <= 1e-9 * max(1.0, np.abs(d_ref).max())
    ref = oracle.optimize(util.to_oracle(g), 20, mode="cpp", solver="qr")
    out = opt.optimize(20)
    assert out["stop"] == ref["stop"] and out["iters"] == ref["iters"]
    np.testing.assert_allclose(out["chi2"], ref["chi2"], rtol=1e-8, atol=1e-12)
    assert util.max_vertex_diff(opt.vertices(), ref["v_pos"], g.v_type) < 1e-8


@pytest.mark.parametrize("lanes", [(1, 1), (2, 1), (4, 2), (8, 8)])
def test_lanes_per_vertex_variants_agree_with_dense(lanes):
    g = synth.make(300, 10, seed=3)
    d_ref, err, _, _ = util.dense_solution(g)
    o = HipOptimizer(pcg_rel_tol=1e-12, lanes_per_pose=lanes[0], lanes_per_lm=lanes[1])
    try:
        o.set_graph(g)
        r = o.solve_step()
        names = "\n".join(e["name"] for e in o.profile_iteration(2))
    finally:
        o.close()
    assert abs(r["chi2"] - err) <= 1e-12 * err
    assert np.abs(r["delta"] - d_ref).max() <= 1e-8 * np.abs(d_ref).max()
    # every arm of the lanes-per-vertex dispatch (8: the arm every other value falls through to) under the name of what it launched
    assert "k_schur_pose<double, %d," % lanes[0] in names and "k_schur_lm<double, %d," % lanes[1] in names, names


@pytest.mark.parametrize("precond", ["amg", "jacobi"])
def test_hipgraph_replay_equals_eager_launches(precond, monkeypatch):
    """tsgo_config.use_graphs: 1 = captured iterations replayed (from the second tsgo_optimize on a structure), 0 = eager, 2 ("auto", the
    default) = eager while the host thread keeps ahead of the device, replay once it has been seen not to (test hook TSGO_FORCE_HOST_SLOW:
    the handle believes its host is slow).  Same bits every way: no atomics anywhere."""
    g = synth.make(2000, 10, seed=5)
    res = []
    for use_graphs, slow in ((True, False), (False, False), ("auto", False), ("auto", True)):
        if slow:
            monkeypatch.setenv("TSGO_FORCE_HOST_SLOW", "1")
        else:
            monkeypatch.delenv("TSGO_FORCE_HOST_SLOW", raising=False)
        o = HipOptimizer(pcg_rel_tol=1e-10, use_graphs=use_graphs, preconditioner=precond, testing=slow)      # the hook lives in the TSGO_TESTING build only
        try:
            o.set_graph(g)
            o.optimize(1)                   # the first call on new tables launches eagerly either way; the graph is captured at the second
            o.set_graph(g)                  # same structure: values refilled, the captured graph (if any) kept
            o.optimize(1)
            o.set_graph(g)
            r = o.optimize(3)
            res.append((r, o.vertices()))
        finally:
            o.close()
    monkeypatch.delenv("TSGO_FORCE_HOST_SLOW", raising=False)
    assert [r["graph_replay"] for r, _ in res] == [True, False, precond == "jacobi", True], [r["graph_replay"] for r, _ in res]      # (block-Jacobi PCG is always replayed under "auto")
    for r, v in res[1:]:
        np.testing.assert_array_equal(res[0][0]["chi2"], r["chi2"])       # bitwise
        np.testing.assert_array_equal(res[0][0]["cg_iters"], r["cg_iters"])
        np.testing.assert_array_equal(res[0][1], v)


@pytest.mark.parametrize("precond", ["amg", "jacobi"])
def test_c2_10k_poses_against_sparse_cpu_twin(precond):
    """BASELINE config 2 (10k poses / 100k LM edges): 5 GN iterations, GPU vs the CPU twin (which runs the
    OTHER preconditioner, so the two solves share nothing but the mathematics)."""
    g = synth.make_config("c2_10k")
    ref = oracle.sparse_optimize(util.to_oracle(g), 5, pcg_tol=1e-12, precond="jacobi" if precond == "amg" else "amg")
    o = HipOptimizer(pcg_rel_tol=1e-12, preconditioner=precond)
    try:
        o.set_graph(g)
        r = o.optimize(5)
        v = o.vertices()
    finally:
        o.close()
    np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=1e-9)             # north_star: 1e-6
    assert util.max_vertex_diff(v, ref["v_pos"], g.v_type) < 1e-7             # north_star: 1e-6
    assert np.all(np.diff(r["chi2"]) < 0)
    if precond == "amg":
        assert r["cg_iters"].max() < 120, r["cg_iters"]                       # block-Jacobi needs ~2 800 here


def test_warm_start_and_lagged_hierarchy_change_the_work_not_the_answer(monkeypatch):
    """PCG warm start (x0 = the extrapolated trend of the previous deltas, order chosen per solve; order 1 = 0.8 * previous
    delta) and the lagged multigrid hierarchy are accelerations: same chi^2 trajectory and vertices as cold starts on a
    hierarchy rebuilt at every linearisation, in fewer PCG iterations."""
    g = synth.make_config("c2_10k", seed=5)
    runs = {}
    for name, warm, max_age in (("default", None, None), ("first_order", 1, None), ("cold_fresh", 0, "1")):
        if max_age is None:
            monkeypatch.delenv("TSGO_HIER_MAX_AGE", raising=False)
        else:
            monkeypatch.setenv("TSGO_HIER_MAX_AGE", max_age)
        o = HipOptimizer(pcg_rel_tol=1e-12, warm_start=warm, testing=max_age is not None)      # TSGO_HIER_MAX_AGE is a research variable: TSGO_TESTING build
        try:
            o.set_graph(g); r = o.optimize(14); runs[name] = (r, o.vertices())
        finally:
            o.close()
    (rb, vb) = runs["cold_fresh"]
    for name in ("default", "first_order"):
        ra, va = runs[name]
        assert ra["iters"] == rb["iters"] == 14 and ra["fallbacks"] == rb["fallbacks"] == 0
        np.testing.assert_allclose(ra["chi2"], rb["chi2"], rtol=1e-9)
        assert util.max_vertex_diff(va, vb, g.v_type) < 1e-8
        assert ra["cg_iters"][0] == rb["cg_iters"][0]                     # the first solve has nothing to start from
        assert ra["cg_iters"][1:].sum() < rb["cg_iters"][1:].sum() + 3 * 13   # lag costs a few iterations, warm start saves more or about as many
    assert runs["default"][0]["cg_iters"][1] == runs["first_order"][0]["cg_iters"][1]      # one delta of history: order 1 either way
    assert runs["default"][0]["cg_iters"].sum() <= runs["first_order"][0]["cg_iters"].sum()   # higher orders are taken only where they predict better
    print("PCG iterations per solve: cold %s, order 1 %s, adaptive order %s" % tuple(list(runs[k][0]["cg_iters"]) for k in ("cold_fresh", "first_order", "default")))


@pytest.mark.parametrize("precond", ["amg", "jacobi"])
def test_collective_path_over_rccl_with_a_single_rank_communicator(precond):
    """The edge-sharded path (eager launches, ncclAllReduce of the pose partials per GN iteration, of every Schur product —
    three per multigrid-preconditioned PCG iteration, one with block-Jacobi — and of the level-0 blocks per hierarchy
    build) on the one GPU this box has: a world-size-1 RCCL communicator makes the engine take it.  Same answer as the
    dense reference path; the multi-shard arithmetic is covered on CPU by tests/test_sharded_gloo.py."""
    g = util.c1_arrays()
    ref = oracle.optimize(util.to_oracle(g), 6, mode="cpp", solver="chol")
    o = HipOptimizer(pcg_rel_tol=1e-12, rank=0, world=1, preconditioner=precond)
    try:
        o.comm_init(o.comm_unique_id())
        o.set_graph(g); r = o.optimize(6); v = o.vertices()
    finally:
        o.close()
    np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=1e-10)
    assert util.max_vertex_diff(v, ref["v_pos"], g.v_type) < 1e-9
    assert abs(r["delta_norm"] - ref["delta_norm"]) < 1e-8
    if precond == "jacobi":
        assert r["cg_iters"].min() > 30        # block-Jacobi counts
    else:
        assert r["cg_iters"].max() < 30 and r["fallbacks"] == 0, r["cg_iters"]      # the multigrid cycle ran through the collectives


def test_collective_path_at_config_2_size_keeps_multigrid_iteration_counts():
    """BASELINE config 2 (10k poses) through the collective path with a one-rank communicator: the same chi^2 trajectory
    and vertices as the hipGraph single-GPU path, multigrid iteration counts (block-Jacobi needs ~2 800 here)."""
    g = synth.make_config("c2_10k")
    runs = {}
    for name in ("graph", "collective"):
        o = HipOptimizer(pcg_rel_tol=1e-12, rank=0, world=1)
        try:
            if name == "collective":
                o.comm_init(o.comm_unique_id())
            o.set_graph(g); r = o.optimize(6); runs[name] = (r, o.vertices())
        finally:
            o.close()
    (ra, va), (rb, vb) = runs["graph"], runs["collective"]
    np.testing.assert_array_equal(ra["chi2"], rb["chi2"])              # same kernels, same order: same bits
    np.testing.assert_array_equal(ra["cg_iters"], rb["cg_iters"])
    np.testing.assert_array_equal(va, vb)
    assert rb["cg_iters"].max() < 60 and rb["fallbacks"] == 0, rb["cg_iters"]
    ref = oracle.sparse_optimize(util.to_oracle(g), 6, pcg_tol=1e-12, precond="jacobi")
    np.testing.assert_allclose(rb["chi2"], ref["chi2"], rtol=1e-9)
    assert util.max_vertex_diff(vb, ref["v_pos"], g.v_type) < 1e-7


@pytest.mark.parametrize("world", [1, 2])
def test_solver_history_survives_set_graph_when_asked_to(world):
    """SURVEY 8f rank 2, "warm-starting PCG across requests" (tsgo_config.warm_requests; the reference re-creates everything per
    message, remote/app/ConnectionHandler.h:18-21).  A front-end sends back the estimates it was returned: (a) the same structure —
    the deltas of the last Gauss-Newton iterations stay in place; (b) the graph grown by 400 poses and what they see — carried
    over by vertex id into the new pose numbering, new poses start from zero; (c) a request that does NOT continue the last one
    (the same graph with estimates that are already converged: the history predicts steps that are not there): the first warm
    start leaves a larger residual than a cold one and the history is dropped.  Every time: the
    same chi^2 trajectory and vertices as a fresh handle to the PCG tolerance, in fewer PCG iterations where the history fits.
    world = 2: two shards through the in-process group take every one of those decisions alike."""
    import threading
    big = synth.make(4400, 10, loop_closures=0, seed=21)
    small = util.first_poses(big, 4000)
    assert small.n_poses == 4000 and 0 < small.n_landmarks < big.n_landmarks and len(small.e_type) < len(big.e_type)

    def returned(g, v):      # what comes back over the wire: f32
        return GraphArrays(g.v_id, g.v_type, v.astype(np.float32).astype(np.float64), g.e_type, g.e_ids, g.e_meas, g.e_inf, g.fixed)

    def run(warm, requests, iterations=6, world=world):
        """`requests`: functions (previous (graph, vertices) or None) -> graph, sent one after the other to ONE handle per rank;
        returns [(result of rank 0, vertices merged over the ranks, graph, results of all ranks)] per request"""
        group = local_group(world) if world > 1 else None
        hs = [HipOptimizer(pcg_rel_tol=1e-12, rank=k, world=world, warm_requests=warm, testing=world > 1) for k in range(world)]
        res = []; prev = None
        try:
            if world > 1:
                for o in hs:
                    o.comm_init_local(group)
            for make in requests:
                g = make(prev)
                outs = [None] * world; errs = []

                def rank_main(rank, g=g, outs=outs, errs=errs):
                    try:
                        hs[rank].set_graph(g); r = hs[rank].optimize(iterations); outs[rank] = (r, hs[rank].vertices())
                    except Exception as e:      # noqa: BLE001
                        errs.append((rank, repr(e)))

                th = [threading.Thread(target=rank_main, args=(k,), daemon=True) for k in range(world)]
                for t in th:
                    t.start()
                for t in th:
                    t.join(timeout=300)
                assert not errs, errs
                assert not any(t.is_alive() for t in th), "a rank is stuck in the in-process all-reduce (the ranks decided differently?)"
                v = outs[0][1].copy()            # poses are replicated; a landmark comes from the shard that owns (and moved) it
                for _, vr in outs[1:]:
                    m = np.any(vr != g.v_pos, axis=1) & (g.v_type == 1)
                    v[m] = vr[m]
                res.append((outs[0][0], v, g, [o[0] for o in outs])); prev = (g, v)
        finally:
            for o in hs:
                o.close()
            if world > 1:
                free_local_group(group)
        return res

    def grown_from(prev):
        g, v = prev
        at = {int(i): k for k, i in enumerate(g.v_id)}
        vp = big.v_pos.copy()
        for k, i in enumerate(big.v_id):
            j = at.get(int(i))
            if j is not None:
                vp[k] = np.float32(v[j]).astype(np.float64)
        return GraphArrays(big.v_id, big.v_type, vp, big.e_type, big.e_ids, big.e_meas, big.e_inf, big.fixed)

    requests = [lambda prev: small,
                lambda prev: returned(*prev),            # (a) same structure, the estimates that came back
                grown_from,                              # (b) grown, old vertices as returned
                lambda prev: settled]                    # (c) same structure as (b), estimates that have converged elsewhere: not a continuation
    vs = run(False, [lambda prev: big], iterations=40, world=1)[0][1]
    settled = GraphArrays(big.v_id, big.v_type, vs, big.e_type, big.e_ids, big.e_meas, big.e_inf, big.fixed)
    warm = run(True, requests)
    for r, _, _, ranks in warm:
        for rr in ranks[1:]:
            np.testing.assert_array_equal(rr["chi2"], r["chi2"]); np.testing.assert_array_equal(rr["cg_iters"], r["cg_iters"])
            assert rr["history_carried"] == r["history_carried"]
    assert [r["history_carried"] for r, _, _, _ in warm] == [0, 1, 1, 2], [r["history_carried"] for r, _, _, _ in warm]
    assert warm[1][0]["structure_reused"] and not warm[2][0]["structure_reused"] and warm[3][0]["structure_reused"]
    # a fresh single handle per request, on exactly the graphs the warm handles were given
    for k, (r, v, g, _) in enumerate(warm):
        rc, vc, _, _ = run(False, [lambda prev, g=g: g], world=1)[0]
        assert rc["history_carried"] == 0
        np.testing.assert_allclose(r["chi2"], rc["chi2"], rtol=1e-9)
        assert util.max_vertex_diff(v, vc, g.v_type) < 1e-8
        print("request %d (%d poses, %d shard(s)): PCG iterations per solve with the history %s, from nothing %s" % (k, g.n_poses, world, list(r["cg_iters"]), list(rc["cg_iters"])))
        if k == 1:
            assert r["cg_iters"][0] < rc["cg_iters"][0] and r["cg_iters"].sum() < rc["cg_iters"].sum()
        if k == 2:
            assert r["cg_iters"].sum() <= rc["cg_iters"].sum() + 3
        if k in (0, 3):
            assert abs(int(r["cg_iters"].sum()) - int(rc["cg_iters"].sum())) <= 3 + 3 * (world - 1)      # nothing carried / dropped at the first solve


@pytest.mark.parametrize("precond,precision", [("amg", 64), ("jacobi", 64), ("amg", 32)])
def test_same_structure_again_only_refills_values_and_equals_a_fresh_engine(precond, precision):
    """tsgo_set_graph with the structure the handle already holds (same ids, types, edges, fixed list) keeps
    layout, multigrid patterns, tables and the captured hipGraph, and refills estimates, measurements and weights — and
    gives, bit for bit, what a fresh engine gives for that graph.  A different structure rebuilds everything."""
    g = synth.make(3000, 10, loop_closures=20, seed=9)
    rng = np.random.default_rng(1)
    g2 = g.copy()
    g2.v_pos[:, :2] += rng.normal(0, 0.05, size=(len(g.v_id), 2))
    g2.v_pos[g.v_type == 0, 2] += rng.normal(0, 0.01, size=int((g.v_type == 0).sum()))
    lm = g.e_type == 1
    g2.e_meas[lm, 0] *= 1.01; g2.e_meas[lm, 1] += 0.002
    g2.e_inf[:] = g.e_inf * 0.75
    tol = 1e-10 if precision == 64 else 1e-5
    fresh = HipOptimizer(pcg_rel_tol=tol, preconditioner=precond, precision=precision, reuse_structure=False)
    try:
        fresh.set_graph(g2); rf = fresh.optimize(5); vf = fresh.vertices()
        assert not rf["structure_reused"]
        fresh.set_graph(g2); rf2 = fresh.optimize(5)               # reuse switched off: rebuilt, same answer
        assert not rf2["structure_reused"]
        np.testing.assert_array_equal(rf["chi2"], rf2["chi2"])
    finally:
        fresh.close()
    o = HipOptimizer(pcg_rel_tol=tol, preconditioner=precond, precision=precision)
    try:
        o.set_graph(g); r0 = o.optimize(3)
        assert not r0["structure_reused"]
        o.set_graph(g2); r = o.optimize(5); v = o.vertices()
        assert r["structure_reused"]          # what it saves is measured at 100k poses; 3 000 poses rebuild in 3 ms either way
        np.testing.assert_array_equal(r["chi2"], rf["chi2"])         # no atomics, same tables, same patterns: same bits
        np.testing.assert_array_equal(r["cg_iters"], rf["cg_iters"])
        np.testing.assert_array_equal(v, vf)
        grown = synth.make(3150, 10, loop_closures=20, seed=9)     # a new structure: rebuilt, and correct
        o.set_graph(grown); r3 = o.optimize(3); v3 = o.vertices()
        assert not r3["structure_reused"]
        if precision == 64:
            ref = oracle.sparse_optimize(util.to_oracle(grown), 3, pcg_tol=1e-12, precond="jacobi" if precond == "amg" else "amg")
            np.testing.assert_allclose(r3["chi2"], ref["chi2"], rtol=1e-8)
            assert util.max_vertex_diff(v3, ref["v_pos"], grown.v_type) < 1e-6
        # a singular ODOM measurement arriving in a refill: reported, and the handle holds no graph afterwards
        o.set_graph(grown)
        bad_grown = grown.copy(); bad_grown.e_meas[np.where(grown.e_type == 0)[0][0]] = 0
        with pytest.raises(RuntimeError, match="singular"):
            o.set_graph(bad_grown)
        o.set_graph(g2); r4 = o.optimize(5)                         # the handle recovers with a full rebuild
        assert not r4["structure_reused"]
        np.testing.assert_array_equal(r4["chi2"], rf["chi2"])
    finally:
        o.close()


def test_one_handle_through_graphs_of_very_different_sizes_equals_fresh_handles():
    """A handle keeps its device slabs, staging buffer and host arrays from request to request (tsgo_hip.hip: Engine::dalloc,
    release): small after large, large after small, the reference's 150-pose case in between — every answer must be, bit
    for bit, what a fresh handle gives (nothing of a previous graph may leak into the next: stale table tails, solver
    history, hierarchy levels that the new graph does not have)."""
    graphs = [synth.make(600, 8, loop_closures=5, seed=1), synth.make(6000, 12, loop_closures=30, seed=2), util.c1_arrays(),
              synth.make(2500, 4, loop_closures=0, seed=3), synth.make(6000, 12, loop_closures=30, seed=2), synth.make(40, 3, seed=4)]
    kept = HipOptimizer(pcg_rel_tol=1e-10)
    try:
        for k, g in enumerate(graphs):
            kept.set_graph(g); r = kept.optimize(4); v = kept.vertices()
            assert not r["structure_reused"]
            fresh = HipOptimizer(pcg_rel_tol=1e-10)
            try:
                fresh.set_graph(g); rf = fresh.optimize(4); vf = fresh.vertices()
            finally:
                fresh.close()
            np.testing.assert_array_equal(r["chi2"], rf["chi2"], err_msg="graph %d" % k)
            np.testing.assert_array_equal(r["cg_iters"], rf["cg_iters"], err_msg="graph %d" % k)
            np.testing.assert_array_equal(v, vf, err_msg="graph %d" % k)
    finally:
        kept.close()


@pytest.mark.parametrize("precond", ["amg", "jacobi"])
def test_python_rules_reproduce_the_reference_python_optimizer_on_the_device(precond):
    """SURVEY 8f rank 4 (the `lambdaVal` the C++ declares and never uses, OptimizerCpu.h:70): rules="python" runs the loop of the
    reference's in-process optimizer, python/optimizer/graph_optimizer.py:20-92 — H + lambda I with its lambda schedule, step lr, b
    zeroed at fixed vertices, stop on ||lr dx|| — on the device.  Pinned by what the reference itself produced: the 10-iteration
    chi^2 trajectory and final vertices of GraphOptimizer.optimize(10, lr=.2) on config 1 (tests/golden/c1_pyopt.npz)."""
    z = util.load("c1_pyopt.npz")
    g = util.c1_arrays()
    o = HipOptimizer(pcg_rel_tol=1e-12, preconditioner=precond, rules="python", lr=0.2)
    try:
        o.set_graph(g); r = o.optimize(10); v = o.vertices()
        np.testing.assert_allclose(r["chi2"], z["chi2"], rtol=1e-9)
        assert util.max_vertex_diff(v, z["v_pos"], g.v_type) < 1e-8
        assert abs(r["lambda_last"] - 1e-3 / 1.1 ** 10) < 1e-12          # chi^2 fell every time: lambda / 1.1 per iteration
        # lr = 1, tiny graphs, a graph whose chi^2 rises (lambda goes up): against the dense restatement of the same loop
        for gg, lr, n in ((g, 1.0, 6), (util.tiny_arrays("tiny_b"), 0.2, 12), (edge_cases.pose_graph_without_landmarks(), 0.2, 8)):
            ref = oracle.optimize(util.to_oracle(gg), n, mode="python", solver="chol", lr=lr)
            o2 = HipOptimizer(pcg_rel_tol=1e-12, preconditioner=precond, rules="python", lr=lr)
            try:
                o2.set_graph(gg); r2 = o2.optimize(n); v2 = o2.vertices()
            finally:
                o2.close()
            assert (r2["iters"], r2["stop"]) == (ref["iters"], ref["stop"])
            np.testing.assert_allclose(r2["chi2"], ref["chi2"], rtol=1e-8)
            scale = max(1.0, np.abs(ref["v_pos"]).max())
            assert util.max_vertex_diff(v2, ref["v_pos"], gg.v_type) < 1e-7 * scale
    finally:
        o.close()


def test_python_rules_at_config_2_against_the_twin():
    g = synth.make_config("c2_10k")
    ref = oracle.sparse_optimize(util.to_oracle(g), 6, pcg_tol=1e-12, precond="jacobi", rules="python", lr=0.5)
    o = HipOptimizer(pcg_rel_tol=1e-12, rules="python", lr=0.5)
    try:
        o.set_graph(g); r = o.optimize(6); v = o.vertices()
    finally:
        o.close()
    np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=1e-9)
    assert util.max_vertex_diff(v, ref["v_pos"], g.v_type) < 1e-7
    assert r["chi2"][-1] < 0.1 * r["chi2"][0]          # lr 0.5 converges much faster than the 0.2 of the C++ loop


def test_bench_tolerance_meets_the_north_star_bar():
    """bench.py runs PCG at rel tol 1e-10 (1e-8 leaves 1.5e-6 on config-2 poses): final chi^2 (relative) and poses (absolute) stay within 1e-6 of
    the dense cpu/eigen restatement on config 1 and of the tightly converged twin on config 2."""
    g = util.c1_arrays()
    ref = oracle.optimize(util.to_oracle(g), 50, mode="cpp", solver="chol")
    o = HipOptimizer(pcg_rel_tol=1e-10)
    try:
        o.set_graph(g)
        r = o.optimize(50)
        assert r["iters"] == ref["iters"] and r["stop"] == ref["stop"]
        assert abs(r["chi2"][-1] - ref["chi2"][-1]) <= 1e-6 * ref["chi2"][-1]
        assert util.max_vertex_diff(o.vertices(), ref["v_pos"], g.v_type) < 1e-6
        g2 = synth.make_config("c2_10k")
        ref2 = oracle.sparse_optimize(util.to_oracle(g2), 10, pcg_tol=1e-12, precond="amg")
        o.set_graph(g2)
        r2 = o.optimize(10)
        assert abs(r2["chi2"][-1] - ref2["chi2"][-1]) <= 1e-6 * ref2["chi2"][-1]
        assert util.max_vertex_diff(o.vertices(), ref2["v_pos"], g2.v_type) < 1e-6
    finally:
        o.close()


def test_f32_mode_tracks_f64_loosely():
    g = util.c1_arrays()
    o = HipOptimizer(precision=32, pcg_rel_tol=1e-5)
    try:
        o.set_graph(g)
        _, _, chi2 = o.linearize()
        r = o.optimize(10)
    finally:
        o.close()
    ref = oracle.optimize(util.to_oracle(g), 10, mode="cpp", solver="chol")
    assert abs(chi2 - ref["chi2"][0]) < 1e-5 * ref["chi2"][0]
    np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=2e-3)            # f32 is NOT the parity mode


def test_f32_mode_against_the_reference_servers_own_arithmetic():
    """precision = 32 is the scalar type the reference server is compiled for (remote/app/main.cpp:40: OptimizerCpu<float>).  The
    dense restatement in float (oracle_optimize_f32) IS that arithmetic; the f64 restatement is what both approximate.  Config 1,
    10 iterations.  Stated bounds (measured: 1.1e-6 / 4.5e-6 / 2.2e-5): every chi^2 of the device's f32 run within 1e-4 of the f64
    restatement and within 1e-4 of the float restatement with a Cholesky solve; vertices within 1e-3 of f64.
    With the solver the reference really calls — colPivHouseholderQr (SolverEigen.h:20) — float arithmetic does NOT follow the
    f64 path at all: Eigen's rank rule drops pivots below eps * n * |max pivot| = 1.2e-7 * 1134 * 1e6 (the gauge term), i.e.
    nearly every unknown, and chi^2 creeps from 114586 to 95946 in 10 iterations instead of 12834.  That is the reference's own
    float behaviour as restated; the device's f32 mode is held to the f64 answer instead, and is NOT compared with it."""
    g = util.c1_arrays()
    o = HipOptimizer(precision=32, pcg_rel_tol=1e-5)
    try:
        o.set_graph(g); r = o.optimize(10); v = o.vertices()
    finally:
        o.close()
    ref64 = oracle.optimize(util.to_oracle(g), 10, mode="cpp", solver="chol")
    ref32 = oracle.optimize(util.to_oracle(g), 10, mode="cpp", solver="chol", precision="f32")
    qr32 = oracle.optimize(util.to_oracle(g), 10, mode="cpp", solver="qr", precision="f32")
    assert r["iters"] == ref32["iters"] == 10
    err_dev = np.abs(r["chi2"] / ref64["chi2"] - 1).max(); err_ref = np.abs(ref32["chi2"] / ref64["chi2"] - 1).max()
    print("f32 at config 1: device vs f64 %.2e, dense float restatement (Cholesky) vs f64 %.2e, device vs float restatement %.2e; vertices vs f64 %.2e; float + pivoted QR ends at chi2 %.0f"
          % (err_dev, err_ref, np.abs(r["chi2"] / ref32["chi2"] - 1).max(), util.max_vertex_diff(v, ref64["v_pos"], g.v_type), qr32["chi2"][-1]))
    np.testing.assert_allclose(r["chi2"], ref64["chi2"], rtol=1e-4)
    np.testing.assert_allclose(r["chi2"], ref32["chi2"], rtol=1e-4)
    assert util.max_vertex_diff(v, ref64["v_pos"], g.v_type) < 1e-3
    assert qr32["chi2"][-1] > 5 * ref64["chi2"][-1]          # documents the rank-rule effect described above


@pytest.mark.parametrize("workload,chi_tol,pose_tol", [("c2_10k", 1e-5, 5e-2), ("c3_100k", 1e-5, 0.25)])
def test_f32_mode_of_record_at_configs_2_and_3(workload, chi_tol, pose_tol):
    """The f32 device mode (PCG tolerance 1e-5, what bench.py --precision 32 runs) against the f64 CPU twin after 10 GN
    iterations at 10k and 100k poses.  Stated bound: chi^2 within 1e-5 relative at every iteration, vertices within 5e-2 m at 10k
    poses and 0.25 m at 100k (measured: 1.6e-7 / 8e-3 and 4.2e-7 / 5e-2; f32 carries 7 digits, coordinates reach 10^2..10^3 m, ten 0.2-damped steps accumulate)."""
    g = synth.make_config(workload)
    ref = oracle.sparse_optimize(util.to_oracle(g), 10, pcg_tol=1e-10, precond="amg")
    o = HipOptimizer(precision=32, pcg_rel_tol=1e-5)
    try:
        o.set_graph(g); r = o.optimize(10); v = o.vertices()
    finally:
        o.close()
    assert (r["iters"], r["stop"]) == (ref["iters"], ref["stop"]) and r["fallbacks"] == 0
    rel = np.abs(r["chi2"] / ref["chi2"] - 1).max(); dv = util.max_vertex_diff(v, ref["v_pos"], g.v_type)
    print("f32 mode at %s: chi2 within %.2e of the f64 twin over 10 iterations, vertices within %.2e, PCG iterations %s" % (workload, rel, dv, list(r["cg_iters"])))
    assert rel < chi_tol
    assert dv < pose_tol


def test_cycle_storage_16_and_32_give_the_same_answer():
    """tsgo_config.cycle_storage: the V-cycle's copies of the hierarchy as packed half floats (default) against f32.  It only
    preconditions: same chi^2 and vertices to solver tolerance, at most two more PCG iterations per solve."""
    g = synth.make(8000, 10, loop_closures=50, seed=23)
    g.fixed = np.array([0, int(g.v_id[-3])], np.uint32)          # a 1e6 gauge block next to ordinary ones: the per-block exponent's case
    res = {}
    for bits in (32, 16):
        o = HipOptimizer(pcg_rel_tol=1e-12, cycle_storage=bits)
        try:
            o.set_graph(g); res[bits] = (o.optimize(6), o.vertices())
        finally:
            o.close()
    (r32, v32), (r16, v16) = res[32], res[16]
    np.testing.assert_allclose(r16["chi2"], r32["chi2"], rtol=1e-10)
    assert util.max_vertex_diff(v16, v32, g.v_type) < 1e-9
    assert r16["fallbacks"] == 0 and np.all(r16["cg_iters"] <= r32["cg_iters"] + 2), (r16["cg_iters"], r32["cg_iters"])
    print("PCG iterations per solve, cycle storage f32 %s, packed half %s" % (list(r32["cg_iters"]), list(r16["cg_iters"])))


def _odometry_chain(n_poses):
    """The poses and ODOM edges of a synthetic graph, first pose fixed: under the analytic ODOM Jacobians a beam of n_poses links."""
    g = synth.make(n_poses, 13, loop_closures=2, seed=7)
    keep = g.e_type == 0; pose = g.v_type == 0
    return GraphArrays(g.v_id[pose], g.v_type[pose], g.v_pos[pose], g.e_type[keep], g.e_ids[keep], g.e_meas[keep], g.e_inf[keep], np.array([0], np.uint32))


def test_ill_conditioned_chain_leaves_the_packed_cycle_format_by_itself():
    """An odometry-only chain under the analytic ODOM Jacobians is a 12 000-link beam: thousands of multigrid PCG iterations per
    solve, and coarse operators that are differences of large entries — rounded to the packed format's 11 bits they are no
    longer positive definite (with `cycle_storage = 16` forced and no way out: breakdown, 20 000 block-Jacobi iterations,
    TSGO_STOP_SOLVER; tools/research/hard_chain.py).  The engine recognises such a structure by its first solve (> 64 iterations)
    and moves its cycle to f32 copies: same run as a handle created with cycle_storage = 32."""
    g = _odometry_chain(12000)
    res = {}
    for bits in (32, 16):
        o = HipOptimizer(pcg_rel_tol=1e-10, odom_jacobian="analytic", cycle_storage=bits)
        try:
            o.set_graph(g); res[bits] = (o.optimize(4), o.vertices())
        finally:
            o.close()
    (r32, v32), (r16, v16) = res[32], res[16]
    print("beam-like chain: f32 cycle %s, default (packed, then f32) %s" % (list(r32["cg_iters"]), list(r16["cg_iters"])))
    assert r32["stop"] == r16["stop"] == "cap" and r32["fallbacks"] == r16["fallbacks"] == 0
    assert r32["cycle_storage_now"] == 32 and r16["cycle_storage_now"] == 32          # the default handle has switched
    np.testing.assert_allclose(r16["chi2"], r32["chi2"], rtol=1e-6)
    assert util.max_vertex_diff(v16, v32, g.v_type) < 1e-3 * max(1.0, float(np.abs(v32).max()) / 100.0)      # the conditioning of a 12k-link beam


def test_a_handle_that_left_the_packed_format_starts_packed_again():
    """What a hard graph drove the cycle to is forgotten at the next tsgo_set_graph, refill or new structure: the handle starts from the
    configured (packed) storage again and does, bit for bit, what a fresh one does.  The chain keeps its 12 000 links (0.07 s per solve;
    chains of 1 000 to 6 000 links leave the packed format too, but their packed and f32 counts lie within a few per cent of each other):
    its first solve took 1 078 PCG iterations on the packed copies, > 64, converged, and left the cycle in f32 copies without a fallback;
    a handle created with cycle_storage = 32 takes 952, which is what a refilled handle that had stayed in f32 would take."""
    chain, small = _odometry_chain(12000), synth.make(600, 8, loop_closures=5, seed=1)
    cfg = dict(pcg_rel_tol=1e-10, odom_jacobian="analytic")
    o, fresh = HipOptimizer(**cfg), HipOptimizer(**cfg)
    try:
        o.set_graph(chain); r1 = o.optimize(1)
        print("chain of %d links: first solve %s PCG iterations, cycle storage now %d" % (chain.v_id.size, list(r1["cg_iters"]), r1["cycle_storage_now"]))
        assert r1["cycle_storage_now"] == 32 and r1["fallbacks"] == 0      # the condition of this test: the chain left the packed format
        o.set_graph(chain); r2 = o.optimize(1)
        assert r2["structure_reused"]
        np.testing.assert_array_equal(r2["chi2"], r1["chi2"])
        np.testing.assert_array_equal(r2["cg_iters"], r1["cg_iters"])      # packed again, and left at the same solve (a handle still in f32 takes fewer)
        assert r2["cycle_storage_now"] == 32
        o.set_graph(small); r3 = o.optimize(3); v3 = o.vertices()
        fresh.set_graph(small); rf = fresh.optimize(3); vf = fresh.vertices()
        assert not r3["structure_reused"] and r3["cycle_storage_now"] == 16
        np.testing.assert_array_equal(r3["chi2"], rf["chi2"])
        np.testing.assert_array_equal(r3["cg_iters"], rf["cg_iters"])
        np.testing.assert_array_equal(v3, vf)
    finally:
        o.close(); fresh.close()


@pytest.mark.parametrize("n_poses,lc", [(3000, 20), (30000, 300)])
def test_pair_lists_built_on_the_device_equal_the_hosts(monkeypatch, n_poses, lc):
    """The hierarchy's pair-list products (T = A P, A' = P^T T on every level) are built on the device (tsgo_sym_kernels.h) with the
    same columns in the same order and the same pairs in the same order as the host builder's (TSGO_HOST_PRODUCTS=1): every number
    computed from them is then the same bit for bit — chi^2, PCG iteration counts, vertices."""
    g = synth.make(n_poses, 10, loop_closures=lc, seed=41)
    res = {}
    for host in (True, False):
        if host:
            monkeypatch.setenv("TSGO_HOST_PRODUCTS", "1")
        else:
            monkeypatch.delenv("TSGO_HOST_PRODUCTS", raising=False)
        o = HipOptimizer(pcg_rel_tol=1e-12, testing=host)      # the host builder is forced in the TSGO_TESTING build; the device builder runs in the PRODUCT library
        try:
            o.set_graph(g); res[host] = (o.optimize(5), o.vertices())
        finally:
            o.close()
    (rh, vh), (rd, vd) = res[True], res[False]
    np.testing.assert_array_equal(rd["chi2"], rh["chi2"])
    np.testing.assert_array_equal(rd["cg_iters"], rh["cg_iters"])
    np.testing.assert_array_equal(vd, vh)


def crowded_place(n_poses=640, window=64, stride=5, seed=47):
    """A crowded place: poses one unit apart along a line, joined by odometry; landmark j is observed by the `window` poses
    [stride * j, stride * j + window), so every landmark has exactly `window` observers and an interior pose 2 * (window - 1) co-observers.
    Noise, information and f32 rounding as toyslam_amd/csrc/host/synth.cpp makes them; estimates = truth + a small drift; pose 0 fixed."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)  # noqa: E731
    P = n_poses
    L = (P - window) // stride + 1
    sig_xy, sig_th, sig_lidar = 0.25, (7.1 * np.pi / 180.0) ** 2, 0.15 * 0.15
    truth = np.zeros((P + L, 3))
    truth[:P, 0] = np.arange(P)
    truth[:P, 1] = 0.5 * np.sin(0.05 * np.arange(P))
    truth[:P, 2] = 0.05 * np.cos(0.05 * np.arange(P))
    truth[P:, 0] = stride * np.arange(L) + 0.5 * window
    truth[P:, 1] = 3.0 + (np.arange(L) % 3)
    v_pos = truth.copy()
    v_pos[1:P] += 0.05 * rng.standard_normal((P - 1, 3)) * [1.0, 1.0, 0.1]
    v_pos[P:, :2] += 0.05 * rng.standard_normal((L, 2))
    e_type, e_ids, e_meas, e_inf = [], [], [], []
    for a in range(P - 1):
        ca, sa = np.cos(truth[a, 2]), np.sin(truth[a, 2])
        d = truth[a + 1] - truth[a]
        mx, my = ca * d[0] + sa * d[1] + sig_xy * rng.standard_normal(), -sa * d[0] + ca * d[1] + sig_xy * rng.standard_normal()
        mt = d[2] + sig_th * rng.standard_normal()
        e_type.append(0); e_ids.append([a, a + 1])
        e_meas.append([np.cos(mt), -np.sin(mt), mx, np.sin(mt), np.cos(mt), my, 0, 0, 1]); e_inf.append([1 / sig_xy, 1 / sig_xy, 1 / sig_th])
    for j in range(L):
        for i in range(stride * j, stride * j + window):
            c, s = np.cos(truth[i, 2]), np.sin(truth[i, 2])
            d = truth[P + j, :2] - truth[i, :2]
            mx, my = c * d[0] + s * d[1] + sig_lidar * rng.standard_normal(), -s * d[0] + c * d[1] + sig_lidar * rng.standard_normal()
            e_type.append(1); e_ids.append([i, P + j])
            e_meas.append([np.hypot(mx, my), np.arctan2(my, mx), 0, 0, 0, 0, 0, 0, 0]); e_inf.append([1 / sig_lidar, 1 / sig_lidar, 0.0])
    v_type = np.r_[np.zeros(P, np.uint32), np.ones(L, np.uint32)]
    return GraphArrays(np.arange(P + L, dtype=np.uint32), v_type, f32(v_pos), np.array(e_type, np.uint32), np.array(e_ids, np.uint32), f32(e_meas), f32(e_inf),
                       np.array([0], np.uint32))


def test_pair_lists_of_a_crowded_place_equal_the_hosts(monkeypatch):
    """test_pair_lists_built_on_the_device_equal_the_hosts on a graph whose rows are long: 640 poses along a line, every landmark observed
    by exactly 64 poses (the most that still couple, host/amg.h: kMaxPairDegree), every interior pose with 126 co-observers — level-0 rows of
    127 blocks and observer lists that fill a wavefront, where the synthetic graphs have a few dozen blocks and about five observers.
    The window of 64 observers at stride 5 coarsens to the limits the engine requires as it is: nothing had to be shrunk."""
    import ctypes as C
    from toyslam_amd import _lib
    g = crowded_place()
    lib = _lib.host_lib()
    info = _lib.tsgo_amg_info()
    cg = g.c_struct()
    _lib.check(lib, lib.tsgo_amg_probe(C.byref(cg), C.byref(info)), "tsgo_amg_probe")
    assert info.rows[0] == 640 and info.blocks[0] > 64 * info.rows[0], (info.rows[0], info.blocks[0])
    res = {}
    for host in (True, False):
        if host:
            monkeypatch.setenv("TSGO_HOST_PRODUCTS", "1")
        else:
            monkeypatch.delenv("TSGO_HOST_PRODUCTS", raising=False)
        o = HipOptimizer(pcg_rel_tol=1e-12, testing=host)      # the host builder is forced in the TSGO_TESTING build; the device builder runs in the PRODUCT library
        try:
            o.set_graph(g); res[host] = (o.optimize(5), o.vertices())
        finally:
            o.close()
    (rh, vh), (rd, vd) = res[True], res[False]
    np.testing.assert_array_equal(rd["chi2"], rh["chi2"])
    np.testing.assert_array_equal(rd["cg_iters"], rh["cg_iters"])
    np.testing.assert_array_equal(vd, vh)
    # one Gauss-Newton step against the CPU twin, at the tolerances of test_c2_10k_poses_against_sparse_cpu_twin (chi^2 1e-9 relative, 1e-7 on the vertices' change)
    o = HipOptimizer(pcg_rel_tol=1e-12)
    try:
        o.set_graph(g); step = o.solve_step()
    finally:
        o.close()
    ref = oracle.sparse_step(util.to_oracle(g), 1e-12, precond="amg")
    print("crowded place: blocks[0] = %d, PCG iterations %s, one step: chi^2 off by %.3g (relative), delta off by %.3g of %.3g" % (
        info.blocks[0], list(rd["cg_iters"]), abs(step["chi2"] - ref["chi2"]) / ref["chi2"], np.abs(step["delta"] - ref["delta"]).max(), np.abs(ref["delta"]).max()))
    np.testing.assert_allclose(step["chi2"], ref["chi2"], rtol=1e-9)
    assert np.abs(step["delta"] - ref["delta"]).max() < 1e-7


@pytest.mark.parametrize("bits", [1, 2, 4, 7])
def test_device_pattern_builders_hand_back_to_the_host(monkeypatch, bits):
    """A row with more distinct columns than the device builders' LDS tables hold (1 024) makes them decline: level 0, or a level's
    two products, is then built by the host after all.  TSGO_SYM_DECLINE makes them decline on an ordinary graph (bit 1: level 0,
    2: every T = A P, 4: A' = R T on the odd levels): whichever mix of builders, the same lists, the same bits."""
    g = synth.make(6000, 10, loop_closures=60, seed=43)
    res = []
    for decline in (0, bits):
        monkeypatch.setenv("TSGO_SYM_DECLINE", str(decline))
        o = HipOptimizer(pcg_rel_tol=1e-12, testing=decline != 0)      # (the product library does not know the variable)
        try:
            o.set_graph(g); res.append((o.optimize(4), o.vertices()))
        finally:
            o.close()
    np.testing.assert_array_equal(res[1][0]["chi2"], res[0][0]["chi2"])
    np.testing.assert_array_equal(res[1][0]["cg_iters"], res[0][0]["cg_iters"])
    np.testing.assert_array_equal(res[1][1], res[0][1])


def test_rejects_bad_graphs_without_crashing(opt):
    g = util.tiny_arrays("tiny_a")
    bad = g.copy(); bad.e_ids[1, 1] = 999
    with pytest.raises(RuntimeError, match="unknown vertex"):
        opt.set_graph(bad)
    bad = g.copy(); bad.e_ids[1] = [0, 1]        # LM edge between two poses
    with pytest.raises(RuntimeError, match="Point2"):
        opt.set_graph(bad)
    opt.set_graph(g)                              # the handle is still usable
    assert opt.optimize(2)["iters"] == 2


def test_c3_full_size_properties():
    """BASELINE config 3 (100k poses / 1M LM edges): size-independent checks at full size."""
    g, truth = synth.make_config("c3_100k", with_truth=True)
    o = HipOptimizer(pcg_rel_tol=1e-8)
    try:
        o.set_graph(g)
        # (1) linearity of the solve: the residual of the returned step is small: H delta = b is checked
        #     through the twin's chi^2 and the GPU's own second linearisation below
        r = o.optimize(3)
        v = o.vertices()
    finally:
        o.close()
    assert r["iters"] == 3 and np.all(np.diff(r["chi2"]) < 0)
    assert r["cg_iters"].max() < 200, r["cg_iters"]        # multigrid keeps the solve at tens of iterations
    # (2) damped GN contracts chi^2 by roughly (1-0.2)^2 per step far from the optimum
    ratio = r["chi2"][1:] / r["chi2"][:-1]
    assert np.all(ratio < 0.9) and np.all(ratio > 0.4)
    # (3) the estimate moves towards the ground truth
    e0 = np.linalg.norm(g.v_pos[:, :2] - truth[:, :2], axis=1).mean()
    e1 = np.linalg.norm(v[:, :2] - truth[:, :2], axis=1).mean()
    assert e1 < e0
    # (4) the fixed vertex stays put (gauge 1e6)
    assert np.abs(v[0] - g.v_pos[0]).max() < 1e-3


def test_c3_one_full_size_step_matches_the_cpu_twin():
    """BASELINE config 3 at FULL size: one Gauss-Newton step (linearise + solve, tol 1e-12) on the GPU against
    the CPU twin of the sparse path (itself pinned to the dense restatement at small sizes)."""
    g = synth.make_config("c3_100k")
    ref = oracle.sparse_step(util.to_oracle(g), 1e-12, precond="amg")
    o = HipOptimizer(pcg_rel_tol=1e-12)
    try:
        o.set_graph(g)
        r = o.solve_step()
    finally:
        o.close()
    assert abs(r["chi2"] - ref["chi2"]) <= 1e-11 * ref["chi2"]
    assert np.abs(r["delta"] - ref["delta"]).max() <= 1e-7 * np.abs(ref["delta"]).max()   # north_star: 1e-6
    assert r["cg_iters"] < 150


def test_aggregates_of_four_on_every_level_still_give_the_same_answer(monkeypatch):
    """Aggregates of 4 on the coarse levels (research knob TSGO_AGGC) give a much weaker hierarchy on this graph — under round
    1's fixed smoother damping an indefinite one.  Whatever the preconditioner does, the stopping rule measures the residual
    itself (r^T D^-1 r), so the answer is the block-Jacobi run's.  Whether a solve had to be repeated with block-Jacobi is
    reported, not required: the fallback path itself is pinned by test_gauge_free_graph_on_the_device (fallbacks >= 1)."""
    g = synth.make(20000, 10, seed=2)
    o = HipOptimizer(pcg_rel_tol=1e-10, preconditioner="jacobi")
    try:
        o.set_graph(g); ref = o.optimize(2); vref = o.vertices()
    finally:
        o.close()
    monkeypatch.setenv("TSGO_AGGC", "4")
    o = HipOptimizer(pcg_rel_tol=1e-10, preconditioner="amg", testing=True)
    try:
        o.set_graph(g); r = o.optimize(2); v = o.vertices()
    finally:
        o.close()
    np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=1e-9)
    assert util.max_vertex_diff(v, vref, g.v_type) < 1e-7
    print("aggregates of 4: PCG iterations %s, solves repeated with block-Jacobi: %d" % (list(r["cg_iters"]), r["fallbacks"]))


@pytest.mark.parametrize("name", sorted(edge_cases.CASES))
def test_edge_case_graphs_match_cpu_eigen(opt, name):
    """Fixed landmarks / repeated fixed ids, vertices no edge touches, sparse 32-bit ids, no ODOM edges at all,
    self loops and repeated edges: 8 iterations against the dense restatement (QR solver, like the reference)."""
    g = edge_cases.CASES[name]()
    ref = oracle.optimize(util.to_oracle(g), 8, mode="cpp", solver="qr")
    opt.set_graph(g)
    r = opt.optimize(8)
    assert r["iters"] == ref["iters"] and r["stop"] == ref["stop"]
    np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=1e-9)
    assert util.max_vertex_diff(opt.vertices(), ref["v_pos"], g.v_type) < 1e-8


def test_every_stop_rule_of_the_reference_is_reached_on_the_device():
    """Error rose three times / plateau / short step / iteration cap (OptimizerCpu.h:140-153,167-177): the device stops in
    the same iteration for the same reason as the dense restatement."""
    cases = {"worse": (edge_cases.pose_graph_without_landmarks(), 50), "plateau": (util.c1_arrays(), 50),
             "converged": (edge_cases.near_optimum(), 50), "cap": (util.c1_arrays(), 7)}
    for want, (g, n) in cases.items():
        ref = oracle.optimize(util.to_oracle(g), n, mode="cpp", solver="chol")
        o = HipOptimizer(pcg_rel_tol=1e-12)
        try:
            o.set_graph(g); r = o.optimize(n)
        finally:
            o.close()
        assert ref["stop"] == want
        assert (r["stop"], r["iters"]) == (ref["stop"], ref["iters"]), (want, r["stop"], r["iters"], ref["iters"])


def test_gauge_free_graph_on_the_device():
    """No fixed vertex (singular H): same chi^2 trajectory as the reference's rank-revealing QR.  How the solves get there is
    reported: a multigrid solve that breaks down on the singular coarsest matrix is repeated — with f32 copies in the cycle
    when it ran on the packed ones, then with block-Jacobi."""
    g = edge_cases.no_fixed_vertex()
    ref = oracle.optimize(util.to_oracle(g), 6, mode="cpp", solver="qr")
    for bits in (16, 32):
        o = HipOptimizer(pcg_rel_tol=1e-12, cycle_storage=bits)
        try:
            o.set_graph(g); r = o.optimize(6)
        finally:
            o.close()
        assert r["iters"] == ref["iters"] and r["stop"] == ref["stop"]
        np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=1e-8)
        print("gauge-free graph, cycle storage %d: PCG %s, block-Jacobi repeats %d, cycle storage at the end %d" % (bits, list(r["cg_iters"]), r["fallbacks"], r["cycle_storage_now"]))


def test_block_jacobi_repeat_of_a_failed_multigrid_solve(monkeypatch):
    """The last line of the safety net (Engine::do_solve): a multigrid-preconditioned solve that broke down is repeated from the same
    right-hand side with block-Jacobi.  TSGO_INJECT_AMG_FAILURE declares the first solve of every tsgo_optimize call broken down
    on a graph where the cycle is healthy: pcg_fallbacks counts it, that solve takes block-Jacobi's iteration count, and chi^2 and
    vertices are those of the undisturbed run."""
    g = synth.make(3000, 10, loop_closures=20, seed=3)
    res = {}
    for inject in (False, True):
        if inject:
            monkeypatch.setenv("TSGO_INJECT_AMG_FAILURE", "1")
        o = HipOptimizer(pcg_rel_tol=1e-12, testing=inject)
        try:
            o.set_graph(g); res[inject] = (o.optimize(4), o.vertices())
        finally:
            o.close()
    (r0, v0), (r1, v1) = res[False], res[True]
    assert r0["fallbacks"] == 0 and r1["fallbacks"] == 1
    assert r1["cg_iters"][0] > 5 * r0["cg_iters"][0]                 # the first solve ran block-Jacobi
    np.testing.assert_allclose(r1["chi2"], r0["chi2"], rtol=1e-10)
    assert util.max_vertex_diff(v1, v0, g.v_type) < 1e-8


def test_the_shipped_library_ignores_test_hooks_and_research_variables(monkeypatch):
    """a production process must not change its numerics, or declare a solver failure, because of an inherited
    environment.  The hooks exist in libtsgo_hip_testing.so only: with all of them set, the product library answers bit for bit
    what it answers without them (and its binary does not contain their names: tests/test_abi_symbols.py)."""
    g = synth.make(3000, 10, loop_closures=20, seed=3)
    res = []
    for hooks in (False, True):
        for name in ("TSGO_INJECT_AMG_FAILURE", "TSGO_FORCE_HOST_SLOW", "TSGO_FORCE_PACED", "TSGO_SYM_DECLINE", "TSGO_HOST_PRODUCTS", "TSGO_AGGC", "TSGO_HIER_MAX_AGE", "TSGO_SWEEPS_LIST"):
            if hooks:
                monkeypatch.setenv(name, "1")
            else:
                monkeypatch.delenv(name, raising=False)
        o = HipOptimizer(pcg_rel_tol=1e-12)
        try:
            o.set_graph(g); res.append((o.optimize(4), o.vertices()))
        finally:
            o.close()
    assert res[1][0]["fallbacks"] == 0 and not res[1][0]["graph_replay"]
    np.testing.assert_array_equal(res[0][0]["chi2"], res[1][0]["chi2"])
    np.testing.assert_array_equal(res[0][0]["cg_iters"], res[1][0]["cg_iters"])
    np.testing.assert_array_equal(res[0][1], res[1][1])


def test_paced_eager_launches_give_the_same_bits_as_bursts_and_replay(monkeypatch):
    """do_solve_paced (the host thread one iteration ahead of the device, paced by the gate kernel's reports) is entered
    only after timing heuristics, so nothing pinned it.  TSGO_FORCE_PACED (TSGO_TESTING build) takes it from the first solve on:
    same bits as eager bursts and as hipGraph replay — through a warm start that already meets the tolerance (0 iterations, at a
    loose tolerance), and through an injected
    multigrid failure whose block-Jacobi repeat runs right after a paced solve (stale gate reports must not end it)."""
    g = synth.make(2500, 10, loop_closures=10, seed=17)

    def run(paced, inject, lead=None, use_graphs=0, tol=1e-10):
        for name, on in (("TSGO_FORCE_PACED", paced), ("TSGO_INJECT_AMG_FAILURE", inject)):
            if on:
                monkeypatch.setenv(name, "1")
            else:
                monkeypatch.delenv(name, raising=False)
        if lead:
            monkeypatch.setenv("TSGO_PACE_LEAD", str(lead))
        else:
            monkeypatch.delenv("TSGO_PACE_LEAD", raising=False)
        o = HipOptimizer(pcg_rel_tol=tol, use_graphs=use_graphs, testing=True)
        try:
            o.set_graph(g)
            a = o.optimize(4)
            b = o.optimize(30)
            return a, b, o.vertices()
        finally:
            o.close()
    base = run(False, False)
    for paced, inject, lead, ug in ((True, False, None, 0), (True, False, 3, 0), (False, False, None, 1)):
        r = run(paced, inject, lead, ug)
        for k in (0, 1):
            np.testing.assert_array_equal(r[k]["chi2"], base[k]["chi2"])
            np.testing.assert_array_equal(r[k]["cg_iters"], base[k]["cg_iters"])
            assert r[k]["stop"] == base[k]["stop"]
        np.testing.assert_array_equal(r[2], base[2])
    # a warm start that already meets the rule (k_warm_scale sets `done`: the first gate reports a finished solve of 0 iterations): at a
    # loose tolerance the extrapolated delta is good enough by itself
    loose_burst, loose_paced = run(False, False, tol=3e-2), run(True, False, 2, tol=3e-2)
    assert loose_burst[1]["cg_iters"].min() == 0, loose_burst[1]["cg_iters"]
    for k in (0, 1):
        np.testing.assert_array_equal(loose_paced[k]["chi2"], loose_burst[k]["chi2"])
        np.testing.assert_array_equal(loose_paced[k]["cg_iters"], loose_burst[k]["cg_iters"])
    np.testing.assert_array_equal(loose_paced[2], loose_burst[2])
    inj_burst, inj_paced = run(False, True), run(True, True, 3)
    assert inj_paced[0]["fallbacks"] == 1 and inj_burst[0]["fallbacks"] == 1
    for k in (0, 1):
        np.testing.assert_array_equal(inj_paced[k]["chi2"], inj_burst[k]["chi2"])
        np.testing.assert_array_equal(inj_paced[k]["cg_iters"], inj_burst[k]["cg_iters"])
    np.testing.assert_array_equal(inj_paced[2], inj_burst[2])
    np.testing.assert_allclose(inj_paced[1]["chi2"][-1], base[1]["chi2"][-1], rtol=1e-9)


def test_vertex_and_edge_order_do_not_matter_on_the_device(opt):
    g = edge_cases.base()
    gs, pv = edge_cases.shuffled_vertices_and_edges()
    opt.set_graph(g); a = opt.optimize(6); va = opt.vertices()
    opt.set_graph(gs); b = opt.optimize(6); vb = opt.vertices()
    np.testing.assert_allclose(a["chi2"], b["chi2"], rtol=1e-10)
    assert util.max_vertex_diff(va[pv], vb, gs.v_type) < 1e-9


def test_randomised_graphs_against_cpu_eigen():
    """Differential soak: 24 random graphs (sizes, observation counts, loop closures, fixed sets, both
    preconditioners alternating) — one exact step and three GN iterations against the dense restatement."""
    rng = np.random.default_rng(1234)
    worst = 0.0
    for trial in range(24):
        n = int(rng.integers(8, 260)); k = int(rng.integers(1, 9)); lc = int(rng.integers(0, 6))
        g = synth.make(n, k, loop_closures=lc, seed=int(rng.integers(0, 10 ** 6)))
        fx = [0] + [int(v) for v in rng.choice(g.v_id, size=int(rng.integers(0, 3)), replace=False)]
        g.fixed = np.array(fx, np.uint32)
        d_ref, err, _, _ = util.dense_solution(g)
        ref = oracle.optimize(util.to_oracle(g), 3, mode="cpp", solver="chol")
        o = HipOptimizer(pcg_rel_tol=1e-12, preconditioner="amg" if trial % 2 == 0 else "jacobi",
                         lanes_per_pose=int(rng.choice([0, 1, 2, 4])), lanes_per_lm=int(rng.choice([0, 1, 2, 4, 8])))
        try:
            o.set_graph(g)
            step = o.solve_step()
            r = o.optimize(3)
            v = o.vertices()
        finally:
            o.close()
        assert abs(step["chi2"] - err) <= 1e-11 * max(err, 1.0), (trial, n, k)
        dd = np.abs(step["delta"] - d_ref).max() / max(np.abs(d_ref).max(), 1e-12)
        worst = max(worst, dd)
        assert dd <= 1e-7, (trial, n, k, lc, dd)
        np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=1e-8)
        assert util.max_vertex_diff(v, ref["v_pos"], g.v_type) < 1e-7, (trial, n, k)
    assert worst <= 1e-7


def test_reset_history_makes_a_pooled_handle_start_like_a_fresh_one():
    """tsgo_reset_history: a handle with tsgo_config.warm_requests that changes hands forgets the solver history it holds —
    the next request, same structure or a new one, runs bit for bit like on a fresh handle."""
    from toyslam_amd.graph import GraphArrays
    g = synth.make(2500, 8, seed=31)
    o = HipOptimizer(pcg_rel_tol=1e-10, warm_requests=True)
    fresh = HipOptimizer(pcg_rel_tol=1e-10, warm_requests=True)
    try:
        o.set_graph(g); r0 = o.optimize(6); v0 = o.vertices()
        g1 = GraphArrays(g.v_id, g.v_type, v0, g.e_type, g.e_ids, g.e_meas, g.e_inf, g.fixed)
        o.set_graph(g1); r1 = o.optimize(6)
        assert r0["history_carried"] == 0 and r1["history_carried"] in (1, 2)
        o.reset_history()
        o.set_graph(g1); r2 = o.optimize(6); v2 = o.vertices()          # same structure: refilled, history forgotten
        fresh.set_graph(g1); rf = fresh.optimize(6); vf = fresh.vertices()
        assert r2["history_carried"] == 0 and r2["structure_reused"]
        np.testing.assert_array_equal(r2["chi2"], rf["chi2"]); np.testing.assert_array_equal(r2["cg_iters"], rf["cg_iters"]); np.testing.assert_array_equal(v2, vf)
        assert r1["cg_iters"].sum() <= r2["cg_iters"].sum()                  # what the history had bought
        g2 = synth.make(2600, 8, seed=31)                                     # a new structure after a reset: nothing carried over either
        o.set_graph(g1); o.optimize(3); o.reset_history()
        o.set_graph(g2); r3 = o.optimize(4)
        fresh.set_graph(g2); rf3 = fresh.optimize(4)
        assert r3["history_carried"] == 0
        np.testing.assert_array_equal(r3["chi2"], rf3["chi2"]); np.testing.assert_array_equal(r3["cg_iters"], rf3["cg_iters"])
    finally:
        o.close(); fresh.close()
