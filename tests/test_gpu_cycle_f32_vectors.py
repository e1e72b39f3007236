"""The multigrid cycle's vectors below level 0 in f32 (tsgo_amg_kernels.h: CycVec).  They only precondition the f64 PCG, so the
answer must be the one the f64 vectors give, with the same iteration counts give or take one.  TSGO_CYCLE_VEC64=1 (host/knobs.h,
testing builds only) restores f64 vectors for the comparison."""
import os

import numpy as np
import pytest

from tests import util
from toyslam_amd import build, synth
from toyslam_amd.optimizer import HipOptimizer


def _run(monkeypatch, g, vec64, iterations=10, **kw):
    if vec64:
        monkeypatch.setenv("TSGO_CYCLE_VEC64", "1")
    else:
        monkeypatch.delenv("TSGO_CYCLE_VEC64", raising=False)
    o = HipOptimizer(pcg_rel_tol=1e-10, testing=vec64, **kw)      # the default: the product library
    try:
        o.set_graph(g)
        r = o.optimize(iterations)
        return r, o.vertices()
    finally:
        o.close()
        monkeypatch.delenv("TSGO_CYCLE_VEC64", raising=False)


def _same_answer_and_counts(g, a, b):
    (r32, v32), (r64, v64) = a, b
    assert r32["fallbacks"] == 0 and r64["fallbacks"] == 0
    assert r32["iters"] == r64["iters"]
    np.testing.assert_allclose(r32["chi2"], r64["chi2"], rtol=1e-10, atol=0)
    assert util.max_vertex_diff(v32, v64, g.v_type) <= 1e-8
    c32, c64 = np.asarray(r32["cg_iters"]), np.asarray(r64["cg_iters"])
    assert np.all(c32 <= c64 + 1), (c32, c64)
    assert c32.sum() <= 1.02 * c64.sum(), (c32, c64)


@pytest.mark.gpu
def test_f32_cycle_vectors_keep_answer_and_counts_at_config_2_size(monkeypatch):
    g = synth.make_config("c2_10k")
    _same_answer_and_counts(g, _run(monkeypatch, g, False), _run(monkeypatch, g, True))


@pytest.mark.gpu
def test_f32_cycle_vectors_keep_answer_and_counts_at_config_3_size(monkeypatch):
    """100k poses: four explicit levels, the factored tail (k_rowdot_wg, k_tail_up) and the dense bottom."""
    g = synth.make_config("c3_100k")
    _same_answer_and_counts(g, _run(monkeypatch, g, False), _run(monkeypatch, g, True))


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(cycle_storage=32), dict(cycle_level0="explicit")], ids=["f32_copies", "explicit_level0"])
def test_f32_cycle_vectors_on_the_other_cycle_paths(monkeypatch, kw):
    g = synth.make(6000, 10, loop_closures=30, seed=23)
    _same_answer_and_counts(g, _run(monkeypatch, g, False, **kw), _run(monkeypatch, g, True, **kw))


@pytest.mark.gpu
def test_eager_launches_and_hipgraph_replay_agree_bitwise_with_f32_cycle_vectors():
    g = synth.make_config("c2_10k")
    res = []
    for use_graphs in (False, True):
        o = HipOptimizer(pcg_rel_tol=1e-10, use_graphs=use_graphs)
        try:
            o.set_graph(g)
            o.optimize(1)                   # the graph is captured at the second tsgo_optimize on these tables
            o.set_graph(g)
            r = o.optimize(4)
            res.append((r, o.vertices()))
        finally:
            o.close()
    assert [r["graph_replay"] for r, _ in res] == [False, True]
    np.testing.assert_array_equal(res[0][0]["chi2"], res[1][0]["chi2"])
    np.testing.assert_array_equal(res[0][0]["cg_iters"], res[1][0]["cg_iters"])
    np.testing.assert_array_equal(res[0][1], res[1][1])


def test_the_cycle_vector_knob_is_absent_from_the_shipped_binaries():
    for path in (build.HIP_SO, build.SERVER):
        if not os.path.exists(path):
            pytest.skip("product binaries not built yet (run __graft_entry__.build())")
        assert b"TSGO_CYCLE_VEC64" not in open(path, "rb").read(), path
    assert b"TSGO_CYCLE_VEC64" in open(build.HIP_TESTING_SO, "rb").read()
