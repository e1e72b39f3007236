"""tsgo_marginals on the device: the diagonal blocks of H^-1 against a dense inverse (config 1), a sparse direct solve (10k poses),
their properties, the state rule (no side effects on the solver) and the error cases."""
import numpy as np
import pytest

from oracle import oracle
from tests import util
from toyslam_amd.graph import GraphArrays
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu


def _dims(g):
    return np.where(g.v_type == 0, 3, 2)


def _dense_blocks(g, v_pos, analytic=False):
    """Diagonal blocks of inv(H), H = the oracle's linearisation at v_pos, per vertex (V, 3, 3)."""
    o = util.to_oracle(GraphArrays(g.v_id, g.v_type, v_pos, g.e_type, g.e_ids, g.e_meas, g.e_inf, g.fixed))
    if analytic:
        oracle.set_odom_jacobian("analytic")
    try:
        H, _b, _err, idx = oracle.linearize(o)
    finally:
        if analytic:
            oracle.set_odom_jacobian("constant")
    Hi = np.linalg.inv(H)
    out = np.zeros((len(g.v_id), 3, 3))
    for v, (k, d) in enumerate(zip(idx, _dims(g))):
        out[v, :d, :d] = Hi[k:k + d, k:k + d]
    return out


def _check_blocks(cov, ref, tol):
    for k in range(len(cov)):
        scale = np.abs(ref[k]).max()
        assert np.abs(cov[k] - ref[k]).max() <= tol * scale, (k, cov[k], ref[k])


def _c1_run(preconditioner="amg", odom_jacobian="constant", g=None, iters=5):
    g = util.c1_arrays() if g is None else g
    o = HipOptimizer(pcg_rel_tol=1e-12, preconditioner=preconditioner, odom_jacobian=odom_jacobian)
    o.set_graph(g)
    o.optimize(iters)
    return g, o


@pytest.mark.parametrize("preconditioner", ["amg", "jacobi"])
@pytest.mark.parametrize("odom_jacobian", ["constant", "analytic"])
def test_c1_against_dense_inverse(preconditioner, odom_jacobian):
    g, o = _c1_run(preconditioner, odom_jacobian)
    try:
        v = o.vertices()
        cov, st = o.marginals(g.v_id, rel_tol=1e-12)
        assert st["columns"] == 3 * int((g.v_type == 0).sum()) + 2 * int((g.v_type == 1).sum())
        assert st["preconditioner"] == (1 if preconditioner == "amg" else 0) and st["fallbacks"] == 0
        assert np.array_equal(o.vertices(), v)          # estimates unchanged
    finally:
        o.close()
    ref = _dense_blocks(g, v, analytic=odom_jacobian == "analytic")
    _check_blocks(cov, ref, 1e-8)
    lm = g.v_type == 1
    assert np.all(cov[lm][:, 2, :] == 0) and np.all(cov[lm][:, :, 2] == 0)
    # the fixed pose is pinned by the gauge term (1e-6 I), and a landmark seen from one pose only is among the blocks checked
    f = int(np.flatnonzero(g.v_id == g.fixed[0])[0])
    assert np.allclose(cov[f], 1e-6 * np.eye(3), rtol=1e-3, atol=1e-12)
    seen = np.bincount(np.concatenate([g.e_ids[g.e_type == 1, 1]]).astype(np.int64), minlength=int(g.v_id.max()) + 1)
    assert (seen[g.v_id[lm]] == 1).any()


def test_c1_virtual_landmarks_against_dense_inverse():
    g = util.with_virtual_landmarks(util.c1_arrays())
    g, o = _c1_run(g=g)
    try:
        v = o.vertices()
        cov, _st = o.marginals(g.v_id, rel_tol=1e-12)
    finally:
        o.close()
    _check_blocks(cov, _dense_blocks(g, v), 1e-8)


def _sparse_H(g, v_pos):
    """H (3 unknowns per vertex; the unused third one of a landmark decoupled with a unit diagonal) from tests/independent.py."""
    import scipy.sparse as sp
    from tests.independent import Linearisation
    lin = Linearisation(GraphArrays(g.v_id, g.v_type, v_pos, g.e_type, g.e_ids, g.e_meas, g.e_inf, g.fixed))
    rows, cols, vals = [], [], []
    for (Ja, ia), (Jb, ib) in [((lin.A, lin.i1), (lin.A, lin.i1)), ((lin.A, lin.i1), (lin.B, lin.i2)),
                               ((lin.B, lin.i2), (lin.A, lin.i1)), ((lin.B, lin.i2), (lin.B, lin.i2))]:
        blk = np.einsum("eki,ek,ekj->eij", Ja, lin.w, Jb)
        r = 3 * ia[:, None, None] + np.arange(3)[None, :, None]
        c = 3 * ib[:, None, None] + np.arange(3)[None, None, :]
        rows.append(np.broadcast_to(r, blk.shape).ravel()); cols.append(np.broadcast_to(c, blk.shape).ravel()); vals.append(blk.ravel())
    V = len(g.v_id)
    d = np.zeros((V, 3))
    d[:, :] = lin.gauge[:, None]
    d[g.v_type == 1, 2] = 1.0
    rows.append(np.arange(3 * V)); cols.append(np.arange(3 * V)); vals.append(d.ravel())
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(3 * V, 3 * V))


def test_c2_against_sparse_direct_solve():
    from scipy.sparse.linalg import splu
    from toyslam_amd import synth
    g = synth.make_config("c2_10k")
    o = HipOptimizer(pcg_rel_tol=1e-10)
    try:
        o.set_graph(g)
        o.optimize(3)
        v = o.vertices()
        poses = np.flatnonzero(g.v_type == 0); lms = np.flatnonzero(g.v_type == 1)
        pick = np.concatenate([poses[np.linspace(0, len(poses) - 1, 30).astype(int)], lms[np.linspace(0, len(lms) - 1, 30).astype(int)]])
        cov, st = o.marginals(g.v_id[pick], rel_tol=1e-12)
        assert st["fallbacks"] == 0
    finally:
        o.close()
    lu = splu(_sparse_H(g, v))
    for k, vtx in enumerate(pick):
        d = 3 if g.v_type[vtx] == 0 else 2
        E = np.zeros((lu.shape[0], d)); E[3 * vtx + np.arange(d), np.arange(d)] = 1
        ref = lu.solve(E)[3 * vtx:3 * vtx + d, :]
        assert np.abs(cov[k, :d, :d] - ref).max() <= 1e-7 * np.abs(ref).max(), (k, vtx)


def test_properties_symmetry_determinism_and_query_forms():
    g, o = _c1_run()
    try:
        ids = g.v_id[::7]
        cov, st = o.marginals(ids, rel_tol=1e-12)
        assert st["batches"] > 1                         # larger than one batch: chunked
        cov2, _ = o.marginals(ids, rel_tol=1e-12)
        assert np.array_equal(cov, cov2)                 # same bits
        for k, vtx in enumerate(ids):
            d = 3 if g.v_type[np.flatnonzero(g.v_id == vtx)[0]] == 0 else 2
            b = cov[k, :d, :d]
            assert np.array_equal(b, b.T)
            np.linalg.cholesky(b)
        rev, _ = o.marginals(ids[::-1], rel_tol=1e-12)
        dup, _ = o.marginals(np.concatenate([ids[:5], ids[:5]]), rel_tol=1e-12)
        one = np.stack([o.marginals([i], rel_tol=1e-12)[0][0] for i in ids[:6]])
    finally:
        o.close()
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    assert rel(rev[::-1], cov) <= 1e-9
    assert rel(dup[:5], cov[:5]) <= 1e-9 and rel(dup[5:], cov[:5]) <= 1e-9
    assert rel(one, cov[:6]) <= 1e-9


def test_marginal_width_one_agrees_with_width_sixteen(monkeypatch):
    """The narrow path (one column per batch, a query's solves gathered before the read-out) against the whole-query packing."""
    g = util.c1_arrays()
    ids = g.v_id[::23]
    kinds = g.v_type[::23]
    poses, lms = int((kinds == 0).sum()), int((kinds == 1).sum())
    assert poses > 0 and lms > 0
    out = {}
    for w in ("16", "1"):
        monkeypatch.setenv("TSGO_MARGINAL_WIDTH", w)
        o = HipOptimizer(pcg_rel_tol=1e-12, testing=True)
        try:
            o.set_graph(g)
            o.optimize(5)
            out[w] = o.marginals(ids, rel_tol=1e-12)
        finally:
            o.close()
    (c16, s16), (c1, s1) = out["16"], out["1"]
    assert s16["batch_width"] == 16 and s1["batch_width"] == 1
    assert s1["batches"] == s1["columns"] == 3 * poses + 2 * lms
    assert np.abs(c1 - c16).max() <= 1e-9 * np.abs(c16).max()


def _chain(n=60):
    v_id = np.arange(n, dtype=np.uint32); v_type = np.zeros(n, np.uint32)
    v_pos = np.zeros((n, 3)); v_pos[:, 0] = np.arange(n)
    e_ids = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1).astype(np.uint32)
    meas = np.tile(np.array([1, 0, 1.0, 0, 1, 0, 0, 0, 1]), (n - 1, 1))
    return GraphArrays(v_id, v_type, v_pos, np.zeros(n - 1, np.uint32), e_ids, meas, np.full((n - 1, 3), 100.0), np.zeros(1, np.uint32))


def test_uncertainty_grows_along_an_odometry_chain():
    g = _chain()
    o = HipOptimizer(pcg_rel_tol=1e-12)
    try:
        o.set_graph(g)
        cov, _ = o.marginals(g.v_id, rel_tol=1e-12)
    finally:
        o.close()
    tr = np.trace(cov, axis1=1, axis2=2)
    assert np.all(np.diff(tr[1:]) > 0), tr


def _run(seq, **kw):
    o = HipOptimizer(pcg_rel_tol=1e-10, **kw)
    try:
        return seq(o)
    finally:
        o.close()


def test_no_side_effects_on_the_solver():
    g = util.c1_arrays()
    ids = g.v_id[::5]

    def a(o, m):
        o.set_graph(g)
        if m:
            o.marginals(ids)
        r = o.optimize(10)
        return o.vertices(), r["chi2"], r["cg_iters"]
    for x, y in zip(_run(lambda o: a(o, False)), _run(lambda o: a(o, True))):
        assert np.array_equal(x, y)

    small = util.first_poses(g, 100)

    def b(o, m):
        o.set_graph(small)
        o.optimize(5)
        if m:
            o.marginals(small.v_id[::3])
        grown = GraphArrays(g.v_id, g.v_type, g.v_pos.copy(), g.e_type, g.e_ids, g.e_meas, g.e_inf, g.fixed)
        vs = o.vertices()
        for k, vid in enumerate(small.v_id):
            grown.v_pos[np.flatnonzero(g.v_id == vid)[0]] = vs[k]
        o.set_graph(grown)
        r = o.optimize(5)
        return o.vertices(), r["chi2"], r["cg_iters"]
    for x, y in zip(_run(lambda o: b(o, False), warm_requests=True), _run(lambda o: b(o, True), warm_requests=True)):
        assert np.array_equal(x, y)

    def c(o, m):
        o.set_graph(g)
        o.optimize(5)
        if m:
            v0 = o.vertices()
            o.marginals(ids)
            assert np.array_equal(o.vertices(), v0)
        r = o.optimize(5)
        return r["stop"], r["iters"], r["chi2"], o.vertices()
    x, y = _run(lambda o: c(o, False)), _run(lambda o: c(o, True))
    assert x[0] == y[0] and x[1] == y[1]
    assert np.abs(x[2] - y[2]).max() <= 1e-9 * np.abs(x[2]).max()


def test_errors_leave_the_handle_usable():
    g = util.c1_arrays()
    o = HipOptimizer()
    try:
        with pytest.raises(RuntimeError, match="no graph"):
            o.marginals([0])
        o.set_graph(g)
        with pytest.raises(RuntimeError, match="unknown vertex id 987654"):
            o.marginals([int(g.v_id[0]), 987654])
        cov, _ = o.marginals(g.v_id[:2])
        assert np.isfinite(cov).all()
        assert o.marginals([])[0].shape == (0, 3, 3)
        free = GraphArrays(g.v_id, g.v_type, g.v_pos, g.e_type, g.e_ids, g.e_meas, g.e_inf, np.zeros(0, np.uint32))
        o.set_graph(free)
        with pytest.raises(RuntimeError, match="fixed vertex"):
            o.marginals(g.v_id[:1])
        o.set_graph(g)
        assert o.optimize(2)["iters"] == 2
    finally:
        o.close()
    o = HipOptimizer(precision=32)
    try:
        o.set_graph(g)
        with pytest.raises(RuntimeError, match="precision"):
            o.marginals(g.v_id[:1])
        assert o.optimize(2)["iters"] == 2
    finally:
        o.close()


def test_c3_multigrid_and_block_jacobi_agree():
    from toyslam_amd import synth
    g = synth.make_config("c3_100k")
    poses = np.flatnonzero(g.v_type == 0); lms = np.flatnonzero(g.v_type == 1)
    pick = g.v_id[np.concatenate([poses[np.linspace(0, len(poses) - 1, 64).astype(int)], lms[np.linspace(0, len(lms) - 1, 64).astype(int)]])]
    out = {}
    for pc in ("amg", "jacobi"):
        o = HipOptimizer(preconditioner=pc)
        try:
            o.set_graph(g)
            out[pc] = o.marginals(pick, rel_tol=1e-11)
        finally:
            o.close()
    (ca, sa), (cj, sj) = out["amg"], out["jacobi"]
    assert sa["preconditioner"] == 1 and sa["fallbacks"] == 0 and sj["preconditioner"] == 0
    for k in range(len(pick)):
        assert np.abs(ca[k] - cj[k]).max() <= 1e-7 * np.abs(cj[k]).max(), k
