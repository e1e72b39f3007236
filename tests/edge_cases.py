"""Edge-case OptGraphs shared by the CPU (twin) and GPU (HIP) parity tests.  Each returns GraphArrays."""
import numpy as np

from toyslam_amd import synth
from toyslam_amd.graph import GraphArrays


def _pose_mat(x, y, th):
    c, s = np.cos(th), np.sin(th)
    return np.array([c, -s, x, s, c, y, 0, 0, 1.0])


def base(n=60, seed=21):
    return synth.make(n, 6, loop_closures=3, seed=seed)


def fixed_landmark_and_duplicate_fixed_ids():
    g = base()
    lm = g.v_id[g.v_type == 1]
    g.fixed = np.array([0, 0, lm[3], lm[3], lm[3], 7], np.uint32)       # multiplicities 2, 3, 1 (OptimizerCpu.h:132-138)
    return g


def isolated_vertices():
    g = base()
    n = len(g.v_id)
    v_id = np.concatenate([g.v_id, [n + 5, n + 9]]).astype(np.uint32)
    v_type = np.concatenate([g.v_type, [1, 0]]).astype(np.uint32)       # a landmark and a pose nobody refers to
    v_pos = np.concatenate([g.v_pos, [[3.0, 4.0, 0.0], [1.0, 2.0, 0.3]]])
    return GraphArrays(v_id, v_type, v_pos, g.e_type, g.e_ids, g.e_meas, g.e_inf, g.fixed)


def sparse_large_ids():
    g = base()
    remap = {int(k): int(1000 + 7919 * i) % (2 ** 31 - 1) + (2 ** 31 if i % 3 == 0 else 0) for i, k in enumerate(g.v_id)}
    f = np.vectorize(lambda k: remap[int(k)], otypes=[np.uint64])
    return GraphArrays(f(g.v_id).astype(np.uint32), g.v_type, g.v_pos, g.e_type, f(g.e_ids).astype(np.uint32), g.e_meas, g.e_inf,
                       f(g.fixed).astype(np.uint32))


def landmark_edges_only():
    g = base()
    keep = g.e_type == 1
    return GraphArrays(g.v_id, g.v_type, g.v_pos, g.e_type[keep], g.e_ids[keep], g.e_meas[keep], g.e_inf[keep], g.fixed)


def pose_graph_without_landmarks():
    """ODOM edges only (a chain plus loop closures): a plain pose graph, every Jacobian -I / +I (EdgeSe2.h:35-37)."""
    g = synth.make(400, 6, loop_closures=12, seed=23)
    keep = g.e_type == 0
    pose = g.v_type == 0
    return GraphArrays(g.v_id[pose], g.v_type[pose], g.v_pos[pose], g.e_type[keep], g.e_ids[keep], g.e_meas[keep], g.e_inf[keep], g.fixed)


def shuffled_vertices_and_edges(seed=5):
    g = base()
    rng = np.random.default_rng(seed)
    pv = rng.permutation(len(g.v_id)); pe = rng.permutation(len(g.e_type))
    return GraphArrays(g.v_id[pv], g.v_type[pv], g.v_pos[pv], g.e_type[pe], g.e_ids[pe], g.e_meas[pe], g.e_inf[pe], g.fixed), pv


def self_loop_and_duplicate_edges():
    g = base()
    e_type = np.concatenate([g.e_type, [0, 1, 1]]).astype(np.uint32)
    lm_edge = np.where(g.e_type == 1)[0][0]
    e_ids = np.concatenate([g.e_ids, [[5, 5]], g.e_ids[[lm_edge, lm_edge]]]).astype(np.uint32)   # ODOM self loop, LM edge x3
    e_meas = np.concatenate([g.e_meas, [_pose_mat(0.1, -0.05, 0.02)], g.e_meas[[lm_edge, lm_edge]] + 0.01])
    e_inf = np.concatenate([g.e_inf, [[4.0, 4.0, 65.0]], g.e_inf[[lm_edge, lm_edge]]])
    return GraphArrays(g.v_id, g.v_type, g.v_pos, e_type, e_ids, e_meas, e_inf, g.fixed)


def no_fixed_vertex():
    g = base()
    g.fixed = np.zeros(0, np.uint32)        # gauge-free: H is singular; the reference's QR returns a minimum-norm-like step
    return g


def non_rigid_odom_measurements():
    """The wire carries an ODOM measurement as ANY 3x3 (DeserializeGraph.h:99-111) and EdgeSe2.h:32 inverts it as
    such: a few measurements with shear / scale in the upper-left block and a last row that is not (0, 0, 1)."""
    g = base()
    od = np.where(g.e_type == 0)[0]
    m = g.e_meas.copy()
    m[od[1]] = m[od[1]] * np.array([1.03, 1.0, 1.0, 1.0, 0.98, 1.0, 1.0, 1.0, 1.0]) + np.array([0, 0.02, 0, -0.01, 0, 0, 0, 0, 0])
    m[od[4]] = m[od[4]] + np.array([0, 0, 0, 0, 0, 0, 0.002, -0.001, 0.01])
    return GraphArrays(g.v_id, g.v_type, g.v_pos, g.e_type, g.e_ids, m, g.e_inf, g.fixed)


def near_optimum(rounds=6):
    """tiny_a re-started from its own optimised vertices until the first step is shorter than 1e-3: the run then stops
    on the reference's third rule ("CONVERGED", OptimizerCpu.h:173-177) after one iteration."""
    from oracle import oracle
    from tests import util
    t = util.tiny_arrays("tiny_a")
    cur = t
    for _ in range(rounds):
        r = oracle.optimize(util.to_oracle(cur), 400, mode="cpp", solver="chol")
        cur = GraphArrays(t.v_id, t.v_type, r["v_pos"].copy(), t.e_type, t.e_ids, t.e_meas, t.e_inf, t.fixed)
    return cur


def zero_residuals(n=48, row=12):
    """Every measurement computed from the estimates, in numbers whose arithmetic is exact: poses on integer grid points with theta = 0
    (cos 1, sin 0), ODOM measurements the integer translations between them, every landmark an integer distance straight ahead of the
    poses that see it (range an integer, bearing atan2(0, d) = 0).  Every residual is 0: chi^2 = 0 and b = 0 (not one of CASES: the
    parity tests compare steps, and there is no step here)."""
    xy = np.array([[2 * (k % row), 3 * (k // row)] for k in range(n)], float)
    v_id = list(range(n)); v_type = [0] * n; v_pos = [[x, y, 0.0] for x, y in xy]
    e_type, e_ids, e_meas, e_inf = [], [], [], []
    for k in range(n - 1):
        for j in ([k + 1] + ([k + row] if k + row < n else [])):      # the chain and the grid's columns (loop closures)
            d = xy[j] - xy[k]
            e_type.append(0); e_ids.append([k, j]); e_meas.append(_pose_mat(d[0], d[1], 0.0)); e_inf.append([4.0, 4.0, 65.0])
    for k in range(0, n, 2):      # a landmark 5 ahead of pose k, seen from k and from the pose to its left on the same row
        lid = n + k // 2
        v_id.append(lid); v_type.append(1); v_pos.append([xy[k, 0] + 5.0, xy[k, 1], 0.0])
        for j in ([k] + ([k - 1] if k % row else [])):
            e_type.append(1); e_ids.append([j, lid]); e_meas.append([xy[k, 0] + 5.0 - xy[j, 0], 0.0, 0, 0, 0, 0, 0, 0, 0]); e_inf.append([9.0, 120.0, 0.0])
    return GraphArrays(np.array(v_id, np.uint32), np.array(v_type, np.uint32), np.array(v_pos), np.array(e_type, np.uint32),
                       np.array(e_ids, np.uint32), np.array(e_meas, float), np.array(e_inf, float), np.array([0], np.uint32))


CASES = {
    "fixed_landmark_dup_fixed": fixed_landmark_and_duplicate_fixed_ids,
    "isolated_vertices": isolated_vertices,
    "sparse_large_ids": sparse_large_ids,
    "landmark_edges_only": landmark_edges_only,
    "pose_graph_without_landmarks": pose_graph_without_landmarks,
    "non_rigid_odom_measurements": non_rigid_odom_measurements,
    "self_loop_dup_edges": self_loop_and_duplicate_edges,
}
