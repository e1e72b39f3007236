"""tsgo_gate_edges without a device: the restatement of tests/gate.py is checked against finite differences, reproduces the use case of
the feature (true loop closures pass the chi^2 gate, false ones do not), and the entry point is declared where the bindings expect it."""
import os
import re

import numpy as np

from tests import gate, independent, util
from toyslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _five_type_candidates(g, rng):
    pose = g.v_id[g.v_type == 0]; lm = g.v_id[g.v_type == 1]
    at = {int(v): k for k, v in enumerate(g.v_id)}
    t, ids, meas, inf = [], [], [], []
    for _ in range(4):
        a, b = rng.choice(pose, 2, replace=False)
        th = rng.uniform(-3, 3)
        t.append(0); ids.append([a, b]); inf.append(rng.uniform(1, 50, 3))
        meas.append([np.cos(th), -np.sin(th), rng.uniform(-3, 3), np.sin(th), np.cos(th), rng.uniform(-3, 3), 0, 0, 1])
    for _ in range(4):
        t.append(1); ids.append([rng.choice(pose), rng.choice(lm)]); inf.append(rng.uniform(1, 50, 3))
        meas.append([rng.uniform(0.5, 8), rng.uniform(-3, 3), 0, 0, 0, 0, 0, 0, 0])
    for _ in range(4):
        a, b = rng.choice(pose, 2, replace=False)
        t.append(2); ids.append([a, b]); inf.append(rng.uniform(1, 50, 3))
        meas.append([rng.uniform(0.5, 8), rng.uniform(-3, 3), rng.uniform(0.5, 8), rng.uniform(-3, 3), 0, 0, 0, 0, 0])
    for _ in range(4):
        a = rng.choice(pose); x = g.v_pos[at[int(a)]]
        t.append(3); ids.append([a, a]); inf.append(rng.uniform(1, 50, 3))
        meas.append([x[0] + rng.normal(), x[1] + rng.normal(), x[2] + rng.uniform(-1, 1), 0, 0, 0, 0, 0, 0])
    for _ in range(4):
        a = rng.choice(lm); x = g.v_pos[at[int(a)]]
        t.append(4); ids.append([a, a]); inf.append(rng.uniform(1, 50, 3))
        meas.append([x[0] + rng.normal(), x[1] + rng.normal(), 0, 0, 0, 0, 0, 0, 0])
    return gate.candidates(t, ids, meas, inf)


def test_jacobians_agree_with_central_differences_of_the_residuals():
    """All five types: d e / d (update of vertex 1 | vertex 2) under independent.apply_update(step = 1), h = 1e-6, against the A and B the
    restatement uses; 1e-6 of the largest Jacobian entry (truncation h^2 |e'''| / 6 plus rounding eps |e| / h for residuals of order 1 - 10)."""
    g = util.c1_arrays()
    rng = np.random.default_rng(12)
    c = _five_type_candidates(g, rng)
    e0, A, B = gate.linearise(g, g.v_pos, c)
    assert np.abs(e0).max() > 0.5
    h = 1e-6
    p = [gate._positions(g, c.e_ids[:, 0]), gate._positions(g, c.e_ids[:, 1])]
    num = np.zeros((2, len(c.e_type), 3, 3))
    for side in (0, 1):
        for j in range(3):
            for k in range(len(c.e_type)):
                if side == 1 and c.e_type[k] >= 3:
                    continue                              # a prior has one vertex: B = 0
                d = np.zeros_like(g.v_pos); d[p[side][k], j] = h
                ep = gate.linearise(g, independent.apply_update(g.v_pos, g.v_type, d, step=1.0), gate.take(c, [k]))[0][0]
                em = gate.linearise(g, independent.apply_update(g.v_pos, g.v_type, -d, step=1.0), gate.take(c, [k]))[0][0]
                num[side, k, :, j] = (ep - em) / (2 * h)
    for k in range(len(c.e_type)):
        for side, J in ((0, A), (1, B)):
            dv = 3 if g.v_type[p[side][k]] == 0 else 2          # a landmark has no third coordinate to move
            scale = max(np.abs(A[k]).max(), np.abs(B[k]).max())
            err = np.abs(num[side, k][:, :dv] - J[k][:, :dv]).max()
            assert err <= 1e-6 * scale, (k, int(c.e_type[k]), side, err, scale)
            assert not J[k][:, dv:].any()
    # every type has a Jacobian that is not a constant matrix or is checked non-trivially: the ODOM ones differ from -I / +I
    odom = c.e_type == 0
    assert np.abs(A[odom] + np.eye(3)).max() > 0.1 and np.abs(B[odom] - np.eye(3)).max() > 0.1


def test_the_gate_separates_true_from_false_loop_closures():
    """The use case: 239 odometry edges and 12 true closures in the graph, Levenberg-Marquardt to convergence, then the other 12 true
    closures and the 13 false ones as candidates.  The chi^2_3 99 % gate accepts every true one and rejects every false one."""
    from tests import robust
    base, cand, is_true = gate.scenario_split()
    assert is_true.sum() == 12 and (~is_true).sum() == 13
    run = robust.dense_lm(base, None, 30)
    assert run["stop"] == "converged"
    r = gate.gate(base, run["v_pos"], cand, analytic=True)
    print("true d2 %.3g .. %.3g, false d2 %.3g .. %.3g" % (r["d2"][is_true].min(), r["d2"][is_true].max(), r["d2"][~is_true].min(), r["d2"][~is_true].max()))
    assert (r["dof"] == 3).all()
    assert (r["d2"][is_true] < gate.CHI2_99[3]).all()
    assert (r["d2"][~is_true] > gate.CHI2_99[3]).all()


def test_header_and_bindings_declare_the_entry_point():
    text = open(os.path.join(ROOT, "include", "tsgo.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+tsgo_gate_edges\s*\(", text)
    assert re.search(r"\btsgo_gate_stats\b", text)
    assert "tsgo_gate_edges" in _lib.DEVICE_SYMBOLS
    fields = [f for f, _t in _lib.tsgo_gate_stats._fields_]
    assert fields == ["candidates", "vertices", "not_pd", "reserved", "solve", "ms_total", "ms_readout"]
    assert "GateEdges" in open(os.path.join(ROOT, "include", "tsgo.hpp")).read()
