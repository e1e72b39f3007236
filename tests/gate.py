"""tsgo_gate_edges (include/tsgo.h) restated in numpy, sharing nothing with the product's arithmetic.

For a graph, estimates and candidate edges (the four edge arrays of a graph):
  e, A, B   types 0 - 2 from independent.Linearisation of a graph that holds the candidates as its edges, under the analytic ODOM Jacobians
            (lm_rules._Jacobians("analytic")); the priors written out: J = blockdiag(R_m^T, 1) for a pose prior, I for a landmark prior
  Sigma     the pair block of np.linalg.inv of the dense oracle's H (how tests/test_gpu_joint_marginals._dense_inverse gets it), under
            either ODOM Jacobian setting of the handle
  S = J Sigma J^T + Omega^-1, d2 = e^T S^-1 e, logdet = ln det S."""
from types import SimpleNamespace

import numpy as np

from oracle import oracle
from tests import independent, lm_rules
from toyslam_amd.graph import GraphArrays

DOF = np.array([3, 2, 2, 3, 2])      # by edge type
CHI2_99 = {3: 11.345, 2: 9.210}


def candidates(e_type, e_ids, e_meas, e_inf):
    K = len(e_type)
    return SimpleNamespace(e_type=np.asarray(e_type, np.uint32).reshape(K), e_ids=np.asarray(e_ids, np.uint32).reshape(K, 2),
                           e_meas=np.asarray(e_meas, np.float64).reshape(K, 9), e_inf=np.asarray(e_inf, np.float64).reshape(K, 3))


def take(c, idx):
    return candidates(c.e_type[idx], c.e_ids[idx], c.e_meas[idx], c.e_inf[idx])


def concat(parts):
    return candidates(*(np.concatenate([getattr(p, f) for p in parts]) for f in ("e_type", "e_ids", "e_meas", "e_inf")))


def edges_of(g, idx):
    return candidates(g.e_type[idx], g.e_ids[idx], g.e_meas[idx], g.e_inf[idx])


def _positions(g, ids):
    order = np.argsort(g.v_id, kind="stable")
    return order[np.searchsorted(g.v_id[order], ids)]


def linearise(g, v_pos, c):
    """e (K, 3), A, B (K, 3, 3) of the candidates at v_pos: rows beyond the type's dof and columns beyond a vertex's size are 0; B = 0 for
    a prior."""
    K = len(c.e_type)
    e = np.zeros((K, 3)); A = np.zeros((K, 3, 3)); B = np.zeros((K, 3, 3))
    low = np.flatnonzero(c.e_type <= 2)
    if len(low):
        h = GraphArrays(g.v_id, g.v_type, np.array(v_pos, dtype=np.float64), c.e_type[low], c.e_ids[low], c.e_meas[low], c.e_inf[low], g.fixed)
        with lm_rules._Jacobians("analytic"):
            lin = independent.Linearisation(h)
        e[low] = lin.e; A[low] = lin.A; B[low] = lin.B
    x = np.asarray(v_pos)[_positions(g, c.e_ids[:, 0])]
    m = c.e_meas
    k = np.flatnonzero(c.e_type == 3)                    # e_t = R_m^T (t - t_m), e_th = wrap(th - m_th), J = blockdiag(R_m^T, 1)
    if len(k):
        cs, sn = np.cos(m[k, 2]), np.sin(m[k, 2])
        dx, dy = x[k, 0] - m[k, 0], x[k, 1] - m[k, 1]
        e[k, 0] = cs * dx + sn * dy; e[k, 1] = -sn * dx + cs * dy
        e[k, 2] = np.arctan2(np.sin(x[k, 2] - m[k, 2]), np.cos(x[k, 2] - m[k, 2]))
        A[k, 0, 0] = cs; A[k, 0, 1] = sn; A[k, 1, 0] = -sn; A[k, 1, 1] = cs; A[k, 2, 2] = 1
    k = np.flatnonzero(c.e_type == 4)                    # e = l - m, J = I
    if len(k):
        e[k, :2] = x[k, :2] - m[k, :2]
        A[k, 0, 0] = A[k, 1, 1] = 1
    return e, A, B


def dense_inverse(g, v_pos, analytic):
    """inv(H) of the dense oracle's linearisation of g (edge types 0 - 2) at v_pos, and the first row of every vertex."""
    assert (g.e_type <= 2).all()
    o = oracle.Graph(g.v_id, g.v_type, v_pos, g.e_type, g.e_ids, g.e_meas, g.e_inf, g.fixed)
    with lm_rules._Jacobians("analytic" if analytic else "constant"):
        H, _b, _err, idx = oracle.linearize(o)
    return np.linalg.inv(H), idx


def gate(g, v_pos, c, analytic, Hinv=None):
    """The records of tsgo_gate_edges for candidates c on graph g at v_pos (analytic: the HANDLE's odom_jacobian, which enters H only).
    dict of e (K, 3), s, d2, logdet (K,), dof (K,), innov (K, 3, 3), and for the bounds of the tests jnorm (the infinity norm of J), sigmax
    (the largest entry of the pair block of Sigma), cond (of S)."""
    Hi, idx = dense_inverse(g, v_pos, analytic) if Hinv is None else Hinv
    e, A, B = linearise(g, v_pos, c)
    K = len(c.e_type)
    p1, p2 = _positions(g, c.e_ids[:, 0]), _positions(g, c.e_ids[:, 1])
    out = dict(e=e, s=np.zeros(K), d2=np.zeros(K), logdet=np.zeros(K), dof=DOF[c.e_type], innov=np.zeros((K, 3, 3)), jnorm=np.zeros(K),
               sigmax=np.zeros(K), cond=np.zeros(K))
    for k in range(K):
        dof = int(DOF[c.e_type[k]])
        d1 = 3 if g.v_type[p1[k]] == 0 else 2
        rows = idx[p1[k]] + np.arange(d1)
        J = A[k, :dof, :d1]
        if c.e_type[k] <= 2:
            d2 = 3 if g.v_type[p2[k]] == 0 else 2
            rows = np.concatenate([rows, idx[p2[k]] + np.arange(d2)])
            J = np.hstack([J, B[k, :dof, :d2]])
        Sig = Hi[np.ix_(rows, rows)]
        Sig = 0.5 * (Sig + Sig.T)
        w = c.e_inf[k, :dof]
        S = J @ Sig @ J.T + np.diag(1.0 / w)
        ek = e[k, :dof]
        out["s"][k] = float((w * ek * ek).sum())
        out["d2"][k] = float(ek @ np.linalg.solve(S, ek))
        out["logdet"][k] = float(np.linalg.slogdet(S)[1])
        out["innov"][k, :dof, :dof] = S
        out["jnorm"][k] = np.abs(J).sum(axis=1).max()
        out["sigmax"][k] = np.abs(Sig).max()
        out["cond"][k] = np.linalg.cond(S)
    return out


def relative_pose_meas(xa, xb):
    """The 3 x 3 ODOM measurement (row-major, 9) that makes the residual of the edge (a, b) zero at the poses xa, xb."""
    c, s = np.cos(xa[2]), np.sin(xa[2])
    d = xb[:2] - xa[:2]
    th = xb[2] - xa[2]
    return np.array([np.cos(th), -np.sin(th), c * d[0] + s * d[1], np.sin(th), np.cos(th), -s * d[0] + c * d[1], 0, 0, 1.0])


# ---- the use case of the issue: the 240-pose outlier scenario of tests/robust.py ------------------------------------------------------
def scenario_split():
    """(base graph, candidates, is_true): the scenario's 239 odometry edges plus every second true loop closure as the graph, the other 12
    true closures and the 13 false ones as candidates."""
    from tests import robust
    g = robust.scenario()
    n_odom, n_true = 239, robust.SCENARIO["closures"]
    assert len(g.e_type) == n_odom + n_true + 13
    keep = np.r_[np.arange(n_odom), np.arange(n_odom, n_odom + n_true)[::2]]
    cand = np.r_[np.arange(n_odom, n_odom + n_true)[1::2], np.arange(n_odom + n_true, len(g.e_type))]
    base = GraphArrays(g.v_id, g.v_type, g.v_pos.copy(), g.e_type[keep], g.e_ids[keep], g.e_meas[keep], g.e_inf[keep], g.fixed)
    return base, edges_of(g, cand), np.arange(len(cand)) < n_true // 2
