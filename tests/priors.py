"""Helpers of the prior tests (edge types 3 and 4, include/tsgo.h): graphs with priors, and the prior terms restated in numpy from the
semantics written in tsgo.h, sharing nothing with the product's arithmetic."""
import numpy as np

from toyslam_amd.graph import GraphArrays

HUBER_DELTA = 1.5


def with_priors(g, frac_pose=0.2, frac_lm=0.2, seed=0, n_far=4, n_dup=3, noise=0.05, weights=((5.0, 20.0), (5.0, 20.0), (10.0, 60.0)),
                fixed=None):
    """A copy of `g` with pose priors on about `frac_pose` of its poses and landmark priors on about `frac_lm` of its landmarks, near
    the current estimates (gaussian `noise`), about `n_far` of each kind far enough off to be in Huber's tail, and `n_dup` vertices of
    each kind that carry a second prior.  The weights are drawn per prior from `weights` = ranges of (w0, w1, w2).  fixed: replaces
    g.fixed."""
    rng = np.random.default_rng(seed)
    pose = np.where(g.v_type == 0)[0]
    lm = np.where(g.v_type == 1)[0]
    pp = rng.choice(pose, size=int(round(frac_pose * len(pose))), replace=False)
    pl = rng.choice(lm, size=int(round(frac_lm * len(lm))), replace=False) if len(lm) else np.zeros(0, int)
    rows = [(3, int(v)) for v in pp] + [(4, int(v)) for v in pl]
    rows += [(3, int(v)) for v in pp[:n_dup]] + [(4, int(v)) for v in pl[:n_dup]]
    rows = [rows[k] for k in rng.permutation(len(rows))]
    far = set(rng.choice(len(rows), size=min(len(rows), 2 * n_far), replace=False).tolist())
    e_type, e_ids, e_meas, e_inf = [], [], [], []
    for k, (t, v) in enumerate(rows):
        m = np.zeros(9); w = np.zeros(3)
        off = rng.normal(0, noise, 3) + (rng.choice([-1.0, 1.0], 3) * 4.0 if k in far else 0.0)
        m[:2] = g.v_pos[v, :2] + off[:2]
        for j in range(3 if t == 3 else 2):
            w[j] = rng.uniform(*weights[j])
        if t == 3:
            th = g.v_pos[v, 2] + 0.1 * off[2]
            m[2] = np.arctan2(np.sin(th), np.cos(th))
        e_type.append(t); e_ids.append([g.v_id[v], g.v_id[v]]); e_meas.append(m); e_inf.append(w)
    return append_edges(g, e_type, e_ids, e_meas, e_inf, fixed)


def append_edges(g, e_type, e_ids, e_meas, e_inf, fixed=None):
    fx = g.fixed if fixed is None else np.asarray(fixed, np.uint32)
    if not len(e_type):
        return GraphArrays(g.v_id, g.v_type, g.v_pos.copy(), g.e_type, g.e_ids, g.e_meas, g.e_inf, fx)
    return GraphArrays(g.v_id, g.v_type, g.v_pos.copy(), np.concatenate([g.e_type, np.asarray(e_type, np.uint32)]),
                       np.concatenate([g.e_ids, np.asarray(e_ids, np.uint32).reshape(-1, 2)]),
                       np.concatenate([g.e_meas, np.asarray(e_meas, np.float64).reshape(-1, 9)]),
                       np.concatenate([g.e_inf, np.asarray(e_inf, np.float64).reshape(-1, 3)]), fx)


def without_priors(g):
    keep = g.e_type <= 2
    return GraphArrays(g.v_id, g.v_type, g.v_pos, g.e_type[keep], g.e_ids[keep], g.e_meas[keep], g.e_inf[keep], g.fixed)


def _huber(chi):
    tail = chi > HUBER_DELTA ** 2
    sq = np.sqrt(np.where(tail, chi, 1.0))
    return np.where(tail, 2 * sq * HUBER_DELTA - HUBER_DELTA ** 2, chi), np.where(tail, HUBER_DELTA / sq, 1.0)


def prior_terms(g, v_pos=None):
    """The priors of `g` at `v_pos` (default g.v_pos): per vertex the 3x3 block they add to H, (V, 3, 3), the vector they add to b,
    (V, 3), and their chi^2 (Huber-robustified, delta 1.5)."""
    v_pos = g.v_pos if v_pos is None else v_pos
    V = len(g.v_id)
    order = np.argsort(g.v_id, kind="stable")
    H = np.zeros((V, 3, 3)); b = np.zeros((V, 3)); chi2 = 0.0
    for t in (3, 4):
        k = np.where(g.e_type == t)[0]
        if not len(k):
            continue
        vi = order[np.searchsorted(g.v_id[order], g.e_ids[k, 0])]
        m, w, x = g.e_meas[k], g.e_inf[k].copy(), v_pos[vi]
        J = np.zeros((len(k), 3, 3))
        e = np.zeros((len(k), 3))
        if t == 3:                                       # e_t = R_m^T (t - t_m), e_th = wrap(th - m_th), J = blockdiag(R_m^T, 1)
            c, s = np.cos(m[:, 2]), np.sin(m[:, 2])
            dx, dy = x[:, 0] - m[:, 0], x[:, 1] - m[:, 1]
            e[:, 0] = c * dx + s * dy; e[:, 1] = -s * dx + c * dy
            e[:, 2] = np.arctan2(np.sin(x[:, 2] - m[:, 2]), np.cos(x[:, 2] - m[:, 2]))
            J[:, 0, 0] = c; J[:, 0, 1] = s; J[:, 1, 0] = -s; J[:, 1, 1] = c; J[:, 2, 2] = 1
        else:                                            # e = l - m, J = I
            w[:, 2] = 0
            e[:, :2] = x[:, :2] - m[:, :2]
            J[:, 0, 0] = J[:, 1, 1] = 1
        rho, hw = _huber((w * e * e).sum(1))
        a = hw[:, None] * w
        np.add.at(H, vi, np.einsum("nki,nk,nkj->nij", J, a, J))
        np.add.at(b, vi, -np.einsum("nki,nk->ni", J, a * e))
        chi2 += float(rho.sum())
    return H, b, chi2


def dense_system(g, lin_factory, check_vectors=2, seed=0):
    """H (dense), b and chi^2 of `g` at its estimates: the linearisation of the graph without its priors (lin_factory =
    independent.Linearisation, whose oracle evaluates edge types 0-2 only) assembled from its per-edge Jacobians and Huber-scaled weights,
    checked against its matrix-free Linearisation.apply_H on `check_vectors` random vectors, plus the prior blocks.  Unknowns in vertex
    order, 3 per pose and 2 per landmark; returns (H, b, chi2, offsets)."""
    lin = lin_factory(without_priors(g))
    Hp, bp, chip = prior_terms(g)
    V = len(g.v_id)
    H4 = np.zeros((V, V, 3, 3))
    np.add.at(H4, (lin.i1, lin.i1), np.einsum("eki,ek,ekj->eij", lin.A, lin.w, lin.A))
    np.add.at(H4, (lin.i2, lin.i2), np.einsum("eki,ek,ekj->eij", lin.B, lin.w, lin.B))
    AB = np.einsum("eki,ek,ekj->eij", lin.A, lin.w, lin.B)
    np.add.at(H4, (lin.i1, lin.i2), AB)
    np.add.at(H4, (lin.i2, lin.i1), AB.transpose(0, 2, 1))
    H4[np.arange(V), np.arange(V)] += lin.gauge[:, None, None] * np.eye(3) + Hp
    dims = np.where(g.v_type == 0, 3, 2)
    mask = (np.arange(3)[None, :] < dims[:, None]).reshape(-1)
    H = H4.transpose(0, 2, 1, 3).reshape(3 * V, 3 * V)[np.ix_(mask, mask)]
    rng = np.random.default_rng(seed)
    for _ in range(check_vectors):
        d = rng.normal(size=(V, 3))
        want = (lin.apply_H(d) + np.einsum("vij,vj->vi", Hp, d)).reshape(-1)[mask]
        got = H @ d.reshape(-1)[mask]
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    b = (lin.gradient() + bp).reshape(-1)[mask]
    off = np.concatenate([[0], np.cumsum(dims)])
    return H, b, lin.chi2 + chip, off


def unpack(x, g):
    """Packed unknowns (3 per pose, 2 per landmark) -> (V, 3)."""
    dims = np.where(g.v_type == 0, 3, 2)
    out = np.zeros((len(g.v_id), 3))
    out[np.arange(3)[None, :] < dims[:, None]] = x
    return out
