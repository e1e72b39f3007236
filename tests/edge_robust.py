"""Robust kernels per EDGE (tsgo_set_edge_robust, include/tsgo.h) restated in numpy on top of tests/robust.py, sharing nothing with the
product's arithmetic.

A per-edge setting is (kernels, entry): `kernels` a palette, each "none" or (name, delta); `entry` one integer per edge of the graph in
input order — 0 leaves the edge to its class's kernel of `setting` (robust.full), k >= 1 gives it kernels[k - 1] whatever its class.
Linearisation and prior_terms are robust.py's with the effective kernel per edge; s = e' Omega e is untouched.  The dense system, chi^2,
the read-out of tsgo_linearize and the rules = 2 loop are robust.py's own functions, run while its two per-class pieces are replaced by
the per-edge ones (per_edge below), so the loop rules exist once.  Also the grid-world generator of the feature's qualifying experiment."""
import contextlib

import numpy as np

from tests import edge_report, init_guess, robust
from tests.init_guess import Builder, relative, wrap


def _override(rho, scale, s, kernels, entry):
    """rho and scale (w) of the edges with a non-zero entry replaced by their palette kernel's; the others keep their class's."""
    for j, kern in enumerate(kernels):
        k = entry == j + 1
        if k.any():
            rho[k], scale[k] = robust.rho_w(kern, s[k])


def _check(kernels, entry, n_edges):
    entry = np.asarray(entry)
    assert entry.shape == (n_edges,) and (len(entry) == 0 or (entry.min() >= 0 and entry.max() <= len(kernels))) and len(kernels) <= 15
    return entry


class Linearisation(robust.Linearisation):
    """robust.Linearisation of a graph without priors; `entry` one value per edge of THAT graph."""

    def __init__(self, g, setting=None, kernels=(), entry=None, dtype=np.float64):
        super().__init__(g, setting, dtype)
        entry = _check(kernels, np.zeros(len(g.e_type), np.int64) if entry is None else entry, len(g.e_type))
        raw = g.e_inf.copy()
        raw[(g.e_type == 1) | (g.e_type == 2), 2] = 0
        rho = self.rho.copy(); scale = np.ones(len(rho), dtype)
        _override(rho, scale, self.s, kernels, entry)
        over = entry > 0
        self.rho = rho
        self.chi2 = float(rho.sum())
        self.chi2_exact = rho.sum()
        self.w = self.w.copy()
        self.w[over] = (raw[over] * scale[over, None]).astype(np.float64)


def prior_terms(g, setting=None, kernels=(), entry=None, v_pos=None, dtype=np.float64):
    """robust.prior_terms with the effective kernel per prior edge; `entry` one value per edge of g (priors and others alike)."""
    setting = robust.full(setting)
    entry = _check(kernels, np.zeros(len(g.e_type), np.int64) if entry is None else entry, len(g.e_type))
    v_pos = g.v_pos if v_pos is None else v_pos
    V = len(g.v_id)
    order = np.argsort(g.v_id, kind="stable")
    H = np.zeros((V, 3, 3)); b = np.zeros((V, 3)); chi2 = dtype(0)
    for t in (3, 4):
        k = np.where(g.e_type == t)[0]
        if not len(k):
            continue
        vi = order[np.searchsorted(g.v_id[order], g.e_ids[k, 0])]
        m, w, x = g.e_meas[k], g.e_inf[k].copy(), v_pos[vi]
        J = np.zeros((len(k), 3, 3)); e = np.zeros((len(k), 3))
        if t == 3:                                       # e_t = R_m^T (t - t_m), e_th = wrap(th - m_th), J = blockdiag(R_m^T, 1)
            c, s_ = np.cos(m[:, 2]), np.sin(m[:, 2])
            dx, dy = x[:, 0] - m[:, 0], x[:, 1] - m[:, 1]
            e[:, 0] = c * dx + s_ * dy; e[:, 1] = -s_ * dx + c * dy
            e[:, 2] = np.arctan2(np.sin(x[:, 2] - m[:, 2]), np.cos(x[:, 2] - m[:, 2]))
            J[:, 0, 0] = c; J[:, 0, 1] = s_; J[:, 1, 0] = -s_; J[:, 1, 1] = c; J[:, 2, 2] = 1
        else:                                            # e = l - m, J = I
            w[:, 2] = 0
            e[:, :2] = x[:, :2] - m[:, :2]
            J[:, 0, 0] = J[:, 1, 1] = 1
        ed = e.astype(dtype)
        s = (w.astype(dtype) * ed * ed).sum(1)
        rho, hw = robust.rho_w(setting[robust.CLASSES[t]], s)
        _override(rho, hw, s, kernels, entry[k])
        a = hw.astype(np.float64)[:, None] * w
        np.add.at(H, vi, np.einsum("nki,nk,nkj->nij", J, a, J))
        np.add.at(b, vi, -np.einsum("nki,nk->ni", J, a * e))
        chi2 += rho.sum()
    return H, b, chi2


@contextlib.contextmanager
def per_edge(g, kernels, entry):
    """While active, robust.py's functions (dense_system, linearisation, chi2_at, dense_lm, dense_gn) evaluate graphs with g's EDGE LIST
    under (kernels, entry): its two per-class pieces are replaced by the per-edge ones above.  Estimates may differ from g's."""
    entry = _check(kernels, entry, len(g.e_type))
    keep = g.e_type <= 2
    n_all, n_base = len(g.e_type), int(keep.sum())

    def lin(base, setting=None, dtype=np.float64):
        assert len(base.e_type) == n_base
        return Linearisation(base, setting, kernels, entry[keep], dtype)

    def pri(graph, setting=None, v_pos=None, dtype=np.float64):
        assert len(graph.e_type) == n_all
        return prior_terms(graph, setting, kernels, entry, v_pos, dtype)

    saved = robust.Linearisation, robust.prior_terms
    robust.Linearisation, robust.prior_terms = lin, pri
    try:
        yield
    finally:
        robust.Linearisation, robust.prior_terms = saved


def linearisation(g, setting, kernels, entry):
    """What tsgo_linearize returns: diag (V, 9), grad (V, 3), chi^2."""
    with per_edge(g, kernels, entry):
        return robust.linearisation(g, setting)


def dense_system(g, setting, kernels, entry, zero_fixed=False):
    with per_edge(g, kernels, entry):
        return robust.dense_system(g, setting, zero_fixed)


def chi2_at(g, setting, kernels, entry, dtype=np.float64):
    with per_edge(g, kernels, entry):
        return robust.chi2_at(g, setting, dtype)


def dense_lm(g, setting, kernels, entry, iterations, lambda0=1e-3, chi2_rel_tol=1e-6, jacobian="analytic"):
    """robust.dense_lm (the rules = 2 loop, its rules untouched) under the per-edge setting."""
    with per_edge(g, kernels, entry):
        return robust.dense_lm(g, setting, iterations, lambda0=lambda0, chi2_rel_tol=chi2_rel_tol, jacobian=jacobian)


def records(g, setting, kernels, entry):
    """edge_report.records with the effective kernel per edge: (E, 6) e0 e1 e2 s rho w."""
    entry = _check(kernels, entry, len(g.e_type))
    rec = edge_report.records(g, setting)
    rho, w = rec[:, 4].copy(), rec[:, 5].copy()
    _override(rho, w, rec[:, 3], kernels, entry)
    return np.column_stack([rec[:, :4], rho, w])


def report(g, setting, kernels, entry):
    rec = records(g, setting, kernels, entry)
    return rec, edge_report.summary(g, rec)      # the class summaries stay indexed by e_type


def effective(g, setting, kernels, entry):
    """The kernel every edge ends up with, as a list."""
    setting = robust.full(setting)
    return [kernels[k - 1] if k else setting[robust.CLASSES[t]] for t, k in zip(g.e_type, entry)]


# ---- the grid world of the qualifying experiment ----------------------------------------------------------------------------------------
def grid_world(n, seed, s_xy=0.03, s_th=0.02, area=12, false_fraction=0.10):
    """(clean, with false closures): n poses on a unit grid walk inside [-area, area]^2 with noisy odometry along the walk, noisy closures
    between half of the pose pairs at most 1 m apart (and at least 12 steps apart), and false_fraction of the closure count (3 at least)
    added as false closures: random pose pairs with a random relative pose and a closure's information.  Estimates are zero (pose 0
    fixed at its truth): take start() of it."""
    rng = np.random.default_rng(seed); P = [[0.0, 0.0, 0.0]]
    for k in range(1, n):
        x, y, th = P[-1]
        if rng.random() < 0.3: th = wrap(th + rng.choice([np.pi / 2, -np.pi / 2]))
        nx, ny = x + np.cos(th), y + np.sin(th)
        if abs(nx) > area or abs(ny) > area: th = wrap(th + np.pi / 2); nx, ny = x + np.cos(th), y + np.sin(th)
        if abs(nx) > area or abs(ny) > area: th = wrap(th + np.pi); nx, ny = x + np.cos(th), y + np.sin(th)
        P.append([nx, ny, th])
    P = np.array(P); inf = (1 / s_xy**2,) * 2 + (1 / s_th**2,); sig = np.array([s_xy, s_xy, s_th])

    def build(with_false):
        b = Builder(seed); b.rng = np.random.default_rng(seed + 1000)
        for k in range(n): b.pose(k, *P[k])
        od = lambda i, j: b.odom_raw(i, j, relative(P[i], P[j]) + b.rng.normal(size=3) * sig, inf)      # noqa: E731
        for k in range(n - 1): od(k, k + 1)
        r2 = np.random.default_rng(seed + 2000); nc = 0
        for i in range(n):
            for j in range(i + 12, n):
                if np.hypot(*(P[i, :2] - P[j, :2])) <= 1.01 and r2.random() < 0.5: od(i, j); nc += 1
        if with_false:
            r3 = np.random.default_rng(seed + 3000)
            for _ in range(max(3, int(round(false_fraction * nc)))):
                i = int(r3.integers(0, n - 20)); j = int(r3.integers(i + 15, n))
                b.odom_raw(i, j, [r3.uniform(-3, 3), r3.uniform(-3, 3), r3.uniform(-1.5, 1.5)], inf)
        b.fixed = [0]; return b.graph("zeros")
    return build(False), build(True)


def start(g):
    """g from the odometry-tree start: init_guess.initialise over its consecutive-id edges."""
    z = g.copy()
    z.v_pos[:], _ = init_guess.initialise(z, init_guess.consecutive_mask(g))
    return z


def chain_exempt(g):
    """(kernels, entry): the consecutive-id ODOM edges (the odometry chain) exempt, every other edge left to its class."""
    return ["none"], init_guess.consecutive_mask(g).astype(np.int64)
