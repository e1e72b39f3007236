"""tsgo_edge_leverage (include/tsgo.h) restated in numpy, sharing nothing with the product's arithmetic.

  A, B, a   rebuilt as posterior.System.__init__ does: types 0 - 2 from robust.Linearisation under lm_rules._Jacobians(...), the priors
            from gate.linearise, weights a = w inf from robust.rho_w.  Under a per-edge setting (kernels, entry: tests/edge_robust.py) the
            effective kernel of every edge.
  y         A delta_first + B delta_second per sample and edge (a prior edge: A delta), from a GIVEN delta (K, V, 3) — the device's own
            samples, or the dense ones of posterior.System.samples
  C, h      (1 / K) sum y y^T, sum_j a_j C_jj;  dof_a = the number of the class's axes with a_j > 0
  exact     the same from a given Sigma = H^-1 instead of samples: C = J Sigma J^T
  gauge     sum_v gamma_v tr(C_v)

Records are (E, 8): c00 c01 c02 c11 c12 c22 h dof_a, the layout of rec_out."""
import contextlib

import numpy as np

from tests import edge_robust, gate, independent, lm_rules, posterior, priors, robust

DOF = gate.DOF
UPPER = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


class Restatement:
    def __init__(self, g, setting=None, jacobian="constant", kernels=(), entry=None):
        setting = robust.full(setting)
        V, E = len(g.v_id), len(g.e_type)
        entry = np.zeros(E, np.int64) if entry is None else np.asarray(entry)
        self.g, self.setting, self.jacobian, self.kernels, self.entry = g, setting, jacobian, kernels, entry
        self.dims = np.where(g.v_type == 0, 3, 2)
        order = np.argsort(g.v_id, kind="stable")
        pos = lambda ids: order[np.searchsorted(g.v_id[order], ids)]
        A = np.zeros((E, 3, 3)); B = np.zeros((E, 3, 3)); a = np.zeros((E, 3))
        low = np.flatnonzero(g.e_type <= 2)
        with lm_rules._Jacobians(jacobian), self.per_edge():
            lin = robust.Linearisation(priors.without_priors(g), setting)
        A[low], B[low], a[low] = lin.A, lin.B, lin.w
        pri = np.flatnonzero(g.e_type >= 3)
        if len(pri):
            e, Ap, _B = gate.linearise(g, g.v_pos, gate.edges_of(g, pri))
            raw = g.e_inf[pri].copy()
            raw[g.e_type[pri] == 4, 2] = 0
            s = (raw * e * e).sum(axis=1)
            w = np.ones(len(pri))
            for t in (3, 4):
                k = g.e_type[pri] == t
                w[k] = robust.rho_w(setting[robust.CLASSES[t]], s[k])[1]
            edge_robust._override(np.zeros(len(pri)), w, s, kernels, entry[pri])
            A[pri], a[pri] = Ap, raw * w[:, None]
        axes = np.arange(3)[None, :] < DOF[g.e_type][:, None]
        a[~axes] = 0      # (an axis the class does not use carries no weight, whatever e_inf holds there)
        self.A, self.B, self.a = A, B, a
        self.i1, self.i2 = pos(g.e_ids[:, 0]), pos(g.e_ids[:, 1])
        self.binary = g.e_type <= 2
        self.dof_a = (a > 0).sum(axis=1).astype(np.float64)
        gauge = np.zeros(V)
        for f in g.fixed:
            gauge[pos(f)] += independent.GAUGE
        self.gauge = gauge

    def per_edge(self):
        """The context in which robust.Linearisation (and with it posterior.System) sees the per-edge setting; nothing without one."""
        return edge_robust.per_edge(self.g, self.kernels, self.entry) if len(self.kernels) else contextlib.nullcontext()

    def system(self):
        """posterior.System of the same graph, setting and Jacobians (a per-edge setting: on edges of types 0 - 2 only)."""
        assert not self.entry[self.g.e_type >= 3].any()
        with self.per_edge():
            return posterior.System(self.g, self.setting, self.jacobian)

    def _pack(self, C):
        h = (self.a * np.diagonal(C, axis1=1, axis2=2)).sum(axis=1)
        return np.column_stack([C[:, i, j] for i, j in UPPER] + [h, self.dof_a])

    def y(self, delta):
        """(K, E, 3)."""
        y = np.einsum("eij,kej->kei", self.A, delta[:, self.i1])
        y[:, self.binary] += np.einsum("eij,kej->kei", self.B[self.binary], delta[:, self.i2[self.binary]])
        return y

    def records(self, delta):
        """(E, 8) from samples delta (K, V, 3), a landmark's third entry 0."""
        y = self.y(np.asarray(delta, np.float64))
        return self._pack(np.einsum("kei,kej->eij", y, y) / len(delta))

    def exact(self, Sigma):
        """(E, 8) from Sigma (n, n) in packed vertex order (3 per pose, 2 per landmark)."""
        V = len(self.dims)
        off = np.concatenate([[0], np.cumsum(self.dims)])
        rows = np.concatenate([3 * v + np.arange(self.dims[v]) for v in range(V)])
        S = np.zeros((3 * V, 3 * V))
        S[np.ix_(rows, rows)] = Sigma
        assert off[-1] == Sigma.shape[0]
        S = S.reshape(V, 3, V, 3)
        blk = lambda p, q: S[p, :, q, :]      # (E, 3, 3)
        A, B = self.A, np.where(self.binary[:, None, None], self.B, 0.0)
        i1, i2 = self.i1, self.i2
        C = np.einsum("eia,eab,ejb->eij", A, blk(i1, i1), A) + np.einsum("eia,eab,ejb->eij", A, blk(i1, i2), B)
        C += np.einsum("eia,eab,ejb->eij", B, blk(i2, i1), A) + np.einsum("eia,eab,ejb->eij", B, blk(i2, i2), B)
        return self._pack(C)

    def h_gauge(self, delta):
        """sum_v gamma_v tr(C_v), C_v = (1 / K) sum delta_v delta_v^T."""
        return float((self.gauge[:, None] * (np.asarray(delta) ** 2).mean(axis=0)).sum())

    def h_gauge_exact(self, Sigma):
        off = np.concatenate([[0], np.cumsum(self.dims)])
        d = np.diag(Sigma)
        return float(sum(self.gauge[v] * d[off[v]:off[v + 1]].sum() for v in np.flatnonzero(self.gauge > 0)))

    def weighted_rows(self, rec):
        """a_j C_jj of every (edge, axis) with a_j > 0, in edge order: the summands of h."""
        diag = rec[:, [0, 3, 5]]
        return (self.a * diag)[self.a > 0]


def fold(rec, e_type):
    """The per-class sums of tsgo_leverage_stats from records: edges, h_sum, dof_sum (in input edge order, as the host folds them)."""
    edges = np.zeros(5, np.int64); h = np.zeros(5); dof = np.zeros(5)
    for e in range(len(rec)):
        c = int(e_type[e])
        edges[c] += 1; h[c] += rec[e, 6]; dof[c] += rec[e, 7]
    return edges, h, dof


def class_scale(rec, e_type):
    """Per edge: the largest |C| entry over the edges of its class."""
    out = np.zeros(len(rec))
    for t in range(5):
        k = e_type == t
        if k.any():
            out[k] = np.abs(rec[k, :6]).max()
    return out
