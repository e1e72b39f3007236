"""tsgo_sample_marginals (include/tsgo.h) restated in numpy, sharing nothing with the product's arithmetic.

  noise     Philox4x32-10 and Box-Muller written out here (philox: Python integers, one counter; philox_words / normals: numpy, many)
  e, A, B   types 0 - 2 from independent.Linearisation (through robust.Linearisation) under lm_rules._Jacobians(...), the priors from
            gate.linearise; weights a = w inf from robust.rho_w
  G         the stacked square-root rows sqrt(a_j) J_e[j, :] of every edge and sqrt(gamma_v) e_axis of every gauge term, so that
            H = G^T G = sum J^T (w Omega) J + gauge and b_k = G^T xi_k have the covariance H by construction
  delta_k   np.linalg.solve(H, b_k), dense

Unknowns are packed in vertex order, 3 per pose and 2 per landmark (priors.unpack)."""
import math

import numpy as np

from tests import edge_info, gate, independent, lm_rules, priors, robust

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
DOF = gate.DOF
KNOWN_ANSWERS = [      # Random123 kat_vectors, philox4x32-10: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK, MASK, MASK, MASK), (MASK, MASK), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox(counter, key):
    """Philox4x32-10 of one counter (4 words) under one key (2 words), in Python integers."""
    c0, c1, c2, c3 = (int(x) & MASK for x in counter)
    k0, k1 = (int(x) & MASK for x in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_words(seed, tag, index, k):
    """The four words of noise(seed, tag, index, k) for arrays index, k (broadcast): uint64 arrays holding 32-bit values, (..., 4)."""
    index, k = np.broadcast_arrays(np.asarray(index, np.uint64), np.asarray(k, np.uint64))
    m = np.uint64(MASK); s32 = np.uint64(32)
    c0, c1, c2, c3 = index & m, np.full(index.shape, tag, np.uint64), k & m, np.zeros(index.shape, np.uint64)
    k0, k1 = np.uint64(int(seed) & MASK), np.uint64((int(seed) >> 32) & MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return np.stack([c0, c1, c2, c3], axis=-1)


def box_muller(words):
    """(..., 4) words -> (..., 4) normals."""
    u = (words.astype(np.float64) + 0.5) / 4294967296.0
    r01, r23 = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    a01, a23 = 2.0 * math.pi * u[..., 1], 2.0 * math.pi * u[..., 3]
    return np.stack([r01 * np.cos(a01), r01 * np.sin(a01), r23 * np.cos(a23), r23 * np.sin(a23)], axis=-1)


def normals(seed, tag, index, k):
    return box_muller(philox_words(seed, tag, index, k))


class System:
    """G, H = G^T G and the bookkeeping of one graph at its estimates, under a robust setting and an ODOM Jacobian kind."""

    def __init__(self, g, setting=None, jacobian="constant"):
        setting = robust.full(setting)
        V, E = len(g.v_id), len(g.e_type)
        dims = np.where(g.v_type == 0, 3, 2)
        self.g, self.dims = g, dims
        self.off = np.concatenate([[0], np.cumsum(dims)])
        n = int(self.off[-1])
        order = np.argsort(g.v_id, kind="stable")
        pos = lambda ids: order[np.searchsorted(g.v_id[order], ids)]
        A = np.zeros((E, 3, 3)); B = np.zeros((E, 3, 3)); a = np.zeros((E, 3))
        low = np.flatnonzero(g.e_type <= 2)
        with lm_rules._Jacobians(jacobian):
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
            A[pri], a[pri] = Ap, raw * w[:, None]
        i1, i2 = pos(g.e_ids[:, 0]), pos(g.e_ids[:, 1])
        G, tags = [], []                             # every row of G and its (tag, index, axis)
        for e_ in range(E):
            for j in range(int(DOF[g.e_type[e_]])):
                row = np.zeros(n)
                sq = math.sqrt(a[e_, j])
                d1 = dims[i1[e_]]
                row[self.off[i1[e_]]:self.off[i1[e_]] + d1] += sq * A[e_, j, :d1]
                if g.e_type[e_] <= 2:
                    d2 = dims[i2[e_]]
                    row[self.off[i2[e_]]:self.off[i2[e_]] + d2] += sq * B[e_, j, :d2]
                G.append(row); tags.append((0, e_, j))
        gauge = np.zeros(V)
        for f in g.fixed:
            gauge[pos(f)] += independent.GAUGE
        for v in np.flatnonzero(gauge > 0):
            for j in range(dims[v]):
                row = np.zeros(n); row[self.off[v] + j] = math.sqrt(gauge[v])
                G.append(row); tags.append((1, int(v), j))
        self.G = np.array(G)
        self.tags = np.array(tags, np.int64)
        self.H = self.G.T @ self.G
        self.gauge = gauge

    def xi(self, seed, K):
        """(rows of G, K): the normal of every row for samples 0 .. K - 1."""
        out = np.zeros((len(self.tags), K))
        ks = np.arange(K)
        for tag in (0, 1):
            sel = np.flatnonzero(self.tags[:, 0] == tag)
            if len(sel):
                nn = normals(seed, tag, self.tags[sel, 1][:, None], ks[None, :])      # (rows, K, 4)
                out[sel] = np.take_along_axis(nn, self.tags[sel, 2][:, None, None].repeat(K, axis=1), axis=2)[..., 0]
        return out

    def samples(self, seed, K):
        """delta (K, V, 3) of the dense solve, and b (n, K)."""
        b = self.G.T @ self.xi(seed, K)
        x = np.linalg.solve(self.H, b)
        return np.stack([priors.unpack(x[:, k], self.g) for k in range(K)]), b

    def packed(self, delta):
        """(K, V, 3) -> (K, n)."""
        mask = np.arange(3)[None, :] < self.dims[:, None]
        return delta[:, mask]

    def inverse_diagonal(self):
        """diag(H^-1) as (V, 3), a landmark's third entry 0."""
        return priors.unpack(np.diag(np.linalg.inv(self.H)).copy(), self.g)


def at(g, v_pos):
    out = g.copy()
    out.v_pos[:] = v_pos
    return out


# ---- the graphs and seeds of the tests ---------------------------------------------------------------------------------------------
SEED = 20260101            # the samples test and the bitwise tests
SEED_STAT, K_STAT = 7, 512
ROBUST = robust.MIXED      # the non-default setting of the five-class graph
BOUND = 6.0                # standard errors


def five_class_graph():
    """robust.c1_five_classes with the edits of edge_info.every_class (one edge with zero information, one with a single zero axis), one
    vertex listed twice in the fixed list and a fixed landmark; c1 has landmarks with a single observation."""
    g = robust.c1_five_classes()
    edges, vals = edge_info.every_class(g)
    g = edge_info.edited(g, vals, edges)
    lm = np.flatnonzero(g.v_type == 1)
    fixed = np.array([g.fixed[0], g.fixed[0], g.v_id[lm[len(lm) // 2]]], np.uint32)
    return priors.append_edges(g, [], [], [], [], fixed=fixed), edges


def single_observation_landmarks(g):
    seen = np.bincount(g.e_ids[g.e_type == 1, 1].astype(np.int64), minlength=int(g.v_id.max()) + 1)
    return g.v_id[(g.v_type == 1) & (seen[g.v_id] == 1)]
