"""Helpers of the vertex-edit tests (tsgo_set_fixed / tsgo_get_fixed / tsgo_set_estimates, include/tsgo.h): the graphs a FRESH handle is
given in place of an edit, and what tsgo_get_fixed must return.  The bitwise comparison is edge_info.assert_same_linearisation."""
import numpy as np

from tests.edge_info import assert_same_linearisation  # noqa: F401  (the tests take it from here)


def counts(g):
    """Occurrences of every vertex in g.fixed, in vertex order: what fixed_counts() returns after a plain set_graph(g)."""
    at = {int(v): k for k, v in enumerate(g.v_id)}
    out = np.zeros(len(g.v_id), np.int32)
    for f in g.fixed:
        out[at[int(f)]] += 1
    return out


def refixed(g, ids, count=1):
    """g with the CANONICAL fixed list after set_fixed(ids, count): the listed ids take their count (0 releases), the others keep theirs;
    the list is the vertices with count > 0 in vertex order, each repeated count times."""
    ids = np.asarray(ids).reshape(-1)
    count = np.broadcast_to(np.asarray(count, np.int64).reshape(-1), ids.shape) if np.size(count) == 1 else np.asarray(count, np.int64).reshape(-1)
    assert len(count) == len(ids) and len(set(int(i) for i in ids)) == len(ids)
    at = {int(v): k for k, v in enumerate(g.v_id)}
    c = counts(g)
    for i, k in zip(ids, count):
        c[at[int(i)]] = k
    out = g.copy()
    out.fixed = np.ascontiguousarray(np.repeat(g.v_id, c), np.uint32)
    return out


def moved(g, ids, pos):
    """g with the estimates of the listed ids replaced by pos (n, 3); a landmark keeps 0 in its third entry (ids=None: every vertex)."""
    out = g.copy()
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    if ids is None:
        rows = np.arange(len(g.v_id))
    else:
        at = {int(v): k for k, v in enumerate(g.v_id)}
        rows = np.array([at[int(i)] for i in np.asarray(ids).reshape(-1)], np.int64)
    assert len(rows) == len(pos)
    out.v_pos[rows] = pos
    out.v_pos[out.v_type == 1, 2] = 0.0
    return out
