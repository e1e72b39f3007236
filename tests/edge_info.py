"""Helpers of the edge-information tests (tsgo_set_edge_information / tsgo_get_edge_information, include/tsgo.h): edited graphs, what
the get call must return, edit lists over a graph's classes, and the restatement facts of the outlier scenario (tests/robust.py) that
tests/test_edge_info_cpu.py pins and tests/test_gpu_edge_info.py relies on."""
import functools

import numpy as np

from tests import edge_report, robust

TWO_AXES = (1, 2, 4)          # LM, virtual landmark, landmark prior: the third entry of e_inf is not used
FLAG_BELOW = 0.01             # a report weight under this flags an edge (the issue's threshold)


def edited(g, e_inf, edges=None):
    """g with the listed e_inf rows replaced (edges=None: all of them)."""
    out = g.copy()
    e_inf = np.asarray(e_inf, np.float64).reshape(-1, 3)
    if edges is None:
        out.e_inf[:] = e_inf
    else:
        out.e_inf[np.asarray(edges, np.int64)] = e_inf
    return out


def held(g, precision=64):
    """What edge_information() returns for a handle of that precision holding g: entries a class does not use are 0, an f32 handle
    holds the float-rounded values."""
    w = g.e_inf.copy()
    w[np.isin(g.e_type, TWO_AXES), 2] = 0
    return w.astype(np.float32).astype(np.float64) if precision == 32 else w


def every_class(g, per_class=3, seed=0):
    """(edges, e_inf): `per_class` edges of every class the graph holds, shuffled, with new values — one of them all zeros, one with a
    single zero axis, the others the old values scaled by factors that are not representable in f32."""
    rng = np.random.default_rng(seed)
    edges = np.concatenate([rng.choice(np.where(g.e_type == t)[0], min(per_class, int((g.e_type == t).sum())), replace=False) for t in range(5)])
    edges = rng.permutation(edges).astype(np.int64)
    vals = g.e_inf[edges] * rng.uniform(0.1, 3.0, size=(len(edges), 3)) + rng.uniform(0.0, 0.5, size=(len(edges), 3))
    vals[0] = 0
    vals[1, 1] = 0
    return edges, vals


def assert_same_linearisation(a, b, what=""):
    """Two (diag, grad, chi2) of tsgo_linearize, bit for bit."""
    for x, y, name in zip(a, b, ("diag", "grad", "chi2")):
        x, y = np.asarray(x), np.asarray(y)
        assert np.array_equal(x, y), "%s: %s differs, largest difference %.3e" % (what, name, np.abs(x - y).max())


# ---- the outlier scenario: what the Cauchy run leaves, what its report flags, and the finish under the plain cost ----------------------
@functools.lru_cache(maxsize=None)
def scenario_after_cauchy():
    """(graph with the false closures at the estimates robust.dense_lm reaches under SCENARIO["robust"], report weights there)."""
    from tests.test_robust_cpu import scenario_references
    g, _clean, _default, cauchy = scenario_references()
    at = g.copy(); at.v_pos[:] = cauchy["v_pos"]
    return at, edge_report.records(at, robust.SCENARIO["robust"])[:, 5]


def scenario_false_edges():
    n_clean = len(robust.scenario_clean().e_type)
    return np.arange(n_clean, len(robust.scenario().e_type))
