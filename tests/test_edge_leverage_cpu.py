"""tsgo_edge_leverage without a GPU: the restatement itself (tests/leverage.py) — its trace identities, the edges whose leverage is
known in closed form, the statistical bound of tests/test_gpu_edge_leverage.py at the seed and K that test uses (which makes it a
condition the reference meets), and the zero-information cases of the five-class graph."""
import functools

import numpy as np
import pytest

from tests import leverage, posterior, util

K_IDENTITY = 64


@functools.lru_cache(maxsize=None)
def _c1(jacobian):
    """c1 at its start: the restatement, the dense system, Sigma = H^-1."""
    R = leverage.Restatement(util.c1_arrays(), None, jacobian)
    S = R.system()
    return R, S, np.linalg.inv(S.H)


@functools.lru_cache(maxsize=None)
def c1_statistics():
    """(restatement, sampled records, exact records, sampled and exact gauge rows) at posterior.SEED_STAT, K_STAT, analytic Jacobians."""
    R, S, Sigma = _c1("analytic")
    d, _b = S.samples(posterior.SEED_STAT, posterior.K_STAT)
    fixed = np.flatnonzero(R.gauge > 0)
    off = np.concatenate([[0], np.cumsum(R.dims)])
    g_smp = np.concatenate([R.gauge[v] * (d[:, v, :R.dims[v]] ** 2).mean(axis=0) for v in fixed])
    g_ref = np.concatenate([R.gauge[v] * np.diag(Sigma)[off[v]:off[v + 1]] for v in fixed])
    return R, R.records(d), R.exact(Sigma), g_smp, g_ref


# ---- 1. trace identities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jacobian", ["constant", "analytic"])
def test_trace_identities_on_c1(jacobian):
    R, S, Sigma = _c1(jacobian)
    n = S.H.shape[0]
    d, _b = S.samples(posterior.SEED_STAT, K_IDENTITY)
    x = S.packed(d)
    q = float(np.einsum("kn,nm,km->k", x, S.H, x).mean())
    t = float(R.records(d)[:, 6].sum()) + R.h_gauge(d)
    print("%s: sum h + gauge %.6f, mean delta^T H delta %.6f" % (jacobian, t, q))
    assert abs(t - q) <= 1e-12 * q
    rec = R.exact(Sigma)
    assert abs(rec[:, 6].sum() + R.h_gauge_exact(Sigma) - n) <= 1e-9 * n
    assert (rec[:, 6] >= -1e-9).all() and (rec[:, 6] <= rec[:, 7] + 1e-9).all()      # h in [0, dof]


# ---- 2. single-observation landmarks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jacobian", ["constant", "analytic"])
def test_the_only_observation_of_a_landmark_has_full_leverage(jacobian):
    R, _S, Sigma = _c1(jacobian)
    g = R.g
    single = posterior.single_observation_landmarks(g)
    k = np.flatnonzero((g.e_type == 1) & np.isin(g.e_ids[:, 1], single))
    assert len(k) == len(single) > 0
    rec = R.exact(Sigma)
    assert np.abs(rec[k, 6] - 2.0).max() <= 1e-9 and (rec[k, 7] == 2).all()
    others = np.setdiff1d(np.flatnonzero(g.e_type == 1), k)
    assert rec[others, 6].max() < 2.0 - 1e-6


# ---- 3. the 6-sigma bound at the seed and K of the GPU test --------------------------------------------------------------------------
def test_statistical_bound_holds_for_the_restatement():
    R, smp, ref, g_smp, g_ref = c1_statistics()
    K = posterior.K_STAT
    ratio = np.concatenate([R.weighted_rows(smp) / R.weighted_rows(ref), g_smp / g_ref])
    bound = posterior.BOUND * np.sqrt(2.0 / K)
    print("%d rows, a_j C_jj over its exact value in [%.3f, %.3f], bound 1 +- %.3f" % (len(ratio), ratio.min(), ratio.max(), bound))
    assert len(ratio) == int((R.a > 0).sum()) + 3      # no row left out: every weighted axis of every edge, the fixed pose's three
    assert np.abs(ratio - 1).max() <= bound


# ---- 4. zero information -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jacobian", ["constant", "analytic"])
def test_zero_information_edges_of_the_five_class_graph(jacobian):
    g, edges = posterior.five_class_graph()
    R = leverage.Restatement(g, posterior.ROBUST, jacobian)
    S = R.system()
    d, _b = S.samples(posterior.SEED, 21)
    for rec, slack in ((R.records(d), posterior.BOUND * np.sqrt(2.0 / 21)), (R.exact(np.linalg.inv(S.H)), 1e-9)):
        zero, one = int(edges[0]), int(edges[1])
        assert (g.e_inf[zero] == 0).all() and g.e_inf[one, 1] == 0 and g.e_inf[one, 0] > 0
        dof = int(leverage.DOF[g.e_type[zero]])
        assert rec[zero, 6] == 0 and rec[zero, 7] == 0
        assert rec[zero, [0, 3]].min() > 0 and (dof == 2 or rec[zero, 5] > 0)      # its C is still there
        assert rec[one, 7] == leverage.DOF[g.e_type[one]] - 1
        assert rec[one, 6] == (R.a[one] * rec[one, [0, 3, 5]]).sum() and 0 < rec[one, 6] <= rec[one, 7] * (1 + slack)
        k2 = leverage.DOF[g.e_type] == 2
        assert not rec[k2][:, [2, 4, 5]].any()
        untouched = np.setdiff1d(np.arange(len(g.e_type)), edges[:2])
        assert (rec[untouched, 7] == leverage.DOF[g.e_type[untouched]]).all()
