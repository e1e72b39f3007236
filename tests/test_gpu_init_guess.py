"""tsgo_init_estimates on the device (`-m gpu`, f64): every shape at which the kernels can go wrong against the sequential restatement
(tests/init_guess.py), the state the call leaves, the effect it exists for (Levenberg-Marquardt from zeros hits its cap, from the tree's
estimates it converges), the edge report after an odometry-only initialisation, and the errors.

Bound of the vertex comparison, 1e-9 absolute on x, y and the wrapped angle difference: the builders keep extents <= 100 and depths <= 5 000,
so composing the same transforms in another association (pointer jumping against parent-to-child) differs by <~ depth * 2^-53 * extent
~ 6e-11, inverting M^-1 back is of the same size, and the landmark mean of <= 9 terms adds ~ 1e-13."""
import functools

import numpy as np
import pytest

from tests import init_guess, lm_rules
from toyslam_amd import _lib
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu

TOL = 1e-9
CASES = init_guess.cases()


@functools.lru_cache(maxsize=None)
def _reference(name):
    g, mask, poses, lms = CASES[name]
    v, st = init_guess.initialise(g, mask, poses, lms)
    return v, st, init_guess.written(g, mask, poses, lms)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_restatement(name):
    g, mask, poses, lms = CASES[name]
    ref_v, ref_st, wr = _reference(name)
    o = HipOptimizer(pcg_rel_tol=1e-12)
    try:
        o.set_graph(g)
        v0 = o.vertices()
        st = o.init_estimates(mask, poses=poses, landmarks=lms)
        v1 = o.vertices()
        st2 = o.init_estimates(mask, poses=poses, landmarks=lms)
        v2 = o.vertices()
    finally:
        o.close()
    d = init_guess.vertex_diff(v1, ref_v, g.v_type)
    print(name, {k: st[k] for k in init_guess.STAT_KEYS}, "max diff %.3g" % d, "ms tree %.3f device %.3f" % (st["ms_tree"], st["ms_device"]))
    for k in init_guess.STAT_KEYS:
        assert st[k] == ref_st[k], (k, st[k], ref_st[k])
        assert st2[k] == ref_st[k], (k, st2[k], ref_st[k])
    if poses:
        assert st["rounds"] == int(np.ceil(np.log2(st["depth_max"] + 1))) and st["tree_edges"] == st["poses_set"]
    assert d <= TOL
    assert wr.sum() == st["poses_set"] + st["landmarks_set"]
    assert np.array_equal(v1[~wr], v0[~wr])                               # roots, fixed vertices, untouched landmarks: bit for bit
    assert np.array_equal(v1[~wr][:, :2], g.v_pos[~wr][:, :2])
    assert np.array_equal(v2, v1)                                         # the second call is a fixed point


# ---- state ----------------------------------------------------------------------------------------------------------------------------
def _lin_close(a, b):
    (d1, g1, c1), (d2, g2, c2) = a, b
    assert abs(c1 - c2) <= 1e-9 * abs(c2), (c1, c2)
    assert np.abs(d1 - d2).max() <= 1e-9 * np.abs(d2).max()
    assert np.abs(g1 - g2).max() <= 1e-9 * np.abs(g2).max()


@pytest.mark.parametrize("precond", ["amg", "jacobi"])
@pytest.mark.parametrize("warm", [False, True])
def test_state_after_the_call_is_that_of_a_fresh_handle_with_those_estimates(precond, warm):
    g = lm_rules.synth_600()
    kw = dict(pcg_rel_tol=1e-12, preconditioner=precond, odom_jacobian="analytic")
    o = HipOptimizer(warm_requests=warm, **kw)
    f = HipOptimizer(**kw)
    try:
        if warm:
            o.set_graph(g); o.optimize(3)      # a first request leaves a history; the second carries it (history_carried would be 1)
        o.set_graph(init_guess.zeroed(g))
        st = o.init_estimates()
        v = o.vertices()
        lin = o.linearize()
        h = g.copy(); h.v_pos[:] = v
        f.set_graph(h)
        _lin_close(lin, f.linearize())
        assert st["poses_set"] == g.n_poses - 1 and st["landmarks_set"] + st["landmarks_unobserved"] == g.n_landmarks
        r, rf = o.optimize(3), f.optimize(3)
        assert r["history_carried"] == 0
        np.testing.assert_allclose(r["chi2"], rf["chi2"], rtol=1e-9)
    finally:
        o.close(); f.close()


def test_the_robust_setting_survives():
    g = lm_rules.synth_600()
    o = HipOptimizer()
    try:
        o.set_robust(odom=("cauchy", 2.0))
        o.set_graph(init_guess.zeroed(g)); o.init_estimates()
        assert o.robust["odom"] == ("cauchy", 2.0)
    finally:
        o.close()


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
TRIALS = 30


def _lm(g, init=None):
    o = HipOptimizer(rules="lm", odom_jacobian="analytic", pcg_rel_tol=1e-12)
    try:
        o.set_graph(g)
        if init is not None:
            o.init_estimates(init[0])
        return o.optimize(TRIALS)
    finally:
        o.close()


@pytest.mark.parametrize("which", ["synth_600", "loop_closure"])
def test_levenberg_marquardt_from_zeros_needs_the_call(which):
    g = lm_rules.synth_600() if which == "synth_600" else lm_rules.loop_closure_pose_graph()
    z = init_guess.zeroed(g)
    ref = _lm(g)
    cold = _lm(z)
    print(which, "generator", ref["iters"], ref["stop"], "%.10f" % ref["chi2_last"], "| zeros", cold["iters"], cold["stop"], "%.6f" % cold["chi2_last"])
    runs = {}
    for name, mask in (("all", None), ("consecutive", init_guess.consecutive_mask(g))):
        runs[name] = r = _lm(z, init=(mask,))
        print(which, "tree", name, r["iters"], r["stop"], "%.10f" % r["chi2_last"], "rel", abs(r["chi2_last"] - ref["chi2_last"]) / ref["chi2_last"])
    assert ref["stop"] == "converged"
    assert cold["stop"] == "cap"
    for name, r in runs.items():
        assert r["stop"] == "converged", name
        assert abs(r["chi2_last"] - ref["chi2_last"]) <= 1e-5 * ref["chi2_last"], name


def test_edge_report_after_an_odometry_only_initialisation_shows_the_false_closure():
    g, mask, planted = init_guess.false_closure()
    o = HipOptimizer()
    try:
        o.set_graph(g)
        st = o.init_estimates(mask)
        rec, summary = o.edge_report()
    finally:
        o.close()
    print("planted", planted, "s", rec["s"][planted], "next", np.sort(rec["s"][g.e_type == 0])[-2], st)
    assert summary["odom"]["s_max_edge"] == planted
    assert rec["s"][planted] > 100 * np.sort(rec["s"][g.e_type == 0])[-2]      # far above the noise of every other ODOM edge


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def _raw(o, what, mask, n_mask):
    rc = o.lib.tsgo_init_estimates(o.h, what, None if mask is None else mask.ctypes.data, n_mask, None)
    return rc, o.lib.tsgo_last_error().decode()


def test_errors_leave_the_handle_usable():
    g, mask, _p, _l = CASES["closures_masked"]
    lib = _lib.hip_lib()
    assert lib.tsgo_init_estimates(None, 0, None, 0, None) < 0 and "null handle" in lib.tsgo_last_error().decode()
    o = HipOptimizer()
    try:
        rc, msg = _raw(o, 0, None, 0)
        assert rc < 0 and "no graph set" in msg
        o.set_graph(g)
        v0 = o.vertices()
        for what in (-1, 4):
            rc, msg = _raw(o, what, None, 0)
            assert rc < 0 and "what" in msg
        short = np.ones(g.n_edges - 1, np.uint8)
        rc, msg = _raw(o, 0, short, len(short))
        assert rc < 0 and "n_mask" in msg
        assert np.array_equal(o.vertices(), v0)                             # nothing was launched
        with pytest.raises(ValueError):
            o.init_estimates(poses=False, landmarks=False)
        st = o.init_estimates(mask)                                          # ... and the handle works
        ref_v, ref_st = init_guess.initialise(g, mask)
        assert st["poses_set"] == ref_st["poses_set"] and init_guess.vertex_diff(o.vertices(), ref_v, g.v_type) <= TOL
    finally:
        o.close()
    f32 = HipOptimizer(precision=32)
    try:
        f32.set_graph(g)
        rc, msg = _raw(f32, 0, None, 0)
        assert rc < 0 and "precision = 64" in msg
    finally:
        f32.close()
    shard = HipOptimizer(rank=0, world=2)
    try:
        rc, msg = _raw(shard, 0, None, 0)
        assert rc < 0 and "world > 1" in msg
    finally:
        shard.close()
