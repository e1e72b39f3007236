"""Robust kernels per edge (tsgo_set_edge_robust, include/tsgo.h) on the device (`-m gpu`): an inactive setting changes no bit, a palette
that repeats the class kernels gives the class path's bits, and linearisation, one solve, the rules = 2 and rules = 3 loops, the edge report,
marginals and samples under a mixed palette against the numpy restatement (tests/edge_robust.py); the setting's lifetime and its errors.
Graphs: the 150-pose c1 golden widened to all five edge classes (robust.c1_five_classes), an 8-pose chain with one closure and one
landmark (slices that are mostly padding) and the outlier scenario of tests/robust.py.

Tolerances are those of the same quantities under the class kernels: tests/test_gpu_robust.py (blocks and gradient 1e-12 of the largest
entry, a single chi^2 1e-11, chi^2 traces 1e-9, the predicted decrease 1e-8, covariances 1e-8 of the largest entry), tests/test_gpu_dogleg.py
(g'g and g'Hg 1e-8) and tests/test_gpu_edge_report.py (F64)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import edge_report, edge_robust, init_guess, lm_rules, robust
from tests.test_gpu_edge_report import F64
from tests.test_gpu_robust import VARIANTS
from toyslam_amd import _lib
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu

PALETTE = ["none", ("cauchy", 0.8), ("geman_mcclure", 2.0)]
CLASS_PALETTE = [robust.full(robust.MIXED)[c] for c in robust.CLASSES]      # entry e_type + 1 = the class's kernel of MIXED


@functools.lru_cache(maxsize=None)
def _graph(vlm=True, with_priors=True):
    return robust.c1_five_classes(vlm, with_priors)


@functools.lru_cache(maxsize=None)
def _small():
    """8 poses on a chain, one closure, one landmark seen twice, from random estimates: every table is one slice of mostly padding."""
    b = init_guess.Builder(21)
    for k, p in enumerate(init_guess._walk(8, step=0.5, turn=0.15)):
        b.pose(k, *p)
    for k in range(7):
        b.odom(k, k + 1, noise=0.05)
    b.odom(0, 7, noise=0.2)
    b.landmark(100, 2.0, 1.0)
    b.lm(2, 100); b.lm(5, 100)
    b.fixed = [0]
    return b.graph("random")


def _mod4(g):
    return np.arange(len(g.e_type)) % 4


def _handle(setting=None, **kw):
    kw.setdefault("pcg_rel_tol", 1e-12)
    o = HipOptimizer(**kw)
    if setting is not None:
        o.set_robust(**setting)
    return o


def _run(g, prepare, n=5, **kw):
    """(linearize(), optimize(n), vertices()) of a fresh handle on g after prepare(handle)."""
    o = _handle(**kw)
    try:
        o.set_graph(g)
        prepare(o)
        return o.linearize(), o.optimize(n), o.vertices()
    finally:
        o.close()


def _assert_same_bits(a, b, what):
    (la, ra, va), (lb, rb, vb) = a, b
    for x, y in zip(la, lb):
        np.testing.assert_array_equal(x, y, err_msg=what)
    np.testing.assert_array_equal(ra["chi2"], rb["chi2"], err_msg=what); np.testing.assert_array_equal(ra["cg_iters"], rb["cg_iters"], err_msg=what)
    np.testing.assert_array_equal(va, vb, err_msg=what)


def _assert_lin(got, ref, what):
    (d, g, c), (d0, g0, c0) = got, ref
    ed = (np.abs(d - d0).max(1) / np.abs(d0).max(1)).max(); eg = np.abs(g - g0).max() / np.abs(g0).max(); ec = abs(c - c0) / c0
    print("%s: blocks %.2e of the block's largest entry, gradient %.2e of the largest entry, chi2 %.2e relative (chi2 %.6f)" % (what, ed, eg, ec, c0))
    assert ed <= 1e-12 and eg <= 1e-12 and ec <= 1e-11, what


# ---- 1. inactive: no bit changes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["c1", "small"])
def test_an_inactive_setting_changes_no_bit(graph):
    g = _graph() if graph == "c1" else _small()

    def zero_mask(o):
        st = o.set_edge_robust(PALETTE, np.zeros(len(g.e_type), np.uint8))
        assert not st["active"] and st["edges_by_entry"][0] == len(g.e_type)

    def set_then_cleared(o):
        assert o.set_edge_robust(PALETTE, _mod4(g))["active"]
        assert not o.clear_edge_robust()["active"]
        kernels, entry = o.edge_robust
        assert kernels == [] and not entry.any()

    never = _run(g, lambda o: None)
    _assert_same_bits(never, _run(g, zero_mask), "all-zero mask")
    _assert_same_bits(never, _run(g, set_then_cleared), "set, then cleared")


# ---- 2. a palette that repeats the class kernels: the class path's bits ------------------------------------------------------------------------
@pytest.mark.parametrize("jacobian", ["constant", "analytic"])
@pytest.mark.parametrize("lanes", [1, 8])
def test_a_palette_equal_to_the_class_kernels_gives_the_class_paths_bits(lanes, jacobian):
    for g in (_graph(), _small()):
        kw = dict(lanes_per_pose=lanes, lanes_per_lm=lanes, odom_jacobian=jacobian)
        a = _run(g, lambda o: o.set_robust(**robust.MIXED), **kw)
        b = _run(g, lambda o: o.set_edge_robust(CLASS_PALETTE, g.e_type + 1), **kw)
        _assert_same_bits(a, b, "%d edges, lanes %d, %s" % (len(g.e_type), lanes, jacobian))


# ---- 3. against the restatement -----------------------------------------------------------------------------------------------------------
def test_linearisation_matches_the_restatement():
    cases = [(_graph(vlm, pri), lanes, jac, "vlm %d priors %d" % (vlm, pri)) for (vlm, pri), lanes, jac in VARIANTS]
    cases += [(_small(), lanes, jac, "small") for lanes in (1, 8) for jac in ("constant", "analytic")]
    for g, lanes, jac, name in cases:
        o = _handle(lanes_per_pose=lanes, lanes_per_lm=lanes, odom_jacobian=jac)
        try:
            o.set_graph(g)
            st = o.set_edge_robust(PALETTE, _mod4(g))
            got = o.linearize()
        finally:
            o.close()
        assert st["active"] and list(st["edges_by_entry"][:4]) == [int((_mod4(g) == k).sum()) for k in range(4)] and st["edges_by_entry"][4:].sum() == 0
        assert sum(st["overridden_by_class"].values()) == int((_mod4(g) > 0).sum())
        with lm_rules._Jacobians(jac):
            ref = edge_robust.linearisation(g, None, PALETTE, _mod4(g))
        _assert_lin(got, ref, "%s lanes %d %s" % (name, lanes, jac))


def test_solve_step_solves_the_restated_dense_system():
    g = _graph()
    H, b, chi, _off = edge_robust.dense_system(g, robust.MIXED, PALETTE, _mod4(g))
    o = _handle(robust.MIXED)
    try:
        o.set_graph(g); o.set_edge_robust(PALETTE, _mod4(g)); s = o.solve_step()
    finally:
        o.close()
    mask = np.arange(3)[None, :] < np.where(g.v_type == 0, 3, 2)[:, None]
    res = np.linalg.norm(H @ s["delta"][mask] - b) / np.linalg.norm(b)
    print("||H delta - b|| / ||b|| = %.2e, %d PCG iterations" % (res, s["cg_iters"]))
    assert res < 1e-9 and abs(s["chi2"] - chi) <= 1e-11 * chi


# ---- 4. rules = 2 and rules = 3 on the outlier scenario, the chain exempt and Cauchy 1.0 on the class ------------------------------------------
def test_rules_2_with_the_chain_exempt_matches_the_dense_loop():
    sc = robust.SCENARIO
    g = robust.scenario()
    kernels, entry = edge_robust.chain_exempt(g)
    ref = edge_robust.dense_lm(g, sc["robust"], kernels, entry, sc["iterations"], lambda0=sc["lambda0"])
    o = _handle(sc["robust"], rules="lm", odom_jacobian="analytic", lm_lambda0=sc["lambda0"])
    try:
        o.set_graph(g); o.set_edge_robust(kernels, entry); r = o.optimize(sc["iterations"])
    finally:
        o.close()
    print("%d trials (restatement %d), %d rejected, %s (restatement %s)" % (r["iters"], ref["iters"], r["rejected"], r["stop"], ref["stop"]))
    assert (r["iters"], r["stop"]) == (ref["iters"], ref["stop"])
    print("chi2 rel %.2e, chi2_trial rel %.2e, pred rel %.2e" % (np.abs(r["chi2"] / ref["chi2"] - 1).max(), np.abs(r["lm_chi2_trial"] / ref["chi2_trial"] - 1).max(),
                                                               np.abs(r["lm_pred"] / ref["pred"] - 1).max()))
    np.testing.assert_allclose(r["chi2"], ref["chi2"], rtol=1e-9)
    np.testing.assert_allclose(r["lm_chi2_trial"], ref["chi2_trial"], rtol=1e-9)
    np.testing.assert_allclose(r["lm_pred"], ref["pred"], rtol=1e-8)
    acc = np.where((r["lm_gain"] > 0) & (r["lm_pred"] > 0))[0]
    acc = acc[acc + 1 < r["iters"]]
    assert len(acc) >= 2
    np.testing.assert_allclose(r["lm_chi2_trial"][acc], r["chi2"][acc + 1], rtol=1e-12)      # the chi^2 pass and the linearisation agree
    assert abs(ref["chi2"][0] - robust.dense_lm(g, sc["robust"], 1, lambda0=sc["lambda0"])["chi2"][0]) > 1e-3 * ref["chi2"][0]      # (the class-wide cost is another one)


def test_rules_3_ghg_and_gg_match_the_restated_dense_system():
    sc = robust.SCENARIO
    g = robust.scenario()
    kernels, entry = edge_robust.chain_exempt(g)
    mask = np.arange(3)[None, :] < np.where(g.v_type == 0, 3, 2)[:, None]
    o = _handle(sc["robust"], rules="dogleg", odom_jacobian="analytic")
    try:
        o.set_graph(g); o.set_edge_robust(kernels, entry)
        for trial in range(3):      # every optimize call starts with a linearisation at the estimates it finds
            cur = g.copy(); cur.v_pos[:] = o.vertices()
            r = o.optimize(1)
            with lm_rules._Jacobians("analytic"):
                H, b, chi, _off = edge_robust.dense_system(cur, sc["robust"], kernels, entry, zero_fixed=True)
            gg, gHg = float(b @ b), float(b @ (H @ b))
            print("trial %d: g'g %.9e (device) %.9e (numpy), g'Hg %.9e (device) %.9e (numpy), chi2 %.6f" % (trial, r["dl_gg"][0], gg, r["dl_gHg"][0], gHg, chi))
            assert abs(r["chi2"][0] - chi) <= 1e-11 * chi
            assert abs(r["dl_gg"][0] - gg) <= 1e-8 * gg
            assert abs(r["dl_gHg"][0] - gHg) <= 1e-8 * gHg
        assert mask.sum() == len(b)
    finally:
        o.close()


# ---- 5. the edge report -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["c1", "small"])
def test_edge_report_records_and_summary(graph):
    g = _graph() if graph == "c1" else _small()
    entry = _mod4(g)
    ref, ref_summ = edge_robust.report(g, robust.MIXED, PALETTE, entry)
    o = _handle(robust.MIXED)
    try:
        o.set_graph(g); o.set_edge_robust(PALETTE, entry)
        rec, summ = o.edge_report()
        none, only = o.edge_report(records=False)
        _d, _g, chi = o.linearize()
    finally:
        o.close()
    edge_report.assert_records(rec["all"], ref, g, *F64, what=graph)
    exempt = entry == 1
    assert np.all(rec["w"][exempt] == 1.0)
    np.testing.assert_array_equal(rec["rho"][exempt], rec["s"][exempt])
    assert none is None and only == summ                             # summary-only: the same pass without its stores
    for c in robust.CLASSES:
        a, b = summ[c], ref_summ[c]
        assert (a["edges"], a["downweighted"], a["s_max_edge"]) == (b["edges"], b["downweighted"], b["s_max_edge"]), c
        for f in ("s_sum", "rho_sum", "s_max"):
            assert abs(a[f] - b[f]) <= 1e-11 * abs(b[f]), (c, f)
    assert abs(summ["chi2"] - ref_summ["chi2"]) <= 1e-11 * ref_summ["chi2"] and abs(summ["chi2"] - chi) <= 1e-11 * chi


# ---- 6. marginals and samples ---------------------------------------------------------------------------------------------------------------
def test_marginals_and_samples_use_the_per_edge_kernels():
    g = _graph()
    entry = _mod4(g)
    ids = g.v_id[np.r_[3, 40, 151]]
    o = _handle()
    try:
        o.set_graph(g); o.set_edge_robust(PALETTE, entry)
        cov, _st = o.marginals(ids, rel_tol=1e-12)
        s1 = o.sample_marginals(4, seed=7, samples=True)
        s2 = o.sample_marginals(4, seed=7, samples=True)
        o.clear_edge_robust()
        s0 = o.sample_marginals(4, seed=7, samples=True)
    finally:
        o.close()
    H, _b, _chi, offs = edge_robust.dense_system(g, None, PALETTE, entry)
    Hi = np.linalg.inv(H)
    H0i = np.linalg.inv(robust.dense_system(g, None)[0])
    at = {int(x): i for i, x in enumerate(g.v_id)}
    for k, i in enumerate(ids):
        a = at[int(i)]; n = offs[a + 1] - offs[a]
        blk = Hi[offs[a]:offs[a + 1], offs[a]:offs[a + 1]]
        err = np.abs(cov[k, :n, :n] - blk).max() / np.abs(blk).max()
        print("vertex %d: %.2e of the block's largest entry" % (i, err))
        assert err <= 1e-8, k
        assert np.abs(H0i[offs[a]:offs[a + 1], offs[a]:offs[a + 1]] - blk).max() > 1e-3 * np.abs(blk).max()      # (the class kernels' covariance is another one)
    np.testing.assert_array_equal(s1["samples"], s2["samples"]); np.testing.assert_array_equal(s1["cov"], s2["cov"])
    assert np.abs(s1["samples"] - s0["samples"]).max() > 1e-6 * np.abs(s0["samples"]).max()


# ---- 7. lifetime --------------------------------------------------------------------------------------------------------------------------
def test_the_setting_survives_what_keeps_values_and_goes_with_set_graph():
    g = _graph()
    entry = _mod4(g).astype(np.uint8)
    moved = lm_rules.perturbed(g, seed=1, sigma_xy=0.05, sigma_th=0.01)
    other = _graph(False, True)
    want = float(edge_robust.chi2_at(g, robust.MIXED, PALETTE, entry))
    o = _handle()
    try:
        o.set_graph(g); o.set_edge_robust(PALETTE, entry)
        o.set_robust(**robust.MIXED)                                   # entry 0 follows the class setting of the moment
        chi = o.linearize()[2]
        assert abs(chi - want) <= 1e-11 * want
        o.set_edge_information(o.edge_information())                   # an edit that changes no value
        kernels, back = o.edge_robust
        assert kernels == PALETTE and np.array_equal(back, entry)
        assert o.linearize()[2] == chi
        o.init_estimates(mask=np.zeros(len(g.e_type), np.uint8), poses=True, landmarks=False)      # no usable edge: nothing moves, the solver restarts
        assert o.linearize()[2] == chi and np.array_equal(o.edge_robust[1], entry)
        o.optimize(2)
        assert o.edge_robust[0] == PALETTE and np.array_equal(o.edge_robust[1], entry)
        for graph in (moved, other):                                   # the same structure (a refill), then another one (a rebuild)
            o.set_graph(graph)
            kernels, back = o.edge_robust
            assert kernels == [] and len(back) == len(graph.e_type) and not back.any()
            got = (o.linearize(), o.optimize(3), o.vertices())
            fresh = _run(graph, lambda f: f.set_robust(**robust.MIXED), n=3)
            _assert_same_bits(got, fresh, "after set_graph")
            o.set_edge_robust(PALETTE, _mod4(graph))                   # (and the next graph drops this one too)
    finally:
        o.close()


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------------
def test_bad_calls_are_refused_with_a_message_and_change_nothing():
    g = _small()
    E = len(g.e_type)
    entry = _mod4(g).astype(np.uint8)
    o = _handle()
    lib = o.lib

    def entries(*kernels):
        ent = (_lib.tsgo_edge_robust_entry * max(1, len(kernels)))()
        for k, (kind, delta) in enumerate(kernels):
            ent[k].kernel, ent[k].delta = kind, delta
        return ent

    def attempt(n, ent, mask, n_mask, handle=None):
        rc = lib.tsgo_set_edge_robust(o.h if handle is None else handle, n, ent, mask.ctypes.data if mask is not None else None, n_mask, None)
        return rc, lib.tsgo_last_error().decode()

    good = entries((0, 0.0), (2, 0.8), (3, 2.0))
    try:
        rc, msg = attempt(3, good, entry, E)
        assert rc < 0 and "no graph" in msg, msg
        o.set_graph(g)
        o.set_edge_robust(PALETTE, entry)
        before = o.linearize()
        rc = lib.tsgo_set_edge_robust(None, 3, good, entry.ctypes.data, E, None)
        assert rc < 0 and "null handle" in lib.tsgo_last_error().decode()
        for what, args in (("n_mask", (3, good, entry, E - 1)), ("n_mask", (3, good, entry[:1], 1)), ("n_entries", (16, good, entry, E)), ("n_entries", (-1, good, entry, E)),
                           ("entries", (3, None, entry, E)), ("entry_of_edge", (3, good, None, E)), ("entries[1].kernel", (3, entries((0, 0.0), (4, 1.0), (3, 2.0)), entry, E)),
                           ("entries[2].kernel", (3, entries((0, 0.0), (2, 1.0), (-1, 2.0)), entry, E)), ("entry_of_edge[3]", (2, good, entry, E)),
                           ("n_mask", (0, None, None, E)), ("n_mask", (0, None, entry, 0))):
            rc, msg = attempt(*args)
            assert rc < 0 and what in msg, (what, msg)
        for bad in (float("nan"), float("inf"), 0.0, -1.0, 9e-7, 1.1e6):
            rc, msg = attempt(3, entries((0, 0.0), (2, bad), (3, 2.0)), entry, E)
            assert rc < 0 and "entries[1].delta" in msg, (bad, msg)
        n = C.c_int32(); ent = (_lib.tsgo_edge_robust_entry * _lib.TSGO_EDGE_ROBUST_MAX)(); out = np.zeros(E, np.uint8)
        assert lib.tsgo_get_edge_robust(None, C.byref(n), ent, out.ctypes.data, E) < 0 and "null handle" in lib.tsgo_last_error().decode()
        assert lib.tsgo_get_edge_robust(o.h, C.byref(n), ent, out.ctypes.data, E - 1) < 0 and "cap_edges" in lib.tsgo_last_error().decode()
        assert lib.tsgo_get_edge_robust(o.h, None, ent, out.ctypes.data, E) < 0 and "n_entries_out" in lib.tsgo_last_error().decode()
        assert lib.tsgo_get_edge_robust(o.h, C.byref(n), None, out.ctypes.data, E) < 0 and "entries_out" in lib.tsgo_last_error().decode()
        assert lib.tsgo_get_edge_robust(o.h, C.byref(n), ent, None, E) < 0 and "entry_of_edge_out" in lib.tsgo_last_error().decode()
        with pytest.raises(ValueError):
            o.set_edge_robust(["cauchy"], entry)
        with pytest.raises(ValueError):
            o.set_edge_robust([("tukey", 1.0)], entry)
        # every refused call left the handle as it was
        kernels, back = o.edge_robust
        assert kernels == PALETTE and np.array_equal(back, entry)
        after = o.linearize()
        for x, y in zip(before, after):
            np.testing.assert_array_equal(x, y)
        # NONE ignores its width; the widths' ends are inside
        assert attempt(3, entries((0, float("nan")), (2, 1e-6), (3, 1e6)), entry, E)[0] == 0
        o.exempt_edges(np.flatnonzero(init_guess.consecutive_mask(g)))
        kernels, back = o.edge_robust
        assert kernels == ["none"] and np.array_equal(back, init_guess.consecutive_mask(g))
    finally:
        o.close()
    f32 = HipOptimizer(precision=32)
    try:
        f32.set_graph(g)
        with pytest.raises(RuntimeError, match="precision = 64"):
            f32.set_edge_robust(PALETTE, entry)
    finally:
        f32.close()
    shard = HipOptimizer(world=2, rank=0, testing=True)
    try:
        with pytest.raises(RuntimeError, match="world > 1"):
            shard.set_edge_robust(PALETTE, entry)
    finally:
        shard.close()
