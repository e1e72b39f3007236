"""The PCG loop around the operators, at LOOSE tolerances, against the plain two-reduction reference of tests/pcg_reference.py: the
iterate after k updates (read out of a capped solve), the step at which the stop rule fires on a ladder of tolerances placed between
the reference's residual ratios, the launch paths, f32 handles, the cap under tsgo_optimize, a zero right-hand side, and the batched
PCG of tsgo_joint_marginals, column by column.  A converged answer does not depend on how PCG got there; these do.

Every solve is a cold start: a fresh handle, set_graph, solve_step (no history, no warm start), use_graphs = 0 unless stated.  Limits,
margins, cap values and tolerances come from the reference alone; tests/test_pcg_reference_cpu.py shows that each planted defect (a
stale gamma in beta, alpha without the Chronopoulos-Gear correction, the rule in the other norm, one update too many) is caught at
every one of them, and prints which combinations were dropped because they cannot tell a defect.  Each test prints distance against
limit and count against reference.  Distances are S-norm distances relative to ||x*||_S."""
import threading

import numpy as np
import pytest

from tests import edge_cases
from tests import pcg_reference as pr
from tests import precond_cases as pc
from toyslam_amd.optimizer import HipOptimizer, free_local_group, local_group

pytestmark = pytest.mark.gpu


def _opts(case, precond, **over):
    kw = dict(testing=True, use_graphs=0, preconditioner=precond)
    kw.update(pc.CASES[case]["kw"])
    kw.update(over)
    return kw


def _solve(case, precond, allow_unconverged=False, g=None, **over):
    g = pr.graph(case) if g is None else g
    with pc.Env(pc.CASES[case]["env"]):
        o = HipOptimizer(**_opts(case, precond, **over))
        try:
            o.set_graph(g)
            return o.solve_step(allow_unconverged=allow_unconverged), g
        finally:
            o.close()


def _pose_part(g, delta):
    return delta[g.v_type == 0].reshape(-1)


def _distance(case, x, x_ref):
    S = pr.system(case)["S"]
    return pr.s_norm(S, x - x_ref) / pr.s_norm(S, pr.x_star(case))


@pytest.mark.parametrize("precond", pr.PRECONDS)
@pytest.mark.parametrize("case", pr.CASES)
def test_iterate_after_k_updates(case, precond):
    """pcg_max_iters = k, pcg_rel_tol = 1e-30, cycle_storage = 32 (a capped solve on packed storage would be repeated on f32 copies): the
    solve returns -22 with the count k, the pose part of delta is x_k, the landmark part the back-substitution of THAT pose part."""
    ref = pr.run(case, precond)
    lim = pr.iterate_limit(case, precond, "f32_f32")
    ks, dropped = pr.cap_values(case, precond, "f32_f32")
    if dropped:
        print("case %s %s: caps %s cannot discriminate a defect (tests/test_pcg_reference_cpu.py): not run" % (case, precond, sorted(dropped)))
    sys_ = pr.system(case)
    bad = []
    for k in ks:
        r, g = _solve(case, precond, allow_unconverged=True, pcg_max_iters=k, pcg_rel_tol=1e-30, cycle_storage=32)
        x = _pose_part(g, r["delta"])
        d = _distance(case, x, ref.x[k - 1])
        dl = r["delta"][g.v_type == 1][:, :2]
        want = pr.landmark_backsub(sys_, x)
        back = float(np.abs(dl - want).max() / np.abs(want).max())
        print("case %s %s k = %2d: rc %d, count %d; distance to x_k %.3e (limit %.3e); back-substitution %.2e" % (case, precond, k, r["rc"], r["cg_iters"], d, lim[k - 1], back))
        assert r["rc"] == -22 and r["cg_iters"] == k
        if not (d <= lim[k - 1] and back <= 1e-12):
            bad.append((k, d, lim[k - 1], back))
    assert not bad, bad


@pytest.mark.parametrize("precond,rung", [("jacobi", None)] + [("amg", r) for r in pr.LADDER_RUNGS])
@pytest.mark.parametrize("case", pr.CASES)
def test_stop_rule_on_the_tolerance_ladder(case, precond, rung):
    """At tol_k the reference stops at exactly k: return code 0, count k, the iterate x_k, the TRUE residual of the returned x (f64, dense
    S) meets the rule to the margin, and the reference's x_{k-1} does not."""
    ref = pr.run(case, precond)
    lim = pr.iterate_limit(case, precond, rung)
    mu = pr.count_margin(case, precond, rung)
    used, dropped = pr.ladder(case, precond, rung)
    what = "case %s %s%s" % (case, precond, " " + rung if rung else "")
    if dropped:
        print("%s: %d tolerances cannot discriminate a defect (tests/test_pcg_reference_cpu.py): not run" % (what, len(dropped)))
    if not used:
        print("%s: no tolerance at which every defect is caught: nothing is run" % what)
    bad = []
    for k, tol, kind in used:
        over = dict(cycle_storage=pc.RUNGS[rung]["storage"]) if rung else {}
        r, g = _solve(case, precond, pcg_rel_tol=tol, **over)
        x = _pose_part(g, r["delta"])
        d = _distance(case, x, ref.x[k - 1])
        res = pr.residual_ratio(case, precond, x)
        before = pr.residual_ratio(case, precond, ref.x[k - 2]) if k > 1 else 1.0
        print("%s tol %.3e (%s): count %d (reference %d); distance to x_k %.3e (limit %.3e); residual / tol %.4f, of x_{k-1} %.4f (margin %.1e)" % (
            what, tol, kind, r["cg_iters"], k, d, lim[k - 1], res / tol, before / tol, mu[k]))
        assert before > tol
        if not (r["rc"] == 0 and r["cg_iters"] == k and d <= lim[k - 1] and res <= tol * (1 + mu[k])):
            bad.append((k, tol, r["cg_iters"], d, lim[k - 1], res / tol))
    assert not bad, bad


def _run_world2(case, precond, **over):
    g = pr.graph(case)
    group = local_group(2)
    out, errs = [None, None], []

    def rank_main(rank):
        try:
            o = HipOptimizer(rank=rank, world=2, **_opts(case, precond, **over))
            try:
                o.comm_init_local(group)
                o.set_graph(g)
                out[rank] = o.solve_step()
            finally:
                o.close()
        except Exception as e:                       # noqa: BLE001 - reported below
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=rank_main, args=(k,), daemon=True) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errs, errs
    assert not any(t.is_alive() for t in th), "a rank is stuck in the in-process all-reduce"
    free_local_group(group)
    return out, g


def test_every_launch_path_stops_at_the_same_step(monkeypatch):
    """dense_bottom, multigrid, one mid-ladder tolerance: bursts (the default of use_graphs = 0), paced eager launches (TSGO_FORCE_PACED,
    testing build), the explicit level-0 matrix in the cycle, and two shards through the in-process group."""
    case, precond, rung = "dense_bottom", "amg", "f32_f32"
    used, _ = pr.ladder(case, precond, rung)
    k, tol, _kind = used[len(used) // 2]
    ref = pr.run(case, precond)
    lim = pr.iterate_limit(case, precond, rung)[k - 1]
    got = {}
    monkeypatch.delenv("TSGO_FORCE_PACED", raising=False)
    r, g = _solve(case, precond, pcg_rel_tol=tol, cycle_storage=32)
    got["bursts"] = (r["cg_iters"], _pose_part(g, r["delta"]))
    monkeypatch.setenv("TSGO_FORCE_PACED", "1")
    r, g = _solve(case, precond, pcg_rel_tol=tol, cycle_storage=32)
    got["paced"] = (r["cg_iters"], _pose_part(g, r["delta"]))
    monkeypatch.delenv("TSGO_FORCE_PACED")
    r, g = _solve(case, precond, pcg_rel_tol=tol, cycle_storage=32, cycle_level0="explicit")
    got["explicit level 0"] = (r["cg_iters"], _pose_part(g, r["delta"]))
    outs, g = _run_world2(case, precond, pcg_rel_tol=tol, cycle_storage=32)
    for rank, r in enumerate(outs):
        got["world 2, rank %d" % rank] = (r["cg_iters"], _pose_part(g, r["delta"]))
    bad = []
    for name, (count, x) in got.items():
        d = _distance(case, x, ref.x[k - 1])
        print("dense_bottom amg tol %.3e, %s: count %d (reference %d); distance to x_k %.3e (limit %.3e)" % (tol, name, count, k, d, lim))
        if not (count == k and d <= lim):
            bad.append((name, count, d))
    assert not bad, bad
    np.testing.assert_array_equal(got["bursts"][1], got["paced"][1])      # the same kernels in the same order: the same bits
    np.testing.assert_array_equal(got["world 2, rank 0"][1], got["world 2, rank 1"][1])


@pytest.mark.parametrize("precond", pr.PRECONDS)
def test_f32_handle_on_the_tolerance_ladder(precond):
    """Engine<float> on dense_bottom, tolerances >= 1e-4: the limit is 8 x the distance between the float64 reference and a float32
    reference on S, b~ rounded to f32 (multigrid: plus the operator's share on the p32_f32 rung); the count is equal, every tolerance
    used being decided at the margin measured the same way."""
    case = pr.F32_CASE
    ref = pr.run(case, precond)
    lim, mu = pr.f32_limits(precond)
    used, _dropped = pr.f32_ladder(precond)
    assert used
    bad = []
    for k, tol, kind in used:
        r, g = _solve(case, precond, pcg_rel_tol=tol, precision=32, cycle_storage=32)
        x = _pose_part(g, r["delta"])
        d = _distance(case, x, ref.x[k - 1])
        res = pr.residual_ratio(case, precond, x)
        print("f32 handle, %s %s tol %.3e (%s): count %d (reference %d); distance to x_k %.3e (limit %.3e); residual / tol %.4f (margin %.1e)" % (
            case, precond, tol, kind, r["cg_iters"], k, d, lim[k - 1], res / tol, mu[k]))
        if not (r["rc"] == 0 and r["cg_iters"] == k and d <= lim[k - 1] and res <= tol * (1 + mu[k])):
            bad.append((k, tol, r["cg_iters"], d, lim[k - 1], res / tol))
    assert not bad, bad


@pytest.mark.parametrize("precond", pr.PRECONDS)
def test_cap_under_optimize_takes_no_step(precond):
    case = "dense_bottom"
    g = pr.graph(case)
    o = HipOptimizer(**_opts(case, precond, pcg_max_iters=3, cycle_storage=32))
    try:
        o.set_graph(g)
        v0 = o.vertices()
        r = o.optimize(5)
        v1 = o.vertices()
    finally:
        o.close()
    assert r["stop"] == "solver_failed" and r["iters"] == 1 and list(r["cg_iters"]) == [3]
    np.testing.assert_array_equal(v1, v0)
    np.testing.assert_array_equal(v1[:, :2], g.v_pos[:, :2])
    assert np.abs(v1[:, 2] - g.v_pos[:, 2]).max() <= 4e-16 * np.pi      # theta is held as (cos, sin) and read back through atan2


@pytest.mark.parametrize("precond", pr.PRECONDS)
def test_zero_right_hand_side(precond):
    """Every measurement computed from the estimates (tests/edge_cases.py: zero_residuals; no such case was asserted on the device):
    b = 0, so `!(gamma > tol2 * gamma0)` is tested at 0 > 0 (k_cg_update) and `gamma == 0` ends k_cg_step: no update, no error."""
    g = edge_cases.zero_residuals()
    o = HipOptimizer(testing=True, use_graphs=0, preconditioner=precond, pcg_rel_tol=1e-8)
    try:
        o.set_graph(g)
        r = o.solve_step()
    finally:
        o.close()
    print("zero right-hand side, %s: count %d, chi^2 %r, max |delta| %r" % (precond, r["cg_iters"], r["chi2"], float(np.abs(r["delta"]).max())))
    assert r["rc"] == 0 and r["cg_iters"] == 0 and r["chi2"] == 0.0
    assert np.all(r["delta"] == 0.0)


# ---- the batched PCG: tsgo_joint_marginals over all poses of level0_only, 120 unit columns ----
def _joint(precond, tol, width=None, order=None):
    g = pr.graph(pr.BATCH_CASE)
    ids = g.v_id[g.v_type == 0]
    ids = ids if order is None else ids[order]
    with pc.Env({} if width is None else {"TSGO_MARGINAL_WIDTH": str(width)}):
        o = HipOptimizer(testing=True, use_graphs=0, preconditioner=precond)
        try:
            o.set_graph(g)
            cov, off, st = o.joint_marginals(ids, rel_tol=tol)
        finally:
            o.close()
    assert list(off) == list(range(0, 3 * len(ids) + 1, 3))
    return cov, st


def _batched_expectation(precond, tol):
    """Per entry (i, j) of (X + X^T) / 2: the reference values with every undecided column at k_c or at k_c + 1 (four combinations), and
    the bound: an entry e_i^T (x_j - ref_j) is at most ||e_i||_{S^-1} ||x_j - ref_j||_S, so the symmetrised entry is within
    sqrt(S^-1_ii S^-1_jj) x the larger of the two columns' limits."""
    cols, Sinv = pr.batched(precond)
    ks, und = pr.batched_counts(precond, tol)
    n = len(cols)
    X0 = np.stack([c["t"].x[k - 1] for c, k in zip(cols, ks)], axis=1)
    X1 = np.stack([c["t"].x[k - 1 + int(u)] for c, k, u in zip(cols, ks, und)], axis=1)
    lim = np.array([max(c["lim"][k - 1], c["lim"][k - 1 + int(u)]) for c, k, u in zip(cols, ks, und)])
    refs = [0.5 * (A + B.T) for A in (X0, X1) for B in (X0, X1)]
    sd = np.sqrt(np.diag(Sinv))
    bound = np.outer(sd, sd) * np.maximum(lim[:, None], lim[None, :])
    assert n == 120
    return refs, bound, ks, und


@pytest.mark.parametrize("tol", pr.BATCH_TOLS)
@pytest.mark.parametrize("precond", pr.PRECONDS)
def test_batched_pcg_column_by_column(precond, tol):
    refs, bound, ks, und = _batched_expectation(precond, tol)
    cov, st = _joint(precond, tol)
    err = np.min([np.abs(cov - R) for R in refs], axis=0)
    worst = float((err / bound).max())
    lo, hi = int(ks.sum()), int(ks.sum() + und.sum())
    print("batched %s tol %.0e (width %d, %d batches): largest entry error / bound %.3e; iterations total %d (reference %d..%d), max %d (reference %d..%d); undecided %d of %d" % (
        precond, tol, st["batch_width"], st["batches"], worst, st["pcg_iters_total"], lo, hi, st["pcg_iters_max"], ks.max(), (ks + und).max(), und.sum(), len(ks)))
    assert st["columns"] == 120 and st["fallbacks"] == 0
    assert lo <= st["pcg_iters_total"] <= hi
    assert ks.max() <= st["pcg_iters_max"] <= (ks + und).max()
    assert worst <= 1.0


@pytest.mark.parametrize("precond", pr.PRECONDS)
def test_a_frozen_column_does_not_depend_on_its_batch(precond):
    """The same query in another order (every column shares its batch with other neighbours, and sits in another slot of it): every
    entry bit-identical, a column's arithmetic being the same whoever runs next to it and for however long.  Across WIDTHS the bits
    may differ — the per-column sums of k_mb_dots and of the product's partials run over kBlock / width elements per workgroup, in
    another grouping — so there the decided columns are held to the limit instead (the research widths are 1, 8 and 16: the other one
    of 8 and 16 is taken)."""
    tol = pr.BATCH_TOLS[1]
    _refs, bound, _ks, und = _batched_expectation(precond, tol)
    cov, st = _joint(precond, tol)
    perm = np.random.default_rng(3).permutation(40)
    rows = (3 * perm[:, None] + np.arange(3)[None, :]).reshape(-1)
    cov_p, _ = _joint(precond, tol, order=perm)
    back = np.empty_like(cov_p)
    back[np.ix_(rows, rows)] = cov_p
    other = 8 if st["batch_width"] == 16 else 16
    cov_w, st_w = _joint(precond, tol, width=other)
    assert st_w["batch_width"] == other
    decided = ~(und[:, None] | und[None, :])
    diff = np.abs(cov_w - cov)[decided] / bound[decided]
    print("batched %s tol %.0e: shuffled query identical: %s; width %d against %d on decided columns: identical %s, largest difference / bound %.3e" % (
        precond, tol, np.array_equal(back, cov), other, st["batch_width"], np.array_equal(cov_w[decided], cov[decided]), float(diff.max())))
    np.testing.assert_array_equal(back, cov)
    assert diff.max() <= 2.0      # (each run within its bound of the reference)
