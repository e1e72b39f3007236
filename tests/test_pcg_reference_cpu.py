"""The conditions under which tests/test_gpu_pcg_trajectory.py means something, from the reference alone (tests/pcg_reference.py, no
GPU): the reference is PCG; the limits the device is held to (rounding: 100 x the f64-to-longdouble drift; multigrid on f32 / packed
cycle storage: 2 x what a perturbation of the operator of size precond_cases.limit(rung) does over 8 seeds; f32 handles: 8 x the
f64-to-f32 distance); the tolerance ladders and their gaps; that every planted defect (pcg_reference.DEFECTS) lies 10 limits from the
clean reference, or changes the count, at every cap value and tolerance the device tests use — what cannot tell a defect is dropped
from the device's parametrisation and printed here; and the undecided share of the batched PCG's columns."""
import numpy as np
import pytest

from tests import pcg_reference as pr
from tests import precond_cases as pc

PAIRS = [(c, p, r) for c in pr.CASES for p in pr.PRECONDS for r in ((None,) if p == "jacobi" else pr.LADDER_RUNGS)]


def test_tolerances_stop_at_exactly_k_on_a_sequence_that_rises():
    r = np.array([1.0, 0.5, 0.2, 0.3, 0.19, 0.1, 0.12, 0.04, 0.039, 0.01])
    got = pr.tolerances(r, gap=1.3)
    assert [k for k, _ in got] == [1, 2, 5, 7, 9]      # 3 and 6 rise, 4 and 8 lie less than 1.3 below the running minimum
    for k, tol in got:
        first = int(np.where(r[1:] <= tol)[0][0]) + 1
        assert first == k
        assert r[k] * np.sqrt(1.3) <= tol * (1 + 1e-15) and tol * np.sqrt(1.3) <= r[:k].min() * (1 + 1e-15)


@pytest.mark.parametrize("case", pr.CASES)
@pytest.mark.parametrize("precond", pr.PRECONDS)
def test_the_reference_is_pcg(case, precond):
    """x_k minimises the S-norm of the error over the Krylov space: the error falls monotonically and the residuals are M-orthogonal;
    the Chronopoulos-Gear recurrences WITH the correction term give the same iterates (the form the "alpha_plain" defect is planted in)."""
    s = pr.system(case)
    S, b, M = s["S"], s["bt"], pr.operator(case, precond)
    t = pr.run(case, precond, "longdouble")
    xs = pr.x_star(case)
    err = np.array([pr.s_norm(S, np.asarray(x, np.float64) - xs) for x in t.x[:20]])
    assert np.all(np.diff(err[:12]) < 0) and err[19] < (0.7 if precond == "jacobi" else 1e-8) * pr.s_norm(S, xs)      # (x* itself is good to 1e-11)
    R = np.array([b - S @ np.asarray(x, np.float64) for x in t.x[:6]])
    G = R @ M @ R.T
    dg = np.sqrt(np.diag(G))
    off = (np.abs(G - np.diag(np.diag(G))) / np.outer(dg, dg)).max(axis=1)
    assert off.max() < 1e-8, off
    # Chronopoulos-Gear, restated with the correction term
    x = np.zeros_like(b); r = b.copy(); p = q = None; g_old = a_old = None
    for k in range(8):
        z = M @ r; sz = S @ z
        g, d = r @ z, z @ sz
        beta = 0.0 if k == 0 else g / g_old
        alpha = g / d if k == 0 else g / (d - beta * g / a_old)
        p = z if k == 0 else z + beta * p
        q = sz if k == 0 else sz + beta * q
        x = x + alpha * p; r = r - alpha * q
        g_old, a_old = g, alpha
        assert pr.s_norm(S, x - np.asarray(t.x[k], np.float64)) <= 1e-10 * pr.s_norm(S, xs), k
    assert t.ratio_M[0] == t.ratio_D[0] == 1.0
    if precond == "jacobi":      # M = D^-1 and x_0 = 0: one and the same ratio (why the block-Jacobi rule's "other norm" is the Euclidean one)
        np.testing.assert_allclose(t.ratio_M[:40], t.ratio_D[:40], rtol=1e-12)


@pytest.mark.parametrize("case", pr.CASES)
@pytest.mark.parametrize("precond", pr.PRECONDS)
def test_rounding_limits(case, precond):
    lim, drift = pr.rounding_limit(case, precond)
    ks = pr.CAP_KS[precond]
    print("case %s %s: drift f64 to longdouble at k = %s: %s; largest over %d steps %.2e" % (case, precond, list(ks), ["%.1e" % drift[k - 1] for k in ks], len(drift), drift.max()))
    assert 0 < drift[:21].max() <= 1e-11      # (indicative: <= 1e-15 up to k = 20 for block-Jacobi; the multigrid operator's entries carry the twin's f64 rounding)
    assert np.all(np.diff(lim) >= 0) and lim[ks[-1] - 1] <= 1e-10


@pytest.mark.parametrize("case,rung", [(c, r) for c in pr.CASES for r in pr.LADDER_RUNGS] + [(pr.F32_CASE, "p32_f32")])
def test_multigrid_operator_limits(case, rung):
    lim, mu, dist, rel = pr.operator_limit(case, rung)
    eps = pc.limit(rung)
    ks = list(pr.CAP_KS["amg"])
    print("case %s rung %s (eps %.2e, %d seeds): distance at k = %s: %s; ratio change: %s" % (case, rung, eps, pr.N_SEEDS, ks, ["%.1e" % dist[k - 1] for k in ks], ["%.1e" % rel[k] for k in ks]))
    assert 0 < dist.max() <= 2 * eps      # a perturbation of relative size eps moves an iterate by about eps of the solution, no more
    assert dist[12] < dist[0]             # ... and less and less of it as the iterate converges
    assert rel[1] > 0 and np.all(np.diff(mu) >= 0)


@pytest.mark.parametrize("case,precond", [(c, p) for c in pr.CASES for p in pr.PRECONDS])
def test_gaps(case, precond):
    gap, n, dec = pr.gap_for(case, precond)
    print("case %s %s: tolerances() at gap %.2f: %d tolerances over %.1f decades" % (case, precond, gap, n, dec))
    assert n >= 4 and dec >= 3
    for rung in ((None,) if precond == "jacobi" else pr.LADDER_RUNGS):
        mu = pr.count_margin(case, precond, rung)
        used, _dropped = pr.ladder(case, precond, rung)
        r = pr.run(case, precond).deciding(precond)
        for k, tol, _kind in used:      # the margin holds on either side of every tolerance used
            assert r[k] * (1 + 2 * mu[k]) <= tol * (1 + 1e-12) and tol * (1 + 2 * mu[k]) <= r[:k].min() * (1 + 1e-12), (case, precond, rung, k, tol)
            assert int(np.where(r[1:] <= tol)[0][0]) + 1 == k
        if precond == "jacobi":
            assert gap >= 1 + 2 * pr.MU_F64


@pytest.mark.parametrize("case,precond,rung", PAIRS)
def test_every_defect_is_caught_where_the_device_is_tested(case, precond, rung):
    """The sensitivity condition, re-derived here from the defect runs: at every cap value used both iterate defects lie >= 10 limits
    from the clean x_k; at every tolerance used every defect changes the count or its stopping iterate lies >= 10 limits away."""
    clean = pr.run(case, precond)
    lim = pr.iterate_limit(case, precond, rung)
    S = pr.system(case)["S"]; den = pr.s_norm(S, pr.x_star(case))
    ks, dropped_k = pr.cap_values(case, precond, rung)
    used, dropped = pr.ladder(case, precond, rung)
    what = "case %s %s%s" % (case, precond, " " + rung if rung else "")
    print("%s: caps used %s; tolerances used %s" % (what, ks, [(k, "%.3e" % tol, kind) for k, tol, kind in used]))
    for k, rep in dropped_k.items():
        print("%s: cap k = %d cannot discriminate (defect distance / limit: %s): dropped" % (what, k, {d: "%.2f" % v for d, v in rep.items()}))
    for k, tol, kind, rep in dropped:
        print("%s: tol %.3e (k = %d, %s) cannot discriminate %s: dropped" % (what, tol, k, kind, [d for d, (kd, far) in rep.items() if kd == k and far < pr.DEFECT_SHARE]))
    for d in ("beta_stale", "alpha_plain"):
        t = pr.run(case, precond, "float64", d)
        dist = pr.distances(case, t.x, clean.x)
        first = 3 if d == "beta_stale" else 2
        assert dist[first - 2] == 0 and dist[first - 1] > 0      # where the defect starts to act
        for k in ks:
            if k >= first:
                assert dist[k - 1] >= pr.DEFECT_SHARE * lim[k - 1], (what, d, k)
    for k, tol, _kind in used:
        assert clean.stop(precond, tol) == k
        for d in pr.DEFECTS:
            t = pr.run(case, precond, "float64", d)
            kd = t.stop(precond, tol)
            if kd == k:
                assert pr.s_norm(S, t.x[kd - 1] - clean.x[k - 1]) / den >= pr.DEFECT_SHARE * lim[k - 1], (what, d, k, tol)
    if rung != "f32_half":      # (packed halves: a limit of 2e-2 of the solution hides every defect at most steps, as in test_precond_twin_cpu.py)
        assert len(ks) >= 1
    if precond == "jacobi":
        assert len(used) >= 4 and pr.decades([tol for _k, tol, _ in used]) >= 1.0      # (how deep a ladder goes depends on where rounding ends it)


@pytest.mark.parametrize("precond", pr.PRECONDS)
def test_f32_handle_limits(precond):
    lim, mu = pr.f32_limits(precond)
    used, dropped = pr.f32_ladder(precond)
    print("f32 handle, %s %s: limit at k = 1, 3, 8, 13: %s; margin: %s; tolerances used %s; dropped %s" % (
        pr.F32_CASE, precond, ["%.1e" % lim[k - 1] for k in (1, 3, 8, 13)], ["%.1e" % mu[k] for k in (1, 3, 8, 13)],
        [(k, "%.3e" % tol, kind) for k, tol, kind in used], [(k, "%.3e" % tol, kind) for k, tol, kind, _ in dropped]))
    assert len(used) >= 2 and all(tol >= pr.F32_TOL_MIN for _k, tol, _ in used)
    assert 1e-8 < lim[0] and lim[12] < 1e-3      # f32 rounding: 6e-8 per operation, far below the first defect (1e-2 and more)


@pytest.mark.parametrize("precond", pr.PRECONDS)
def test_batched_columns_are_decided(precond):
    cols, _Sinv = pr.batched(precond)
    assert len(cols) == 120
    for tol in pr.BATCH_TOLS:
        ks, und = pr.batched_counts(precond, tol)
        lim = max(c["lim"][k - 1] for c, k in zip(cols, ks))
        print("batched %s tol %.0e: k_c from %d to %d, sum %d; undecided %d of %d; largest limit %.2e, largest margin %.2e" % (
            precond, tol, ks.min(), ks.max(), ks.sum(), und.sum(), len(ks), lim, max(c["mu"][k] for c, k in zip(cols, ks))))
        assert und.mean() <= pr.UNDECIDED_SHARE
        assert ks.max() > ks.min()      # the columns stop at different steps: some are frozen while others run on
        # an extra update of a frozen column is visible: the next iterate lies >= 10 limits away for most columns
        far = np.array([pr.s_norm(pr.system(pr.BATCH_CASE)["S"], c["t"].x[k] - c["t"].x[k - 1]) / np.sqrt(_Sinv[j, j]) / c["lim"][k - 1] for j, (c, k) in enumerate(zip(cols, ks))])
        print("   one update too many: distance / limit, median %.1f, share below 10: %.2f" % (np.median(far), (far < pr.DEFECT_SHARE).mean()))
        assert (far >= pr.DEFECT_SHARE).mean() >= (0.9 if precond == "jacobi" else 0.5)


def test_zero_residual_graph_has_no_right_hand_side():
    from oracle import oracle
    from tests import edge_cases, util
    g = edge_cases.zero_residuals()
    H, b, chi2, _idx = oracle.linearize(util.to_oracle(g))
    assert chi2 == 0.0 and np.all(b == 0.0)
    assert np.linalg.eigvalsh(H).min() > 0
