"""The conditions under which tests/test_gpu_warm_start.py means something, from the reference alone (tests/warm_reference.py, no GPU):
the coefficients do what they are for (order m predicts the next delta of d_k = a^k q(k), q of degree m - 1, to rounding); the planted
cases make the rule pick exactly the orders 1 to 5 with every decision a factor 2 from a tie, the tie case sits exactly on it; `done` is
decided by decades wherever it is asserted; the three observed runs (dense solves) have no decision within 1 % of a tie and take orders
1 to 5 between them; and every planted defect (warm_reference.DEFECTS) is caught by compare() — the comparisons and limits the device is held
to — on at least one case.  The table of which case catches which defect is printed."""
import numpy as np
import pytest

from tests import warm_reference as wr


def test_coefficients():
    a = 0.8
    np.testing.assert_allclose(wr.coefficients(a, 1), [a])
    np.testing.assert_allclose(wr.coefficients(a, 2), [2 * a, -a * a])      # x0 = 1.6 d1 - 0.64 d2
    np.testing.assert_allclose(wr.coefficients(a, 4), [3.2, -3.84, 2.048, -0.4096])
    for m in range(1, wr.MAX_WARM + 1):      # a = 1, constant history: every order predicts the constant
        assert abs(wr.coefficients(1.0, m).sum() - 1) < 1e-14


@pytest.mark.parametrize("a", [0.8, 0.4, 0.5])
@pytest.mark.parametrize("m", range(1, wr.MAX_WARM + 1))
def test_order_m_continues_a_trend_of_degree_m_minus_1(m, a):
    rng = np.random.default_rng(m)
    g = rng.normal(size=(m, 50))
    q = lambda k: sum(g[i] * float(k) ** i for i in range(m))      # noqa: E731
    d = lambda k: a ** k * q(k)                                   # noqa: E731
    n = 9
    hist = np.array([d(n - j) for j in range(m)])                 # newest first
    want = d(n + 1)
    got = wr.predict(hist, a, m)
    scale = np.abs(wr.coefficients(a, m)) @ np.abs(hist)
    assert np.all(np.abs(got - want) <= 64 * m * 2.0 ** -53 * scale)
    if m > 1:      # ... and the order below does not
        assert np.abs(wr.predict(hist, a, m - 1) - want).max() > 1e-6 * np.abs(want).max()
    # the error of order m at the newest delta is that of predicting it from the ones before it
    hist2 = np.array([d(n + 1 - j) for j in range(m + 1)])
    e = wr.errors(hist2, a, m)
    assert e[m - 1] <= 1e-24 * np.sum(want ** 2) * (1 + np.sum(scale ** 2) / np.sum(want ** 2)) and (m == 1 or e[m - 2] > 1e-12 * np.sum(want ** 2))


@pytest.mark.parametrize("setting", list(wr.OBSERVED))
def test_fast_system_is_the_dense_system(setting):
    """What the observed runs on the device are compared with, at the device's own estimates, is system_of() computed faster."""
    st = wr.OBSERVED[setting]
    oj = st["kw"].get("odom_jacobian", "constant")
    g = wr.observed(setting)[3]["graph"]
    slow, fast = wr.observed(setting)[3]["system"], wr.fast_system(g, oj, st["python"], wr.PY_LAMBDA if st["python"] else 0.0)
    for k in ("S", "bt", "Dinv", "mag"):
        assert np.abs(slow[k] - fast[k]).max() <= 1e-13 * np.abs(slow[k]).max(), k
    assert slow["deg_max"] == fast["deg_max"]
    d = wr.observed(setting)[3]["delta"]
    assert np.abs(fast["delta"] - d).max() <= 1e-10 * np.abs(d).max()


def test_orders_the_engine_can_test():
    assert wr.orders(1, 6) == (1, 0) and wr.orders(2, 6) == (2, 1) and wr.orders(6, 6) == (6, 5)      # order 6 is allowed but never tested
    assert wr.orders(6, 2) == (2, 2) and wr.orders(6, 1) == (1, 1) and wr.orders(3, 0) == (1, 0)


def _reference(name, amg=True):
    c = wr.CASES[name]
    s = wr.case_system(name)
    hist = wr.planted(name)[::-1][:wr.MAX_WARM]
    return wr.warm_start(hist, c["a"], c["cap"], s["S"], s["bt"], s["Dinv"], wr.PLANT_TOL, amg), s


def test_planted_cases_decide_by_a_factor_two():
    orders = {}
    for name, c in wr.CASES.items():
        ref, _s = _reference(name)
        if c["kind"] == "cold":
            assert ref["warmed"] == 0
            continue
        assert ref["warmed"] == 1
        orders[name] = ref["order"]
        print("case %-11s n_prev %d n_tested %d n_max %d order %d; errors %s; decision ratios %s; scale %.3e" % (
            name, ref["n_prev"], ref["n_tested"], ref["n_max"], ref["order"], ["%.2e" % e for e in ref["err"]], ["%.3g" % r for r in ref["ratios"]], ref["scale"]))
        if c["kind"] == "tie":
            assert ref["ratios"] == [1.0] and ref["order"] == 1      # exactly on the margin: strict < keeps order 1
        elif c["kind"] != "zeros":
            assert all(r < 0.5 or r > 2 for r in ref["ratios"]), (name, ref["ratios"])
        if c["kind"] == "trend":
            assert ref["n_tested"] == 5 and len(ref["ratios"]) == 4
    assert orders == wr.EXPECTED_ORDER
    assert {orders[n] for n, c in wr.CASES.items() if c["kind"] == "trend"} == {1, 2, 3, 4, 5}
    assert wr.CASES["tie"]["a"] == 0.5


def test_planted_tie_is_exact_in_any_precision():
    d = wr.planted("tie")
    for dt in (np.float32, np.float64):
        h = d.astype(dt)[::-1]
        assert np.array_equal(h.astype(np.float64), d[::-1])
        e1 = h[0] - dt(0.5) * h[1]; e2 = h[0] - (dt(1.0) * h[1] - dt(0.25) * h[2])
        for perm in (np.arange(len(e1)), np.random.default_rng(0).permutation(len(e1))):
            s1 = dt(0); s2 = dt(0)
            for i in perm:
                s1 += e1[i] * e1[i]; s2 += e2[i] * e2[i]
            assert 4 * s2 == s1 and s1 > 0
    assert np.abs(d[2][:3 * wr.BLOCK]).sum() > 0 and np.abs(d[2][3 * wr.BLOCK:]).sum() > 0      # both workgroups hold part of it


def test_done_is_decided_by_decades_where_it_is_asserted():
    for name, c in wr.CASES.items():
        if c["kind"] == "cold":
            continue
        ref, s = _reference(name)
        # what rounding can add to rdr on the device: the floor of compare() at the reference's own x0
        eb = wr.r0_bound(s, s["bt"], ref["x0"], wr.U[64]) + wr.B_TOL[64] * np.abs(s["bt"]).max()
        ede = float(eb @ (np.abs(s["Dinv"]) @ eb))
        floor = 2 * np.sqrt(ref["rdr"] * ede) + ede
        ratio = ref["rdr"] / (wr.PLANT_TOL ** 2 * ref["bdb"])
        hi = (ref["rdr"] + floor) / (wr.PLANT_TOL ** 2 * ref["bdb"])
        print("case %-11s rdr / (tol^2 bdb) = %.3e (with the rounding floor %.3e): done %d" % (name, ratio, hi, ref["done"]))
        assert (ref["done"] == 1) == (name == "x_star")
        assert hi < 0.25 if ref["done"] else ratio > 4
    # a pcg_rel_tol = 0.5 handle after four steps: the warm start meets the rule with a factor 4 to spare
    ref = wr.observed_reference("constant", 4, tol=0.5)
    print("observed constant, after 4 steps: rdr / bdb = %.4f against tol^2 = 0.25" % (ref["rdr"] / ref["bdb"]))
    assert ref["rdr"] < 0.25 * 0.25 * ref["bdb"] and ref["done"] == 1


def test_observed_runs_have_no_decision_near_a_tie():
    orders, closest = {}, {}
    for setting in wr.OBSERVED:
        picked, ratios = [], []
        for k in range(1, wr.OBS_STEPS + 1):
            ref = wr.observed_reference(setting, k)
            assert ref["warmed"] == 1 and ref["done"] == 0 and ref["scale"] > 1
            picked.append(ref["order"]); ratios += ref["ratios"]
        r = np.array(ratios)
        closest[setting] = r[np.argmin(np.abs(np.log(r)))]
        orders[setting] = picked
        print("observed %-8s orders %s; decision ratio closest to a tie %.4f of %d" % (setting, picked, closest[setting], len(r)))
        assert np.all(np.abs(r - 1) > wr.TIE_BAND)      # every comparison counts: none is skipped
    assert {m for p in orders.values() for m in p} >= {1, 2, 3}


def test_every_defect_is_caught_by_the_device_comparisons():
    caught = {d: [] for d in wr.DEFECTS}
    for name, c in wr.CASES.items():
        s = wr.case_system(name)
        for amg in (True, False):
            clean = wr.emulate(wr.planted(name), c["a"], c["cap"], s["S"], s["bt"], s["Dinv"], wr.PLANT_TOL, amg)
            bad, _fig = wr.compare(clean, c["a"], c["cap"], s, wr.PLANT_TOL, amg, planted=wr.planted(name))
            assert not bad, (name, bad)
        for d in wr.DEFECTS:
            out = wr.emulate(wr.planted(name), c["a"], c["cap"], s["S"], s["bt"], s["Dinv"], wr.PLANT_TOL, True, defect=d)
            bad, _fig = wr.compare(out, c["a"], c["cap"], s, wr.PLANT_TOL, True, planted=wr.planted(name))
            if bad:
                caught[d].append((name, bad[0]))
    for d in wr.DEFECTS:
        print("defect %-17s caught by %d cases: %s" % (d, len(caught[d]), ", ".join(n for n, _ in caught[d])))
        for n, why in caught[d][:2]:
            print("      %s: %s" % (n, why))
    assert all(caught[d] for d in wr.DEFECTS), {d: len(v) for d, v in caught.items()}
    # the defects that need a particular case: the read stride needs two workgroups, the margin needs a tie (all-zero errors are one too)
    assert [n for n, _ in caught["margin_le"]] == ["tie", "zeros"]
    assert "trend1_g40" not in [n for n, _ in caught["first_block_only"]] and "trend1" in [n for n, _ in caught["first_block_only"]]
