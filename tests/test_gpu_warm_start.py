"""The PCG warm start on the device, read out of a handle by tsgo_testing_warm_start (include/tsgo_testing.h), against the plain numpy
restatement of tests/warm_reference.py applied to the history the device itself holds: the history (k_save_x / k_save_update and the
host's rotation of six buffers), the prediction errors and the stride they are summed with, the order taken (margin 4, strictly), the
start x0 (k_pack_x), r0 = b~ - S x0 (k_warm_residual), the scale of the stop rule and the early `done` (k_warm_scale), and the history
across tsgo_set_graph under warm_requests (in place; k_gather_hist by vertex id).

Planted histories exercise every order, an exact tie, the rotation, the caps and the cold cases; observed ones are what twelve
optimize(1) calls leave, compared with dense solves.  warm_reference.compare() holds every comparison and limit;
tests/test_warm_reference_cpu.py shows that each planted defect is caught by them and that no decision asserted here is near a tie.
Every test prints its figures before it asserts."""
import numpy as np
import pytest

from oracle import oracle
from tests import util
from tests import warm_reference as wr
from toyslam_amd import synth
from toyslam_amd.optimizer import HipOptimizer

pytestmark = pytest.mark.gpu

KEYS = ("chi2", "cg_iters", "stop", "iters", "delta_norm")


def _handle(precond, precision=64, tol=wr.PLANT_TOL, **kw):
    return HipOptimizer(testing=True, use_graphs=0, preconditioner=precond, precision=precision, pcg_rel_tol=tol, **kw)


def _report(what, out, fig, bad):
    print("%s: warmed %d n_prev %d n_tested %d n_max %d order %d done %d carried %d scale %.6e; b %.2e; sums: bdb %.3e rdr %.3e (relative %.3e)%s" % (
        what, out["warmed"], out["n_prev"], out["n_tested"], out["n_max"], out["order"], out["done"], out["carried"], out["scale"], fig.get("b", np.nan),
        fig.get("bdb", np.nan), fig.get("rdr", np.nan), fig.get("rdr_raw", np.nan), "".join("\n    FAILED " + b for b in bad)))


PLANTED = [(n, p, 64) for n in wr.CASES for p in ("amg", "jacobi")] + [(n, p, 32) for n, c in wr.CASES.items() if c.get("f32") for p in ("amg", "jacobi")]


@pytest.mark.parametrize("name,precond,precision", PLANTED)
def test_planted_history(name, precond, precision):
    c = wr.CASES[name]
    s = wr.case_system(name)
    plant = wr.planted(name)
    o = _handle(precond, precision, **c["kw"])
    bad = []
    try:
        o.set_graph(wr.graph(c["graph"]))
        for fused in (0, 1):
            out = o.testing_warm_start(plant, fused)
            b, fig = wr.compare(out, c["a"], c["cap"], s, wr.PLANT_TOL, precond == "amg", precision, planted=plant)
            _report("planted %s %s f%d fused %d" % (name, precond, precision, fused), out, fig, b)
            if c["kind"] == "cold":
                if out["warmed"] != 0:
                    b.append("warmed on a handle that cannot warm-start")
            elif out["order"] != wr.EXPECTED_ORDER[name]:
                b.append("order %d, the case is built for %d" % (out["order"], wr.EXPECTED_ORDER[name]))
            if c["kind"] == "zeros" and out["scale"] != 1.0:
                b.append("an all-zero history must leave scale = 1")
            if c["kind"] == "x_star" and out["done"] != (1 if precond == "amg" else 0):
                b.append("x0 = x*: done %d" % out["done"])
            bad += ["fused %d: %s" % (fused, t) for t in b]
    finally:
        o.close()
    assert not bad, bad


def _observe(monkeypatch, setting, precond, drains, precision=64, tol=wr.OBS_TOL):
    if drains:
        monkeypatch.setenv("TSGO_STEP_DRAINS", "1")
    else:
        monkeypatch.delenv("TSGO_STEP_DRAINS", raising=False)
    sset = wr.OBSERVED[setting]
    a, step = 1.0 - sset["step"], sset["step"]
    oj, python = sset["kw"].get("odom_jacobian", "constant"), sset["python"]
    lam = wr.PY_LAMBDA if python else 0.0
    # f64: 1e-8 of the delta's largest entry, the bound of the one-solve parity tests.  f32: the solve stops at `tol` in the D^-1 norm of
    # the residual and every vector carries 2^-24: the deltas agree with the dense ones to a few per cent at best once they have shrunk;
    # the comparisons that bind an f32 handle are compare()'s, on its own history
    hist_tol = 1e-8 if precision == 64 else 5e-2
    o = _handle(precond, precision, tol, **sset["kw"])
    bad, orders = [], []
    try:
        g = wr.graph("g300").copy()
        pose = g.v_type == 0
        o.set_graph(g)
        fs = wr.fast_system(g, oj, python, lam)      # the dense system and step at the estimates the device is at, step after step
        deltas = []
        for k in range(1, wr.OBS_STEPS + 1):
            r = o.optimize(1)
            deltas.append(fs["delta"])
            before = g.v_pos[pose].copy()
            g.v_pos[:] = o.vertices()
            fs = wr.fast_system(g, oj, python, lam)
            out = o.testing_warm_start()
            b, fig = wr.compare(out, a, wr.MAX_WARM, fs, tol, precond == "amg", precision, n_prev=min(k, wr.MAX_WARM))
            worst = 0.0
            for j in range(len(out["hist"])):
                d = deltas[k - 1 - j]
                worst = max(worst, float(np.abs(out["hist"][j] - d).max() / np.abs(d).max()))
            if not worst <= hist_tol:
                b.append("history differs from the dense deltas by %.2e of their largest entry (limit %.0e)" % (worst, hist_tol))
            # ... and it is the step that was taken: the poses moved by `step` of the dense delta (oracle.update_pose)
            d = deltas[-1].reshape(-1, 3)
            moved = np.array([oracle.update_pose(before[i], step * d[i]) for i in range(len(d))])
            off = np.abs(moved - g.v_pos[pose]); off[:, 2] = np.abs(util.angle_diff(moved[:, 2], g.v_pos[pose][:, 2]))
            if precision == 64 and not off.max() <= step * hist_tol * np.abs(d).max() + 1e-12:
                b.append("the poses are not where step * the dense delta takes them: %.2e" % off.max())
            want = wr.observed_reference(setting, k, precond == "amg", tol)
            if precision == 64 and out["order"] != want["order"]:
                b.append("order %d, the dense run takes %d" % (out["order"], want["order"]))
            if out["done"] != 0:
                b.append("done at pcg_rel_tol = %.0e" % tol)
            _report("observed %s %s f%d%s step %2d (cg %d, history to dense %.2e)" % (setting, precond, precision, " drains" if drains else "", k, r["cg_iters"][0], worst), out, fig, b)
            orders.append(out["order"])
            bad += ["step %d: %s" % (k, t) for t in b]
    finally:
        o.close()
    print("observed %s %s f%d%s: orders %s" % (setting, precond, precision, " drains" if drains else "", orders))
    assert not bad, bad


@pytest.mark.parametrize("drains", [False, True])
@pytest.mark.parametrize("precond", ["amg", "jacobi"])
@pytest.mark.parametrize("setting", list(wr.OBSERVED))
def test_observed_history(monkeypatch, setting, precond, drains):
    _observe(monkeypatch, setting, precond, drains)


def test_observed_history_f32(monkeypatch):
    _observe(monkeypatch, "constant", "amg", False, precision=32, tol=1e-5)


def test_loose_tolerance_ends_the_solve_before_its_first_iteration():
    """pcg_rel_tol = 0.5, four steps: the start already meets the rule (the reference's ratio is below a quarter of tol^2,
    tests/test_warm_reference_cpu.py), k_warm_scale sets `done`."""
    o = _handle("amg", tol=0.5)
    try:
        o.set_graph(wr.graph("g300"))
        for _ in range(4):
            o.optimize(1)
        out = o.testing_warm_start()
        print("tol 0.5 after four steps: warmed %d order %d done %d rdr / bdb %.4f scale %.3e" % (out["warmed"], out["order"], out["done"], out["rdr"] / out["bdb"], out["scale"]))
        assert out["warmed"] == 1 and out["done"] == 1 and out["rdr"] < 0.25 * out["bdb"]
        assert o.optimize(1)["cg_iters"][0] == 0
    finally:
        o.close()


def _pose_rows(g, ids):
    """Row of every id of `ids` among g's poses (graph order), -1 where g has no such pose."""
    pose_ids = g.v_id[g.v_type == 0]
    at = {int(v): k for k, v in enumerate(pose_ids)}
    return np.array([at.get(int(v), -1) for v in ids])


def test_history_across_requests():
    big = synth.make(330, 10, loop_closures=4, seed=5)
    base = util.first_poses(big, 300)
    o = _handle("amg", tol=wr.OBS_TOL, warm_requests=True)
    try:
        o.set_graph(base)
        for _ in range(6):
            o.optimize(1)
        first = o.testing_warm_start()
        assert first["warmed"] == 1 and first["n_prev"] == 6 and first["n_tested"] == 5 and first["carried"] == 0
        # the same graph again with the estimates it returned: the history stays in place
        again = base.copy(); again.v_pos[:] = o.vertices()
        o.set_graph(again)
        out = o.testing_warm_start()
        s = wr.system_of(again)
        bad, fig = wr.compare(out, 0.8, wr.MAX_WARM, s, wr.OBS_TOL, True, n_prev=6, carried=1)
        _report("same graph again", out, fig, bad)
        np.testing.assert_array_equal(out["hist"], first["hist"])
        np.testing.assert_array_equal(out["err"], first["err"])
        assert not bad, bad
        assert out["scale"] > 1      # what do_solve keeps a carried history for
        # 30 poses appended, the vertex order shuffled, the same ids: the history is gathered by vertex id
        perm = np.random.default_rng(3).permutation(len(big.v_id))
        grown = big.copy()
        old_row = {int(v): k for k, v in enumerate(again.v_id)}
        for k, v in enumerate(grown.v_id):
            if int(v) in old_row:
                grown.v_pos[k] = again.v_pos[old_row[int(v)]]
        grown.v_id, grown.v_type, grown.v_pos = grown.v_id[perm].copy(), grown.v_type[perm].copy(), grown.v_pos[perm].copy()
        o.set_graph(grown)
        out2 = o.testing_warm_start()
        rows = _pose_rows(again, grown.v_id[grown.v_type == 0])
        assert (rows < 0).sum() == 30
        want = np.zeros((6, len(rows), 3))
        want[:, rows >= 0] = first["hist"].reshape(6, -1, 3)[:, rows[rows >= 0]]
        s2 = wr.system_of(grown)
        bad, fig = wr.compare(out2, 0.8, wr.MAX_WARM, s2, wr.OBS_TOL, True, n_prev=6, carried=1)
        # (err is carried, not recomputed: the rows of the new poses are zero in every delta and add nothing to it)
        _report("grown graph", out2, fig, bad)
        np.testing.assert_array_equal(out2["hist"], want.reshape(6, -1))
        np.testing.assert_array_equal(out2["err"], first["err"])
        assert not bad, bad
        # fewer than half the poses shared: nothing is continued
        o.set_graph(util.first_poses(big, 120))
        out3 = o.testing_warm_start()
        print("a third graph with 120 of 330 poses: warmed %d n_prev %d carried %d" % (out3["warmed"], out3["n_prev"], out3["carried"]))
        assert out3["warmed"] == 0 and out3["n_prev"] == 0 and out3["carried"] == 0
    finally:
        o.close()


@pytest.mark.parametrize("drains", [False, True])
@pytest.mark.parametrize("precond", ["amg", "jacobi"])
def test_the_hook_leaves_no_trace(monkeypatch, precond, drains):
    if drains:
        monkeypatch.setenv("TSGO_STEP_DRAINS", "1")
    else:
        monkeypatch.delenv("TSGO_STEP_DRAINS", raising=False)
    g = wr.graph("g300")
    plant = wr.planted("plant7")
    res = []
    for hook in (True, False):
        o = _handle(precond, tol=1e-10)
        try:
            o.set_graph(g)
            a = o.optimize(3)
            if hook:
                seen = o.testing_warm_start()
                assert seen["warmed"] == 1 and seen["n_prev"] == 3
                for fused in (0, 1):
                    assert o.testing_warm_start(plant, fused)["n_prev"] == 6
                again = o.testing_warm_start()
                for k in ("n_prev", "n_tested", "order", "scale", "bdb", "rdr"):
                    assert again[k] == seen[k], k
                np.testing.assert_array_equal(again["hist"], seen["hist"]); np.testing.assert_array_equal(again["x0"], seen["x0"])
                np.testing.assert_array_equal(again["err"], seen["err"])
            b = o.optimize(3)
            res.append((a, b, o.vertices()))
        finally:
            o.close()
    for ra, rb in zip(res[0][:2], res[1][:2]):
        for k in KEYS:
            np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    np.testing.assert_array_equal(res[0][2], res[1][2])


def test_refusals_leave_the_handle_usable():
    g = wr.graph("g40")
    n = 3 * int((g.v_type == 0).sum())
    o = _handle("amg")
    try:
        with pytest.raises(RuntimeError, match="no graph"):
            o.testing_warm_start()
        o.set_graph(g)
        with pytest.raises(RuntimeError, match="bad argument"):
            o.testing_warm_start(np.zeros((13, n)))
        with pytest.raises(RuntimeError, match="bad argument"):
            o.testing_warm_start(np.zeros((2, n)), fused=2)
        with pytest.raises(RuntimeError, match="bad argument"):
            o.testing_warm_start(fused=-1)
        assert o.lib.tsgo_testing_warm_start(o.h, 0, None, 0, None) < 0 and "bad argument" in o.lib.tsgo_last_error().decode()
        assert o.lib.tsgo_testing_warm_start(o.h, 2, None, 0, None) < 0
        assert o.lib.tsgo_testing_warm_start(None, 0, None, 0, None) < 0 and "null handle" in o.lib.tsgo_last_error().decode()
        out = o.testing_warm_start()
        assert out["warmed"] == 0 and out["n_prev"] == 0 and np.abs(out["b"]).max() > 0
        assert o.optimize(2)["iters"] == 2
        assert o.testing_warm_start()["warmed"] == 1
    finally:
        o.close()
    shard = HipOptimizer(world=2, rank=0, testing=True)
    try:
        with pytest.raises(RuntimeError, match="world > 1"):
            shard.testing_warm_start()
    finally:
        shard.close()
