"""Levenberg-Marquardt with step acceptance (tsgo_config.rules = 2) without a GPU: the ABI layout of the new fields, the dense restatement
of the loop (tests/lm_rules.py) on the c1 fixture, and the input conditions of the GPU parity cases (tests/test_gpu_lm_rules.py), checked
here on the reference alone so that those cannot pass vacuously."""
import ctypes as C
import functools

import numpy as np

from tests import lm_rules
from toyslam_amd import _lib


def test_config_gains_the_lm_fields_behind_every_existing_one():
    names = [f for f, _t in _lib.tsgo_config._fields_]
    assert names[-2:] == ["lm_lambda0", "lm_chi2_rel_tol"]
    assert names[:-2] == ["device", "precision", "pcg_rel_tol", "pcg_max_iters", "lanes_per_pose", "lanes_per_lm", "use_graphs", "rank", "world", "verbose",
                          "preconditioner", "xcd_map", "warm_start", "rules", "lr", "odom_jacobian", "reuse_structure", "cycle_level0", "cycle_storage",
                          "warm_requests"]
    buf = (C.c_uint8 * (C.sizeof(_lib.tsgo_config) + 64))(*([0xAB] * (C.sizeof(_lib.tsgo_config) + 64)))
    cfg = _lib.tsgo_config.from_buffer(buf)
    _lib.host_lib().tsgo_default_config(C.byref(cfg))
    assert (cfg.lm_lambda0, cfg.lm_chi2_rel_tol) == (1e-3, 1e-6)
    # every field in front of them keeps its default, and the library writes nothing behind the struct the bindings declare
    want = dict(device=0, precision=64, pcg_rel_tol=1e-10, pcg_max_iters=20000, lanes_per_pose=0, lanes_per_lm=0, use_graphs=2, rank=0, world=1, verbose=0,
                preconditioner=1, xcd_map=1, warm_start=6, rules=0, lr=0.2, odom_jacobian=0, reuse_structure=1, cycle_level0=0, cycle_storage=16, warm_requests=0)
    assert {k: getattr(cfg, k) for k in want} == want
    assert bytes(buf[C.sizeof(_lib.tsgo_config):]) == b"\xab" * 64


def test_stats_gain_the_lm_traces_behind_every_existing_field():
    names = [f for f, _t in _lib.tsgo_stats._fields_]
    assert names[-5:] == ["steps_rejected", "lm_lambda", "lm_gain", "lm_pred", "lm_chi2_trial"]
    assert names[-6] == "graph_replay"
    assert _lib.tsgo_stats.steps_rejected.offset == _lib.tsgo_stats.graph_replay.offset + 4
    assert C.sizeof(_lib.tsgo_stats) == _lib.tsgo_stats.lm_lambda.offset + 4 * 8 * _lib.TSGO_MAX_TRACE


@functools.lru_cache(maxsize=None)
def _c1(case):
    if case == "plain":
        return lm_rules.dense_lm(lm_rules.c1_plain(), 30)
    return lm_rules.dense_lm(lm_rules.c1_perturbed(), lm_rules.C1_PERTURBED["iterations"], lambda0=lm_rules.C1_PERTURBED["lambda0"])


def test_dense_loop_on_c1_descends_converges_and_needs_fewer_linearisations_than_the_fixed_step():
    r = _c1("plain")
    acc = r["accepted"]
    assert r["stop"] == "converged"
    after = np.r_[r["chi2"][0], r["chi2_trial"][acc]]
    assert np.all(np.diff(after) <= 0)
    assert np.all(np.diff(r["chi2"]) <= 0)             # ... and the chi^2 the trials linearise at never rises either
    gn = lm_rules.dense_gn(lm_rules.c1_plain(), 50)
    print("linearisations: lm %d (%d rejected), fixed step %d (%s)" % (r["iters"], r["rejected"], gn["iters"], gn["stop"]))
    assert r["iters"] < gn["iters"]
    assert r["chi2_trial"][acc][-1] <= gn["chi2"][-1] * (1 + 1e-3)


def test_lambda_follows_the_rule():
    r = _c1("perturbed")
    np.testing.assert_allclose(lm_rules.lambda_trace(lm_rules.C1_PERTURBED["lambda0"], r["rho"], r["pred"]), r["lam"], rtol=1e-15)
    k = int(np.where(~r["accepted"])[0][0])
    assert r["lam"][k + 1] == 2 * r["lam"][k] and r["chi2"][k + 1] == r["chi2"][k]


def test_the_perturbed_case_rejects_and_accepts_and_no_decision_is_near_the_boundary():
    for case in ("plain", "perturbed"):
        r = _c1(case)
        print(case, "trials", r["iters"], "rejected", r["rejected"], "stop", r["stop"], "rho", np.array2string(r["rho"], precision=3))
        tol = np.array([lm_rules.rho_tolerance(c, p) for c, p in zip(r["chi2"], r["pred"])])
        assert np.all(np.abs(r["rho"]) > 10 * tol), (r["rho"], tol)
        assert np.all(r["pred"] > 0)
    r = _c1("perturbed")
    assert r["rejected"] >= 1 and int(r["accepted"].sum()) >= 3
    assert np.all(np.diff(np.r_[r["chi2"][0], r["chi2_trial"][r["accepted"]]]) <= 0)


def test_a_loop_closure_pose_graph_is_refused_at_first_under_the_constant_jacobians():
    """The input of the GPU tests `a rejected step leaves no trace` and `the point of the feature`."""
    g = lm_rules.loop_closure_pose_graph()
    r = lm_rules.dense_lm(g, 1, lambda0=lm_rules.LOOP_LAMBDA0, jacobian="constant")
    assert not r["accepted"][0] and abs(r["rho"][0]) > 10 * lm_rules.rho_tolerance(r["chi2"][0], r["pred"][0])
    assert r["pred"][0] > 0 and r["chi2_trial"][0] > r["chi2"][0]         # the model promised a decrease; the full step raised chi^2
