"""Powell's dogleg (tsgo_config.rules = 3) on the CPU alone: the ABI of the new structs and entry points, the layouts that must not move,
and the QUALIFICATION of the cases tests/test_gpu_dogleg.py runs on the device — on the dense restatement (tests/dogleg.py) every trial of
every case takes its decisions well away from their boundaries, so that the device run can be compared decision by decision, and every
case shows what it is there for (a rejection, a shrinking accepted step, a doubled radius, the three kinds of step), so that none passes
vacuously."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from tests import dogleg, lm_rules
from toyslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_the_new_structs_have_the_header_s_shape():
    T = _lib.TSGO_MAX_TRACE
    assert [f for f, _t in _lib.tsgo_dogleg_params._fields_] == ["radius0", "radius_min", "radius_max", "chi2_rel_tol"]
    assert C.sizeof(_lib.tsgo_dogleg_params) == 32
    assert [f for f, _t in _lib.tsgo_dogleg_trace._fields_] == ["trials", "solves", "kind", "solved", "radius", "step_norm", "gg", "gHg", "gd", "dd", "radius_last"]
    assert _lib.tsgo_dogleg_trace.kind.offset == 8 and _lib.tsgo_dogleg_trace.radius.offset == 8 + 2 * 4 * T
    assert C.sizeof(_lib.tsgo_dogleg_trace) == 8 + 2 * 4 * T + 6 * 8 * T + 8
    text = open(os.path.join(ROOT, "include", "tsgo.h")).read()
    m = re.search(r"typedef struct tsgo_dogleg_params \{([^}]*)\}", text)
    assert re.findall(r"\b(radius0|radius_min|radius_max|chi2_rel_tol)\b", m.group(1)) == ["radius0", "radius_min", "radius_max", "chi2_rel_tol"]
    m = re.search(r"typedef struct tsgo_dogleg_trace \{(.*?)\} tsgo_dogleg_trace;", text, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"\b([A-Za-z_]+)(?:\[TSGO_MAX_TRACE\])?\s*[,;]", body) == ["trials", "solves", "kind", "solved", "radius", "step_norm", "gg", "gHg", "gd", "dd", "radius_last"]
    assert "TSGO_STOP_RADIUS = 6" in text


def test_defaults_through_the_host_library():
    host = _lib.host_lib()
    p = _lib.tsgo_dogleg_params(-1, -1, -1, -1)
    host.tsgo_default_dogleg(C.byref(p))
    assert (p.radius0, p.radius_min, p.radius_max, p.chi2_rel_tol) == (1e4, 1e-9, 1e9, 1e-6)
    assert (p.radius0, p.radius_min, p.radius_max, p.chi2_rel_tol) == tuple(dogleg.DEFAULTS[k] for k in ("radius0", "radius_min", "radius_max", "chi2_rel_tol"))
    host.tsgo_default_dogleg(None)      # a NULL pointer is ignored


def test_symbols_are_listed_where_they_belong():
    assert "tsgo_default_dogleg" in _lib.HOST_SYMBOLS
    for s in ("tsgo_set_dogleg", "tsgo_get_dogleg", "tsgo_get_dogleg_trace"):
        assert s in _lib.DEVICE_SYMBOLS and s not in _lib.HOST_SYMBOLS


def test_config_and_stats_layouts_did_not_move():
    assert [f for f, _t in _lib.tsgo_config._fields_][-2:] == ["lm_lambda0", "lm_chi2_rel_tol"]
    assert [f for f, _t in _lib.tsgo_stats._fields_][-5:] == ["steps_rejected", "lm_lambda", "lm_gain", "lm_pred", "lm_chi2_trial"]
    assert C.sizeof(_lib.tsgo_stats) == _lib.tsgo_stats.lm_lambda.offset + 4 * 8 * _lib.TSGO_MAX_TRACE
    assert len(_lib.tsgo_config._fields_) == 22 and len(_lib.tsgo_stats._fields_) == 28
    text = open(os.path.join(ROOT, "include", "tsgo.h")).read()
    cfg = re.search(r"typedef struct tsgo_config \{(.*?)\} tsgo_config;", text, flags=re.S).group(1)
    assert "dogleg" not in re.sub(r"/\*.*?\*/", "", cfg, flags=re.S) and "radius" not in re.sub(r"/\*.*?\*/", "", cfg, flags=re.S)


# ---- the radius rule ----------------------------------------------------------------------------------------------------------------------
def test_radius_rule():
    assert dogleg.next_radius(8.0, 0.1, 1, 6.0) == 1.5                    # a poor gain shrinks to a quarter of the step, accepted or not
    assert dogleg.next_radius(8.0, -2.0, 0, 6.0) == 1.5
    assert dogleg.next_radius(8.0, float("nan"), 2, 6.0) == 1.5           # a NaN shrinks (and rejects)
    assert dogleg.next_radius(8.0, 0.9, 1, 8.0) == 16.0 and dogleg.next_radius(8.0, 0.9, 2, 8.0) == 16.0
    assert dogleg.next_radius(8.0, 0.9, 0, 3.0) == 8.0                    # a Gauss-Newton step inside the region says nothing about the radius
    assert dogleg.next_radius(8.0, 0.5, 1, 8.0) == 8.0
    assert dogleg.next_radius(8e8, 0.9, 1, 8e8) == 1e9                    # capped
    tr, last = dogleg.radius_trace(4.0, [0.9, 0.1, 0.5], [1.0, 1.0, 1.0], [1, 1, 0], [4.0, 8.0, 1.0])
    np.testing.assert_array_equal(tr, [4.0, 8.0, 2.0])
    assert last == 2.0


def test_step_kinds_on_a_small_system():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(6, 6)); H = A @ A.T + 0.1 * np.eye(6); b = rng.normal(size=6)
    d_gn = np.linalg.solve(H, b)
    cauchy = (b @ b) / (b @ H @ b) * np.linalg.norm(b)
    assert cauchy < np.linalg.norm(d_gn)
    k0, d0 = dogleg.step_of(b, d_gn, H, 2 * np.linalg.norm(d_gn))
    k2, d2 = dogleg.step_of(b, d_gn, H, 0.5 * cauchy)
    k1, d1 = dogleg.step_of(b, d_gn, H, 0.5 * (cauchy + np.linalg.norm(d_gn)))
    assert (k0, k1, k2) == (0, 1, 2)
    np.testing.assert_array_equal(d0, d_gn)
    assert abs(np.linalg.norm(d2) - 0.5 * cauchy) < 1e-12 and abs(np.linalg.norm(d1) - 0.5 * (cauchy + np.linalg.norm(d_gn))) < 1e-12
    model = lambda d: 2 * b @ d - d @ H @ d       # noqa: E731  (the decrease the model predicts: larger along the dogleg path as the radius grows)
    assert 0 < model(d2) < model(d1) < model(d0)


# ---- qualification of the GPU cases -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref(case):
    return dogleg.reference(case)


def _qualify(case):
    """No trial of the reference sits near a decision boundary: the accept test, the two thresholds of the radius rule, the two tests that
    choose the kind of step; and every predicted decrease is positive."""
    _g, r, _kw, _n, _jac = _ref(case)
    n, alpha = np.sqrt(r["gg"]), r["gg"] / r["gHg"]
    tol = np.array([lm_rules.rho_tolerance(c, p) for c, p in zip(r["chi2"], r["pred"])])
    print(case, "kinds", r["kind"], "solved", r["solved"], "stop", r["stop"], "\n  radius", r["radius"], "\n  gain", r["rho"], "\n  pred", r["pred"], "\n  chi2", r["chi2"],
          "\n  chi2_trial", r["chi2_trial"], "\n  sqrt(dd)/radius", np.sqrt(r["dd"]) / r["radius"], "\n  alpha n/radius", alpha * n / r["radius"])
    assert np.all(r["pred"] > 0)
    assert np.all(np.abs(r["rho"]) > 10 * tol)
    assert np.all(np.abs(r["rho"] - 0.25) > 0.05) and np.all(np.abs(r["rho"] - 0.75) > 0.05)
    assert np.all(np.abs(np.sqrt(r["dd"]) / r["radius"] - 1) > 1e-3) and np.all(np.abs(alpha * n / r["radius"] - 1) > 1e-3)
    # the closed form of the header (H d_gn = b) against the dense 2 b'd - d'Hd, on every trial
    c1c2 = {0: lambda k: (0.0, 1.0), 2: lambda k: (r["radius"][k] / n[k], 0.0)}
    for k in range(r["iters"]):
        if r["kind"][k] == 1:
            a = r["dd"][k] - 2 * alpha[k] * r["gd"][k] + alpha[k] ** 2 * r["gg"][k]; h = alpha[k] * r["gd"][k] - alpha[k] ** 2 * r["gg"][k]
            c = alpha[k] ** 2 * r["gg"][k] - r["radius"][k] ** 2
            beta = (-h + np.sqrt(h * h - a * c)) / a
            assert 0 < beta < 1
            c1, c2 = alpha[k] * (1 - beta), beta
        else:
            c1, c2 = c1c2[int(r["kind"][k])](k)
        closed = 2 * (c1 * r["gg"][k] + c2 * r["gd"][k]) - (c1 * c1 * r["gHg"][k] + 2 * c1 * c2 * r["gg"][k] + c2 * c2 * r["gd"][k])
        assert abs(closed - r["pred"][k]) <= 1e-8 * abs(r["pred"][k])
        assert abs(np.sqrt(c1 * c1 * r["gg"][k] + 2 * c1 * c2 * r["gd"][k] + c2 * c2 * r["dd"][k]) - r["step_norm"][k]) <= 1e-9 * r["step_norm"][k]
    rt, last = dogleg.radius_trace(r["radius"][0], r["rho"], r["pred"], r["kind"], r["step_norm"])
    np.testing.assert_array_equal(rt, r["radius"])
    assert last == r["radius_last"]
    return r


def test_case_a_rejects_once_shrinks_on_an_accepted_step_and_doubles_twice():
    r = _qualify("A")
    assert r["iters"] == 10 and r["stop"] == "cap"
    np.testing.assert_array_equal(r["kind"], [0, 0, 0, 1, 1, 1, 1, 1, 0, 0])
    np.testing.assert_array_equal(np.where(~r["accepted"])[0], [2])
    assert abs(r["rho"][2] - (-0.0225)) < 2e-3
    assert r["radius"][3] == 0.25 * r["step_norm"][2] and abs(r["radius"][3] - 113.07) < 0.01
    assert r["solves"] == 9 and list(r["solved"]) == [1, 1, 1, 0, 1, 1, 1, 1, 1, 1]
    shrunk = r["accepted"] & (r["rho"] < 0.25)
    assert shrunk.sum() == 1 and abs(r["rho"][shrunk][0] - 0.13) < 0.02
    k = int(np.where(shrunk)[0][0])
    assert r["radius"][k + 1] == 0.25 * r["step_norm"][k] < r["radius"][k]
    # the radius doubles twice after the rejection (trials 3, 4), and twice again after the accepted step that shrank it (trials 6, 7)
    assert k == 5
    np.testing.assert_array_equal(np.where(r["radius"][1:] == 2 * r["radius"][:-1])[0], [3, 4, 6, 7])


def test_case_b_walks_out_along_the_gradient_and_doubles_every_time():
    r = _qualify("B")
    assert r["iters"] == 5 and r["stop"] == "cap" and r["rejected"] == 0
    np.testing.assert_array_equal(r["kind"], [2, 2, 1, 1, 1])
    np.testing.assert_array_equal(r["radius"], [1, 2, 4, 8, 16])


def test_case_c_three_rejections_on_one_solve():
    r = _qualify("C")
    assert r["iters"] == 3 and r["stop"] == "cap" and r["rejected"] == 3 and not r["accepted"].any()
    assert r["solves"] == 1 and list(r["solved"]) == [1, 0, 0]
    np.testing.assert_array_equal(r["kind"], [0, 1, 1])
    assert np.all(r["chi2_trial"] > r["chi2"]) and np.all(r["chi2"] == r["chi2"][0])
    for k in ("gg", "gHg", "gd", "dd"):
        assert np.all(r[k] == r[k][0])


@pytest.mark.parametrize("variant", ["plain", "vlm", "priors"])
def test_case_d_takes_dogleg_steps_so_that_ghg_enters_pred(variant):
    g, r = _ref("D_" + variant)[:2]
    assert {"vlm": (g.e_type == 2).sum() > 20, "priors": (g.e_type >= 3).sum() > 100 and len(g.fixed) == 0}.get(variant, True)
    _qualify("D_" + variant)
    assert r["iters"] == 5
    assert np.all(r["kind"][:4] == 1)
    # with the default radius these graphs take Gauss-Newton steps only, where gHg never enters: that would be no test of the g'Hg pass
    wide = dogleg.dense_dogleg(g, 2)
    assert np.all(wide["kind"] == 0)


def test_c1_plain_converges_with_gauss_newton_steps():
    r = _qualify("c1_plain")
    assert r["stop"] == "converged" and r["iters"] == 5 and r["rejected"] == 0
    assert np.all(r["kind"] == 0) and r["solves"] == r["iters"]


def test_the_numbers_the_feature_was_proposed_with():
    """The loop-closure graph under the constant Jacobians: three trials, three rejections, ONE linearisation and solve, where the
    Levenberg-Marquardt restatement runs three of each; c1_perturbed from radius 1e4: lower after 16 trials than that loop."""
    r = _ref("C")[1]
    assert (r["solves"], r["rejected"]) == (1, 3)
    g = lm_rules.c1_perturbed()
    d = dogleg.dense_dogleg(g, 16, radius0=1e4)
    kept = np.r_[d["chi2"][0], d["chi2_trial"][d["accepted"]]]
    assert abs(kept[0] / 2.098e6 - 1) < 1e-3 and abs(kept[-1] / 619.0 - 1) < 1e-3 and d["rejected"] == 1
    assert np.all(np.diff(kept) < 0)
