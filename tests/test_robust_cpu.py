"""Selectable robust kernels per edge class (tsgo_set_robust, include/tsgo.h) on the host side: the declarations, the numpy restatement
(tests/robust.py) against the references that exist already and against its own derivatives, the device's arithmetic (tsgo_math.h:
robust_eval) compiled for the host, and the outlier scenario the GPU tests run, qualified on the dense reference alone."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import independent, lm_rules, priors, robust, util
from toyslam_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["none", ("huber", 1.5), ("huber", 0.5), ("cauchy", 1.5), ("cauchy", 0.5), ("geman_mcclure", 1.5), ("geman_mcclure", 0.5)]


def _grid(delta):
    """s from 1e-6 to 1e6, three per decade, with 0 and both sides of delta^2."""
    d2 = delta * delta
    return np.unique(np.r_[0.0, np.logspace(-6, 6, 37), d2 * (1 - 1e-3), d2, d2 * (1 + 1e-3)])


# ---- 1. declarations ------------------------------------------------------------------------------------------------------------------
def test_the_abi_declares_the_robust_entry_points():
    text = open(os.path.join(ROOT, "include", "tsgo.h")).read()
    for name in ("tsgo_default_robust", "tsgo_set_robust", "tsgo_get_robust"):
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert re.search(r"TSGO_ROBUST_NONE = 0, TSGO_ROBUST_HUBER = 1, TSGO_ROBUST_CAUCHY = 2, TSGO_ROBUST_GEMAN_MCCLURE = 3", text)
    assert "tsgo_default_robust" in _lib.HOST_SYMBOLS
    assert "tsgo_set_robust" in _lib.DEVICE_SYMBOLS and "tsgo_get_robust" in _lib.DEVICE_SYMBOLS
    assert _lib.ROBUST_KERNELS == dict(none=0, huber=1, cauchy=2, geman_mcclure=3)
    assert _lib.ROBUST_CLASSES == robust.CLASSES
    r = _lib.tsgo_robust
    assert [(n, t) for n, t in r._fields_] == [("kernel", C.c_int32 * 5), ("reserved", C.c_int32), ("delta", C.c_double * 5)]
    assert (r.kernel.offset, r.reserved.offset, r.delta.offset, C.sizeof(r)) == (0, 20, 24, 64)


def test_both_libraries_export_them_and_the_default_is_huber_1_5():
    host = _lib.host_lib()
    assert hasattr(host, "tsgo_default_robust")
    libs = [host]
    if os.path.exists(build.HIP_SO):
        hip = _lib.hip_lib()
        for name in ("tsgo_default_robust", "tsgo_set_robust", "tsgo_get_robust"):
            assert hasattr(hip, name), name
        libs.append(hip)
        r = _lib.tsgo_robust()
        hip.tsgo_default_robust(C.byref(r))
        assert hip.tsgo_set_robust(None, C.byref(r)) < 0 and b"tsgo_set_robust" in hip.tsgo_last_error()
        assert hip.tsgo_get_robust(None, C.byref(r)) < 0
    for lib in libs:
        r = _lib.tsgo_robust()
        r.reserved = 7
        lib.tsgo_default_robust(C.byref(r))
        assert list(r.kernel) == [1] * 5 and list(r.delta) == [1.5] * 5 and r.reserved == 0
    assert os.path.exists(build.HIP_SO), "libtsgo_hip.so is not built: tsgo_set_robust(NULL, ...) was not called"


# ---- 2. the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", ["c1", "c1_five_classes"])
def test_huber_1_5_is_the_existing_reference_exactly(graph):
    g = util.c1_arrays() if graph == "c1" else robust.c1_five_classes()
    base = priors.without_priors(g)
    ref, new = independent.Linearisation(base), robust.Linearisation(base, robust.everywhere(("huber", 1.5)))
    np.testing.assert_array_equal(new.w, ref.w)
    assert new.chi2 == ref.chi2 and ref.n_tail > 1000
    for a, b in zip(robust.prior_terms(g, None), priors.prior_terms(g)):
        np.testing.assert_array_equal(a, b)
    H, b, chi, off = robust.dense_system(g)
    H0, b0, chi0, off0 = priors.dense_system(g, independent.Linearisation)
    np.testing.assert_array_equal(H, H0); np.testing.assert_array_equal(b, b0); np.testing.assert_array_equal(off, off0)
    assert chi == chi0


@pytest.mark.parametrize("kernel", KERNELS, ids=str)
def test_the_weight_is_the_derivative_of_rho(kernel):
    """Central differences in long double with h = 1e-6 s.  Truncation: h^2 / 6 times the third derivative = 1e-12 s^2 / 6 times it, a few
    1e-12 w for these kernels: 1e-9 w allows for it.  Rounding: each rho carries a few eps of ITSELF (a saturated kernel has rho = delta^2
    where w = 1e-12), so the quotient carries 8 eps rho / h."""
    delta = 1.5 if kernel == "none" else kernel[1]
    s = _grid(delta)[1:]
    s = s[s != delta * delta].astype(np.longdouble)      # (Huber is C1 only at delta^2: a difference across it is first order; both sides stay)
    h = s * np.longdouble(1e-6)
    rho, w = robust.rho_w(kernel, s)
    fd = (robust.rho_w(kernel, s + h)[0] - robust.rho_w(kernel, s - h)[0]) / (2 * h)
    assert np.all(np.abs(fd - w) <= 1e-9 * w + 8 * np.finfo(np.longdouble).eps * rho / h)
    assert np.all(w > 0) and np.all(w <= 1) and np.all(rho <= s) and np.all(rho >= 0)
    r0, w0 = robust.rho_w(kernel, np.zeros(1))
    assert r0[0] == 0 and w0[0] == 1


@pytest.mark.parametrize("graph", ["tiny_c", "tiny_a"])      # (tiny_c has no ODOM edge, tiny_a has)
@pytest.mark.parametrize("setting", ["none", ("huber", 0.5), ("cauchy", 1.0), ("geman_mcclure", 2.0), "mixed"], ids=str)
def test_the_gradient_of_the_robustified_chi2_is_minus_two_b(setting, graph):
    """tiny_c plus a few priors: d(sum rho)/dx by central differences (h = 1e-5: rounding 2e-16 chi^2 / h, truncation h^2 f''' / 6, both far
    below 1e-6 of the largest entry for a chi^2 of a few thousand) equals -2 b, because every kernel's weight is w = rho'."""
    g = priors.with_priors(util.tiny_arrays(graph), frac_pose=1.0, frac_lm=1.0, seed=3, n_far=1, n_dup=1)
    setting = robust.MIXED if setting == "mixed" else robust.everywhere(setting)
    assert set(np.unique(g.e_type)) >= ({1, 3, 4} if graph == "tiny_c" else {0, 1, 3, 4})
    with lm_rules._Jacobians("analytic"):
        _d, b, chi = robust.linearisation(g, setting)
        fd = np.zeros_like(b)
        h = 1e-5
        for v in range(len(g.v_id)):
            for k in range(3 if g.v_type[v] == 0 else 2):
                up, dn = g.copy(), g.copy()
                up.v_pos[v, k] += h; dn.v_pos[v, k] -= h
                fd[v, k] = float(robust.chi2_at(up, setting) - robust.chi2_at(dn, setting)) / (2 * h)
    print("chi2 %.3f, max |2b| %.3e, max |fd + 2b| %.3e" % (chi, np.abs(2 * b).max(), np.abs(fd + 2 * b).max()))
    assert np.abs(fd + 2 * b).max() <= 1e-6 * np.abs(2 * b).max()


# ---- 3. the device arithmetic on the host ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_arithmetic(tmp_path_factory):
    """(kind, delta, s) rows and what tests/cpp/robust_eval_dump.cpp printed for them; compiled and run once."""
    exe = str(tmp_path_factory.mktemp("robust") / "robust_eval_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "toyslam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "robust_eval_dump.cpp"), "-o", exe])
    rows = [(k, d, float(s)) for k in range(4) for d in (0.5, 1.5) for s in _grid(d)]
    text = "".join("%d %r %r\n" % r for r in rows)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    vals = np.array([[float.fromhex(x) for x in ln.split()] for ln in out if ln])
    assert len(vals) == len(rows)
    return np.array(rows), vals


def _ulps(a, b, dtype):
    return np.abs(a - b) / np.spacing(np.abs(b).astype(dtype)).astype(np.float64)


def test_robust_eval_on_the_host_matches_numpy(device_arithmetic):
    rows, vals = device_arithmetic
    names = ("none", "huber", "cauchy", "geman_mcclure")
    worst64 = worst32 = 0.0
    for kind in range(4):
        for d in (0.5, 1.5):
            k = (rows[:, 0] == kind) & (rows[:, 1] == d)
            s = rows[k, 2]
            rho, w = robust.rho_w("none" if kind == 0 else (names[kind], d), s)
            u64 = max(_ulps(vals[k, 0], rho, np.float64).max(), _ulps(vals[k, 1], w, np.float64).max())
            s32 = s.astype(np.float32).astype(np.float64)                  # what the float instantiation was handed
            rho32, w32 = robust.rho_w("none" if kind == 0 else (names[kind], d), s32)
            u32 = max(_ulps(vals[k, 2], rho32, np.float32).max(), _ulps(vals[k, 3], w32, np.float32).max())
            worst64, worst32 = max(worst64, u64), max(worst32, u32)
            assert vals[k, 0][s == 0] == 0 and vals[k, 1][s == 0] == 1 and vals[k, 2][s == 0] == 0 and vals[k, 3][s == 0] == 1
            assert np.all(np.isfinite(vals[k]))
    print("worst difference from numpy: %.2f ulp (f64), %.2f ulp (f32)" % (worst64, worst32))
    assert worst64 <= 4 and worst32 <= 4


def test_huber_1_5_through_robust_eval_is_the_old_huber_bit_for_bit(device_arithmetic):
    rows, vals = device_arithmetic
    k = (rows[:, 0] == 1) & (rows[:, 1] == 1.5)
    assert k.sum() > 30 and (rows[k, 2] > 2.25).sum() > 10 and (rows[k, 2] < 2.25).sum() > 10
    np.testing.assert_array_equal(vals[k, 0:4], vals[k, 4:8])


# ---- 4. the outlier scenario ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scenario_references():
    """(graph with false closures, optimum of the clean graph, dense LM under the default, dense LM under CAUCHY(1.0) on ODOM)."""
    sc = robust.SCENARIO
    clean = robust.dense_lm(robust.scenario_clean(), None, sc["iterations"], lambda0=sc["lambda0"])
    g = robust.scenario()
    return g, clean, robust.dense_lm(g, None, sc["iterations"], lambda0=sc["lambda0"]), robust.dense_lm(g, sc["robust"], sc["iterations"], lambda0=sc["lambda0"])


def test_cauchy_on_odometry_ends_nearer_the_clean_optimum_than_the_default():
    g, clean, default, cauchy = scenario_references()
    n_pose, n_odom = int((g.v_type == 0).sum()), int((g.e_type == 0).sum())
    n_false = n_odom - int((robust.scenario_clean().e_type == 0).sum())
    assert n_pose <= 300 and not np.any(g.v_type == 1) and 0.04 <= n_false / n_odom <= 0.06
    assert clean["stop"] == "converged"
    e_default = robust.mean_pose_error(default["v_pos"], clean["v_pos"], g.v_type)
    e_cauchy = robust.mean_pose_error(cauchy["v_pos"], clean["v_pos"], g.v_type)
    print("%d poses, %d ODOM edges of which %d false; mean pose error against the clean optimum: default %.4f (%d trials, %s), CAUCHY(1.0) on ODOM %.4f (%d trials, %s)"
          % (n_pose, n_odom, n_false, e_default, default["iters"], default["stop"], e_cauchy, cauchy["iters"], cauchy["stop"]))
    assert e_cauchy < e_default
    # what the device is compared on (tests/test_gpu_robust.py): no decision of either run sits near the accept / reject boundary
    for run in (default, cauchy):
        tol = np.array([lm_rules.rho_tolerance(c, p) for c, p in zip(run["chi2"], run["pred"])])
        assert np.all(np.abs(run["rho"]) > 10 * tol)
        assert np.all(np.diff(np.r_[run["chi2"][0], run["chi2_trial"][run["accepted"]]]) < 0)
