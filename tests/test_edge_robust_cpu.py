"""Robust kernels per edge (tsgo_set_edge_robust) without a GPU: the numpy restatement (tests/edge_robust.py) against the per-class one it
extends, the effect that qualifies the feature — on a grid world from the odometry-tree start, Cauchy on the closures alone needs about
half the linearise + solve pairs of Cauchy on the whole ODOM class — and the C++ wrapper's demo."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import edge_robust, init_guess, priors, robust

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 60
CAUCHY = ("cauchy", 1.0)


# ---- 1. the restatement adds nothing where it should add nothing ---------------------------------------------------------------------------
def _same_bits(a, b):
    np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("setting", [None, robust.MIXED], ids=["default", "mixed"])
def test_zero_entries_and_class_equal_entries_restate_the_class_kernels_bit_for_bit(setting):
    g = robust.c1_five_classes()
    full = robust.full(setting)
    palette = [full[c] for c in robust.CLASSES]
    for kernels, entry in (([], np.zeros(len(g.e_type), np.int64)), (palette, g.e_type.astype(np.int64) + 1)):
        base = priors.without_priors(g)
        a, b = robust.Linearisation(base, setting), edge_robust.Linearisation(base, setting, kernels, entry[g.e_type <= 2])
        for f in ("s", "rho", "w", "chi2_exact"):
            _same_bits(getattr(a, f), getattr(b, f))
        for x, y in zip(robust.prior_terms(g, setting), edge_robust.prior_terms(g, setting, kernels, entry)):
            _same_bits(x, y)
        for x, y in zip(robust.linearisation(g, setting), edge_robust.linearisation(g, setting, kernels, entry)):
            _same_bits(x, y)
        for x, y in zip(robust.dense_system(g, setting, zero_fixed=True), edge_robust.dense_system(g, setting, kernels, entry, zero_fixed=True)):
            _same_bits(x, y)
        ra, rb = robust.dense_lm(g, setting, 3), edge_robust.dense_lm(g, setting, kernels, entry, 3)
        for f in ("chi2", "pred", "chi2_trial", "rho", "v_pos"):
            _same_bits(ra[f], rb[f])
    assert robust.Linearisation.__module__ == "tests.robust" and robust.prior_terms.__module__ == "tests.robust"      # per_edge put robust.py back


def test_an_entry_changes_its_edges_and_no_others():
    g = robust.c1_five_classes()
    kernels = ["none", ("cauchy", 0.8), ("geman_mcclure", 2.0)]
    entry = np.arange(len(g.e_type)) % 4
    rec, summ = edge_robust.report(g, None, kernels, entry)
    ref = edge_robust.edge_report.records(g, None)
    np.testing.assert_array_equal(rec[:, :4], ref[:, :4])                       # e and s do not depend on the kernel
    np.testing.assert_array_equal(rec[entry == 0], ref[entry == 0])
    exempt = entry == 1
    np.testing.assert_array_equal(rec[exempt, 4], rec[exempt, 3]); assert np.all(rec[exempt, 5] == 1.0)
    for t in range(5):                                                          # every class meets every entry and 0, and some kernel's tail
        for k in range(4):
            assert ((g.e_type == t) & (entry == k)).sum() >= 2, (t, k)
        assert (rec[(g.e_type == t) & (entry > 1), 5] < 1).any(), t
    assert [summ[c]["edges"] for c in robust.CLASSES] == [int((g.e_type == t).sum()) for t in range(5)]
    d, gr, chi = edge_robust.linearisation(g, None, kernels, entry)
    assert abs(chi - rec[:, 4].sum()) <= 1e-12 * chi
    assert abs(chi - robust.linearisation(g, None)[2]) > 1e-3 * chi


# ---- 2. the effect ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_runs(seed):
    """error and trials of the three settings on grid_world(200, seed) from the tree start, against the clean graph's optimum."""
    clean, g = edge_robust.grid_world(200, seed)
    ref = robust.dense_lm(edge_robust.start(clean), robust.everywhere("none"), CAP)
    assert ref["stop"] == "converged"
    z = edge_robust.start(g)
    runs = dict(default=robust.dense_lm(z, None, CAP), class_wide=robust.dense_lm(z, dict(odom=CAUCHY), CAP),
                closures=edge_robust.dense_lm(z, dict(odom=CAUCHY), *edge_robust.chain_exempt(g), CAP))
    return {k: (robust.mean_pose_error(r["v_pos"], ref["v_pos"], g.v_type), r["iters"], r["stop"]) for k, r in runs.items()}


def test_cauchy_on_the_closures_alone_needs_fewer_trials_than_on_the_whole_class():
    """Measured when the feature was written (mean pose error against the clean optimum / trials; the default stops at the cap of 60):

        seed   Huber 1.5 (default)   Cauchy 1.0 on class ODOM   Cauchy 1.0 on closures, chain exempt
        0      10.4050 / 60          0.1063 / 39                0.0824 / 22
        1       8.4687 / 60          0.0505 / 31                0.0425 / 15
        2       7.1654 / 60          0.0918 / 39                0.0894 / 17
        3       3.4663 / 60          0.0720 / 38                0.0506 / 16
    """
    print("seed | Huber 1.5 (default) | Cauchy 1.0 on class ODOM | Cauchy 1.0 on closures, chain exempt   (error / trials, stop)")
    rows = {seed: grid_runs(seed) for seed in range(4)}
    for seed, r in rows.items():
        print("%4d | %s" % (seed, " | ".join("%.4f / %d, %s" % r[k] for k in ("default", "class_wide", "closures"))))
    for seed, r in rows.items():
        assert r["default"][2] == "cap" and r["default"][1] == CAP, seed
        assert r["class_wide"][2] == "converged" and r["closures"][2] == "converged", seed
        assert r["closures"][1] < r["class_wide"][1], seed
        assert r["closures"][0] <= 1.5 * r["class_wide"][0], seed


def test_on_the_repositorys_scenario_the_two_settings_end_the_same():
    """robust.scenario() starts near the optimum: printed only, nothing is claimed there."""
    sc = robust.SCENARIO
    g = robust.scenario()
    clean = robust.dense_lm(robust.scenario_clean(), None, CAP, lambda0=sc["lambda0"])
    for what, z in (("its own start", g), ("the odometry-tree start", edge_robust.start(g))):
        a = robust.dense_lm(z, sc["robust"], CAP, lambda0=sc["lambda0"])
        b = edge_robust.dense_lm(z, sc["robust"], *edge_robust.chain_exempt(g), CAP, lambda0=sc["lambda0"])
        print("scenario from %s: Cauchy 1.0 on the ODOM class %.4f / %d trials; on the closures, chain exempt %.4f / %d trials"
              % (what, robust.mean_pose_error(a["v_pos"], clean["v_pos"], g.v_type), a["iters"], robust.mean_pose_error(b["v_pos"], clean["v_pos"], g.v_type), b["iters"]))


def test_the_chain_mask_of_the_grid_world_is_its_odometry():
    clean, g = edge_robust.grid_world(200, 0)
    chain = init_guess.consecutive_mask(g)
    assert chain.sum() == 199 and np.all(chain[:199] == 1)
    n_false = len(g.e_type) - len(clean.e_type)
    n_closures = len(clean.e_type) - 199
    print("grid world, seed 0: %d closures, %d false" % (n_closures, n_false))
    assert n_false == max(3, int(round(0.10 * n_closures)))
    np.testing.assert_array_equal(g.e_meas[:len(clean.e_type)], clean.e_meas)      # the false closures are appended, nothing else moves


# ---- 3. the wrapper ---------------------------------------------------------------------------------------------------------------------
def test_the_cpp_demo_compiles_against_the_wrapper(tmp_path):
    lib_dir = os.path.join(ROOT, "toyslam_amd")
    if not os.path.exists(os.path.join(lib_dir, "libtsgo_hip.so")):
        pytest.fail("toyslam_amd/libtsgo_hip.so is not built (run __graft_entry__.build())")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "edge_robust_demo.cpp"), "-o", str(tmp_path / "edge_robust_demo"),
                           "-L" + lib_dir, "-ltsgo_hip", "-Wl,-rpath," + lib_dir])
