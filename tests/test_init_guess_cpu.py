"""tsgo_init_estimates without a GPU: the host tree (tsgo_init_tree) against the sequential restatement (tests/init_guess.py) on every
shape the device tests run, the restatement itself against the oracle's ODOM residual (zero on every tree edge of a rigid graph), the
effect the feature exists for (dense Levenberg-Marquardt from zeros hits its cap; from the tree's estimates it converges to the optimum of
the run from the generator's start), and a translation unit that calls OptimizerHip::InitEstimates under -Wall -Wextra -Werror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests import init_guess, lm_rules, util
from toyslam_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = init_guess.cases()


def _host_tree(g, mask):
    lib = _lib.host_lib()
    n = len(g.v_id)
    parent = np.full(n, -7, np.int32); edge = np.full(n, -7, np.int32); depth = np.full(n, -7, np.int32)
    st = _lib.tsgo_init_stats()
    cg = g.c_struct()
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    _lib.check(lib, lib.tsgo_init_tree(C.byref(cg), None if m is None else m.ctypes.data, 0 if m is None else len(m), parent.ctypes.data,
                                       edge.ctypes.data, depth.ctypes.data, C.byref(st)), "tsgo_init_tree")
    return parent, edge, depth, {f: getattr(st, f) for f, _t in st._fields_}


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_tree_equals_the_restatement(name):
    g, mask, _poses, _lms = CASES[name]
    parent, edge, depth, st = _host_tree(g, mask)
    rp, re_, rd, _order, counts = init_guess.tree(g, mask)
    np.testing.assert_array_equal(parent, rp)
    np.testing.assert_array_equal(edge, re_)
    np.testing.assert_array_equal(depth, rd)
    for k, v in counts.items():
        assert st[k] == v, (k, st[k], v)
    assert st["poses_set"] == st["landmarks_set"] == st["landmarks_unobserved"] == 0      # a device call's alone


def test_host_tree_errors():
    lib = _lib.host_lib()
    g, _m, _p, _l = CASES["chain_5"]
    cg = g.c_struct()
    short = np.ones(g.n_edges - 1, np.uint8)
    assert lib.tsgo_init_tree(C.byref(cg), short.ctypes.data, len(short), None, None, None, None) < 0
    assert b"n_mask" in lib.tsgo_last_error()
    assert lib.tsgo_init_tree(None, None, 0, None, None, None, None) < 0
    assert lib.tsgo_init_tree(C.byref(cg), None, 0, None, None, None, None) == 0      # every output is optional


@pytest.mark.parametrize("name", ["chain_9", "chain_300_mixed", "chain_5000", "star_70", "closures", "closures_masked", "two_fixed", "two_components"])
def test_tree_edges_have_zero_odometry_residual_after_the_restatement(name):
    """Rigid measurements: T_child = T_parent o (t, theta) makes the edge's ODOM residual zero; s = sum_k inf_k e_k^2 <= 1e-18 max(inf) (1 + extent^2)."""
    g, mask, _p, _l = CASES[name]
    z = init_guess.zeroed(g)
    v, _st = init_guess.initialise(z, mask, poses=True, landmarks=False)
    _parent, edge, _d, _o, _c = init_guess.tree(z, mask)
    out = z.copy(); out.v_pos[:] = v
    keep = out.e_type <= 1
    o = util.to_oracle(out)
    e, _A, _B = oracle.edge_eval(o)
    s = (out.e_inf * e * e).sum(axis=1)
    te = edge[edge >= 0]
    assert keep[te].all()
    extent = float(np.abs(v[:, :2]).max())
    bound = 1e-18 * float(out.e_inf[te].max()) * (1.0 + extent * extent)
    assert len(te) == int((out.v_type == 0).sum()) - int(_c["roots_fixed"] + _c["roots_free"])
    assert s[te].max() <= bound, (s[te].max(), bound)


# ---- the effect: DESIGN.md section 16's table -----------------------------------------------------------------------------------------
TRIALS = 30
REL = 1e-5      # ten times the stop rule's resolution (lm_chi2_rel_tol = 1e-6), on both runs
_runs = {}


def _final(r):
    return float(r["chi2_trial"][-1] if r["accepted"][-1] else r["chi2"][-1])


def _graph(which):
    return lm_rules.synth_600() if which == "synth_600" else lm_rules.loop_closure_pose_graph()


def _run(which, start):
    key = (which, start)
    if key not in _runs:
        g = _graph(which)
        if start != "generator":
            z = init_guess.zeroed(g)
            if start != "zeros":
                mask = None if start == "tree_all" else init_guess.consecutive_mask(g)
                z.v_pos[:], _st = init_guess.initialise(z, mask)
            g = z
        _runs[key] = lm_rules.dense_lm(g, TRIALS)
    return _runs[key]


@pytest.mark.parametrize("which", ["synth_600", "loop_closure"])
def test_from_zeros_the_loop_hits_its_cap(which):
    r = _run(which, "zeros")
    print(which, "zeros", r["iters"], r["stop"], _final(r))
    assert r["stop"] == "cap"


@pytest.mark.parametrize("start", ["tree_all", "tree_consecutive"])
@pytest.mark.parametrize("which", ["synth_600", "loop_closure"])
def test_from_the_tree_the_loop_converges_to_the_generator_runs_optimum(which, start):
    ref, r = _run(which, "generator"), _run(which, start)
    print(which, start, r["iters"], r["stop"], "%.10f" % _final(r), "generator:", ref["iters"], ref["stop"], "%.10f" % _final(ref))
    assert ref["stop"] == "converged"
    assert r["stop"] == "converged"
    assert abs(_final(r) - _final(ref)) <= REL * _final(ref)


def test_wrapper_init_estimates_compiles_without_warnings(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                           os.path.join(ROOT, "tests", "cpp", "init_estimates_demo.cpp"), "-o", str(tmp_path / "init_estimates_demo.o")])
