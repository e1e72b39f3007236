"""The multigrid preconditioner as an OPERATOR: what tsgo_testing_apply (include/tsgo_testing.h) reads out of a handle, column by
column, against dense S (products) and against the f64 CPU twin of the cycle (oracle.twin_precond) in the energy norm of S.  PCG
converges to the same answer with any SPD M^-1, so the parity tests cannot see a wrong cycle; these can.

Cases, inputs and the distance: tests/precond_cases.py.  Every test asserts which branch of launch_vcycle_v it ran from the kernel names
of tsgo_profile_iteration, and that the twin ran on a hierarchy of the same level sizes (and, where tsgo_amg_probe can build it — default
layout options, constant Jacobians — of the same checksum).

The batched cycle of tsgo_marginals (which = 3) keeps every vector in the handle's type (f64) and reads the hierarchy's block-indexed
f32 matrices (HT<T>), never the packed cycle-format copies; its level-0 products read the f64 planes: it belongs to the first rung.

Products: the bound c * 3 deg_max * u * (|S| |x|) holds entry by entry only for a product that sums the entries of S.  The implicit
product never forms S: it sums Hpp x and W (Dl^-1 (W^T x)), which cancel (an entry of S of 2e-19 comes out of terms of order 1, and
carries their rounding: measured 2e-17 there, relative error of the whole column 6e-16).  The bound is therefore taken with the
magnitude of the terms actually summed (tests/precond_cases.py: product_bound), in place of |S| — for the explicit level-0 matrix too,
whose blocks are the same sums.  u is 2^-53 for PCG's product on an f64 handle and 2^-24 for everything in f32: the in-cycle product
and both products of an f32 handle (precision = 32), whose planes are linearised in f32 as well.

The ladder (precond_cases.LADDER) has the issue's three rungs on f64 handles and two more on f32 handles (cycle storage f32 / packed
halves); the sensitivity condition on the limits is checked on the CPU (tests/test_precond_twin_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

from tests import precond_cases as pc
from toyslam_amd import _lib
from toyslam_amd.optimizer import HipOptimizer


def _handle(case, rung=None, **over):
    c = pc.CASES[case]
    kw = dict(pcg_rel_tol=1e-10, testing=True)
    kw.update(c["kw"])
    env = dict(c["env"])
    if rung is not None:
        kw["cycle_storage"] = pc.RUNGS[rung]["storage"]
        kw["precision"] = pc.RUNGS[rung]["precision"]
        if pc.RUNGS[rung]["vec64"]:
            env["TSGO_CYCLE_VEC64"] = "1"
    kw.update(over)
    g = c["graph"]()
    with pc.Env(env):
        o = HipOptimizer(**kw)
        o.set_graph(g)
    return o, g, env


def _branch_and_hierarchy(o, g, case, env, info, tname="double"):
    c = pc.CASES[case]
    with pc.Env(env):
        names = ["%s | %s" % (e["name"], e["where"]) for e in o.profile_iteration(2)]
        rows = [int(r) for r in (lv.rows for lv in _levels(o))]
    text = "\n".join(names)
    for k in c["must"]:
        assert k.replace("double", tname) in text, (case, k, names)
    assert "k_schur_pose<%s" % tname in text and "k_schur_lm<%s" % tname in text and "k_cg_step<%s" % tname in text, names
    for k in c["must_not"]:
        assert k not in text, (case, k, names)
    assert rows == info["rows"][1:-1], (rows, info["rows"])
    if not c["kw"].get("lanes_per_pose") and c["kw"].get("odom_jacobian", "constant") == "constant":
        with pc.Env(c["env"]):
            ai = _lib.tsgo_amg_info(); cg = g.c_struct()
            assert _lib.hip_testing_lib().tsgo_amg_probe(C.byref(cg), C.byref(ai)) == 0
        assert ai.checksum == info["checksum"] and list(ai.rows[:ai.n_levels]) == info["rows"]
    return text


def _levels(o):
    arr = (_lib.tsgo_cycle_level * 16)()
    n = o.lib.tsgo_cycle_probe(o.h, 1, arr, 16)
    assert n >= 0
    return [arr[k] for k in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("case,rung", pc.PAIRS)
def test_cycle_matches_the_twin_and_products_match_dense_S(case, rung):
    S, mag, R, Z, info = pc.reference(case)
    p32 = pc.RUNGS[rung]["precision"] == 32
    uv = np.random.default_rng(13).normal(size=(S.shape[0], 2))      # linearity: two interior (Gaussian) vectors
    o, g, env = _handle(case, rung)
    try:
        text = _branch_and_hierarchy(o, g, case, env, info, "float" if p32 else "double")
        assert ("double>" if pc.RUNGS[rung]["vec64"] else "float>") in text.split("k_restrict")[1].split("|")[0]
        with pc.Env(env):
            y0 = o.testing_apply(0, R); y1 = o.testing_apply(1, R)
            z = o.testing_apply(2, R); z_again = o.testing_apply(2, R)
            zuv = o.testing_apply(2, uv)
            zl = o.testing_apply(2, 0.75 * uv[:, 0] - 1.5 * uv[:, 1])
    finally:
        o.close()
    if case == "mixed_analytic":      # what the case is there for, from the twin's tables and both operators
        agg = info["agg"]
        assert set(np.unique(g.e_type)) == {0, 1, 2, 3, 4}
        assert (agg == agg[pc.MIXED_FIXED_POSE]).sum() > 1 and (agg == agg[pc.MIXED_DEAD_POSE]).sum() == 1
        dead = slice(3 * pc.MIXED_DEAD_POSE, 3 * pc.MIXED_DEAD_POSE + 3)
        assert np.abs(S[dead]).max() == 0 and np.abs(Z[dead]).max() == 0 and np.abs(z[dead]).max() == 0      # the `dead` rule: kept out of every level
    deg = pc.deg_max(S); want = S @ R
    # PCG's own product, in the handle's precision
    b0 = pc.product_bound(mag, R, 2.0 ** -24 if p32 else 2.0 ** -53, deg) + 1e-300
    # the in-cycle product: f32 copies of planes and vector (implicit), or the explicit matrix in the cycle's storage: f32, or packed
    # halves — an 11-bit significand under the block's common exponent: 2^-11 max|block| per entry on top of the f32 arithmetic
    b1 = pc.product_bound(mag, R, 2.0 ** -24, deg) + 1e-300
    if pc.CASES[case]["kw"].get("cycle_level0") == "explicit" and pc.RUNGS[rung]["storage"] == 16:
        P = S.shape[0] // 3
        bmax = np.abs(S).reshape(P, 3, P, 3).max(axis=(1, 3))
        b1 = b1 + 2.0 ** -11 * (np.repeat(np.repeat(bmax, 3, 0), 3, 1) @ np.abs(R))
    r0 = float((np.abs(y0 - want) / b0).max()); r1 = float((np.abs(y1 - want) / b1).max())
    print("case %s rung %s: product error / bound: PCG %.3e, in-cycle %.3e" % (case, rung, r0, r1))
    d = pc.energy_distance(z, Z, S)
    # linearity: M(a u + b v) against a M u + b M v, relative to |a| ||M u||_S + |b| ||M v||_S: the product bound's factor times the
    # cycle's depth (two transfers or sweeps per level and side), in f32: on every rung the level-0 products inside the cycle read the
    # f32 copies of the pose records (the explicit level 0 does not: it stays far below)
    a, b = 0.75, -1.5
    e = zl - a * zuv[:, 0] - b * zuv[:, 1]
    nS = lambda v: float(np.sqrt(max(v @ S @ v, 0.0)))      # noqa: E731
    lin = nS(e) / (abs(a) * nS(zuv[:, 0]) + abs(b) * nS(zuv[:, 1]))
    depth = 4 * len(info["rows"])
    u = 2.0 ** -24
    lin_bound = pc.C_PRODUCT * 3 * deg * depth * u
    print("case %s rung %s: distance to the twin max %.3e median %.3e; linearity %.3e (bound %.3e)" % (case, rung, d.max(), np.median(d), lin, lin_bound))
    np.testing.assert_array_equal(z, z_again)
    assert r0 <= 1.0 and r1 <= 1.0, (r0, r1)
    assert lin <= lin_bound, (lin, lin_bound)
    assert d.max() <= pc.limit(rung), (case, rung, float(d.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [k for k, c in pc.CASES.items() if c["full"]])
@pytest.mark.parametrize("rung", [r for r in pc.RUNGS if pc.RUNGS[r]["precision"] == 64])
def test_what_pcg_needs_from_the_whole_matrix(case, rung):
    S, _mag, R, Z, info = pc.reference(case)      # R = I: Z is the twin's matrix
    o, g, env = _handle(case, rung)
    try:
        with pc.Env(env):
            M = o.testing_apply(2, R)
    finally:
        o.close()
    assert np.linalg.norm(M - M.T) / np.linalg.norm(M) <= pc.limit(rung)
    assert np.linalg.eigvalsh(0.5 * (M + M.T)).min() > 0
    w = np.linalg.eigvals(M @ S); wt = np.linalg.eigvals(Z @ S)
    assert np.abs(w.imag).max() <= pc.limit(rung) * np.abs(w).max() and w.real.min() > 0
    assert w.real.max() / w.real.min() <= 1.1 * wt.real.max() / wt.real.min()


@pytest.mark.gpu
def test_block_jacobi_operator_is_the_inverse_diagonal_blocks():
    case = "level0_only"
    S, _mag, R, _Z, _info = pc.reference(case)
    o, _g, env = _handle(case, preconditioner="jacobi")
    try:
        M = o.testing_apply(2, R)
        with pytest.raises(RuntimeError):
            o.testing_apply(1, R[:, :1])
    finally:
        o.close()
    P = S.shape[0] // 3
    D = np.zeros_like(S)
    for i in range(P):
        D[3 * i:3 * i + 3, 3 * i:3 * i + 3] = np.linalg.inv(S[3 * i:3 * i + 3, 3 * i:3 * i + 3])
    # a 3x3 inverse by cofactors: the bound of a 3-term product chain, scaled by the block's condition number
    kappa = max(np.linalg.cond(S[3 * i:3 * i + 3, 3 * i:3 * i + 3]) for i in range(P))
    assert np.abs(M - D).max() <= pc.C_PRODUCT * 9 * 2.0 ** -53 * kappa * np.abs(D).max()


@pytest.mark.gpu
def test_batched_cycle_matches_the_twin_and_columns_do_not_couple():
    case = "dense_bottom"
    S = pc.reference(case)[0]
    rng = np.random.default_rng(11)
    X = rng.normal(size=(S.shape[0], 16))
    Zt, _ = pc.twin(case, X)
    o, _g, env = _handle(case, "vec64_f32")
    try:
        with pc.Env(env):
            zb = o.testing_apply(3, X)
            zeros = o.testing_apply(3, np.concatenate([X[:, :1], np.zeros((S.shape[0], 15))], axis=1))
            single = o.testing_apply(2, X)
    finally:
        o.close()
    d = pc.energy_distance(zb, Zt, S)
    print("batched cycle to the twin: max %.3e; to the single-column cycle: max %.3e" % (d.max(), pc.energy_distance(zb, single, S).max()))
    assert d.max() <= pc.limit("vec64_f32")
    # a column's result does not depend on its neighbours: with 15 others and with 15 zero columns (which is also what a call with
    # fewer columns than the batch is wide computes: the unused columns of the batch are zero)
    np.testing.assert_array_equal(zeros[:, 0], zb[:, 0])


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_a_probe_call_leaves_the_next_solve_unchanged(which):
    case = "dense_bottom"
    S = pc.reference(case)[0]
    x = np.random.default_rng(5).normal(size=(S.shape[0], 2))
    o, _g, env = _handle(case, "vec64_f32")
    o_ref, _g2, _e = _handle(case, "vec64_f32")
    try:
        with pc.Env(env):
            o.testing_apply(which, x)
            a = o.solve_step(); b = o_ref.solve_step()
    finally:
        o.close(); o_ref.close()
    np.testing.assert_array_equal(a["delta"], b["delta"])
    assert a["cg_iters"] == b["cg_iters"] and a["chi2"] == b["chi2"]
