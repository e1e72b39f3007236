"""The lane sums of the kernels (csrc/tsgo_kernels.h: lane_xor, group_sum, wave_sum, block_sum2) run in the VALU — DPP moves and
permlane swaps — instead of through __shfl_xor.  They must be the SAME sums, bit for bit:

  - the sums themselves, in one workgroup on seeded values (tsgo_testing_lane_sums, include/tsgo_testing.h), against the xor butterfly
    written out in numpy: lane i adds the value of lane i ^ m, masks in the kernel's order, np.float32 / np.float64 adds.  This is what
    settles which half of a permlane swap a lane takes and which way row_shl / row_shr move;
  - whole solves on a graph whose plan has 8 lanes per landmark, a level with 64 lanes per row and the dense bottom — the shapes
    tests/precond_cases.py does not reach — on libtsgo_hip.so against libtsgo_hip_plain.so (TSGO_SHUFFLE_SUMS: the __shfl_xor forms,
    k_cg_step's and the gates' sums one after the other), as tests/test_gpu_kernarg_preload.py does for the cases of precond_cases."""
import ctypes as C
import os

import numpy as np
import pytest

from toyslam_amd import _lib, build, synth
from toyslam_amd.graph import GraphArrays
from toyslam_amd.optimizer import HipOptimizer

GROUPS = (1, 2, 4, 8, 16, 32, 64)
N = 256      # kBlock: one workgroup, four waves


# ---- the butterfly in numpy ---------------------------------------------------------------------------------------------------------
def inputs(dtype, seed=184):
    """256 values of mixed sign, magnitudes spread over 2^-20 .. 2^20 with full mantissas: the sum of any two is rounded, so another
    partner or another order changes bits.  The seed is the first (of 1 .. 199) for which, in BOTH types and in all four waves, the
    ascending butterfly, the descending one and the left-to-right sum are three different numbers (most seeds leave some wave's sums
    equal in two of the orders: a few large values decide them); the test below holds the inputs to that."""
    rng = np.random.default_rng(seed)
    v = rng.choice([-1.0, 1.0], N) * (1.0 + rng.random(N)) * np.exp2(rng.uniform(-20, 20, N))
    return v.astype(dtype)


def butterfly(v, masks):
    """Every lane of every 64-lane wave: v[i] += v[i ^ m] for the masks in order, in v's own type."""
    v = v.copy()
    lane = np.arange(N)
    for m in masks:
        v = v + v[lane ^ m]      # one rounded add per lane (numpy adds arrays of a type in that type)
    return v


def group_sum(v, G):
    return butterfly(v, [m for m in (1, 2, 4, 8, 16, 32) if m < G])


def wave_sum(v):
    return butterfly(v, [32, 16, 8, 4, 2, 1])


def block_sum(v):
    """wave_sum, then the four waves' results added in order 0, 1, 2, 3; every thread gets the same value."""
    w = wave_sum(v)[::64]
    s = w[0]
    for k in range(1, 4):
        s = s + w[k]
    return np.full(N, s, v.dtype)


def expected(v):
    rows = [group_sum(v, G) for G in GROUPS] + [wave_sum(v), block_sum(v), block_sum(v[::-1].copy())]
    return np.stack(rows)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_numpy_butterfly_can_see_a_wrong_order_or_partner(dtype):
    """No GPU: on these inputs the butterfly's result differs from a plain left-to-right sum, from the butterfly with its masks reversed,
    and from lane to lane within a wave — so a sum in another order, or with another partner in one round, cannot pass."""
    v = inputs(dtype)
    assert v.dtype == dtype and butterfly(v, [1]).dtype == dtype
    asc, desc = group_sum(v, 64), wave_sum(v)
    seq = []
    for w in range(4):
        s = dtype(0)
        for x in v[w * 64:(w + 1) * 64]:
            s = dtype(s + x)
        seq.append(s)
    for w in range(4):
        a, d = asc[w * 64:(w + 1) * 64], desc[w * 64:(w + 1) * 64]
        assert len(set(a.tolist())) == 1 and len(set(d.tolist())) == 1      # a butterfly leaves every lane the same bits (commutative adds)
        assert a[0] != d[0], "ascending and descending masks give the same bits: the inputs cannot tell the orders apart"
        assert a[0] != seq[w] and d[0] != seq[w]
    # a wrong partner in one round (xor 4 taken as a rotation by 4 inside the row of 16, the likeliest slip of row_shl / row_shr)
    lane = np.arange(N)
    wrong = v + v[(lane & ~15) | ((lane + 4) & 15)]
    assert (wrong != butterfly(v, [4])).any()
    # and a wrong half of a swap (the lane's own value instead of the partner's)
    assert ((v + v) != butterfly(v, [16])).all() and ((v + v) != butterfly(v, [32])).all()
    for G in GROUPS[1:]:
        assert (group_sum(v, G) != group_sum(v, G // 2)).any()


@pytest.mark.gpu
def test_lane_sums_equal_the_butterfly_bit_for_bit():
    lib = _lib.hip_testing_lib()
    v32, v64 = inputs(np.float32), inputs(np.float64)
    o32, o64 = np.full((len(GROUPS) + 3, N), np.nan, np.float32), np.full((len(GROUPS) + 3, N), np.nan, np.float64)
    _lib.check(lib, lib.tsgo_testing_lane_sums(v32.ctypes.data, v64.ctypes.data, o32.ctypes.data, o64.ctypes.data), "tsgo_testing_lane_sums")
    names = ["group_sum<%d>" % G for G in GROUPS] + ["wave_sum", "block_sum2 a", "block_sum2 b"]
    for got, v in ((o32, v32), (o64, v64)):
        want = expected(v)
        for k, name in enumerate(names):
            np.testing.assert_array_equal(got[k], want[k], err_msg="%s, %s" % (name, v.dtype))


# ---- whole solves, both builds --------------------------------------------------------------------------------------------------------
def hub_graph():
    """~2 000 poses, landmarks seen from ~20 poses each (8 lanes per landmark) and six hub landmarks seen from 150-400 poses."""
    g = synth.make(2000, 12, lm_obs_target=20.0, loop_closures=20, seed=17)
    rng = np.random.default_rng(5)
    poses, lms = g.v_id[g.v_type == 0], g.v_id[g.v_type == 1]
    pos = {int(i): p for i, p in zip(g.v_id, g.v_pos)}
    et, ids, meas, inf = [], [], [], []
    for hub, n in zip(lms[:6], (400, 300, 250, 200, 150, 150)):
        for p in rng.choice(poses, n, replace=False):
            x, y, th = pos[int(p)]
            dx, dy = pos[int(hub)][0] - x, pos[int(hub)][1] - y
            z = np.array([np.cos(th) * dx + np.sin(th) * dy, -np.sin(th) * dx + np.cos(th) * dy]) + rng.normal(0, 0.05, 2)
            et.append(1); ids.append([p, hub]); meas.append([z[0], z[1]] + [0.0] * 7); inf.append([4.0, 4.0, 0.0])
    have = set(map(tuple, g.e_ids[g.e_type == 1].tolist()))
    keep = [k for k, pq in enumerate(ids) if (int(pq[0]), int(pq[1])) not in have]
    sel = lambda a, dt: np.asarray(a, dt)[keep]
    return GraphArrays(g.v_id, g.v_type, g.v_pos, np.concatenate([g.e_type, sel(et, np.uint32)]), np.concatenate([g.e_ids, sel(ids, np.uint32)]),
                       np.concatenate([g.e_meas, sel(meas, np.float64)]), np.concatenate([g.e_inf, sel(inf, np.float64)]), g.fixed)


def lanes_for(avg_row):      # Engine::lanes_for, engine/engine_launch.inc
    return 4 if avg_row <= 4 else (8 if avg_row <= 12 else (32 if avg_row <= 40 else 64))


def plan(g):
    """(lanes per landmark, [lanes per row of the sweeps of every explicit level >= 1], rows per level) from the host probes."""
    lib = _lib.host_lib()
    cg = g.c_struct()
    lay, amg = _lib.tsgo_layout_info(), _lib.tsgo_amg_info()
    _lib.check(lib, lib.tsgo_layout_probe(C.byref(cg), 0, 1, 0, 0, C.byref(lay)), "tsgo_layout_probe")
    _lib.check(lib, lib.tsgo_amg_probe(C.byref(cg), C.byref(amg)), "tsgo_amg_probe")
    rows = [int(amg.rows[l]) for l in range(amg.n_levels)]
    lpr = [lanes_for(amg.blocks[l] / max(1, rows[l])) for l in range(1, amg.n_levels - 1)]
    return int(lay.lanes_per_lm), lpr, rows


def test_the_hub_graph_has_the_plan_the_comparison_is_there_for():
    """No GPU.  8 lanes per landmark; an explicit level whose rows take 64 lanes (none has the 4 096 rows at which the sweeps go to 16);
    a last explicit level of at most 256 rows, which the cycle applies as one dense operator, above a dense coarsest level."""
    g_lm, lpr, rows = plan(hub_graph())
    print(g_lm, lpr, rows)
    assert g_lm == 8
    assert 64 in lpr and max(rows[1:]) < 4096
    assert len(rows) >= 3 and rows[-2] <= 256 and rows[-1] <= 28


@pytest.fixture(scope="module")
def plain_lib():
    if not os.path.exists(build.HIP_PLAIN_SO):
        pytest.fail("%s is missing — run __graft_entry__.build()" % build.HIP_PLAIN_SO)
    lib = C.CDLL(build.HIP_PLAIN_SO)
    _lib._declare_host(lib)
    _lib._declare_device(lib)
    return lib


def _run(monkeypatch, lib, g):
    with monkeypatch.context() as m:
        if lib is not None:
            m.setattr(_lib, "hip_lib", lambda: lib)
        o = HipOptimizer(pcg_rel_tol=1e-10)
        try:
            assert o.lib is (lib if lib is not None else _lib.hip_lib())
            o.set_graph(g)
            step = o.solve_step()
            opt = o.optimize(3)
            return step, opt, o.vertices()
        finally:
            o.close()


@pytest.mark.gpu
def test_both_builds_agree_bit_for_bit_on_the_hub_graph(plain_lib, monkeypatch):
    g = hub_graph()
    step_a, opt_a, v_a = _run(monkeypatch, None, g)
    step_b, opt_b, v_b = _run(monkeypatch, plain_lib, g)
    assert step_a["cg_iters"] > 0 and np.isfinite(step_a["delta"]).all() and np.abs(step_a["delta"]).max() > 0
    np.testing.assert_array_equal(step_a["delta"], step_b["delta"])
    np.testing.assert_array_equal(np.float64(step_a["chi2"]), np.float64(step_b["chi2"]))
    assert step_a["cg_iters"] == step_b["cg_iters"]
    assert opt_a["iters"] == opt_b["iters"] and opt_a["stop"] == opt_b["stop"]
    np.testing.assert_array_equal(opt_a["chi2"], opt_b["chi2"])
    np.testing.assert_array_equal(opt_a["cg_iters"], opt_b["cg_iters"])
    np.testing.assert_array_equal(v_a, v_b)
