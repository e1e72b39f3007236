"""The graphs, options and inputs of the preconditioner-operator tests (tests/test_precond_twin_cpu.py on the CPU twin alone,
tests/test_gpu_precond_operator.py on the device), and the f64 arithmetic both share: the energy-norm distance between two operators.

Every case names the branch of Engine::launch_vcycle_v (engine/engine_launch.inc) it is there for, by the kernels an iteration must and
must not launch.  The shapes follow from host/amg.h: aggregates of 4 / 4 / 8 nodes, coarsening stops at <= 28 block rows (kCoarsestMax);
the hierarchy of P poses is therefore [P, ~P/4, ~P/16, ...] down to the first level of at most 28 rows, which is the dense one.

No case has a hub landmark (more than kMaxPairDegree = 64 observers: the synthetic graphs aim at 5), and the probe builds its hierarchy
for the linearisation it probes, so the explicit level-0 matrix of cycle_level0 = 1 is S itself up to its storage format.

Not reached below 1 500 poses: lanes_for_sweep's 16-lane rows (a coarse level of >= 4 096 rows needs > 16 000 poses) and the XCD-aware
workgroup map (>= 64 workgroups of a block-row kernel: > 4 000 rows at 4 lanes per row).  They stay with the 10k / 100k-pose parity tests."""
import os

import numpy as np

from oracle import oracle
from tests import priors, util
from toyslam_amd import synth
from toyslam_amd.graph import GraphArrays

KNOBS = ("TSGO_AGG_LIST", "TSGO_AGG0", "TSGO_AGGC", "TSGO_SWEEPS_LIST", "TSGO_CYCLE_VEC64", "TSGO_FUSE_POST", "TSGO_FOLD_GATE", "TSGO_MARGINAL_WIDTH")


def _mixed(with_priors=False):
    """Edge types 0-2 (0-4 with_priors) in one graph; a pose nobody refers to (the prolongator's `dead` rule); a second fixed pose in
    the middle of the trajectory, hence in the middle of an aggregate."""
    g = synth.make(130, 6, loop_closures=4, seed=5)
    g = util.with_virtual_landmarks(g, fraction=0.3, seed=2)
    g = priors.with_priors(g, frac_pose=0.1 if with_priors else 0.0, frac_lm=0.1 if with_priors else 0.0, seed=3, n_far=2 if with_priors else 0,
                           n_dup=1 if with_priors else 0, fixed=[0, 61])
    n = int(g.v_id.max()) + 7
    return GraphArrays(np.concatenate([g.v_id, [n]]).astype(np.uint32), np.concatenate([g.v_type, [0]]).astype(np.uint32),
                       np.concatenate([g.v_pos, [[1.0, 2.0, 0.3]]]), g.e_type, g.e_ids, g.e_meas, g.e_inf, g.fixed)


# name: graph, environment (testing builds read it), HipOptimizer options, kernels an iteration must / must not launch, and whether the
# whole matrix of the operator is read (the two smallest)
CASES = {
    "level0_only": dict(graph=lambda: synth.make(40, 6, loop_closures=3, seed=1), env={}, kw={}, full=True,
                        must=["k_dense_apply", "k_restrict"], must_not=["k_bottom_apply", "k_coarse_tail", "k_tail_up", "k_bcsr_residual"]),
    "dense_bottom": dict(graph=lambda: synth.make(120, 6, loop_closures=4, seed=3), env={}, kw={}, full=True,
                         must=["k_bottom_apply"], must_not=["k_coarse_tail", "k_tail_up", "k_dense_apply", "k_bcsr_residual"]),
    "coarse_tail_nu2": dict(graph=lambda: synth.make(120, 6, loop_closures=4, seed=3), env={"TSGO_SWEEPS_LIST": "2"}, kw={}, full=False,
                            must=["k_coarse_tail", "pre-sweep L1", "post-sweep L1"], must_not=["k_bottom_apply", "k_tail_up", "k_dense_apply"]),
    "factored_tail": dict(graph=lambda: synth.make(500, 8, loop_closures=10, seed=2), env={}, kw={}, full=False,
                          must=["k_rowdot_wg", "k_tail_up"], must_not=["k_coarse_tail", "k_dense_apply", "k_bottom_apply"]),
    "launched_bottom": dict(graph=lambda: synth.make(1200, 6, loop_closures=20, seed=4), env={"TSGO_AGG_LIST": "4,64"}, kw={}, full=False,
                            must=["k_dense_apply", "k_prolong_add", "residual L1"], must_not=["k_coarse_tail", "k_bottom_apply", "k_tail_up"]),
    "explicit_level0": dict(graph=lambda: synth.make(120, 6, loop_closures=4, seed=3), env={}, kw=dict(cycle_level0="explicit"), full=False,
                            must=["k_bcsr_apply", "k_smooth0", "k_bottom_apply"], must_not=["k_schur_lm<double, 1, 0, 1>", "k_schur_lm<double, 2, 0, 1>", "k_schur_lm<double, 4, 0, 1>", "k_schur_lm<double, 8, 0, 1>"]),
    # edge types 0-4 (the priors restated in numpy for dense S, tests/priors.py; the twin linearises them itself), two lanes per pose
    "mixed_analytic": dict(graph=lambda: _mixed(True), env={}, kw=dict(odom_jacobian="analytic", lanes_per_pose=2), full=False,
                           must=["k_bottom_apply", ", 1, 1>", "k_schur_pose<double, 2,", "k_schur_lm<double"], must_not=["k_coarse_tail", "k_tail_up"]),
}
MIXED_FIXED_POSE, MIXED_DEAD_POSE = 61, 130      # mixed_analytic: the fixed pose inside an aggregate, the pose without edges (graph order)

# The ladder of the comparison with the twin: cycle vectors and cycle storage on an f64 handle — and the two rungs an f32 handle
# (Engine<float>: every plane, the diagonal inverses and the level-0 vectors in f32) can stand on.
RUNGS = {"vec64_f32": dict(vec64=True, storage=32, precision=64), "f32_f32": dict(vec64=False, storage=32, precision=64),
         "f32_half": dict(vec64=False, storage=16, precision=64),
         "p32_f32": dict(vec64=False, storage=32, precision=32), "p32_half": dict(vec64=False, storage=16, precision=32)}
P32_CASES = ("dense_bottom", "factored_tail")      # a one-level and a multi-level hierarchy
PAIRS = [(c, r) for c in CASES for r in RUNGS if RUNGS[r]["precision"] == 64 or c in P32_CASES]

# The largest distance to the twin over all cases and inputs per rung, measured on an MI355X; the device tests
# assert MARGIN x that: every rung is deterministic, the margin is for compilers and reduction orders.
LADDER = {"vec64_f32": 8.695e-05, "f32_f32": 8.704e-05, "f32_half": 8.844e-03, "p32_f32": 5.368e-05, "p32_half": 3.212e-03}
MARGIN = 4.0
# Product bound: C_PRODUCT * 3 deg_max * u * (mag |x|).  3 deg_max counts the terms of a row of the explicit matrix; the implicit product
# forms every term through the landmark: rotate into the pose frame (2 products + 1 sum per component), weight, the 2x2 inverse
# block (2 products + 1 sum), weight, rotate back (2 + 1) and the lever-arm row: 16 rounded operations in a chain per term.
# mag: the terms the product really sums, |Hpp| + |Hpl| |Hll^-1| |Hlp| (oracle.schur_dense), as the largest entry of each 3x3 block.
C_PRODUCT = 16.0


def limit(rung):
    return MARGIN * LADDER[rung]


def product_bound(mag, X, u, deg_max):
    return C_PRODUCT * 3 * deg_max * u * (mag @ np.abs(X))


def deg_max(S):
    P = S.shape[0] // 3
    nz = np.abs(S).reshape(P, 3, P, 3).sum(axis=(1, 3)) > 0
    return int(nz.sum(axis=1).max())


_REF = {}


def reference(case):
    """(S, block magnitudes, inputs R, the twin's M^-1 R, the twin's info) of a case, computed once."""
    if case not in _REF:
        g = CASES[case]["graph"]()
        S, mag = schur(case, with_magnitude=True)
        P = S.shape[0] // 3
        # block by block: every term passes through rotations between the world and the pose frame and through lever arms, which mix
        # the three components of a block (an isotropic weight makes c s (a0 - a1) vanish in H while both products were rounded)
        mag = np.repeat(np.repeat(mag.reshape(P, 3, P, 3).max(axis=(1, 3)), 3, 0), 3, 1)
        _, info = twin(case, np.zeros((3 * P, 1)))
        R = inputs(g, info, CASES[case]["full"])
        Z, info = twin(case, R)
        _REF[case] = (S, mag, R, Z, info)
    return _REF[case]


def transpose_pose(g):
    """The pose whose prolongator block the "transpose" defect hits: the middle one, which inputs() does not aim a unit vector at."""
    return n_poses(g) // 2


class Env:
    """The research variables of a case, set for the time a handle (or the twin) is built and used; every knob is removed first."""

    def __init__(self, env):
        self.env = dict(env)

    def __enter__(self):
        self.keep = {k: os.environ.get(k) for k in KNOBS}
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def n_poses(g):
    return int((g.v_type == 0).sum())


def inputs(g, info, full=False, seed=7):
    """Columns (3 P, n): every unit vector (full), or 32 seeded Gaussians, the per-pose rigid-motion modes (1,0,0), (0,1,0), (-y,x,1)
    and the unit vectors of the first pose, the last pose and one pose of a smallest and of a largest level-0 aggregate (info: what
    the twin reports)."""
    P = n_poses(g)
    if full:
        return np.eye(3 * P)
    xy = g.v_pos[g.v_type == 0][:, :2]
    cols = [np.random.default_rng(seed).normal(size=(3 * P, 32))]
    rig = np.zeros((3 * P, 3))
    rig[0::3, 0] = 1; rig[1::3, 1] = 1; rig[0::3, 2] = -xy[:, 1]; rig[1::3, 2] = xy[:, 0]; rig[2::3, 2] = 1
    cols.append(rig)
    poses = [0, P - 1] + list(info["agg_extremes"])
    assert transpose_pose(g) not in poses
    e = np.zeros((3 * P, 3 * len(poses)))
    for k, p in enumerate(poses):
        for c in range(3):
            e[3 * p + c, 3 * k + c] = 1
    cols.append(e)
    return np.concatenate(cols, axis=1)


def energy_distance(Z, Zref, S):
    """Per column: ||Z - Zref||_S / ||Zref||_S (0 where Zref vanishes in that norm and Z equals it)."""
    E = Z - Zref
    num = np.sqrt(np.maximum(np.einsum("ij,ij->j", E, S @ E), 0))
    den = np.sqrt(np.maximum(np.einsum("ij,ij->j", Zref, S @ Zref), 0))
    out = np.zeros_like(num)
    nz = den > 0
    out[nz] = num[nz] / den[nz]
    out[~nz & (num > 0)] = np.inf
    return out


def twin(case, R, level0="implicit", perturb=None):
    """The twin's preconditioner of the case on the columns of R, under the case's environment and options; (Z, info)."""
    c = CASES[case]
    g = c["graph"]()
    oracle.set_odom_jacobian(c["kw"].get("odom_jacobian", "constant"))
    oracle.set_cycle_level0(c["kw"].get("cycle_level0", level0))
    try:
        with Env({k: v for k, v in c["env"].items()}):
            return oracle.twin_precond(util.to_oracle(g), R, lanes_per_pose=c["kw"].get("lanes_per_pose", 0), lanes_per_lm=c["kw"].get("lanes_per_lm", 0),
                                       perturb=perturb, transpose_pose=transpose_pose(g))
    finally:
        oracle.set_odom_jacobian("constant"); oracle.set_cycle_level0("implicit")


def schur(case, with_magnitude=False):
    """Dense S of the case (and, asked for, the magnitude matrix of oracle.schur_dense)."""
    c = CASES[case]
    oracle.set_odom_jacobian(c["kw"].get("odom_jacobian", "constant"))
    try:
        g = c["graph"]()
        if (g.e_type >= 3).any():      # priors: restated in numpy (tests/priors.py), on top of the dense restatement of edge types 0-2
            return oracle.schur_dense(util.to_oracle(priors.without_priors(g)), diag_add=priors.prior_terms(g)[0], with_magnitude=with_magnitude)
        return oracle.schur_dense(util.to_oracle(g), with_magnitude=with_magnitude)
    finally:
        oracle.set_odom_jacobian("constant")
