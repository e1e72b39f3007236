"""Twin-side checks of the preconditioner-operator tests (no GPU): the reference the device is compared with is itself a symmetric
positive definite preconditioner of dense S, and the limits asserted on the device (tests/test_gpu_precond_operator.py: 4 x the measured
ladder) are small against what a subtly wrong cycle does to the operator — a smoother damping 5 % off, one sweep too many, one
prolongator block transposed (oracle.twin_precond's deliberate defects)."""
import numpy as np
import pytest

from oracle import oracle
from tests import precond_cases as pc


@pytest.mark.parametrize("case", list(pc.CASES))
def test_the_twin_is_an_spd_preconditioner_of_dense_S(case):
    S, _mag, R, Z, info = pc.reference(case)
    if pc.CASES[case]["full"]:
        M = Z
        assert np.linalg.norm(M - M.T) <= 1e-12 * np.linalg.norm(M)
        w = np.linalg.eigvals(M @ S)
        assert np.abs(w.imag).max() <= 1e-10 * np.abs(w).max() and w.real.min() > 0
        assert w.real.max() / w.real.min() < 20
    # (r, M r) > 0 and a symmetric form on the inputs everywhere
    G = R.T @ Z
    assert np.abs(G - G.T).max() <= 1e-10 * np.abs(G).max()
    assert (np.diag(G) >= 0).all() and (np.diag(G) == 0).sum() <= 6      # (the unit vectors of a pose without edges, listed as last pose and as smallest aggregate: M r = 0 there)


@pytest.mark.parametrize("case", list(pc.CASES))
def test_the_device_limits_are_small_against_a_subtly_wrong_cycle(case):
    """Condition: the limits of the two tight rungs at most 1/10, the packed-half limit at most 1/3, of the smallest distance a defect
    causes in this case.  A defect that cannot act on a case (one more coarse sweep where no coarse level sweeps) is left out, by name."""
    S, _mag, R, Z, info = pc.reference(case)
    dist = {}
    for p in oracle.PERTURBATIONS:
        if p == "nu" and info["sweeping_levels"] == 0:
            print("case %s: no coarse level runs sweeps, the nu defect does not apply" % case)
            continue
        Zp, _ = pc.twin(case, R, perturb=p)
        d = pc.energy_distance(Zp, Z, S)
        if p == "transpose" and pc.CASES[case]["full"]:      # every unit vector is an input there: leave out the three aimed at the defect's pose
            k = 3 * pc.transpose_pose(pc.CASES[case]["graph"]())
            d = np.delete(d, [k, k + 1, k + 2])
        dist[p] = float(d.max())
        assert dist[p] > 0
    smallest = min(dist.values())
    for rung, share in (("vec64_f32", 10.0), ("f32_f32", 10.0), ("f32_half", 3.0)) + ((("p32_f32", 10.0), ("p32_half", 3.0)) if case in pc.P32_CASES else ()):
        ratio = smallest / pc.limit(rung)
        print("case %s rung %s: defects %s; smallest / limit = %.1f (needs >= %.0f)" % (case, rung, {k: "%.3e" % v for k, v in dist.items()}, ratio, share))
        if rung.endswith("_half") and ratio < share:
            which = min(dist, key=dist.get)
            print("case %s: packed halves cannot discriminate the %s defect (distance %.3e, limit %.3e%s)" % (case, which, dist[which], pc.limit(rung), ": the limit exceeds the defect" if ratio < 1 else ""))
            continue
        assert ratio >= share, (case, rung, dist, pc.limit(rung))
