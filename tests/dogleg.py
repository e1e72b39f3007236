"""A dense restatement of Powell's dogleg trust-region loop of tsgo_config.rules = 3 (include/tsgo.h: tsgo_set_dogleg), numpy only.

One solve: H, b, chi^2 of lm_rules._system (the dense system of the Levenberg-Marquardt restatement: b zeroed at fixed vertices, the gauge
term inside H), H d_gn = b by LAPACK, and the four scalars as plain dot products with the dense H.  One trial: the step d formed AS A VECTOR
from the header's case table, pred = 2 b'd - d'Hd from the dense H (never the header's closed form, which assumes H d_gn = b),
step_norm = |d|, the step by independent.apply_update(step=1), chi^2 at the trial point by lm_rules.chi2_at, the gain ratio, accept / reject,
the radius rule and the stops as the header states them.  A rejected trial reuses the solve.  It shares nothing with the product but the
text of that comment."""
import numpy as np

from tests import independent, lm_rules, priors

DEFAULTS = dict(radius0=1e4, radius_min=1e-9, radius_max=1e9, chi2_rel_tol=1e-6)
DELTA_TOL = 1e-3


def next_radius(radius, gain, kind, step_norm, radius_max=DEFAULTS["radius_max"]):
    """The radius after a trial."""
    if not gain >= 0.25:
        return 0.25 * step_norm
    if gain > 0.75 and kind != 0:
        return min(2.0 * radius, radius_max)
    return radius


def radius_trace(radius0, gain, pred, kind, step_norm, radius_max=DEFAULTS["radius_max"]):
    """The radius of every trial, and the one the next trial would have used, from a run's own gain / kind / step_norm traces: the update
    rule applied to the run's own decisions (pred is taken for symmetry with lm_rules.lambda_trace: the radius rule reads the gain alone)."""
    r, out = float(radius0), []
    for g, _p, k, s in zip(gain, pred, kind, step_norm):
        out.append(r)
        r = next_radius(r, g, k, s, radius_max)
    return np.array(out), r


def step_of(b, d_gn, H, radius):
    """(kind, d) of one trial."""
    gg, dd, gHg = float(b @ b), float(d_gn @ d_gn), float(b @ (H @ b))
    alpha, n = gg / gHg, np.sqrt(gg)
    if np.sqrt(dd) <= radius:
        return 0, d_gn.copy()
    if alpha * n >= radius:
        return 2, (radius / n) * b
    pc = alpha * b                                   # the Cauchy point, inside the region; d_gn outside: one crossing in between
    u = d_gn - pc
    qa, qh, qc = float(u @ u), float(pc @ u), float(pc @ pc) - radius * radius
    beta = (-qh + np.sqrt(qh * qh - qa * qc)) / qa
    return 1, pc + beta * u


def dense_dogleg(g, trials, radius0=DEFAULTS["radius0"], radius_min=DEFAULTS["radius_min"], radius_max=DEFAULTS["radius_max"],
                 chi2_rel_tol=DEFAULTS["chi2_rel_tol"], jacobian="analytic"):
    """The loop on a copy of g.  Returns per-trial arrays chi2, kind, solved, radius, step_norm, gg, gHg, gd, dd, pred, chi2_trial, rho,
    accepted, and stop, v_pos, rejected, iters, solves, radius_last."""
    cur = g.copy()
    radius = float(radius0)
    keys = ("chi2", "kind", "solved", "radius", "step_norm", "gg", "gHg", "gd", "dd", "pred", "chi2_trial", "rho", "accepted")
    tr = {k: [] for k in keys}
    stop, solves, rejected, need_solve = "cap", 0, 0, True
    H = b = d_gn = None
    chi = 0.0
    with lm_rules._Jacobians(jacobian):
        for _ in range(trials):
            solved = need_solve
            if solved:
                H, b, chi = lm_rules._system(cur)
                d_gn = np.linalg.solve(H, b)
                solves += 1; need_solve = False
            gg = float(b @ b)
            rec = dict(chi2=chi, solved=int(solved), radius=radius, gg=gg, gHg=float(b @ (H @ b)), gd=float(b @ d_gn), dd=float(d_gn @ d_gn))
            if gg == 0:
                rec.update(kind=0, step_norm=0.0, pred=0.0, chi2_trial=chi, rho=0.0, accepted=False)
                for k in keys:
                    tr[k].append(rec[k])
                stop = "converged"; break
            kind, d = step_of(b, d_gn, H, radius)
            pred = float(2 * (b @ d) - d @ (H @ d))
            step_norm = float(np.linalg.norm(d))
            trial = cur.copy()
            trial.v_pos[:] = independent.apply_update(cur.v_pos, g.v_type, priors.unpack(d, g), step=1.0)
            chi_t = lm_rules.chi2_at(trial)
            rho = (chi - chi_t) / pred if pred != 0 else 0.0
            ok = bool(rho > 0 and pred > 0)
            rec.update(kind=kind, step_norm=step_norm, pred=pred, chi2_trial=chi_t, rho=rho, accepted=ok)
            for k in keys:
                tr[k].append(rec[k])
            radius = next_radius(radius, rho, kind, step_norm, radius_max)
            if ok:
                cur = trial
                if step_norm < DELTA_TOL or chi - chi_t <= chi2_rel_tol * chi:
                    stop = "converged"; break
                need_solve = True
            else:
                rejected += 1
                if radius < radius_min:
                    stop = "radius"; break
    out = {k: np.array(v) for k, v in tr.items()}
    out["accepted"] = out["accepted"].astype(bool)
    out.update(stop=stop, v_pos=cur.v_pos, rejected=rejected,
               iters=len(out["chi2"]), solves=solves, radius_last=radius)
    return out


# ---- the cases tests/test_dogleg_cpu.py qualifies and tests/test_gpu_dogleg.py runs ----------------------------------------------------
def _synth_d(variant):
    return lm_rules.perturbed(lm_rules.synth_600(variant), seed=4, sigma_xy=0.5, sigma_th=0.2)


CASES = {
    # name: (graph factory, keyword arguments of dense_dogleg / HipOptimizer(dl_*), trial cap, Jacobians)
    "A": (lm_rules.c1_perturbed, dict(radius0=1e4), 10, "analytic"),
    "B": (lm_rules.c1_perturbed, dict(radius0=1.0), 5, "analytic"),
    "C": (lm_rules.loop_closure_pose_graph, dict(), 3, "constant"),
    "D_plain": (lambda: _synth_d("plain"), dict(radius0=2.0), 5, "analytic"),
    "D_vlm": (lambda: _synth_d("vlm"), dict(radius0=2.0), 5, "analytic"),
    "D_priors": (lambda: _synth_d("priors"), dict(radius0=2.0), 5, "analytic"),
    "c1_plain": (lm_rules.c1_plain, dict(), 30, "analytic"),
}


def reference(case):
    """(graph, dense loop, keyword arguments, trial cap, Jacobians) of a case."""
    make, kw, n, jac = CASES[case]
    g = make()
    return g, dense_dogleg(g, n, jacobian=jac, **kw), kw, n, jac
