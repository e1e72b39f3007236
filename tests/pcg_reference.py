"""A plain restatement of the PCG loop around the operators (numpy, no GPU), for tests/test_pcg_reference_cpu.py (the conditions under
which a comparison with the device means something) and tests/test_gpu_pcg_trajectory.py (the comparison).

The kernels (k_cg_update, k_cg_step + iter_gate_body, k_mb_alpha / k_mb_beta) run the Chronopoulos-Gear form: one reduction point per
iteration, alpha = gamma / (delta - beta gamma / alpha_old).  pcg() here is the textbook form with two reductions, p^T S p formed from
p itself, so that the two share nothing but the mathematics.  Everything is dense: S from oracle.schur_dense, the reduced right-hand
side from the same dense linearisation, the multigrid operator as the matrix of the f64 twin (precond_cases.twin on the identity).

The stop rules, restated from the code:
  block-Jacobi (k_cg_update): done at the first k with r_k^T M r_k <= tol^2 r_0^T M r_0 (M = D^-1, x_0 = 0);
  multigrid (iter_gate_body): done at the first k >= 1 with r_k^T D^-1 r_k <= tol^2 b^T D^-1 b;
the count reported is the number of vector updates, k.  With x_0 = 0 and M = D^-1 the two ratios are the same numbers: the "other
norm" of the block-Jacobi rule is therefore taken as the Euclidean one, ||r_k|| / ||b||.

DEFECTS (in the manner of oracle.PERTURBATIONS): "beta_stale" (beta from the gamma two steps back), "alpha_plain" (alpha = gamma /
delta, delta = z^T S z, without the correction term: the loop is then written in the Chronopoulos-Gear form, where that omission
means something), "other_norm" (the stop rule tested in the other preconditioner's norm), "extra_update" (one update too many after
the rule is met).  The first two change the iterates, the last two only where the loop stops."""
import functools

import numpy as np

from oracle import oracle
from tests import precond_cases as pc
from tests import priors, util

DEFECTS = ("beta_stale", "alpha_plain", "other_norm", "extra_update")
DTYPES = {"float32": np.float32, "float64": np.float64, "longdouble": np.longdouble}


def reduced_system(g, odom_jacobian="constant"):
    """(S, b~, Dinv) of the graph at its estimates, rows in graph pose order: S from oracle.schur_dense (priors restated in numpy and
    added to the diagonal blocks, as precond_cases.schur does), b~ = b_p - H_pl H_ll^-1 b_l from the same dense linearisation, Dinv
    (3 P, 3 P) block diagonal: the inverses of the 3x3 diagonal blocks of S (zero for a pose without edges, whose block is zero)."""
    s = _system(g, odom_jacobian)
    return s["S"], s["bt"], s["Dinv"]


def _system(g, odom_jacobian="constant"):
    oracle.set_odom_jacobian(odom_jacobian)
    try:
        has_priors = bool((g.e_type >= 3).any())
        og = util.to_oracle(priors.without_priors(g) if has_priors else g)
        H, b, chi2, idx = oracle.linearize(og)
        Hp = bp = None
        if has_priors:
            Hp, bp, chip = priors.prior_terms(g)
            chi2 += chip
            for v in range(len(g.v_id)):
                m = 3 if g.v_type[v] == 0 else 2
                H[idx[v]:idx[v] + m, idx[v]:idx[v] + m] += Hp[v][:m, :m]
                b[idx[v]:idx[v] + m] += bp[v][:m]
        S = oracle.schur_dense(og, diag_add=Hp)
    finally:
        oracle.set_odom_jacobian("constant")
    pose = np.where(g.v_type == 0)[0]; lm = np.where(g.v_type == 1)[0]
    ip = (idx[pose][:, None] + np.arange(3)[None, :]).reshape(-1)
    il = (idx[lm][:, None] + np.arange(2)[None, :]).reshape(-1)
    P, L = len(pose), len(lm)
    bt = b[ip].copy()
    Hlp = np.zeros((2 * L, 3 * P)); inv = np.zeros((L, 2, 2)); bl = np.zeros(2 * L)
    if L:
        Hlp = H[np.ix_(il, ip)]
        k = np.arange(L)
        inv = np.linalg.pinv(H[np.ix_(il, il)].reshape(L, 2, L, 2)[k, :, k, :], hermitian=True)
        bl = b[il]
        bt -= Hlp.T @ np.einsum("lxy,ly->lx", inv, bl.reshape(L, 2)).reshape(-1)
    Dinv = np.zeros_like(S)
    for i in range(P):
        Dinv[3 * i:3 * i + 3, 3 * i:3 * i + 3] = np.linalg.pinv(S[3 * i:3 * i + 3, 3 * i:3 * i + 3], hermitian=True)
    return dict(S=S, bt=bt, Dinv=Dinv, Hlp=Hlp, Hll_inv=inv, bl=bl, pose=pose, lm=lm, chi2=chi2)


def landmark_backsub(sys_, x):
    """dl = H_ll^-1 (b_l - H_lp x) = u - D_l^-1 W^T x, (L, 2) in the graph's landmark order: the back-substitution of ANY pose vector."""
    L = len(sys_["lm"])
    return np.einsum("lxy,ly->lx", sys_["Hll_inv"], (sys_["bl"] - sys_["Hlp"] @ x).reshape(L, 2))


class Trajectory:
    """What pcg() returns: x[k - 1] = x_k and the residual ratios of r_k for k = 1..n (index 0 of the ratio arrays is k = 0, where
    ratio_M = ratio_D = ratio_2 = 1): ratio_M = sqrt(r^T M r / r_0^T M r_0), ratio_D = sqrt(r^T D^-1 r / b^T D^-1 b), ratio_2 = ||r|| / ||b||."""

    def __init__(self, x, ratio_M, ratio_D, ratio_2, defect):
        self.x, self.ratio_M, self.ratio_D, self.ratio_2, self.defect = x, ratio_M, ratio_D, ratio_2, defect

    def deciding(self, precond):
        """The ratios the stop rule of `precond` ("jacobi" / "amg") looks at, k = 0..n."""
        if self.defect == "other_norm":
            return self.ratio_2 if precond == "jacobi" else self.ratio_M
        return self.ratio_M if precond == "jacobi" else self.ratio_D

    def stop(self, precond, tol):
        """The count the loop reports at `tol`: the first k >= 1 whose deciding ratio is <= tol (None: not within the n steps run)."""
        hit = np.where(self.deciding(precond)[1:] <= tol)[0]
        if not len(hit):
            return None
        return int(hit[0]) + 1 + (1 if self.defect == "extra_update" else 0)


def pcg(S, b, M, Dinv, n, dtype="float64", defect=None):
    """Textbook two-reduction PCG from x_0 = 0 on S x = b with the preconditioner matrix M, n steps in `dtype` ("float32", "float64",
    "longdouble"; every operand is rounded to it first).  Returns a Trajectory: x_k and the residual ratios for k = 1..n.  defect: None
    or one of DEFECTS."""
    with np.errstate(all="ignore"):      # (a deliberate defect may diverge)
        return _pcg(S, b, M, Dinv, n, dtype, defect)


def _pcg(S, b, M, Dinv, n, dtype, defect):
    assert defect is None or defect in DEFECTS
    dt = DTYPES[dtype] if isinstance(dtype, str) else dtype
    S, b, M, Dinv = (np.asarray(a).astype(dt) for a in (S, b, M, Dinv))
    x = np.zeros_like(b); r = b.copy()
    z = M @ r
    p = z.copy()
    gamma = r @ z
    g0, d0, n0 = gamma, r @ (Dinv @ r), r @ r
    gammas = [gamma]
    xs, rM, rD, r2 = [], [1.0], [1.0], [1.0]
    q = None
    for k in range(n):
        if gamma == 0:      # nothing left to correct: the iterate stays
            xs.append(x.copy()); rM.append(0.0); rD.append(float(np.sqrt(max(r @ (Dinv @ r), 0) / d0)) if d0 > 0 else 0.0); r2.append(float(np.sqrt(r @ r / n0)) if n0 > 0 else 0.0)
            continue
        if defect == "alpha_plain":      # Chronopoulos-Gear: p = z + beta p, q = S z + beta q, alpha from delta = z^T S z alone
            sz = S @ z
            beta = 0 if k == 0 else gamma / gammas[-2]
            p = z + beta * p if k else z.copy()
            q = sz + beta * q if k else sz
            alpha = gamma / (z @ sz)
        else:
            q = S @ p
            alpha = gamma / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        z = M @ r
        g_new = r @ z
        gammas.append(g_new)
        if defect != "alpha_plain":
            den = gammas[-3] if (defect == "beta_stale" and len(gammas) >= 3) else gamma
            p = z + (g_new / den) * p
        gamma = g_new
        xs.append(x.copy())
        rM.append(float(np.sqrt(max(g_new, 0) / g0))); rD.append(float(np.sqrt(max(r @ (Dinv @ r), 0) / d0))); r2.append(float(np.sqrt(r @ r / n0)))
    return Trajectory(np.array(xs), np.array(rM), np.array(rD), np.array(r2), defect)


def tolerances(ratios, gap=1.3):
    """ratios: k = 0..n (ratios[0] = 1).  For every k >= 1 whose ratio lies a factor >= gap below the running minimum of all earlier
    ones: (k, tol_k = sqrt(ratio_k * running-min_{k-1})).  At tol_k the loop stops at exactly k — the first crossing: the ratios are not
    monotone — and tol_k is a factor >= sqrt(gap) from the ratio on either side."""
    out = []
    run = float(ratios[0])
    for k in range(1, len(ratios)):
        if ratios[k] > 0 and ratios[k] * gap <= run:
            out.append((k, float(np.sqrt(ratios[k] * run))))
        run = min(run, float(ratios[k]))
    return out


def s_norm(S, v):
    with np.errstate(all="ignore"):      # (a diverged defect run: infinitely far)
        e = float(v @ (S @ v))
    return float(np.sqrt(max(e, 0.0))) if np.isfinite(e) else np.inf


# ---- the cases of the device tests, and everything about them that is computed from the reference alone (once per process) ----
CASES = ("level0_only", "dense_bottom", "factored_tail", "mixed_analytic")
PRECONDS = ("jacobi", "amg")
CAP_KS = {"jacobi": (1, 2, 3, 5, 8, 13, 21), "amg": (1, 2, 3, 5, 8, 13)}
N_STEPS = {"jacobi": 240, "amg": 24}      # how far the reference runs: the tolerance ladders come out of these steps
LADDER_RUNGS = ("f32_f32", "f32_half")    # multigrid, tolerance ladder: cycle storage f32 / packed halves on an f64 handle
ROUNDING_FACTOR = 100.0                   # device limit = this x the running maximum of the f64-to-longdouble drift
U64 = 2.0 ** -53                          # ... and of one rounding of the result to f64: where both runs happen to round alike (the unit column
                                          # of a fixed pose after one step) the drift reads 0, and no f64 result is better than u
DEFECT_SHARE = 10.0                       # a defect must lie this many limits from the clean reference, or change the count
N_SEEDS = 8
MU_F64 = 1e-6                             # block-Jacobi in f64: the margin of the deciding ratio (rounding moves it by ~1e-13)


def graph(case):
    return pc.CASES[case]["graph"]()


@functools.lru_cache(maxsize=None)
def system(case):
    return _system(graph(case), pc.CASES[case]["kw"].get("odom_jacobian", "constant"))


@functools.lru_cache(maxsize=None)
def operator(case, precond):
    """The preconditioner as a dense matrix: D^-1, or the twin's cycle on the identity, symmetrised."""
    s = system(case)
    if precond == "jacobi":
        return s["Dinv"]
    Z, _info = pc.twin(case, np.eye(s["S"].shape[0]))
    return 0.5 * (Z + Z.T)


@functools.lru_cache(maxsize=None)
def run(case, precond, dtype="float64", defect=None):
    s = system(case)
    return pcg(s["S"], s["bt"], operator(case, precond), s["Dinv"], N_STEPS[precond], dtype, defect)


@functools.lru_cache(maxsize=None)
def x_star(case):
    s = system(case)
    return np.linalg.lstsq(s["S"], s["bt"], rcond=None)[0]


def distances(case, X, Xref):
    """||X_k - Xref_k||_S / ||x*||_S for the rows k the two have in common."""
    s = system(case)
    n = min(len(X), len(Xref))
    den = s_norm(s["S"], x_star(case))
    return np.array([s_norm(s["S"], np.asarray(X[k], np.float64) - np.asarray(Xref[k], np.float64)) for k in range(n)]) / den


@functools.lru_cache(maxsize=None)
def rounding_limit(case, precond):
    """limit[k - 1] for the iterate x_k of an f64 device run: ROUNDING_FACTOR x the running maximum of drift(1..k), drift = the S-norm
    distance between the float64 and the longdouble run relative to ||x*||_S.  Another summation order is another realisation of the
    same rounding walk; the factor covers that.  The drift is taken as at least u = 2^-53 (U64)."""
    d = distances(case, run(case, precond, "float64").x, run(case, precond, "longdouble").x)
    return ROUNDING_FACTOR * np.maximum(U64, np.maximum.accumulate(d)), d


def _sym_root(M):
    w, V = np.linalg.eigh(M)
    return V * np.sqrt(np.maximum(w, 0.0))[None, :]


@functools.lru_cache(maxsize=None)
def operator_limit(case, rung):
    """Multigrid on cycle storage f32 / packed halves: the device's M is within eps = pc.limit(rung) of the twin's in the energy norm.
    The reference is run with M + eps L E L^T (M = L L^T, E random symmetric with ||E||_2 = 1) for N_SEEDS seeds; returns (iterate limit
    per k = 2 x the largest S-norm distance seen, index k - 1; mu per k = 2 x the largest relative change of the deciding ratio at any
    step up to k, index k: the rule at k looks at the ratio of k and at the running minimum before it; the two raw)."""
    s = system(case)
    M = operator(case, "amg")
    Lr = _sym_root(M)
    eps = pc.limit(rung)
    clean = run(case, "amg")
    dist = np.zeros(N_STEPS["amg"]); rel = np.zeros(N_STEPS["amg"] + 1)
    for seed in range(N_SEEDS):
        E = np.random.default_rng(100 + seed).normal(size=M.shape)
        E = 0.5 * (E + E.T)
        E /= np.abs(np.linalg.eigvalsh(E)).max()
        t = pcg(s["S"], s["bt"], M + eps * (Lr @ E @ Lr.T), s["Dinv"], N_STEPS["amg"])
        dist = np.maximum(dist, distances(case, t.x, clean.x))
        a, b = t.ratio_D, clean.ratio_D
        rel = np.maximum(rel, np.where(b > 0, np.abs(a / np.where(b > 0, b, 1.0) - 1), np.inf))
    return 2 * dist, 2 * np.maximum.accumulate(rel), dist, rel


def iterate_limit(case, precond, rung=None):
    """The limit of ||x_k(device) - x_k(reference)||_S / ||x*||_S per k (index k - 1): rounding, plus — multigrid — the operator's."""
    lim = rounding_limit(case, precond)[0].copy()
    if precond == "amg":
        lim[:N_STEPS["amg"]] += operator_limit(case, rung or "f32_f32")[0]
    return lim


def count_margin(case, precond, rung=None):
    """mu[k], k = 0..N_STEPS: the relative margin of the deciding ratio at step k (and of the running minimum before it): MU_F64, or —
    once rounding has grown past it — ROUNDING_FACTOR x the largest relative change of the ratio between the float64 and the longdouble
    run up to k; multigrid: plus the operator's."""
    a, b = run(case, precond, "float64").deciding(precond), run(case, precond, "longdouble").deciding(precond)
    rel = np.where(b > 0, np.abs(a / np.where(b > 0, b, 1.0) - 1), np.inf)
    mu = np.maximum(MU_F64, ROUNDING_FACTOR * np.maximum.accumulate(rel))
    if precond == "amg":
        mu = mu + operator_limit(case, rung or "f32_f32")[1]
    return mu


GAPS = (1.3, 1.1, 1.03, 1.01)      # every one far above 1 + 2 MU_F64


def decades(tols):
    return float(np.log10(max(tols) / min(tols))) if len(tols) else 0.0


@functools.lru_cache(maxsize=None)
def gap_for(case, precond):
    """The largest gap of GAPS at which tolerances() on the reference's deciding ratios returns >= 4 tolerances over >= 3 decades (the
    block-Jacobi ratios of the larger graphs fall by a per cent or two per step: no step lies 1.3 below everything before it)."""
    r = run(case, precond).deciding(precond)
    for gap in GAPS:
        t = [tol for _k, tol in tolerances(r, gap)]
        if len(t) >= 4 and decades(t) >= 3:
            return gap, len(t), decades(t)
    return GAPS[-1], len(t), decades(t)


def candidates(ratios, other, mu, gap=1.3):
    """Tolerances at which the loop stops at exactly k with the margin mu[k] on either side, [(k, tol, kind)]:
    "gap": what tolerances() returns, kept where sqrt(running-min_{k-1} / ratio_k) >= 1 + 2 mu[k];
    "norms": tol = sqrt(ratio_k * other_k) where the rule's own ratio has its first crossing at k and the OTHER norm's ratio of the same
    residual lies a factor >= (1 + 2 mu[k])^2 above it (and below the running minimum): the rule tested in the other norm runs on."""
    out = []
    for k, tol in tolerances(ratios, gap):
        if tol >= ratios[k] * (1 + 2 * mu[k]):
            out.append((k, tol, "gap"))
    run_ = float(ratios[0])
    for k in range(1, len(ratios)):
        if 0 < ratios[k] < run_ and other[k] < run_ and other[k] >= ratios[k] * (1 + 2 * mu[k]) ** 2:
            out.append((k, float(np.sqrt(ratios[k] * other[k])), "norms"))
        # ... and the mirror image: the other norm's ratio of the PREVIOUS residual lies that factor BELOW the rule's own, which is the
        # running minimum: between the two the rule goes on to k, and the rule tested in the other norm has already stopped
        if k >= 2 and ratios[k - 1] == run_ and 0 < other[k - 1] and other[k - 1] * (1 + 2 * mu[k]) ** 2 <= run_:
            tol = float(np.sqrt(other[k - 1] * run_))
            if ratios[k] * (1 + 2 * mu[k]) <= tol:
                out.append((k, tol, "norms"))
        run_ = min(run_, float(ratios[k]))
    return sorted(out, key=lambda e: -e[1])


def _caught(case, precond, k, tol, lim):
    """{defect: (count under the defect, distance of its stopping iterate from the clean x_k in limits)} and the verdict: every defect
    changes the count or lies DEFECT_SHARE limits away."""
    clean = run(case, precond)
    S = system(case)["S"]; den = s_norm(S, x_star(case))
    rep = {}
    for d in DEFECTS:
        t = run(case, precond, "float64", d)
        kd = t.stop(precond, tol)
        far = np.inf if kd is None or kd > len(t.x) else s_norm(S, t.x[kd - 1] - clean.x[k - 1]) / den / lim[k - 1]
        rep[d] = (kd, float(far))
    return rep, all(kd != k or far >= DEFECT_SHARE for kd, far in rep.values())


TOL_FLOOR = 1e-7      # the ladders stay above it: three decades and more lie above, and the f32 cycle's margins grow without bound below
MAX_LADDER = 6


@functools.lru_cache(maxsize=None)
def ladder(case, precond, rung=None):
    """The tolerances of the stop-rule tests on the device: the candidates() >= TOL_FLOOR at which every defect is caught, thinned to
    MAX_LADDER spread over the decades.  Returns (used [(k, tol, kind)], dropped [(k, tol, kind, report)])."""
    tr = run(case, precond)
    other = tr.ratio_2 if precond == "jacobi" else tr.ratio_M
    lim = iterate_limit(case, precond, rung)
    used, dropped = [], []
    for k, tol, kind in candidates(tr.deciding(precond), other, count_margin(case, precond, rung), gap_for(case, precond)[0]):
        if tol < TOL_FLOOR:
            continue
        rep, ok = _caught(case, precond, k, tol, lim)
        (used if ok else dropped).append((k, tol, kind) if ok else (k, tol, kind, rep))
    if len(used) > MAX_LADDER:
        pick = sorted(set(int(round(v)) for v in np.linspace(0, len(used) - 1, MAX_LADDER)))
        used = [used[j] for j in pick]
    return used, dropped


@functools.lru_cache(maxsize=None)
def cap_values(case, precond, rung=None):
    """The caps k of the iterate tests at which both iterate defects lie DEFECT_SHARE limits from the clean x_k (beta_stale cannot act
    before x_3, alpha_plain not before x_2: the first steps are kept, they check the start of the recurrences).  (used, dropped {k: report})."""
    clean = run(case, precond)
    lim = iterate_limit(case, precond, rung)
    used, dropped = [], {}
    for k in CAP_KS[precond]:
        rep = {d: float(distances(case, run(case, precond, "float64", d).x, clean.x)[k - 1] / lim[k - 1]) for d in ("beta_stale", "alpha_plain")}
        need = [d for d in rep if not (d == "beta_stale" and k < 3) and not (d == "alpha_plain" and k < 2)]
        if all(rep[d] >= DEFECT_SHARE for d in need):
            used.append(k)
        else:
            dropped[k] = rep
    return used, dropped


# ---- f32 handles (Engine<float>): dense_bottom, tolerances >= 1e-4 ----
F32_CASE, F32_FACTOR, F32_TOL_MIN = "dense_bottom", 8.0, 1e-4


@functools.lru_cache(maxsize=None)
def f32_limits(precond):
    """(iterate limit per k, index k - 1; mu per k, index k) of an f32 handle: F32_FACTOR x the distance (the relative change of the
    deciding ratio, running maximum) between the float64 reference and a float32 reference on S, b~ rounded to f32 — plus, multigrid,
    the operator's share on the p32_f32 rung."""
    a, b = run(F32_CASE, precond, "float64"), run(F32_CASE, precond, "float32")
    d = distances(F32_CASE, b.x, a.x)
    ra, rb = a.deciding(precond), b.deciding(precond)
    rel = np.maximum.accumulate(np.abs(rb / ra - 1))
    lim, mu = F32_FACTOR * np.maximum.accumulate(d), F32_FACTOR * rel
    if precond == "amg":
        ol = operator_limit(F32_CASE, "p32_f32")
        lim = lim + ol[0]; mu = mu + ol[1]
    return lim, mu


@functools.lru_cache(maxsize=None)
def f32_ladder(precond):
    tr = run(F32_CASE, precond)
    other = tr.ratio_2 if precond == "jacobi" else tr.ratio_M
    lim, mu = f32_limits(precond)
    used, dropped = [], []
    for k, tol, kind in candidates(tr.deciding(precond), other, mu, gap_for(F32_CASE, precond)[0]):
        if tol < F32_TOL_MIN:
            continue
        rep, ok = _caught(F32_CASE, precond, k, tol, lim)
        (used if ok else dropped).append((k, tol, kind) if ok else (k, tol, kind, rep))
    if len(used) > 4:
        pick = sorted(set(int(round(v)) for v in np.linspace(0, len(used) - 1, 4)))
        used = [used[j] for j in pick]
    return used, dropped


def residual_ratio(case, precond, x):
    """The deciding ratio of the stop rule for ANY pose vector x, from the true residual b~ - S x in f64."""
    s = system(case)
    r = s["bt"] - s["S"] @ x
    return float(np.sqrt(max(r @ (s["Dinv"] @ r), 0.0) / (s["bt"] @ (s["Dinv"] @ s["bt"]))))


# ---- the batched PCG of tsgo_marginals / tsgo_joint_marginals (k_mb_alpha / k_mb_beta): unit right-hand sides, column by column ----
# Its rule is the same under both preconditioners: a column is done at the first k >= 1 with r^T D^-1 r <= tol^2 b^T D^-1 b, and then frozen.
BATCH_CASE = "level0_only"
BATCH_TOLS = (1e-2, 1e-3, 1e-5)
BATCH_STEPS = {"jacobi": 120, "amg": 24}
UNDECIDED_SHARE = 0.25


@functools.lru_cache(maxsize=None)
def batched(precond):
    """Per unit column j of the pose block: the trajectory, the iterate limit per k (index k - 1, relative to ||S^-1 e_j||_S: rounding as
    in rounding_limit, plus the operator's share on the batched cycle's rung, vec64_f32) and the margin mu per k (index k)."""
    s = system(BATCH_CASE)
    S, Dinv = s["S"], s["Dinv"]
    M = operator(BATCH_CASE, precond)
    n = BATCH_STEPS[precond]
    Sinv = np.linalg.inv(S)
    Lr = _sym_root(M) if precond == "amg" else None
    eps = pc.limit("vec64_f32")
    Es = []
    for seed in range(N_SEEDS if precond == "amg" else 0):
        E = np.random.default_rng(300 + seed).normal(size=M.shape); E = 0.5 * (E + E.T)
        Es.append(M + eps * (Lr @ (E / np.abs(np.linalg.eigvalsh(E)).max()) @ Lr.T))
    cols = []
    for j in range(S.shape[0]):
        b = np.zeros(S.shape[0]); b[j] = 1.0
        t = pcg(S, b, M, Dinv, n)
        tl = pcg(S, b, M, Dinv, n, "longdouble")
        den = np.sqrt(Sinv[j, j])
        dist = lambda X, Y: np.array([s_norm(S, np.asarray(X[k], np.float64) - np.asarray(Y[k], np.float64)) for k in range(n)]) / den      # noqa: E731
        relc = lambda a, c: np.where(c > 0, np.abs(a / np.where(c > 0, c, 1.0) - 1), np.inf)      # noqa: E731
        lim = ROUNDING_FACTOR * np.maximum(U64, np.maximum.accumulate(dist(t.x, tl.x)))
        mu = np.maximum(MU_F64, ROUNDING_FACTOR * np.maximum.accumulate(relc(t.ratio_D, tl.ratio_D)))
        d = np.zeros(n); rel = np.zeros(n + 1)
        for Mp in Es:
            tp = pcg(S, b, Mp, Dinv, n)
            d = np.maximum(d, dist(tp.x, t.x)); rel = np.maximum(rel, relc(tp.ratio_D, t.ratio_D))
        cols.append(dict(t=t, lim=lim + 2 * d, mu=mu + 2 * np.maximum.accumulate(rel)))
    return cols, Sinv


def batched_counts(precond, tol):
    """(k_c per column, undecided per column): undecided when the deciding ratio at k_c, or the running minimum before it, lies within a
    factor 1 + mu of tol."""
    cols, _ = batched(precond)
    ks, und = [], []
    for c in cols:
        r = c["t"].ratio_D
        hit = np.where(r[1:] <= tol)[0]
        assert len(hit), "the reference did not run far enough for tol %.1e" % tol
        k = int(hit[0]) + 1
        mu = c["mu"][k]
        ks.append(k); und.append(bool(r[k] * (1 + mu) > tol or r[:k].min() < tol * (1 + mu)))
    return np.array(ks), np.array(und)
