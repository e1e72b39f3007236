"""Graduated non-convexity with the truncated-least-squares surrogate (tsgo_gnc, include/tsgo.h) restated in numpy, sharing nothing with
the product: the weight function, the outer loop on the dense restatements of tests/robust.py (residuals by edge_report.records, the inner
solver robust.dense_lm with every class's kernel "none"), and the chain / closure split of the outlier scenario (robust.scenario()).

The loop is the header's: a probe at the start gives q_max = max over subject edges of s / barc2[class]; 2 q_max - 1 <= 0 ends with
"all_inliers"; otherwise mu = 1 / (2 q_max - 1) and every round reweights at the current estimates (s always from the BASE information),
runs the inner solver on the graph with w * base, stops "binary" when every subject weight of the round was 0 or 1, else mu *= mu_step."""
import functools

import numpy as np

from tests import edge_report, robust

NONE = robust.everywhere("none")
BARC2_DEFAULT = np.array([11.345, 9.210, 9.210, 11.345, 9.210])      # 99 % chi^2 quantiles: 3 dof (types 0, 3), 2 dof (types 1, 2, 4)


def tls_weight(q, mu):
    """w(q; mu): 1 up to mu / (mu + 1), 0 from (mu + 1) / mu on, sqrt(mu (mu + 1) / q) - mu in between; float64, elementwise."""
    q = np.asarray(q, np.float64)
    mu = np.float64(mu)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mid = np.sqrt(mu * (mu + 1.0) / q) - mu
    return np.where(q <= mu / (mu + 1.0), 1.0, np.where(q >= (mu + 1.0) / mu, 0.0, mid))


def subject_edges(g, barc2, subject=None):
    """Boolean (E,): the class has barc2 > 0 and the mask (None: every edge) names the edge."""
    barc2 = np.asarray(barc2, np.float64)
    m = np.ones(len(g.e_type), bool) if subject is None else np.asarray(subject).reshape(-1) != 0
    return m & (barc2[g.e_type] > 0)


def s_base(g, base, v_pos):
    """s = sum_k base_k e_k^2 per edge at v_pos."""
    at = g.copy(); at.e_inf[:] = base; at.v_pos[:] = v_pos
    return edge_report.records(at, NONE)[:, 3]


def weights_at(g, base, v_pos, barc2, subj, mu):
    """(w (E,), s (E,)): the weights of one round at v_pos; 1 on edges that are not subject."""
    s = s_base(g, base, v_pos)
    w = np.ones(len(s))
    w[subj] = tls_weight(s[subj] / np.asarray(barc2, np.float64)[g.e_type[subj]], mu)
    return w, s


def gnc_tls(g, barc2=BARC2_DEFAULT, subject=None, inner=10, mu_step=1.4, rounds_max=64, lambda0=1e-3):
    """The loop.  Returns dict(rounds, stop, q_max, mu, cost, n_zero, n_one, n_between (per round), w (last round), v_pos, chi2 (of the
    graph with w * base at the final estimates, kernels "none"), inner_iters (per round))."""
    barc2 = np.asarray(barc2, np.float64)
    base = g.e_inf.copy()
    subj = subject_edges(g, barc2, subject)
    assert subj.any()
    v = g.v_pos.copy()
    q_max = float((s_base(g, base, v)[subj] / barc2[g.e_type[subj]]).max())
    out = dict(rounds=0, stop="all_inliers", q_max=q_max, mu=[], cost=[], n_zero=[], n_one=[], n_between=[], inner_iters=[], w=np.ones(len(base)))
    if not 2.0 * q_max - 1.0 > 0.0:
        out.update(v_pos=v, chi2=float(robust.chi2_at(g, NONE)))
        return out
    mu = 1.0 / (2.0 * q_max - 1.0)
    out["stop"] = "rounds"
    cur = g.copy()
    for _ in range(rounds_max):
        w, s = weights_at(g, base, v, barc2, subj, mu)
        cur = g.copy(); cur.e_inf[:] = w[:, None] * base; cur.v_pos[:] = v
        out["mu"].append(mu); out["cost"].append(float((w[subj] * s[subj]).sum()))
        out["n_zero"].append(int((w[subj] == 0).sum())); out["n_one"].append(int((w[subj] == 1).sum()))
        out["n_between"].append(int(((w[subj] != 0) & (w[subj] != 1)).sum()))
        out["rounds"] += 1; out["w"] = w
        if inner > 0:
            res = robust.dense_lm(cur, NONE, inner, lambda0=lambda0)
            v = res["v_pos"].copy(); out["inner_iters"].append(res["iters"])
        if out["n_between"][-1] == 0:
            out["stop"] = "binary"; break
        mu *= mu_step
    cur.v_pos[:] = v
    out.update(v_pos=v, chi2=float(robust.chi2_at(cur, NONE)))
    for k in ("mu", "cost", "n_zero", "n_one", "n_between", "inner_iters"):
        out[k] = np.array(out[k])
    return out


# ---- the outlier scenario -------------------------------------------------------------------------------------------------------------
def scenario_split():
    """(chain, true closures, false closures): index arrays into the edges of robust.scenario() — the generator's odometry, the closures
    of scenario_clean() behind it, the false closures appended last."""
    n_clean, n_all = len(robust.scenario_clean().e_type), len(robust.scenario().e_type)
    n_true = robust.SCENARIO["closures"]
    return np.arange(0, n_clean - n_true), np.arange(n_clean - n_true, n_clean), np.arange(n_clean, n_all)


def scenario_closure_mask():
    """The per-edge mask of the scenario: closures (true and false) subject, the chain exempt (known inliers)."""
    chain, true, false = scenario_split()
    m = np.zeros(len(chain) + len(true) + len(false), np.uint8)
    m[true] = 1; m[false] = 1
    return m


SCENARIO_INNER = 3      # inner LM cap of the scenario runs below (and of the device test that follows them)


@functools.lru_cache(maxsize=None)
def scenario_run(closures_only=True, inner=SCENARIO_INNER):
    """gnc_tls on robust.scenario(), ODOM threshold 11.345: the closures subject (the run that works) or the whole class (the collapse)."""
    g = robust.scenario()
    return gnc_tls(g, BARC2_DEFAULT, scenario_closure_mask() if closures_only else None, inner=inner, lambda0=robust.SCENARIO["lambda0"])


# ---- the five-class graph of the reweighting tests --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def c1_case(seed=12, fraction=0.6):
    """(robust.c1_five_classes(), a random per-edge mask that names about `fraction` of the edges of every class)."""
    g = robust.c1_five_classes()
    return g, (np.random.default_rng(seed).random(len(g.e_type)) < fraction).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def c1_run(inner=5, rounds_max=3):
    """gnc_tls on c1_case() with the default thresholds: every class subject under the mask."""
    g, mask = c1_case()
    return gnc_tls(g, BARC2_DEFAULT, mask, inner=inner, rounds_max=rounds_max)
