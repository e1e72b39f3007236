"""Max-mixture edges (tsgo_max_mixture, include/tsgo.h) restated in numpy, sharing nothing with the product: the constants k, the costs,
the strict argmin, the outer loop on the dense restatements of tests/robust.py (residuals by edge_report.records under "none", as
gnc.s_base takes them; the inner solver robust.dense_lm with every class's kernel "none"), and the two closure-or-nothing scenarios.

The loop is the header's: nothing is selected at first; pass r evaluates c_m = s_e + k_m at the current estimates (s always from the BASE
information) and selects the first smallest cost of every group; no change (r > 0) stops "stable"; otherwise the graph gets base for the
winners and 0 for the losers; r == rounds_max stops "rounds"; otherwise the inner solver runs and the next pass follows."""
import functools

import numpy as np

from tests import gnc, priors, robust

NONE = robust.everywhere("none")
THREE_AXES = (0, 3)      # ODOM and pose prior; LM, virtual landmark and landmark prior use two


def axes(e_type):
    return np.where(np.isin(e_type, THREE_AXES), 3, 2)


def flat(groups):
    """(off (G + 1,), member (M,)) of a list of edge-index lists."""
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    return off, np.concatenate([np.asarray(g, np.int64) for g in groups])


def constants(e_type, base, member, log_weight=None):
    """k_m = -(ln b_0 + ln b_1 [+ ln b_2]) - 2 log_weight_m, summed in that order."""
    lw = np.zeros(len(member)) if log_weight is None else np.asarray(log_weight, np.float64).reshape(-1)
    k = np.zeros(len(member))
    for m, e in enumerate(member):
        ln = np.log(base[e, 0])
        for a in range(1, int(axes(e_type[e:e + 1])[0])):
            ln = ln + np.log(base[e, a])
        k[m] = -ln - 2.0 * lw[m]
    return k


def select(cost, off):
    """(selected position per group, the winners' costs): a cost that is not finite counts as +inf, the comparison is strict (the first
    of equal minima), a group of +inf costs selects position 0."""
    c = np.where(np.isfinite(cost), cost, np.inf)
    sel = np.array([int(np.argmin(c[a:b])) for a, b in zip(off[:-1], off[1:])], np.int64)      # argmin: the first of equal minima, 0 when all are inf
    return sel, c[off[:-1] + sel]


def gaps(cost, off):
    """Per group: second-smallest minus smallest cost (inf for a group of one)."""
    c = np.where(np.isfinite(cost), cost, np.inf)
    out = []
    for a, b in zip(off[:-1], off[1:]):
        s = np.sort(c[a:b])
        out.append(np.inf if len(s) == 1 else s[1] - s[0] if np.isfinite(s[0]) else 0.0)      # (a group of +inf costs is a tie)
    return np.array(out)


def switched(base, off, member, sel):
    """The information diagonals with base for each winner, 0 for each loser, base for the edges in no group."""
    inf = base.copy()
    inf[member] = 0
    win = member[off[:-1] + sel]
    inf[win] = base[win]
    return inf


def max_mixture(g, groups, log_weight=None, inner=5, rounds_max=32, lambda0=1e-3):
    """The loop.  Returns dict(rounds, passes, stop, n_changed, cost_sum, gap_min (per pass: the smallest gap of any group), selected,
    selected_edge, cost (last pass, flat), e_inf (what the tables hold at the end), v_pos, inner_iters, inner_stop (per round))."""
    off, member = flat(groups)
    base = g.e_inf.copy()
    base[axes(g.e_type) == 2, 2] = 0
    k = constants(g.e_type, base, member, None if log_weight is None else np.concatenate([np.asarray(w, np.float64).reshape(-1) for w in log_weight]))
    v = g.v_pos.copy()
    prev = np.full(len(groups), -1, np.int64)
    out = dict(rounds=0, passes=0, stop="rounds", n_changed=[], cost_sum=[], gap_min=[], inner_iters=[], inner_stop=[])
    held = base.copy()
    r = 0
    while True:
        cost = gnc.s_base(g, base, v)[member] + k
        sel, win = select(cost, off)
        changed = int((sel != prev).sum())
        out["n_changed"].append(changed); out["cost_sum"].append(float(win.sum())); out["gap_min"].append(float(gaps(cost, off).min()))
        out["passes"] += 1
        if changed == 0:
            out["stop"] = "stable"; break
        held = switched(base, off, member, sel)
        prev = sel
        if r == rounds_max:
            break
        if inner > 0:
            cur = g.copy(); cur.e_inf[:] = held; cur.v_pos[:] = v
            res = robust.dense_lm(cur, NONE, inner, lambda0=lambda0)
            v = res["v_pos"].copy(); out["inner_iters"].append(res["iters"]); out["inner_stop"].append(res["stop"])
        out["rounds"] += 1
        r += 1
    out.update(selected=sel, selected_edge=member[off[:-1] + sel], cost=cost, e_inf=held, v_pos=v)
    for key in ("n_changed", "cost_sum", "gap_min", "inner_iters"):
        out[key] = np.array(out[key])
    return out


# ---- closure or nothing: the outlier scenario with a null twin per closure -----------------------------------------------------------
def null_twins(g, edges, kappa):
    """(g with a twin of each listed edge appended — the same type, ids and measurement, information x kappa —, the groups [edge, twin])."""
    edges = np.asarray(edges, np.int64)
    out = priors.append_edges(g, g.e_type[edges], g.e_ids[edges], g.e_meas[edges], g.e_inf[edges] * kappa)
    return out, [[int(e), len(g.e_type) + i] for i, e in enumerate(edges)]


SCENARIO_INNER = 5                                               # inner LM cap of the scenario runs (and of the device test that follows them)
SCENARIOS = {"cauchy": 1e-6, "perturbed": 1e-8}                  # start -> kappa


@functools.lru_cache(maxsize=None)
def scenario(start):
    """(graph, groups, true, false): robust.scenario() with a null twin of each of its 37 closures (24 true, 13 false), from `start`:
    "cauchy" — the estimates robust.dense_lm reaches under CAUCHY(1.0) on ODOM (robust.SCENARIO), kappa 1e-6; "perturbed" — the
    scenario's own perturbed estimates, kappa 1e-8.  true / false: positions of the true / false closures in `groups`."""
    g = robust.scenario()
    _chain, true, false = gnc.scenario_split()
    closures = np.concatenate([true, false])
    if start == "cauchy":
        from tests.test_robust_cpu import scenario_references
        g = g.copy(); g.v_pos[:] = scenario_references()[3]["v_pos"]
    tw, groups = null_twins(g, closures, SCENARIOS[start])
    return tw, groups, np.arange(len(true)), np.arange(len(true), len(closures))


@functools.lru_cache(maxsize=None)
def scenario_run(start):
    g, groups, _true, _false = scenario(start)
    return max_mixture(g, groups, inner=SCENARIO_INNER, lambda0=robust.SCENARIO["lambda0"])
