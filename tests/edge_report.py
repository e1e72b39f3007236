"""The per-edge residual report (tsgo_edge_report, include/tsgo.h) restated in numpy, sharing nothing with the product.

Per edge, in the edge order of the graph: the residual e (classes 0 - 2 from the dense oracle's own edge functions through
independent.Linearisation, classes 3 and 4 by the prior formulas of robust.prior_terms), s = sum_k inf_k e_k^2 with the raw g.e_inf (third
entry zeroed where the class has two components), rho and w by robust.rho_w with the class's kernel of `setting`.  On top the per-class
summary: counts, how many edges have w < 1, the sums, the largest s and its edge (lowest index among equal ones: np.argmax's rule)."""
import numpy as np

from tests import independent, priors, robust

FIELDS = ("edges", "downweighted", "s_sum", "rho_sum", "s_max", "s_max_edge")
TWO_COMPONENTS = (1, 2, 4)


def residuals(g):
    """e (E, 3) at g's estimates."""
    E = len(g.e_type)
    e = np.zeros((E, 3))
    low = g.e_type <= 2
    if low.any():
        e[low] = independent.Linearisation(priors.without_priors(g)).e
    order = np.argsort(g.v_id, kind="stable")
    for t in (3, 4):
        k = np.where(g.e_type == t)[0]
        if not len(k):
            continue
        x = g.v_pos[order[np.searchsorted(g.v_id[order], g.e_ids[k, 0])]]
        m = g.e_meas[k]
        if t == 3:                                       # e_t = R_m^T (t - t_m), e_th = wrap(th - m_th)
            c, s = np.cos(m[:, 2]), np.sin(m[:, 2])
            dx, dy = x[:, 0] - m[:, 0], x[:, 1] - m[:, 1]
            e[k, 0] = c * dx + s * dy; e[k, 1] = -s * dx + c * dy
            e[k, 2] = np.arctan2(np.sin(x[:, 2] - m[:, 2]), np.cos(x[:, 2] - m[:, 2]))
        else:                                            # e = l - m
            e[k, :2] = x[:, :2] - m[:, :2]
    return e


def records(g, setting=None):
    """(E, 6): e0 e1 e2 s rho w."""
    setting = robust.full(setting)
    e = residuals(g)
    raw = g.e_inf.copy()
    raw[np.isin(g.e_type, TWO_COMPONENTS), 2] = 0
    s = (raw * e * e).sum(axis=1)
    rho = np.zeros_like(s); w = np.ones_like(s)
    for t, c in enumerate(robust.CLASSES):
        k = g.e_type == t
        if k.any():
            rho[k], w[k] = robust.rho_w(setting[c], s[k])
    return np.column_stack([e, s, rho, w])


def summary(g, rec):
    """{class: dict of FIELDS} plus "chi2" (the five rho_sum in class order)."""
    out, chi2 = {}, 0.0
    for t, c in enumerate(robust.CLASSES):
        k = np.where(g.e_type == t)[0]
        if len(k):
            worst = int(k[np.argmax(rec[k, 3])])         # the first of equal maxima: the lowest index
            out[c] = dict(edges=len(k), downweighted=int((rec[k, 5] < 1).sum()), s_sum=float(rec[k, 3].sum()), rho_sum=float(rec[k, 4].sum()),
                          s_max=float(rec[worst, 3]), s_max_edge=worst)
        else:
            out[c] = dict(edges=0, downweighted=0, s_sum=0.0, rho_sum=0.0, s_max=0.0, s_max_edge=-1)
        chi2 += out[c]["rho_sum"]
    out["chi2"] = chi2
    return out


def report(g, setting=None):
    rec = records(g, setting)
    return rec, summary(g, rec)


def coordinate_scale(g):
    return max(1.0, float(np.abs(g.v_pos).max()))


def assert_records(got, ref, g, tol_e, tol_s, tol_w, what=""):
    """The bounds of the issue: e against tol_e x max(1, largest |vertex coordinate|), s and rho against tol_s x the class's largest s,
    w against tol_w.  Prints every figure before it asserts."""
    scale = coordinate_scale(g)
    worst = dict(e=0.0, s=0.0, rho=0.0, w=0.0)
    for t in range(5):
        k = g.e_type == t
        if not k.any():
            continue
        smax = max(float(ref[k, 3].max()), np.finfo(np.float64).tiny)
        worst["e"] = max(worst["e"], float(np.abs(got[k, :3] - ref[k, :3]).max()) / scale)
        worst["s"] = max(worst["s"], float(np.abs(got[k, 3] - ref[k, 3]).max()) / smax)
        worst["rho"] = max(worst["rho"], float(np.abs(got[k, 4] - ref[k, 4]).max()) / smax)
        worst["w"] = max(worst["w"], float(np.abs(got[k, 5] - ref[k, 5]).max()))
    print("%s: e %.2e of the coordinate scale %.1f, s %.2e and rho %.2e of the class's largest s, w %.2e" % (what, worst["e"], scale, worst["s"], worst["rho"], worst["w"]))
    assert np.all(np.isfinite(got)), what
    assert worst["e"] <= tol_e and worst["s"] <= tol_s and worst["rho"] <= tol_s and worst["w"] <= tol_w, (what, worst)
    return worst
