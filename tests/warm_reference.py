"""A plain restatement of the PCG warm start (numpy, no GPU), for tests/test_warm_reference_cpu.py (the conditions under which a
comparison with the device means something) and tests/test_gpu_warm_start.py (the comparison, through tsgo_testing_warm_start).

The rule, from the history `hist` of solved pose deltas (newest first: hist[0] is the delta of the last Gauss-Newton step), a = 1 - step
(what a damped step leaves of its delta) and the cap (tsgo_config.warm_start):
  coefficients  c[m][j] = (-1)^j C(m, j + 1) a^(j + 1), j = 0 .. m - 1: order m continues the polynomial of degree m - 1 through the last m
                values of d_k / a^k;
  errors        e_m = ||hist[0] - sum_j c[m][j] hist[j + 1]||^2: what order m would have made of predicting the newest delta from the ones
                before it, for m = 1 .. n_tested = min(n_prev - 1, cap, 5) — the delta was recorded when n_prev - 1 deltas were held, and
                the recording kernel tests kMaxWarm - 1 = 5 orders at most;
  order         1, then every m = 2 .. min(n_tested, n_max) in turn with MARGIN * e_m < the best error so far (strictly); n_max =
                max(1, min(n_prev, cap, 6)).  Only tested orders are taken: order 6 is never reached;
  start         x0 = sum_j c[order][j] hist[j], r0 = b~ - S x0;
  scale         bdb / rdr when rdr > 0 and bdb > rdr, else 1, with bdb = b~' D^-1 b~ and rdr = r0' D^-1 r0 (the stop rule goes on
                measuring against the right-hand side);
  done          not (rdr > tol^2 bdb): the start already meets the rule.  Multigrid PCG only.
S, b~ and D^-1 are dense (pcg_reference.reduced_system).  Nothing here follows the kernels' loops: coefficients come from math.comb, sums
from numpy.

DEFECTS are planted into emulate(), which returns what tsgo_testing_warm_start returns; compare() is the ONE set of comparisons and limits,
used on the device's read-out by the GPU tests and on emulate()'s by the CPU test, which shows that every defect is caught by them."""
import functools
import math

import numpy as np

from oracle import oracle
from tests import pcg_reference as pr
from tests import precond_cases as pc
from tests import util
from toyslam_amd import synth

MAX_WARM = 6
MARGIN = 4.0
U = {64: 2.0 ** -53, 32: 2.0 ** -24}
DTYPE = {64: np.float64, 32: np.float32}
DEFECTS = ("sign", "a_power", "oldest_first", "first_block_only", "margin_le", "n_tested_minus_1", "scale_inverted", "scale_missing")
BLOCK = 256            # poses per workgroup of the thread-per-pose kernels

# The device's b~ against the dense one, relative to its largest entry: 1e-10 in f64 (the linearisation tests' level; 9e5 roundings).  An
# f32 handle linearises in f32: the same number of roundings of 2^-24.
B_TOL = {64: 1e-10, 32: 1e-10 * U[32] / U[64]}
# bdb and rdr against the reference's (compare(): bdb as a relative difference; rdr as the size, relative to b, of the perturbation of r0
# that explains its difference).  SUMS_MEASURED is the largest figure seen over every case of tests/test_gpu_warm_start.py on an MI355X
# (planted and observed, both preconditioners, both recording kernels), the limit is MARGIN x that (precond_cases.MARGIN: the kernels
# are deterministic, the margin is for compilers and reduction orders).  f64: bdb 7.158e-12 and rdr 5.987e-12, both at step 12 of the
# observed rules = 1 run under block-Jacobi, where b has shrunk by 1e-5 and its own difference is 6.9e-11 of its largest entry.  f32:
# bdb 1.171e-07 (observed run, step 11), rdr 2.900e-06 (planted degree-4 trend: x0 sums five f32 products with coefficients up to 6.4).
# Above 1e-9 in f64 would be a finding, not a limit.
SUMS_MEASURED = {64: 7.158e-12, 32: 2.900e-06}
SUMS_LIMIT = {p: pc.MARGIN * v for p, v in SUMS_MEASURED.items()}


# ---- the rule ----
def coefficients(a, m):
    return np.array([(-1) ** j * math.comb(m, j + 1) * a ** (j + 1) for j in range(m)])


def predict(vs, a, m):
    """sum_j c[m][j] vs[j]: vs newest first, at least m rows."""
    return coefficients(a, m) @ np.asarray(vs, np.float64)[:m]


def orders(n_prev, cap):
    """(n_max, n_tested) of a warm start from n_prev held deltas."""
    n_max = max(1, min(n_prev, cap, MAX_WARM))
    return n_max, min(max(n_prev - 1, 0), cap, MAX_WARM - 1, n_max)


def errors(hist, a, n_tested):
    hist = np.asarray(hist, np.float64)
    return np.array([float(np.sum((hist[0] - predict(hist[1:], a, m)) ** 2)) for m in range(1, n_tested + 1)])


def choose(err, n_max):
    """(order, decision ratios): ratio_m = MARGIN e_m / best-so-far for every m compared; order m is taken when it is < 1."""
    m, ratios = 1, []
    best = err[0] if len(err) else 0.0
    for j in range(2, min(len(err), n_max) + 1):
        e = err[j - 1]
        ratios.append(MARGIN * e / best if best > 0 else np.inf)
        if MARGIN * e < best:
            best, m = e, j
    return m, ratios


def start(hist, a, order, S, b, Dinv, tol):
    x0 = predict(hist, a, order)
    r0 = b - S @ x0
    bdb, rdr = float(b @ (Dinv @ b)), float(r0 @ (Dinv @ r0))
    scale = bdb / rdr if (rdr > 0 and bdb > rdr) else 1.0
    return dict(x0=x0, r0=r0, bdb=bdb, rdr=rdr, scale=scale, done=int(not (rdr > tol * tol * bdb)))


def warm_start(hist, a, cap, S, b, Dinv, tol, amg):
    """Everything the rule yields from a history (n_prev, 3 P), newest first."""
    hist = np.asarray(hist, np.float64)
    n_prev = len(hist)
    warmed = int(cap > 0 and n_prev > 0 and a > 0)
    n_max, n_tested = orders(n_prev, cap)
    out = dict(warmed=warmed, n_prev=n_prev, n_max=n_max, n_tested=n_tested)
    if not warmed:
        return out
    err = errors(hist, a, n_tested)
    order, ratios = choose(err, n_max)
    out.update(err=err, order=order, ratios=ratios)
    out.update(start(hist, a, order, S, b, Dinv, tol))
    if not amg:
        out["done"] = 0
    return out


# ---- the same with a defect planted, in the shape of the device's read-out ----
def emulate(planted, a, cap, S, b, Dinv, tol, amg, defect=None, precision=64):
    """What tsgo_testing_warm_start would return after `planted` (oldest first) on a device with `defect` (None: a correct one, in exact
    f64 arithmetic on the deltas rounded to the handle's precision)."""
    assert defect is None or defect in DEFECTS
    hist = np.asarray(planted, np.float64).astype(DTYPE[precision]).astype(np.float64)[::-1][:MAX_WARM]
    n_prev = len(hist)
    n_max, n_tested = orders(n_prev, cap)
    warmed = int(cap > 0 and n_prev > 0 and a > 0)
    out = dict(warmed=warmed, n_prev=n_prev, n_max=n_max, n_tested=n_tested, carried=0, order=0, done=0, err=np.zeros(MAX_WARM), scale=0.0, bdb=0.0, rdr=0.0,
               hist=hist.copy(), b=b.copy(), x0=np.zeros_like(b), r0=np.zeros_like(b))
    if not warmed:
        return out
    if defect == "n_tested_minus_1":
        n_tested = max(n_tested - 1, 0)
        out["n_tested"] = n_tested

    def coef(m):
        c = coefficients(a, m)
        if defect == "sign":
            c = np.abs(c)
        if defect == "a_power":
            c = c / a
        return c

    def pred(vs, m):
        vs = vs[::-1] if defect == "oldest_first" else vs
        return coef(m) @ vs[:m]

    rows = slice(0, 3 * BLOCK) if defect == "first_block_only" else slice(None)
    err = np.array([float(np.sum((hist[0] - pred(hist[1:], m))[rows] ** 2)) for m in range(1, n_tested + 1)])
    order = 1
    best = err[0] if len(err) else 0.0
    for j in range(2, min(n_tested, n_max) + 1):
        e = err[j - 1]
        if (MARGIN * e <= best) if defect == "margin_le" else (MARGIN * e < best):
            best, order = e, j
    x0 = pred(hist, order)
    r0 = b - S @ x0
    bdb, rdr = float(b @ (Dinv @ b)), float(r0 @ (Dinv @ r0))
    scale = bdb / rdr if (rdr > 0 and bdb > rdr) else 1.0
    if defect == "scale_inverted":
        scale = rdr / bdb if (rdr > 0 and bdb > rdr) else 1.0
    if defect == "scale_missing":
        scale = 1.0
    out["err"][:n_tested] = err
    out.update(order=order, x0=x0, r0=r0, bdb=bdb, rdr=rdr, scale=scale, done=int(amg and not (rdr > tol * tol * bdb)))
    return out


# ---- the comparisons ----
def x0_bound(hist, a, m, u):
    """Componentwise: m products with a rounded coefficient and m - 1 sums."""
    return 2 * (m + 2) * u * (np.abs(coefficients(a, m)) @ np.abs(hist[:m]))


def r0_bound(sys_, b, x0, u):
    return pc.product_bound(sys_["mag"], x0, u, sys_["deg_max"]) + u * np.abs(b)


def compare(out, a, cap, sys_, tol, amg, precision=64, planted=None, n_prev=None, carried=0):
    """The device's read-out `out` against the rule.  planted: the deltas given to the hook (oldest first; hist must equal them, rounded
    to the handle's precision), or None with n_prev, the number of deltas the handle must hold (the caller compares hist itself).
    Returns (failures, figures): a list of texts, empty when everything holds, and the measured relative differences of bdb and rdr."""
    u, dt = U[precision], DTYPE[precision]
    S, bt, Dinv = sys_["S"], sys_["bt"], sys_["Dinv"]
    bad, fig = [], {}
    hist = np.asarray(out["hist"], np.float64)
    if planted is not None:
        want = np.asarray(planted, np.float64).astype(dt).astype(np.float64)[::-1][:MAX_WARM]
        n_prev = len(want)
        if not (cap > 0 and a > 0):
            hist = want      # a handle that cannot warm-start returns the counters and b alone
        elif hist.shape != want.shape or not np.array_equal(hist, want):
            bad.append("hist is not the planted deltas, newest first")
    ref = warm_start(hist, a, cap, S, bt, Dinv, tol, amg)
    for k, want in (("warmed", ref["warmed"]), ("n_prev", n_prev), ("n_tested", ref["n_tested"]), ("n_max", ref["n_max"]), ("carried", carried)):
        if out[k] != want:
            bad.append("%s %d, expected %d" % (k, out[k], want))
    db = float(np.abs(out["b"] - bt).max() / np.abs(bt).max())
    fig["b"] = db
    if not db <= B_TOL[precision]:
        bad.append("b differs from the dense b~ by %.2e of its largest entry (limit %.1e)" % (db, B_TOL[precision]))
    if not ref["warmed"] or not out["warmed"] or len(hist) != ref["n_prev"]:
        return bad, fig
    m = ref["order"]
    if out["order"] != m:
        bad.append("order %d, expected %d (decision ratios %s)" % (out["order"], m, ["%.3g" % r for r in ref["ratios"]]))
    # err[m]: the device's sum against the rule's, within the rounding of its terms
    P = len(bt) // 3
    for k in range(ref["n_tested"]):
        c = coefficients(a, k + 1)
        delta = 2 * (k + 3) * u * (np.abs(hist[0]) + np.abs(c) @ np.abs(hist[1:k + 2]))
        e = ref["err"][k]
        nd = float(np.linalg.norm(delta))
        lim = 2 * np.sqrt(e) * nd + nd * nd + 3 * P * u * e
        if not abs(out["err"][k] - e) <= lim:
            bad.append("err[%d] %.17g, expected %.17g (difference %.2e, limit %.2e)" % (k, out["err"][k], e, abs(out["err"][k] - e), lim))
    if np.any(out["err"][ref["n_tested"]:] != 0):
        bad.append("err beyond n_tested is not zero")
    # x0 against the prediction from the device's own history
    xw = predict(hist, a, m)
    over = np.abs(out["x0"] - xw) - x0_bound(hist, a, m, u)
    if not over.max() <= 0:
        bad.append("x0 is off the order-%d prediction by %.2e beyond its rounding bound" % (m, over.max()))
    # r0 against b - S x0 of the device's own b and x0
    rw = out["b"] - S @ out["x0"]
    rb = r0_bound(sys_, out["b"], out["x0"], u)
    over = np.abs(out["r0"] - rw) - rb
    if not over.max() <= 0:
        bad.append("r0 is off b - S x0 by %.2e beyond the product bound" % over.max())
    # scale from the two sums of the same read-out, in the handle's precision
    bdb, rdr = out["bdb"], out["rdr"]
    sw = bdb / rdr if (rdr > 0 and bdb > rdr) else 1.0
    if not abs(out["scale"] - sw) <= 2 * float(np.spacing(dt(sw))):
        bad.append("scale %.17g, expected %.17g from bdb / rdr of the same read-out" % (out["scale"], sw))
    # the two sums against the reference's.  bdb: the relative difference.  rdr: r0 is what S x0 leaves of b, 1 / sqrt(scale) of it, so a
    # perturbation eta of r0 of the size eps of b (in the D^-1 norm: eta' D^-1 eta = eps^2 bdb) moves rdr by up to 2 sqrt(rdr bdb) eps +
    # bdb eps^2 — a relative difference of rdr that grows with sqrt(scale) for the same rounding, and means nothing where x0 is the
    # solution itself and r0 IS rounding.  The figure held to the limit is that eps: the size, relative to b, of the perturbation of r0
    # that explains the difference.
    fig["bdb"] = abs(bdb - ref["bdb"]) / ref["bdb"]
    root = np.sqrt(ref["rdr"] * ref["bdb"])
    fig["rdr"] = float((np.sqrt(root * root + ref["bdb"] * abs(rdr - ref["rdr"])) - root) / ref["bdb"])
    fig["rdr_raw"] = abs(rdr - ref["rdr"]) / ref["rdr"] if ref["rdr"] > 0 else 0.0
    for k in ("bdb", "rdr"):
        if not fig[k] <= SUMS_LIMIT[precision]:
            bad.append("%s %.17g, reference %.17g: difference %.2e (limit %.1e)" % (k, out[k], ref[k], fig[k], SUMS_LIMIT[precision]))
    if out["done"] != ref["done"]:
        bad.append("done %d, expected %d (rdr / (tol^2 bdb) = %.3g)" % (out["done"], ref["done"], ref["rdr"] / (tol * tol * ref["bdb"]) if ref["bdb"] > 0 else np.nan))
    return bad, fig


# ---- the graphs and their dense systems ----
GRAPHS = {"g300": lambda: synth.make(300, 10, loop_closures=4, seed=5),      # 300 poses: two workgroups of the thread-per-pose kernels
          "g40": pc.CASES["level0_only"]["graph"]}                             # 40 poses: one


@functools.lru_cache(maxsize=None)
def graph(name):
    return GRAPHS[name]()


def system_of(g, odom_jacobian="constant", python=False):
    """Dense S, b~, D^-1 (pcg_reference), the magnitudes and the row degree of precond_cases.product_bound, and x* = S^-1 b~.
    python: b as rules = 1 linearises it, zeroed at the fixed vertices before the landmarks are eliminated."""
    s = dict(pr._system(g, odom_jacobian))
    if python:
        L = len(s["lm"])
        w = s["Hlp"].T @ np.einsum("lxy,ly->lx", s["Hll_inv"], s["bl"].reshape(L, 2)).reshape(-1) if L else 0.0
        bp = s["bt"] + w
        pose_ids = g.v_id[s["pose"]]
        for k in np.where(np.isin(pose_ids, g.fixed))[0]:
            bp[3 * k:3 * k + 3] = 0
        assert not np.isin(g.v_id[s["lm"]], g.fixed).any()
        s["bt"] = bp - w
    oracle.set_odom_jacobian(odom_jacobian)
    try:
        _S, mag = oracle.schur_dense(util.to_oracle(g), with_magnitude=True)
    finally:
        oracle.set_odom_jacobian("constant")
    P = len(s["pose"])
    s["mag"] = np.repeat(np.repeat(mag.reshape(P, 3, P, 3).max(axis=(1, 3)), 3, 0), 3, 1)      # block by block, as precond_cases.reference
    s["deg_max"] = pc.deg_max(s["S"])
    s["x_star"] = np.linalg.solve(s["S"], s["bt"])
    return s


def fast_system(g, odom_jacobian="constant", python=False, lam=0.0):
    """system_of() for the estimates a device run is at, step after step: the same dense quantities from ONE dense linearisation by
    matrix products (tests/test_warm_reference_cpu.py holds it to system_of), and `delta`, the pose part of the dense Gauss-Newton step
    (H + lam I) d = b at those estimates.  Graphs of edge types 0-2."""
    assert not (g.e_type >= 3).any()
    oracle.set_odom_jacobian(odom_jacobian)
    try:
        H, b, _chi2, idx = oracle.linearize(util.to_oracle(g))
    finally:
        oracle.set_odom_jacobian("constant")
    pose = np.where(g.v_type == 0)[0]; lm = np.where(g.v_type == 1)[0]
    P, L = len(pose), len(lm)
    if python:
        for v in np.where(np.isin(g.v_id, g.fixed))[0]:
            b[idx[v]:idx[v] + (3 if g.v_type[v] == 0 else 2)] = 0
    ip = (idx[pose][:, None] + np.arange(3)[None, :]).reshape(-1)
    il = (idx[lm][:, None] + np.arange(2)[None, :]).reshape(-1)
    Hpp, Hpl = H[np.ix_(ip, ip)], H[np.ix_(ip, il)]
    k = np.arange(L)
    blocks = H[np.ix_(il, il)].reshape(L, 2, L, 2)[k, :, k, :]

    def reduce(shift):
        inv = np.linalg.pinv(blocks + shift * np.eye(2)[None], hermitian=True)
        T = np.einsum("plx,lxy->ply", Hpl.reshape(3 * P, L, 2), inv).reshape(3 * P, 2 * L)
        S = Hpp + shift * np.eye(3 * P) - T @ Hpl.T
        return 0.5 * (S + S.T), b[ip] - T @ b[il], inv

    S, bt, inv = reduce(0.0)
    mag = np.abs(Hpp) + np.einsum("plx,lxy->ply", np.abs(Hpl).reshape(3 * P, L, 2), np.abs(inv)).reshape(3 * P, 2 * L) @ np.abs(Hpl).T
    mag = 0.5 * (mag + mag.T)
    kk = np.arange(P)
    Dinv = np.zeros_like(S)
    Dinv.reshape(P, 3, P, 3)[kk, :, kk, :] = np.linalg.pinv(S.reshape(P, 3, P, 3)[kk, :, kk, :], hermitian=True)
    out = dict(S=S, bt=bt, Dinv=Dinv, mag=np.repeat(np.repeat(mag.reshape(P, 3, P, 3).max(axis=(1, 3)), 3, 0), 3, 1), deg_max=pc.deg_max(S))
    Sl, bl, _ = reduce(lam) if lam else (S, bt, None)
    out["delta"] = np.linalg.solve(Sl, bl)
    out["x_star"] = out["delta"] if not lam else np.linalg.solve(S, bt)
    return out


@functools.lru_cache(maxsize=None)
def system(name, python=False):
    return system_of(graph(name), "constant", python)


# ---- the planted cases ----
PLANT_TOL = 1e-6       # pcg_rel_tol of the planted handles: `done` is decided by many decades either way (test_warm_reference_cpu.py)
RHO = 10.0             # a trend's term of degree i is this many times smaller than the one of degree i - 1
NOISE = 1e-3           # ... and the noise this share of its smallest term


OFFSET = 2e-3          # a trend's prediction lies this far from x*, relative to ||x*||, in a random direction: scale comes to about 10^3


def trend(n, deg, n_rows, a, seed, target=None, noise=NOISE):
    """n deltas, oldest first: d_k = a^k q(k) + noise, q a vector polynomial of degree deg in t = k - (n - 1) whose term of degree i has
    the size RHO^-i of the constant one: the i-th difference of q, which is what order i leaves of it, falls by RHO from order to order
    down to the noise.  target: what order deg + 1 predicts for the next delta, a^n q(1), without the noise (the constant term is
    chosen for it); None: a random one."""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(deg + 1, n_rows)) / np.sqrt(n_rows)
    if target is not None:
        g[1:] *= np.linalg.norm(target) / a ** n
        g[0] = target / a ** n - sum(g[i] * RHO ** -i / math.factorial(i) for i in range(1, deg + 1))
    size = np.linalg.norm(g[0])
    t = np.arange(n) - (n - 1.0)
    q = sum(np.outer(t ** i / math.factorial(i), g[i]) * RHO ** -i for i in range(deg + 1))
    q = q + noise * RHO ** -deg * size * rng.normal(size=q.shape) / np.sqrt(n_rows)
    return (a ** np.arange(n))[:, None] * q


def near_solution(name, seed, python=False):
    """x* of the graph's system plus OFFSET ||x*|| in a random direction: where the planted trends point."""
    xs = system(name, python)["x_star"]
    e = np.random.default_rng(seed).normal(size=xs.shape)
    return xs + OFFSET * np.linalg.norm(xs) * e / np.linalg.norm(e)


def tie(n_rows, seed):
    """Three deltas for a = 0.5 with e_1 = 4 ||w||^2 and e_2 = ||w||^2 in small integers: MARGIN e_2 == e_1 whatever the summation order
    and the precision.  d3 - a d2 = 2 w; d3 - 2 a d2 + a^2 d1 = w."""
    rng = np.random.default_rng(seed)
    w = rng.integers(-3, 4, size=n_rows).astype(np.float64)
    z = rng.integers(-3, 4, size=n_rows).astype(np.float64)
    return np.array([4 * z - 4 * w, 2 * z, 2 * w + z])


def _cases():
    c = {}
    for deg in range(5):      # the reference picks exactly order deg + 1
        c["trend%d" % deg] = dict(graph="g300", kw={}, a=0.8, cap=6, plant=lambda n, deg=deg: trend(6, deg, n, 0.8, 40 + deg, near_solution("g300", 140 + deg)), kind="trend", f32=True)
    # degree 5: order 6 would continue it exactly, but only orders 1 .. 5 are ever measured, and only measured orders are taken
    c["trend5"] = dict(graph="g300", kw={}, a=0.8, cap=6, plant=lambda n: trend(6, 5, n, 0.8, 45, near_solution("g300", 145)), kind="trend")
    c["trend1_g40"] = dict(graph="g40", kw={}, a=0.8, cap=6, plant=lambda n: trend(6, 1, n, 0.8, 51, near_solution("g40", 151)), kind="trend")
    c["tie"] = dict(graph="g300", kw=dict(rules="python", lr=0.5), a=0.5, cap=6, plant=lambda n: tie(n, 60), kind="tie")
    for k in (1, 2, 7, 12):   # the rotation: only six deltas are kept
        c["plant%d" % k] = dict(graph="g300", kw={}, a=0.8, cap=6, plant=lambda n, k=k: trend(k, 1, n, 0.8, 70 + k, near_solution("g300", 170 + k)), kind="rotation")
    c["zeros"] = dict(graph="g300", kw={}, a=0.8, cap=6, plant=lambda n: np.zeros((3, n)), kind="zeros")
    c["x_star"] = dict(graph="g300", kw={}, a=0.8, cap=6, plant=lambda n: system("g300")["x_star"][None, :] / 0.8, kind="x_star")
    for cap in (1, 2, 6):
        c["cap%d" % cap] = dict(graph="g300", kw=dict(warm_start=cap), a=0.8, cap=cap, plant=lambda n: trend(6, 2, n, 0.8, 80, near_solution("g300", 180)), kind="cap")
    c["cap0"] = dict(graph="g300", kw=dict(warm_start=0), a=0.8, cap=0, plant=lambda n: trend(3, 1, n, 0.8, 81), kind="cold")
    c["lr1"] = dict(graph="g300", kw=dict(rules="python", lr=1.0), a=0.0, cap=6, plant=lambda n: trend(3, 1, n, 0.8, 82), kind="cold")
    return c


CASES = _cases()
EXPECTED_ORDER = {"trend0": 1, "trend1": 2, "trend2": 3, "trend3": 4, "trend4": 5, "trend5": 5, "trend1_g40": 2, "tie": 1, "plant1": 1, "plant2": 1, "plant7": 2,
                  "plant12": 2, "zeros": 1, "x_star": 1, "cap1": 1, "cap2": 2, "cap6": 3}


def case_system(name):
    c = CASES[name]
    return system(c["graph"], c["kw"].get("rules") == "python")


@functools.lru_cache(maxsize=None)
def planted(name):
    return CASES[name]["plant"](len(case_system(name)["bt"]))


# ---- the observed runs: twelve optimize(1) calls on g300, restated with dense solves ----
OBSERVED = {"constant": dict(kw=dict(odom_jacobian="constant"), step=0.2, python=False),
            "analytic": dict(kw=dict(odom_jacobian="analytic"), step=0.2, python=False),
            "python": dict(kw=dict(rules="python", lr=0.6, odom_jacobian="analytic"), step=0.6, python=True)}
OBS_STEPS = 12
OBS_TOL = 1e-12
PY_LAMBDA = 1e-3 / 1.1      # rules = 1: every optimize call starts lambda at 1e-3 and divides it by 1.1 before its first linearisation
TIE_BAND = 0.01             # no decision of an observed run lies within 1 % of a tie


def dense_step(g, odom_jacobian, python):
    """The full delta (V, 3) of one Gauss-Newton step at g's estimates: H d = b dense (util.dense_solution), or under rules = 1
    (H + lambda I) d = b with b zeroed at the fixed vertices."""
    oracle.set_odom_jacobian(odom_jacobian)
    try:
        if not python:
            return util.dense_solution(g)[0]
        o = util.to_oracle(g)
        H, b, _err, idx = oracle.linearize(o, python_mode=True)
        x = np.linalg.solve(H + PY_LAMBDA * np.eye(len(b)), -b)
        d = np.zeros((len(o.v_id), 3))
        for i in range(len(o.v_id)):
            m = 3 if o.v_type[i] == 0 else 2
            d[i, :m] = x[idx[i]:idx[i] + m]
        return d
    finally:
        oracle.set_odom_jacobian("constant")


def advance(g, d, step):
    """g with every vertex moved by step * d (oracle.update_pose for poses; a landmark's position is added to)."""
    out = g.copy()
    for i in range(len(g.v_id)):
        if g.v_type[i] == 0:
            out.v_pos[i] = oracle.update_pose(g.v_pos[i], step * d[i])
        else:
            out.v_pos[i, :2] = g.v_pos[i, :2] + step * d[i, :2]
    return out


@functools.lru_cache(maxsize=None)
def observed(setting):
    """Per step k = 0 .. OBS_STEPS: the graph at the estimates BEFORE step k, its dense system and — k < OBS_STEPS — the dense pose delta
    of step k (3 P,).  Entry k is what the hook sees after k optimize(1) calls."""
    s = OBSERVED[setting]
    g = graph("g300")
    oj = s["kw"].get("odom_jacobian", "constant")
    out = []
    for k in range(OBS_STEPS + 1):
        d = dense_step(g, oj, s["python"]) if k < OBS_STEPS else None
        out.append(dict(graph=g, system=system_of(g, oj, s["python"]), delta=None if d is None else d[g.v_type == 0].reshape(-1)))
        if d is not None:
            g = advance(g, d, s["step"])
    return out


def observed_reference(setting, k, amg=True, tol=OBS_TOL):
    """The rule on the dense deltas of the steps before k (k >= 1), at the dense system of step k."""
    run = observed(setting)
    hist = np.array([run[j]["delta"] for j in range(k - 1, max(k - 1 - MAX_WARM, -1), -1)])
    s = run[k]["system"]
    return warm_start(hist, 1.0 - OBSERVED[setting]["step"], MAX_WARM, s["S"], s["bt"], s["Dinv"], tol, amg)
