"""ctypes access to the CPU oracle (oracle/libtsgo_oracle.so) — TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg import this module.
Nothing in toyslam_amd/ may.  Build the library with `make -C oracle` (or __graft_entry__.build()).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

u32p = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
ALLREDUCE_FN = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.c_int64, C.c_void_p)
_GRAPH = [C.c_int, u32p, u32p, f64p, C.c_int, u32p, u32p, f64p, f64p, C.c_int, u32p]


def build(force=False):
    so = os.path.join(_HERE, "libtsgo_oracle.so")
    if force or not os.path.exists(so):
        subprocess.check_call(["make", "-C", _HERE] + (["-B"] if force else []), stdout=subprocess.DEVNULL)
    return so


def default_threads():
    """Threads for the twin's OpenMP loops: the process's CPU share, capped at 8 (a GPU box shows every
    logical CPU of the host; oversubscribed OpenMP barriers spin for milliseconds)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(8, n))


def set_threads(n):
    lib().oracle_set_threads(int(n))


def set_odom_jacobian(kind):
    """"constant" (the reference: A = -I, B = +I, EdgeSe2.h:35-37) or "analytic" (the extension of SURVEY 8f rank 4).  Process-wide:
    every oracle entry point, dense and twin, follows it.  Tests that switch it switch it back."""
    lib().oracle_set_odom_jacobian({"constant": 0, "analytic": 1}[kind])


def set_cycle_level0(kind):
    """"implicit" (default) or "explicit": what the twin's two products inside the multigrid cycle read (tsgo_config.cycle_level0)."""
    lib().oracle_set_cycle_level0({"implicit": 0, "explicit": 1}[kind])


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(build())
        for sfx in ("f64", "f32"):
            getattr(L, "oracle_edge_eval_" + sfx).argtypes = _GRAPH + [f64p, f64p, f64p]
            getattr(L, "oracle_linearize_" + sfx).argtypes = _GRAPH + [C.c_int, C.c_void_p, f64p, f64p, i32p]
            getattr(L, "oracle_optimize_" + sfx).argtypes = _GRAPH + [f64p, C.c_int, C.c_int, C.c_int, C.c_double,
                                                                      f64p, i32p, i32p, f64p]
        L.oracle_solve_f64.argtypes = [f64p, f64p, C.c_int, C.c_int]
        L.oracle_update_pose_f64.argtypes = [f64p, f64p]
        L.oracle_last_phase_seconds.argtypes = [f64p]; L.oracle_last_phase_seconds.restype = None
        L.oracle_num_unknowns.argtypes = [C.c_int, u32p]
        L.oracle_sparse_step.argtypes = _GRAPH + [C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, ALLREDUCE_FN, C.c_void_p,
                                                  f64p, f64p, i32p]
        L.oracle_sparse_optimize.argtypes = _GRAPH + [f64p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                                      ALLREDUCE_FN, C.c_void_p, f64p, i32p, i32p, i32p, f64p,
                                                      f64p, f64p, C.c_int, C.c_double]
        L.oracle_twin_precond.argtypes = _GRAPH + [C.c_int, C.c_int, C.c_int, C.c_int, f64p, f64p, C.c_void_p, C.c_void_p, f64p, i32p]
        L.oracle_twin_perturb.argtypes = [C.c_double, C.c_int, C.c_int]; L.oracle_twin_perturb.restype = None
        L.oracle_set_threads.argtypes = [C.c_int]
        L.oracle_set_threads.restype = None
        L.oracle_set_threads(default_threads())
        _LIB = L
    return _LIB


class Graph:
    """SoA OptGraph as the oracle consumes it (doubles on the host side).

    v_pos[i] = (x, y, theta) for poses, (x, y, 0) for landmarks; e_meas[i] = 3x3 row-major for ODOM,
    (range, bearing, 0...) for LM; e_inf[i] = diagonal of the information matrix (3 slots)."""

    def __init__(self, v_id, v_type, v_pos, e_type, e_ids, e_meas, e_inf, fixed):
        self.v_id = np.ascontiguousarray(v_id, np.uint32)
        self.v_type = np.ascontiguousarray(v_type, np.uint32)
        self.v_pos = np.ascontiguousarray(v_pos, np.float64).reshape(-1, 3)
        self.e_type = np.ascontiguousarray(e_type, np.uint32)
        self.e_ids = np.ascontiguousarray(e_ids, np.uint32).reshape(-1, 2)
        self.e_meas = np.ascontiguousarray(e_meas, np.float64).reshape(-1, 9)
        self.e_inf = np.ascontiguousarray(e_inf, np.float64).reshape(-1, 3)
        self.fixed = np.ascontiguousarray(fixed, np.uint32)

    @classmethod
    def from_npz(cls, z, as_wire=False):
        g = cls(z["v_id"], z["v_type"], z["v_pos"], z["e_type"], z["e_ids"], z["e_meas"], z["e_inf"], z["fixed"])
        return g.rounded_to_wire() if as_wire else g

    def rounded_to_wire(self):
        r = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
        return Graph(self.v_id, self.v_type, r(self.v_pos), self.e_type, self.e_ids, r(self.e_meas),
                     r(self.e_inf), self.fixed)

    def copy(self):
        return Graph(self.v_id.copy(), self.v_type.copy(), self.v_pos.copy(), self.e_type.copy(),
                     self.e_ids.copy(), self.e_meas.copy(), self.e_inf.copy(), self.fixed.copy())

    @property
    def n_unknowns(self):
        return int(3 * (self.v_type == 0).sum() + 2 * (self.v_type == 1).sum())

    def args(self):
        fx = self.fixed if len(self.fixed) else np.zeros(1, np.uint32)
        return [len(self.v_id), self.v_id, self.v_type, self.v_pos, len(self.e_type), self.e_type, self.e_ids,
                self.e_meas, self.e_inf, len(self.fixed), fx]


def _sfx(precision):
    return {"f64": "f64", "f32": "f32", 64: "f64", 32: "f32"}[precision]


def edge_eval(g, precision="f64"):
    E = len(g.e_type)
    e = np.zeros((E, 3)); A = np.zeros((E, 9)); B = np.zeros((E, 9))
    rc = getattr(lib(), "oracle_edge_eval_" + _sfx(precision))(*g.args(), e, A, B)
    if rc:
        raise RuntimeError("oracle_edge_eval rc=%d" % rc)
    return e, A, B


def linearize(g, python_mode=False, precision="f64", want_H=True):
    n = g.n_unknowns
    H = np.zeros((n, n)) if want_H else None
    b = np.zeros(n); err = np.zeros(1); idx = np.zeros(len(g.v_id), np.int32)
    rc = getattr(lib(), "oracle_linearize_" + _sfx(precision))(
        *g.args(), int(python_mode), H.ctypes.data if want_H else None, b, err, idx)
    if rc < 0:
        raise RuntimeError("oracle_linearize rc=%d" % rc)
    return H, b, float(err[0]), idx


STOP = {0: "cap", 1: "worse", 2: "plateau", 3: "converged", 4: "solver_failed"}


def optimize(g, iterations, mode="cpp", solver="chol", lr=0.2, precision="f64"):
    """Dense `cpu eigen` restatement.  Returns dict(v_pos, chi2, iters, stop, delta_norm)."""
    out = np.zeros_like(g.v_pos); chi2 = np.zeros(max(iterations, 1))
    ir = np.zeros(1, np.int32); sr = np.zeros(1, np.int32); dn = np.zeros(1)
    rc = getattr(lib(), "oracle_optimize_" + _sfx(precision))(
        *g.args(), out, iterations, {"cpp": 0, "python": 1, "cpp_on_python_linearisation": 2}[mode], {"qr": 0, "chol": 1}[solver], lr, chi2, ir, sr, dn)
    if rc:
        raise RuntimeError("oracle_optimize rc=%d" % rc)
    return dict(v_pos=out, chi2=chi2[:ir[0]].copy(), iters=int(ir[0]), stop=STOP[int(sr[0])], delta_norm=float(dn[0]))


def last_phase_seconds():
    """(linearise, dense solve, vertex update) wall seconds of this thread's last optimize() call."""
    out = np.zeros(3)
    lib().oracle_last_phase_seconds(out)
    return out


def solve(H, b, solver="qr"):
    h = np.ascontiguousarray(H, np.float64).copy(); x = np.ascontiguousarray(b, np.float64).copy()
    rc = lib().oracle_solve_f64(h, x, len(x), {"qr": 0, "chol": 1}[solver])
    if rc:
        raise RuntimeError("oracle_solve rc=%d" % rc)
    return x


def update_pose(xyt, d):
    x = np.ascontiguousarray(xyt, np.float64).copy()
    lib().oracle_update_pose_f64(x, np.ascontiguousarray(d, np.float64))
    return x


def _hook(allreduce):
    """Wrap a python callable(np.ndarray) -> None (in-place sum over shards) as the C hook."""
    if allreduce is None:
        return C.cast(None, ALLREDUCE_FN)

    def cb(ptr, n, _ctx):
        allreduce(np.ctypeslib.as_array(ptr, shape=(n,)))
    return ALLREDUCE_FN(cb)


PRECOND = {"jacobi": 0, "amg": 1}


def sparse_step(g, pcg_tol=1e-12, max_cg=100000, rank=0, world=1, allreduce=None, precond="jacobi"):
    """One GN step by the sparse CPU twin (implicit-Schur PCG): dict(delta, chi2, cg_iters)."""
    d = np.zeros((len(g.v_id), 3)); chi = np.zeros(1); it = np.zeros(1, np.int32)
    h = _hook(allreduce)
    rc = lib().oracle_sparse_step(*g.args(), pcg_tol, max_cg, PRECOND[precond], rank, world, h, None, d, chi, it)
    if rc:
        raise RuntimeError("oracle_sparse_step rc=%d" % rc)
    return dict(delta=d, chi2=float(chi[0]), cg_iters=int(it[0]))


def sparse_optimize(g, iterations, pcg_tol=1e-12, max_cg=100000, rank=0, world=1, allreduce=None, precond="jacobi", rules="cpp", lr=0.2):
    """Full GN loop by the sparse CPU twin with the reference's stop rules (rules="python": the loop of the reference's
    in-process Python optimizer instead — lambda * I, step lr)."""
    out = np.zeros_like(g.v_pos); chi2 = np.zeros(max(iterations, 1)); cg = np.zeros(max(iterations, 1), np.int32)
    ir = np.zeros(1, np.int32); sr = np.zeros(1, np.int32); dn = np.zeros(1); tl = np.zeros(1); ts = np.zeros(1)
    h = _hook(allreduce)
    rc = lib().oracle_sparse_optimize(*g.args(), out, iterations, pcg_tol, max_cg, PRECOND[precond], rank, world, h, None, chi2, ir, sr,
                                      cg, dn, tl, ts, {"cpp": 0, "python": 1}[rules], float(lr))
    if rc:
        raise RuntimeError("oracle_sparse_optimize rc=%d" % rc)
    n = int(ir[0])
    return dict(v_pos=out, chi2=chi2[:n].copy(), iters=n, stop=STOP[int(sr[0])], delta_norm=float(dn[0]),
                cg_iters=cg[:n].copy(), seconds_linearize=float(tl[0]), seconds_solve=float(ts[0]))


def schur_dense(g, diag_add=None, with_magnitude=False):
    """The reduced pose system as a dense f64 matrix: S = Hpp - Hpl Hll^-1 Hlp from the dense restatement's H, rows and columns in
    the order of the graph's pose vertices (3 per pose).  Follows set_odom_jacobian like every other entry point.  diag_add: (V, 3, 3)
    blocks added to the vertices' diagonal blocks of H first (the dense restatement knows edge types 0-2: the caller restates priors).
    with_magnitude: also |Hpp| + |Hpl| |Hll^-1| |Hlp|, the size of the terms a product that never forms S sums (>= |S| entry by entry)."""
    H, _b, _err, idx = linearize(g)
    pose = np.where(g.v_type == 0)[0]; lm = np.where(g.v_type == 1)[0]
    if diag_add is not None:
        for v in range(len(g.v_id)):
            m = 3 if g.v_type[v] == 0 else 2
            H[idx[v]:idx[v] + m, idx[v]:idx[v] + m] += diag_add[v][:m, :m]
    ip = (idx[pose][:, None] + np.arange(3)[None, :]).reshape(-1)
    il = (idx[lm][:, None] + np.arange(2)[None, :]).reshape(-1)
    S = H[np.ix_(ip, ip)].copy()
    mag = np.abs(S)
    if len(il):
        Hpl = H[np.ix_(ip, il)]
        Hll = H[np.ix_(il, il)]
        k = np.arange(len(lm))
        blocks = Hll.reshape(len(lm), 2, len(lm), 2)[k, :, k, :]          # landmarks couple to poses only: Hll is block diagonal
        assert np.isclose(np.abs(Hll).sum(), np.abs(blocks).sum(), rtol=1e-12)
        inv = np.linalg.pinv(blocks, hermitian=True)                      # (a landmark without edges has a zero block and adds nothing)
        S -= np.einsum("plx,lxy,qly->pq", Hpl.reshape(len(ip), len(lm), 2), inv, Hpl.reshape(len(ip), len(lm), 2), optimize=True)
        a = np.abs(Hpl).reshape(len(ip), len(lm), 2)
        mag += np.einsum("plx,lxy,qly->pq", a, np.abs(inv), a, optimize=True)
    S = 0.5 * (S + S.T)
    return (S, 0.5 * (mag + mag.T)) if with_magnitude else S


PERTURBATIONS = ("omega", "nu", "transpose")


def twin_precond(g, R, precond="amg", lanes_per_pose=0, lanes_per_lm=0, perturb=None, transpose_pose=0):
    """The sparse twin's preconditioner on the columns of R (3 P rows in the order of the graph's pose vertices), f64 throughout:
    level-0 pre-smoothing, the cycle of the coarse levels, prolongation and level-0 post-smoothing ("amg"), or the inverse diagonal
    blocks of S ("jacobi").  The hierarchy is the one host/amg.h builds under the process's TSGO_AGG* / TSGO_SWEEPS_LIST variables and
    the given layout options; set_cycle_level0 and set_odom_jacobian apply.  perturb: None, or one deliberate defect — "omega" (the
    smoother damping of every level times 1.05), "nu" (one more sweep per side on the coarse levels), "transpose" (the self block of
    the level-0 prolongator row of pose `transpose_pose` transposed).
    Returns (Z, info): info = dict(rows=[block rows per level, the dense one last], checksum, omega=[damping per level],
    sweeping_levels=coarse levels that run sweeps, agg_min / agg_max=the smallest / largest level-0 aggregate,
    agg_extremes=a pose of each, agg=the level-0 aggregate of every pose)."""
    R = np.asarray(R, np.float64)
    cols = np.ascontiguousarray(R.reshape(R.shape[0], -1).T)
    Z = np.zeros_like(cols)
    info = np.zeros(14, np.int64); ck = C.c_uint64(); om = np.zeros(8); agg = np.zeros(max(R.shape[0] // 3, 1), np.int32)
    L = lib()
    L.oracle_twin_perturb(*{None: (1.0, 0, -1), "omega": (1.05, 0, -1), "nu": (1.0, 1, -1), "transpose": (1.0, 0, int(transpose_pose))}[perturb])
    try:
        rc = L.oracle_twin_precond(*g.args(), PRECOND[precond], int(lanes_per_pose), int(lanes_per_lm), cols.shape[0], cols, Z,
                                   info.ctypes.data, C.addressof(ck), om, agg)
    finally:
        L.oracle_twin_perturb(1.0, 0, -1)
    if rc:
        raise RuntimeError("oracle_twin_precond rc=%d" % rc)
    n = int(info[0])
    return np.ascontiguousarray(Z.T).reshape(R.shape), dict(rows=[int(v) for v in info[1:1 + n]], checksum=int(ck.value), omega=om[:max(n - 1, 0)].copy(),
                                                           sweeping_levels=int(info[9]), agg_max=int(info[10]), agg_min=int(info[13]), agg_extremes=(int(info[11]), int(info[12])), agg=agg)
