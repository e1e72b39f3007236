"""Python host side of the device optimizer.

HipOptimizer wraps the C ABI one-to-one.  GraphOptimizer mirrors the reference's in-process
python/optimizer/graph_optimizer.py:11-92 (`GraphOptimizer(graph).optimize(iterations)`) but runs the
`cpu eigen` rules of remote/optimizer/OptimizerCpu.h:25-183 on the GPU.
"""
import ctypes as C

import numpy as np

from . import _lib
from .graph import GraphArrays

STOP = {0: "cap", 1: "worse", 2: "plateau", 3: "converged", 4: "solver_failed", 5: "damping", 6: "radius"}


class HipOptimizer:
    def __init__(self, device=0, precision=64, pcg_rel_tol=1e-10, pcg_max_iters=20000, lanes_per_pose=0,
                 lanes_per_lm=0, use_graphs="auto", rank=0, world=1, preconditioner="amg", xcd_map=None, warm_start=None,
                 reuse_structure=None, rules="cpp", lr=0.2, odom_jacobian="constant", cycle_level0="implicit", cycle_storage=16, warm_requests=False, lm_lambda0=None, lm_chi2_rel_tol=None,
                 dl_radius0=None, dl_radius_min=None, dl_radius_max=None, dl_chi2_rel_tol=None, testing=False):
        # testing=True: libtsgo_hip_testing.so (the same sources with -DTSGO_TESTING: hooks, research variables, in-process group)
        # (TSGO_PY_TESTING_LIB=1: research scripts under tools/research and tests/research that set hook / research variables pick the
        # testing library without being edited; it selects which LIBRARY this Python wrapper loads, the product library reads nothing)
        import os
        self.lib = _lib.hip_testing_lib() if (testing or os.environ.get("TSGO_PY_TESTING_LIB") == "1") else _lib.hip_lib()
        cfg = _lib.tsgo_config()
        self.lib.tsgo_default_config(C.byref(cfg))
        cfg.device, cfg.precision, cfg.pcg_rel_tol, cfg.pcg_max_iters = device, precision, pcg_rel_tol, pcg_max_iters
        cfg.lanes_per_pose, cfg.lanes_per_lm, cfg.use_graphs = lanes_per_pose, lanes_per_lm, self._use_graphs(use_graphs)
        cfg.rank, cfg.world = rank, world
        cfg.preconditioner = {"jacobi": 0, "amg": 1}[preconditioner]
        if xcd_map is not None:
            cfg.xcd_map = int(xcd_map)
        if warm_start is not None:
            cfg.warm_start = int(warm_start)
        if reuse_structure is not None:
            cfg.reuse_structure = int(reuse_structure)
        cfg.rules, cfg.lr = {"cpp": 0, "python": 1, "lm": 2, "dogleg": 3}[rules], float(lr)
        # rules="lm": Levenberg-Marquardt with step acceptance (tsgo_config.rules = 2); meant for odom_jacobian="analytic"
        if lm_lambda0 is not None:
            cfg.lm_lambda0 = float(lm_lambda0)
        if lm_chi2_rel_tol is not None:
            cfg.lm_chi2_rel_tol = float(lm_chi2_rel_tol)
        cfg.odom_jacobian = {"constant": 0, "analytic": 1}[odom_jacobian]
        cfg.cycle_level0 = {"implicit": 0, "explicit": 1}[cycle_level0]
        cfg.cycle_storage = {16: 16, 32: 32}[cycle_storage]
        cfg.warm_requests = 1 if warm_requests else 0
        self.cfg = cfg
        self.h = C.c_void_p()
        _lib.check(self.lib, self.lib.tsgo_create(C.byref(cfg), C.byref(self.h)), "tsgo_create")
        # rules="dogleg": Powell's dogleg trust-region loop (tsgo_config.rules = 3); its parameters go through tsgo_set_dogleg
        if any(v is not None for v in (dl_radius0, dl_radius_min, dl_radius_max, dl_chi2_rel_tol)):
            try:
                self.set_dogleg(radius0=dl_radius0, radius_min=dl_radius_min, radius_max=dl_radius_max, chi2_rel_tol=dl_chi2_rel_tol)
            except Exception:
                self.close()
                raise
        self.n_vertices = 0
        self.n_edges = 0
        self._v_in = None
        self._ids_types = None

    @staticmethod
    def _use_graphs(v):
        """tsgo_config.use_graphs: "auto" / 2 (eager while the host keeps ahead), True / 1 (replay), False / 0 (eager)."""
        if v == "auto":
            return 2
        if isinstance(v, bool):
            return int(v)
        if v in (0, 1, 2):
            return int(v)
        raise ValueError("use_graphs must be 'auto', True, False, 0, 1 or 2")

    def close(self):
        if self.h:
            self.lib.tsgo_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_graph(self, g: GraphArrays):
        cg = g.c_struct()
        _lib.check(self.lib, self.lib.tsgo_set_graph(self.h, C.byref(cg)), "tsgo_set_graph")
        self.n_vertices = len(g.v_id)
        self.n_edges = len(g.e_type)
        self._ids_types = (g.v_id, g.v_type)      # joint_marginals: the row count of each queried id
        self._v_in = g.v_pos.copy() if self.cfg.world > 1 else None    # a shard returns its own landmarks; the others keep their input

    def reset_history(self):
        """warm_requests: the next set_graph starts the solver from nothing (a pooled handle changing hands)."""
        self.lib.tsgo_reset_history(self.h)

    def set_robust(self, odom=None, lm=None, virtual=None, pose_prior=None, lm_prior=None, all=None):
        """Robust kernel per edge class (tsgo_set_robust): each value "none" or (name, delta), name one of "huber", "cauchy",
        "geman_mcclure"; `all` sets every class, a class argument overrides it, a class left out keeps what the handle has.  Takes effect
        at the next linearisation and survives set_graph."""
        r = _lib.tsgo_robust()
        _lib.check(self.lib, self.lib.tsgo_get_robust(self.h, C.byref(r)), "tsgo_get_robust")
        for k, v in enumerate((odom, lm, virtual, pose_prior, lm_prior)):
            v = all if v is None else v
            if v is None:
                continue
            name, delta = (v, r.delta[k]) if isinstance(v, str) else v
            if name not in _lib.ROBUST_KERNELS or (isinstance(v, str) and name != "none"):
                raise ValueError('a robust kernel is "none" or (name, delta) with name in %s' % sorted(_lib.ROBUST_KERNELS))
            r.kernel[k], r.delta[k] = _lib.ROBUST_KERNELS[name], float(delta)
        _lib.check(self.lib, self.lib.tsgo_set_robust(self.h, C.byref(r)), "tsgo_set_robust")

    @property
    def robust(self):
        """The handle's setting read back (tsgo_get_robust): {class: "none" or (name, delta)}."""
        r = _lib.tsgo_robust()
        _lib.check(self.lib, self.lib.tsgo_get_robust(self.h, C.byref(r)), "tsgo_get_robust")
        names = {v: k for k, v in _lib.ROBUST_KERNELS.items()}
        return {c: "none" if r.kernel[k] == 0 else (names[r.kernel[k]], r.delta[k]) for k, c in enumerate(_lib.ROBUST_CLASSES)}

    def set_edge_robust(self, kernels, entry_of_edge):
        """Robust kernels per EDGE (tsgo_set_edge_robust): `kernels` a palette of at most 15 entries, each "none" or (name, delta) as in
        set_robust; entry_of_edge one integer per edge of the graph given to set_graph, in its order: 0 leaves the edge to its class's
        kernel (set_robust), k >= 1 gives it kernels[k - 1] whatever its class.  An all-zero entry_of_edge is the same as
        clear_edge_robust().  Survives set_robust, set_edge_information, init_estimates, gnc and optimize; the next set_graph drops it.
        Returns the call's stats: edges_by_entry, overridden_by_class ({class: count}), active, ms_total."""
        kernels = list(kernels)
        ent = (_lib.tsgo_edge_robust_entry * max(1, len(kernels)))()
        for k, v in enumerate(kernels):
            name, delta = (v, 0.0) if isinstance(v, str) else v
            if name not in _lib.ROBUST_KERNELS or (isinstance(v, str) and name != "none"):
                raise ValueError('a robust kernel is "none" or (name, delta) with name in %s' % sorted(_lib.ROBUST_KERNELS))
            ent[k].kernel, ent[k].delta = _lib.ROBUST_KERNELS[name], float(delta)
        of = np.asarray(entry_of_edge)
        if of.size and (of.min() < 0 or of.max() > 255):
            raise ValueError("entry_of_edge values must be within [0, 255]")
        of = np.ascontiguousarray(of.reshape(-1), dtype=np.uint8)
        return self._set_edge_robust(len(kernels), ent if kernels else None, of.ctypes.data if len(of) else None, len(of))

    def _set_edge_robust(self, n_entries, entries, mask, n_mask):
        st = _lib.tsgo_edge_robust_stats()
        _lib.check(self.lib, self.lib.tsgo_set_edge_robust(self.h, n_entries, entries, mask, n_mask, C.byref(st)), "tsgo_set_edge_robust")
        return dict(edges_by_entry=np.array(st.edges_by_entry[:], dtype=np.int64),
                    overridden_by_class={c: st.overridden_by_class[k] for k, c in enumerate(_lib.ROBUST_CLASSES)}, active=bool(st.active), ms_total=st.ms_total)

    def exempt_edges(self, edges):
        """The listed edges (indices into the edge arrays, or a boolean mask over them) take no robust kernel at all — rho = s and w = 1
        exactly, e.g. the odometry chain — and every other edge keeps its class's: set_edge_robust with one "none" entry."""
        of = np.zeros(self.n_edges, dtype=np.uint8)
        of[np.asarray(edges)] = 1
        return self.set_edge_robust(["none"], of)

    def clear_edge_robust(self):
        """Back to the class kernels alone: the handle then runs exactly what it ran before set_edge_robust."""
        return self._set_edge_robust(0, None, None, 0)

    @property
    def edge_robust(self):
        """The per-edge setting read back (tsgo_get_edge_robust): (kernels, entry_of_edge) as set_edge_robust takes them; ([], zeros) when
        none is active."""
        n = C.c_int32()
        ent = (_lib.tsgo_edge_robust_entry * _lib.TSGO_EDGE_ROBUST_MAX)()
        of = np.zeros(self.n_edges, dtype=np.uint8)
        _lib.check(self.lib, self.lib.tsgo_get_edge_robust(self.h, C.byref(n), ent, of.ctypes.data if self.n_edges else None, self.n_edges), "tsgo_get_edge_robust")
        names = {v: k for k, v in _lib.ROBUST_KERNELS.items()}
        return ["none" if ent[k].kernel == 0 else (names[ent[k].kernel], ent[k].delta) for k in range(n.value)], of

    def set_dogleg(self, radius0=None, radius_min=None, radius_max=None, chi2_rel_tol=None):
        """Parameters of the dogleg loop (tsgo_set_dogleg; read by rules="dogleg" only): an argument left out keeps what the handle has.
        They belong to the handle and survive set_graph; every optimize call starts at radius0."""
        p = _lib.tsgo_dogleg_params()
        _lib.check(self.lib, self.lib.tsgo_get_dogleg(self.h, C.byref(p)), "tsgo_get_dogleg")
        for k, v in (("radius0", radius0), ("radius_min", radius_min), ("radius_max", radius_max), ("chi2_rel_tol", chi2_rel_tol)):
            if v is not None:
                setattr(p, k, float(v))
        _lib.check(self.lib, self.lib.tsgo_set_dogleg(self.h, C.byref(p)), "tsgo_set_dogleg")

    @property
    def dogleg(self):
        """The handle's dogleg parameters read back (tsgo_get_dogleg) as a dict."""
        p = _lib.tsgo_dogleg_params()
        _lib.check(self.lib, self.lib.tsgo_get_dogleg(self.h, C.byref(p)), "tsgo_get_dogleg")
        return {f: getattr(p, f) for f, _t in p._fields_}

    def dogleg_trace(self, n=None):
        """tsgo_get_dogleg_trace of the handle's last optimize as a dict: trials, solves, radius_last and the per-trial arrays kind, solved,
        radius, step_norm, gg, gHg, gd, dd (the first n entries; default min(trials, TSGO_MAX_TRACE)).  All zero after a run under other rules."""
        tr = _lib.tsgo_dogleg_trace()
        _lib.check(self.lib, self.lib.tsgo_get_dogleg_trace(self.h, C.byref(tr)), "tsgo_get_dogleg_trace")
        n = min(tr.trials, _lib.TSGO_MAX_TRACE) if n is None else n
        out = dict(trials=tr.trials, solves=tr.solves, radius_last=tr.radius_last)
        for k in ("kind", "solved"):
            out[k] = np.array(getattr(tr, k)[:n], dtype=np.int64)
        for k in ("radius", "step_norm", "gg", "gHg", "gd", "dd"):
            out[k] = np.array(getattr(tr, k)[:n])
        return out

    def optimize(self, iterations):
        st = _lib.tsgo_stats()
        _lib.check(self.lib, self.lib.tsgo_optimize(self.h, iterations, C.byref(st)), "tsgo_optimize")
        n = st.trace_len
        tr = self.dogleg_trace(n)
        return dict(# rules="dogleg": the per-trial trace of tsgo_get_dogleg_trace (zeros under the other rules) and the linearise + solve pairs run
                    dl_kind=tr["kind"], dl_solved=tr["solved"], dl_radius=tr["radius"], dl_step_norm=tr["step_norm"], dl_gg=tr["gg"], dl_gHg=tr["gHg"],
                    dl_gd=tr["gd"], dl_dd=tr["dd"], solves=tr["solves"], dl_radius_last=tr["radius_last"],
iters=st.iterations_run, stop=STOP[st.stop_reason], chi2=np.array(st.chi2[:n]), chi2_last=st.chi2_last,
                    cg_iters=np.array(st.pcg_iters[:n]), delta_norm=st.last_delta_norm, ms_total=st.ms_total,
                    ms_linearize=st.ms_linearize, ms_solve=st.ms_solve, ms_update=st.ms_update, ms_setup=st.ms_setup, structure_reused=bool(st.structure_reused), lambda_last=st.lambda_last,
                    n_pose=st.n_pose, n_lm=st.n_lm, n_odom_edges=st.n_odom_edges, n_lm_edges=st.n_lm_edges,
                    cg_total=st.pcg_iters_total, fallbacks=st.pcg_fallbacks, cycle_storage_now=st.cycle_storage_now, history_carried=st.history_carried, graph_replay=bool(st.graph_replay),
                    # rules="lm": per-trial traces (zeros under the other rules); trial k was accepted when lm_gain[k] > 0 and lm_pred[k] > 0
                    rejected=st.steps_rejected, lm_lambda=np.array(st.lm_lambda[:n]), lm_gain=np.array(st.lm_gain[:n]), lm_pred=np.array(st.lm_pred[:n]),
                    lm_chi2_trial=np.array(st.lm_chi2_trial[:n]))

    def vertices(self):
        out = np.zeros((self.n_vertices, 3)) if self._v_in is None else np.ascontiguousarray(self._v_in.copy())
        _lib.check(self.lib, self.lib.tsgo_get_vertices(self.h, out.ctypes.data), "tsgo_get_vertices")
        return out

    def linearize(self):
        diag = np.zeros((self.n_vertices, 9)); grad = np.zeros((self.n_vertices, 3)); chi = C.c_double()
        _lib.check(self.lib, self.lib.tsgo_linearize(self.h, diag.ctypes.data, grad.ctypes.data, C.byref(chi)),
                   "tsgo_linearize")
        return diag, grad, chi.value

    def solve_step(self, allow_unconverged=False):
        """One linearisation and one solve (tsgo_solve_step): dict(delta, chi2, cg_iters, rc).  allow_unconverged=True: a solve that
        stopped at pcg_max_iters (-22) does not raise; delta is then the iterate after cg_iters = pcg_max_iters updates and rc is -22."""
        d = np.zeros((self.n_vertices, 3)); chi = C.c_double(); it = C.c_int32()
        rc = self.lib.tsgo_solve_step(self.h, d.ctypes.data, C.byref(chi), C.byref(it))
        if not (allow_unconverged and rc == -22):
            _lib.check(self.lib, rc, "tsgo_solve_step")
        return dict(delta=d, chi2=chi.value, cg_iters=it.value, rc=rc)

    def marginals(self, ids, rel_tol=0.0):
        """Marginal covariances (diagonal blocks of H^-1 at the current estimates) of the vertices `ids`, in order: cov[k] is the 3x3
        block of a pose, or the 2x2 block of a landmark in cov[k, :2, :2] (zeros elsewhere).  rel_tol <= 0: the handle's pcg_rel_tol."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).reshape(-1))
        cov = np.zeros((len(ids), 3, 3))
        st = _lib.tsgo_marginal_stats()
        _lib.check(self.lib, self.lib.tsgo_marginals(self.h, ids.ctypes.data if len(ids) else None, len(ids), float(rel_tol),
                                                      cov.ctypes.data, C.byref(st)), "tsgo_marginals")
        return cov, {f: getattr(st, f) for f, _t in st._fields_}

    def joint_marginals(self, ids, rel_tol=0.0):
        """Joint marginal covariance of the vertices `ids` (the block of H^-1 over them, cross blocks included): cov (D, D), rows and
        columns in query order, 3 per pose and 2 per landmark; offsets (len(ids) + 1,): the rows of ids[k] are offsets[k]:offsets[k + 1].
        rel_tol <= 0: the handle's pcg_rel_tol."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).reshape(-1))
        idp = ids.ctypes.data if len(ids) else None
        dim = C.c_int32()
        _lib.check(self.lib, self.lib.tsgo_joint_marginals(self.h, idp, len(ids), float(rel_tol), None, 0, C.byref(dim), None),
                   "tsgo_joint_marginals")
        D = dim.value
        v_id, v_type = self._ids_types
        order = np.argsort(v_id, kind="stable")
        dims = np.where(v_type[order[np.searchsorted(v_id, ids, sorter=order)]] == 0, 3, 2) if len(ids) else np.zeros(0, np.int64)
        offsets = np.concatenate([[0], np.cumsum(dims)]).astype(np.int64)
        assert offsets[-1] == D, (offsets[-1], D)
        cov = np.zeros((D, D))
        st = _lib.tsgo_marginal_stats()
        _lib.check(self.lib, self.lib.tsgo_joint_marginals(self.h, idp, len(ids), float(rel_tol), cov.ctypes.data if D else None, D * D,
                                                            C.byref(dim), C.byref(st)), "tsgo_joint_marginals")
        return cov, offsets, {f: getattr(st, f) for f, _t in st._fields_}

    def sample_marginals(self, n_samples, seed=0, rel_tol=0.0, samples=False):
        """Posterior samples by perturb-and-MAP and the marginal covariance of EVERY vertex from their second moments
        (tsgo_sample_marginals): dict(cov (V, 3, 3) in the vertex order of the graph given to set_graph, a landmark's block in
        cov[v, :2, :2]; samples (K, V, 3) with samples=True, else None; stats).  A variance has relative standard error sqrt(2 / K).
        rel_tol <= 0: the handle's pcg_rel_tol."""
        K, V = int(n_samples), self.n_vertices
        cov = np.zeros((V, 3, 3))
        smp = np.zeros((K, V, 3)) if samples and 1 <= K <= 65536 else None      # (outside that range the call refuses before it looks at samples_out)
        st = _lib.tsgo_sample_stats()
        _lib.check(self.lib, self.lib.tsgo_sample_marginals(self.h, K, int(seed) & 0xFFFFFFFFFFFFFFFF, float(rel_tol), cov.ctypes.data, V,
                                                             smp.ctypes.data if smp is not None else None, smp.size if smp is not None else 0,
                                                             C.byref(st)), "tsgo_sample_marginals")
        stats = {f: getattr(st, f) for f, _t in st._fields_ if f not in ("solve", "reserved")}
        stats["solve"] = {f: getattr(st.solve, f) for f, _t in st.solve._fields_}
        return dict(cov=cov, samples=smp, stats=stats)

    def edge_leverage(self, n_samples, seed=0, rel_tol=0.0):
        """Leverage of every edge from posterior samples (tsgo_edge_leverage), in the edge order of the graph given to set_graph:
        dict(cov (E, 3, 3) symmetric, C = J Sigma J^T of the predicted measurement (the dof-2 classes in cov[e, :2, :2]); h (E,) =
        tr(Omega_a C); dof (E,) the number of weighted axes; redundancy = dof - h (not clamped: sampling noise may take it just below
        0); all, the (E, 8) records (c00, c01, c02, c11, c12, c22, h, dof_a); stats).  The samples are those of sample_marginals for the
        same (n_samples, seed); a diagonal entry of C has relative standard error sqrt(2 / K).  rel_tol <= 0: the handle's pcg_rel_tol."""
        K, E = int(n_samples), self.n_edges
        arr = np.zeros((max(E, 1), 8))
        st = _lib.tsgo_leverage_stats()
        _lib.check(self.lib, self.lib.tsgo_edge_leverage(self.h, K, int(seed) & 0xFFFFFFFFFFFFFFFF, float(rel_tol), arr.ctypes.data, E, C.byref(st)),
                   "tsgo_edge_leverage")
        arr = arr[:E]
        cov = np.zeros((E, 3, 3))
        for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            cov[:, a, b] = arr[:, k]; cov[:, b, a] = arr[:, k]
        stats = {f: getattr(st, f) for f, _t in st._fields_ if f not in ("solve", "reserved", "edges", "h_sum", "dof_sum")}
        for f in ("edges", "h_sum", "dof_sum"):
            stats[f] = np.array(getattr(st, f))
        stats["solve"] = {f: getattr(st.solve, f) for f, _t in st.solve._fields_}
        return dict(cov=cov, h=arr[:, 6], dof=arr[:, 7], redundancy=arr[:, 7] - arr[:, 6], all=arr, stats=stats)

    def edge_report(self, records=True):
        """Per-edge residual report at the current estimates under the handle's robust setting (tsgo_edge_report): (rec, summary).
        rec: dict of views over one (E, 6) array in the edge order of the graph given to set_graph — e (E, 3), s, rho, w (E,) — and the
        array itself as rec["all"]; None with records=False (summary only: no per-edge buffer on the device, nothing copied back).
        summary: {class: dict(edges, downweighted, s_sum, rho_sum, s_max, s_max_edge)} over _lib.ROBUST_CLASSES, plus "chi2"."""
        st = _lib.tsgo_edge_report_stats()
        rec = None
        if records:
            arr = np.zeros((self.n_edges, 6))
            _lib.check(self.lib, self.lib.tsgo_edge_report(self.h, arr.ctypes.data, self.n_edges, C.byref(st)), "tsgo_edge_report")
            rec = dict(e=arr[:, 0:3], s=arr[:, 3], rho=arr[:, 4], w=arr[:, 5], all=arr)
        else:
            _lib.check(self.lib, self.lib.tsgo_edge_report(self.h, None, 0, C.byref(st)), "tsgo_edge_report")
        summary = {c: {f: getattr(st.cls[k], f) for f, _t in _lib.tsgo_edge_class_summary._fields_} for k, c in enumerate(_lib.ROBUST_CLASSES)}
        summary["chi2"] = st.chi2
        return rec, summary

    def gate_edges(self, e_type, e_ids=None, e_meas=None, e_inf=None, rel_tol=0.0, innovation=False):
        """Mahalanobis gate of candidate edges against the joint marginal of their vertices (tsgo_gate_edges).  The candidates come as
        the four edge arrays of a graph (e_type (K,), e_ids (K, 2), e_meas (K, 9), e_inf (K, 3)), or as one object that has them as
        attributes (a GraphArrays whose edges are the candidates); they are not added to the graph.  Returns (res, stats): res a dict of
        arrays in candidate order — e (K, 3), s, d2, logdet (K,), dof, status (K,) integers, with innovation=True also innov (K, 3, 3),
        S in the leading dof x dof — and stats a dict of tsgo_gate_stats (its `solve` a dict of tsgo_marginal_stats).  Accept a
        candidate when d2 is below the chi^2 quantile of its dof (99 %: 11.345 for 3, 9.210 for 2).  rel_tol <= 0: the handle's
        pcg_rel_tol."""
        if e_ids is None:
            e_type, e_ids, e_meas, e_inf = e_type.e_type, e_type.e_ids, e_type.e_meas, e_type.e_inf
        e_type = np.ascontiguousarray(np.asarray(e_type, dtype=np.uint32).reshape(-1))
        K = len(e_type)
        e_ids = np.ascontiguousarray(np.asarray(e_ids, dtype=np.uint32).reshape(K, 2))
        e_meas = np.ascontiguousarray(np.asarray(e_meas, dtype=np.float64).reshape(K, 9))
        e_inf = np.ascontiguousarray(np.asarray(e_inf, dtype=np.float64).reshape(K, 3))
        rec = np.zeros((K, 8))
        innov = np.zeros((K, 3, 3)) if innovation else None
        st = _lib.tsgo_gate_stats()
        ptr = (lambda a: a.ctypes.data) if K else (lambda a: None)
        _lib.check(self.lib, self.lib.tsgo_gate_edges(self.h, K, ptr(e_type), ptr(e_ids), ptr(e_meas), ptr(e_inf), float(rel_tol), ptr(rec),
                                                       innov.ctypes.data if innovation and K else None, C.byref(st)), "tsgo_gate_edges")
        res = dict(e=rec[:, 0:3], s=rec[:, 3], d2=rec[:, 4], dof=rec[:, 5].astype(np.int64), logdet=rec[:, 6], status=rec[:, 7].astype(np.int64))
        if innovation:
            res["innov"] = innov
        stats = {f: getattr(st, f) for f, _t in st._fields_ if f not in ("solve", "reserved")}
        stats["solve"] = {f: getattr(st.solve, f) for f, _t in st.solve._fields_}
        return res, stats

    def init_estimates(self, mask=None, poses=True, landmarks=True):
        """Initial estimates from an odometry spanning tree (tsgo_init_estimates): poses composed along the tree from its roots (the
        fixed poses; a component without one keeps its lowest-index pose), then landmarks as the mean of their observations.  mask: one
        entry per edge of the graph, nonzero = this ODOM edge may enter the tree (entries of other edges are ignored); None = every ODOM
        edge.  Returns tsgo_init_stats as a dict.  The estimates change; the solver restarts as after a set_graph that refills values."""
        what = (_lib.INIT_POSES if poses else 0) | (_lib.INIT_LANDMARKS if landmarks else 0)
        if what == 0:
            raise ValueError("init_estimates: poses and landmarks are both False")
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        st = _lib.tsgo_init_stats()
        _lib.check(self.lib, self.lib.tsgo_init_estimates(self.h, what, None if m is None else m.ctypes.data, 0 if m is None else len(m), C.byref(st)),
                   "tsgo_init_estimates")
        return {f: getattr(st, f) for f, _t in st._fields_}

    def set_edge_information(self, e_inf, edges=None):
        """Replace the information diagonal of edges of the graph the handle holds, in place on the device (tsgo_set_edge_information).
        edges: integer positions in the edge arrays of the graph given to set_graph (the numbering of edge_report), e_inf (n, 3) in the
        same order; edges=None: e_inf is (n_edges, 3), every edge in order.  The estimates, the robust setting and the solver's history
        stay; the next set_graph replaces every weight with what it carries.  Returns tsgo_edge_info_stats as a dict."""
        e_inf = np.ascontiguousarray(np.asarray(e_inf, dtype=np.float64).reshape(-1, 3))
        n = len(e_inf)
        idx = None
        if edges is not None:
            idx = np.ascontiguousarray(np.asarray(edges).reshape(-1).astype(np.int64))
            if len(idx) != n:
                raise ValueError("set_edge_information: %d edges listed but e_inf has %d rows" % (len(idx), n))
        st = _lib.tsgo_edge_info_stats()
        _lib.check(self.lib, self.lib.tsgo_set_edge_information(self.h, n, idx.ctypes.data if idx is not None and n else None,
                                                                 e_inf.ctypes.data if n else None, C.byref(st)), "tsgo_set_edge_information")
        out = {f: getattr(st, f) for f, _t in st._fields_ if f != "reserved"}
        out["edges_by_class"] = {c: st.edges_by_class[k] for k, c in enumerate(_lib.ROBUST_CLASSES)}
        return out

    def disable_edges(self, edges):
        """Switch edges off: information 0, where an edge contributes exactly nothing (set_edge_information with zeros)."""
        idx = np.asarray(edges).reshape(-1)
        return self.set_edge_information(np.zeros((len(idx), 3)), idx)

    def edge_information(self):
        """The information diagonals the handle holds now (tsgo_get_edge_information): (n_edges, 3) in input edge order, widened from the
        handle's precision; an entry the edge's type does not use is 0."""
        out = np.zeros((self.n_edges, 3))
        _lib.check(self.lib, self.lib.tsgo_get_edge_information(self.h, out.ctypes.data if self.n_edges else None, self.n_edges), "tsgo_get_edge_information")
        return out

    def set_fixed(self, ids, count=1):
        """Which vertices are fixed, edited in place on the device (tsgo_set_fixed).  ids: vertex ids of the graph the handle holds;
        count: one integer, or one per id: the multiplicity of the id in the fixed list, 0 releases it.  Unlisted vertices keep theirs.
        The estimates, every weight edit, the robust settings and the solver's history stay; the next set_graph installs the list it
        carries.  Moving the anchor: release(old) and set_fixed(new) — or one call, set_fixed([old, new], [0, 1]).  Returns
        tsgo_vertex_edit_stats as a dict."""
        ids = np.ascontiguousarray(np.asarray(ids).reshape(-1).astype(np.uint32))
        cnt = np.full(len(ids), int(count), dtype=np.int64) if np.ndim(count) == 0 else np.asarray(count, dtype=np.int64).reshape(-1)
        if len(cnt) != len(ids):
            raise ValueError("set_fixed: %d ids listed but count has %d entries" % (len(ids), len(cnt)))
        if len(cnt) and (cnt.min() < -2**31 or cnt.max() >= 2**31):
            raise ValueError("set_fixed: a count does not fit 32 bits")
        cnt = np.ascontiguousarray(cnt.astype(np.int32))
        st = _lib.tsgo_vertex_edit_stats()
        n = len(ids)
        _lib.check(self.lib, self.lib.tsgo_set_fixed(self.h, n, ids.ctypes.data if n else None, cnt.ctypes.data if n else None, C.byref(st)), "tsgo_set_fixed")
        return {f: getattr(st, f) for f, _t in st._fields_}

    def release(self, ids):
        """The listed vertices are fixed no longer (set_fixed with count 0)."""
        return self.set_fixed(ids, 0)

    def fixed_counts(self):
        """How often each vertex occurs in the fixed list the handle holds now (tsgo_get_fixed): (n_vertices,) int32 in the vertex order
        of the graph given to set_graph."""
        out = np.zeros(self.n_vertices, dtype=np.int32)
        _lib.check(self.lib, self.lib.tsgo_get_fixed(self.h, out.ctypes.data if self.n_vertices else None, self.n_vertices), "tsgo_get_fixed")
        return out

    def set_vertices(self, pos, ids=None):
        """Replace the estimates of vertices of the graph the handle holds, in place on the device (tsgo_set_estimates).  pos (n, 3):
        (x, y, theta) per listed id, a landmark's third entry is ignored; ids=None: pos is (n_vertices, 3), every vertex in order.  The
        other estimates keep their bits.  Weight edits, the robust settings and a set_fixed stay; the solver restarts as after
        init_estimates.  Returns tsgo_vertex_edit_stats as a dict."""
        pos = np.ascontiguousarray(np.asarray(pos, dtype=np.float64).reshape(-1, 3))
        n = len(pos)
        idp = None
        if ids is not None:
            idp = np.ascontiguousarray(np.asarray(ids).reshape(-1).astype(np.uint32))
            if len(idp) != n:
                raise ValueError("set_vertices: %d ids listed but pos has %d rows" % (len(idp), n))
        st = _lib.tsgo_vertex_edit_stats()
        _lib.check(self.lib, self.lib.tsgo_set_estimates(self.h, n, idp.ctypes.data if idp is not None else None, pos.ctypes.data if n else None,
                                                          C.byref(st)), "tsgo_set_estimates")
        return {f: getattr(st, f) for f, _t in st._fields_}

    def gnc(self, barc2=None, subject=None, mu_step=None, rounds_max=None, inner_iterations=None, keep_weights=True, weights=True):
        """Graduated non-convexity with the truncated-least-squares surrogate (tsgo_gnc): rounds of on-device reweighting, each followed
        by optimize(inner_iterations) under the handle's own rules and robust setting (textbook GNC: set_robust(all="none") first).
        barc2: the inlier threshold on s per class, a dict over _lib.ROBUST_CLASSES (classes left out keep the default, the 99 % chi^2
        quantile; a value <= 0 exempts the class) or a sequence of five.  subject: one entry per edge, nonzero = the edge may be
        down-weighted; None = every edge of a class with barc2 > 0.  Edges that are not subject are known inliers: weight 1, never
        written.  keep_weights=False restores the information the handle held before the call, bit for bit.  Returns a dict: w (n_edges,)
        the last round's weights (None with weights=False: nothing but a few partials per round is copied back), rounds, stop, q_max,
        the per-round traces mu, cost, chi2_inner, inner_iters, inner_stop, n_zero, n_one, n_between, and subject_by_class,
        cg_total, ms_total, ms_reweight, ms_inner."""
        p = _lib.tsgo_gnc_params()
        self.lib.tsgo_default_gnc(C.byref(p))
        if isinstance(barc2, dict):
            for k, c in enumerate(_lib.ROBUST_CLASSES):
                if c in barc2:
                    p.barc2[k] = float(barc2[c])
            if set(barc2) - set(_lib.ROBUST_CLASSES):
                raise ValueError("gnc: barc2 has unknown classes %s" % sorted(set(barc2) - set(_lib.ROBUST_CLASSES)))
        elif barc2 is not None:
            vals = [float(v) for v in barc2]
            if len(vals) != 5:
                raise ValueError("gnc: barc2 is a dict over %s or five numbers" % (_lib.ROBUST_CLASSES,))
            for k, v in enumerate(vals):
                p.barc2[k] = v
        if mu_step is not None:
            p.mu_step = float(mu_step)
        if rounds_max is not None:
            p.rounds_max = int(rounds_max)
        if inner_iterations is not None:
            p.inner_iterations = int(inner_iterations)
        p.keep_weights = 1 if keep_weights else 0
        m = None if subject is None else np.ascontiguousarray(np.asarray(subject).reshape(-1) != 0, dtype=np.uint8)
        w = np.ones(self.n_edges) if weights else None
        st = _lib.tsgo_gnc_stats()
        _lib.check(self.lib, self.lib.tsgo_gnc(self.h, C.byref(p), None if m is None else m.ctypes.data, 0 if m is None else len(m),
                                               w.ctypes.data if weights and self.n_edges else None, self.n_edges, C.byref(st)), "tsgo_gnc")
        n = st.rounds
        return dict(w=w, rounds=n, stop=_lib.GNC_STOP[st.stop_reason], q_max=st.q_max, mu=np.array(st.mu[:n]), cost=np.array(st.cost[:n]),
                    chi2_inner=np.array(st.chi2_inner[:n]), inner_iters=np.array(st.inner_iterations_run[:n], dtype=np.int64),
                    inner_stop=[STOP[k] for k in st.inner_stop[:n]], n_zero=np.array(st.n_zero[:n], dtype=np.int64),
                    n_one=np.array(st.n_one[:n], dtype=np.int64), n_between=np.array(st.n_between[:n], dtype=np.int64),
                    subject_by_class={c: st.subject_by_class[k] for k, c in enumerate(_lib.ROBUST_CLASSES)}, cg_total=st.pcg_iters_total,
                    ms_total=st.ms_total, ms_reweight=st.ms_reweight, ms_inner=st.ms_inner)

    def max_mixture(self, groups, log_weight=None, rounds_max=None, inner_iterations=None, keep_selection=True):
        """Max-mixture edges (tsgo_max_mixture): `groups` is a list of lists of input edge indices, each list the alternatives of one
        measurement (graph.with_null_twins builds the closure-or-nothing case).  Per pass the device evaluates every member's cost
        s - sum ln(information) - 2 log_weight at the current estimates, switches the cheapest member of each group on and the others
        off (information 0), then runs optimize(inner_iterations) under the handle's own rules and robust settings; the loop stops when
        no group changes.  log_weight: shaped like `groups`, one entry per member; None = 0 everywhere.
        keep_selection=False restores the information the handle held before the call, bit for bit.  Returns a dict: rounds, passes,
        stop ("stable", "rounds", "solver"), selected (n_groups,) positions inside the groups, selected_edge (n_groups,) the edges they
        name, cost (one array per group), the per-pass traces n_changed and cost_sum, the per-round traces chi2_inner, inner_iters and
        inner_stop, members_by_class, cg_total, ms_total, ms_select, ms_inner."""
        groups = [np.asarray(g, dtype=np.int64).reshape(-1) for g in groups]
        off = np.zeros(len(groups) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(g) for g in groups])
        member = np.ascontiguousarray(np.concatenate(groups)) if groups else np.zeros(0, np.int64)
        lw = None
        if log_weight is not None:
            flat = [np.asarray(w, dtype=np.float64).reshape(-1) for w in log_weight]
            if [len(w) for w in flat] != [len(g) for g in groups]:
                raise ValueError("max_mixture: log_weight must be shaped like groups (one list per group, one entry per member)")
            lw = np.ascontiguousarray(np.concatenate(flat)) if flat else np.zeros(0)
        p = _lib.tsgo_mixture_params()
        self.lib.tsgo_default_mixture(C.byref(p))
        if rounds_max is not None:
            p.rounds_max = int(rounds_max)
        if inner_iterations is not None:
            p.inner_iterations = int(inner_iterations)
        p.keep_selection = 1 if keep_selection else 0
        sel = np.zeros(len(groups), dtype=np.int32)
        cost = np.zeros(len(member))
        st = _lib.tsgo_mixture_stats()
        _lib.check(self.lib, self.lib.tsgo_max_mixture(self.h, C.byref(p), len(groups), off.ctypes.data, member.ctypes.data if len(member) else None,
                                                       None if lw is None else lw.ctypes.data, sel.ctypes.data if len(sel) else None, len(sel),
                                                       cost.ctypes.data if len(cost) else None, len(cost), C.byref(st)), "tsgo_max_mixture")
        n, k = st.rounds, st.passes
        return dict(rounds=n, passes=k, stop=_lib.MIX_STOP[st.stop_reason], selected=sel,
                    selected_edge=np.array([g[s] for g, s in zip(groups, sel)], dtype=np.int64), cost=[cost[a:b] for a, b in zip(off[:-1], off[1:])],
                    n_changed=np.array(st.n_changed[:k], dtype=np.int64), cost_sum=np.array(st.cost_sum[:k]),
                    chi2_inner=np.array(st.chi2_inner[:n]), inner_iters=np.array(st.inner_iterations_run[:n], dtype=np.int64),
                    inner_stop=[STOP[i] for i in st.inner_stop[:n]],
                    members_by_class={c: st.members_by_class[i] for i, c in enumerate(_lib.ROBUST_CLASSES)}, cg_total=st.pcg_iters_total,
                    ms_total=st.ms_total, ms_select=st.ms_select, ms_inner=st.ms_inner)

    def time_kernel(self, which, reps=50):
        us = C.c_double(); nbytes = C.c_double()
        _lib.check(self.lib, self.lib.tsgo_time_kernel(self.h, which, reps, C.byref(us), C.byref(nbytes)),
                   "tsgo_time_kernel")
        return us.value, nbytes.value

    def level_sweep_times(self, reps=100):
        """Per coarse level of the V-cycle: (us per smoothing sweep, algorithmic bytes per sweep, sweeps per cycle)."""
        arr = (_lib.tsgo_cycle_level * 16)()
        n = self.lib.tsgo_cycle_probe(self.h, reps, arr, 16)
        _lib.check(self.lib, min(n, 0), "tsgo_cycle_probe")
        return [(arr[k].us_per_sweep, arr[k].bytes_per_sweep, arr[k].sweeps_per_cycle) for k in range(n)]

    def profile_iteration(self, reps=20):
        """In-situ per-kernel timing of one PCG iteration: list of dict(name, where, launches, us, bytes) in launch order."""
        arr = (_lib.tsgo_prof_entry * 128)()
        n = self.lib.tsgo_profile_iteration(self.h, reps, arr, 128)
        _lib.check(self.lib, min(n, 0), "tsgo_profile_iteration")
        return [dict(name=arr[k].name.decode(), where=arr[k].where.decode(), launches=arr[k].launches_per_iteration, us=arr[k].us, bytes=arr[k].bytes)
                for k in range(n)]

    def testing_apply(self, which, x):
        """tsgo_testing_apply (testing=True handles): the operator `which` on the columns of x, shape (3 P,) or (3 P, n) in the order of
        the graph's pose vertices; returns the same shape.  0 / 1: S x by PCG's / the cycle's product, 2: M^-1 x, 3: the batched cycle."""
        x = np.asarray(x, np.float64)
        cols = np.ascontiguousarray(x.reshape(x.shape[0], -1).T)      # one column per row: what the C side walks
        out = np.zeros_like(cols)
        _lib.check(self.lib, self.lib.tsgo_testing_apply(self.h, int(which), cols.ctypes.data, out.ctypes.data, cols.shape[0]), "tsgo_testing_apply")
        return np.ascontiguousarray(out.T).reshape(x.shape)

    def testing_warm_start(self, plant=None, fused=0):
        """tsgo_testing_warm_start (testing=True handles): what the PCG warm start decides and writes, as a dict of the fields of
        tsgo_testing_warm_out; vectors (3 P,) in the order of the graph's pose vertices, hist (n_prev, 3 P) newest first.  plant: None
        (the history the handle holds) or (n, 3 P) deltas, oldest first, recorded through k_save_x (fused=0) or k_save_update (fused=1)
        after the history is forgotten.  The handle is left as it was."""
        P = int((self._ids_types[1] == 0).sum()) if self._ids_types is not None else 0
        n = 0 if plant is None else len(plant)
        pl = None if plant is None else np.ascontiguousarray(np.asarray(plant, np.float64).reshape(n, 3 * P))
        hist = np.zeros((6, 3 * P)); b = np.zeros(3 * P); x0 = np.zeros(3 * P); r0 = np.zeros(3 * P)
        out = _lib.tsgo_testing_warm_out()
        out.hist, out.b, out.x0, out.r0 = hist.ctypes.data, b.ctypes.data, x0.ctypes.data, r0.ctypes.data
        _lib.check(self.lib, self.lib.tsgo_testing_warm_start(self.h, n, pl.ctypes.data if n else None, int(fused), C.byref(out)), "tsgo_testing_warm_start")
        res = {f: getattr(out, f) for f in ("warmed", "n_prev", "n_tested", "n_max", "order", "done", "carried", "scale", "bdb", "rdr")}
        res.update(err=np.array(out.err[:]), hist=hist[:out.n_prev].copy(), b=b, x0=x0, r0=r0)
        return res

    def comm_init_local(self, group):
        """group: a handle from local_group(world) shared by the handles of this process (one thread each)."""
        _lib.check(self.lib, self.lib.tsgo_comm_init_local(self.h, group), "tsgo_comm_init_local")

    def comm_unique_id(self):
        buf = (C.c_uint8 * 128)()
        _lib.check(self.lib, self.lib.tsgo_comm_unique_id(buf), "tsgo_comm_unique_id")
        return bytes(buf)

    def comm_init(self, uid: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        _lib.check(self.lib, self.lib.tsgo_comm_init(self.h, buf), "tsgo_comm_init")

    def comm_selftest(self):
        """One element through the solver's all-reduce; returns the communicator's own rank count (1 without one)."""
        n = C.c_int32()
        _lib.check(self.lib, self.lib.tsgo_comm_selftest(self.h, C.byref(n)), "tsgo_comm_selftest")
        return n.value

    def comm_time_allreduce(self, n_elements, reps=50):
        """Microseconds per all-reduce of n_elements numbers of the handle's precision on its communicator (every rank calls it alike)."""
        us = C.c_double()
        _lib.check(self.lib, self.lib.tsgo_comm_time_allreduce(self.h, int(n_elements), int(reps), C.byref(us)), "tsgo_comm_time_allreduce")
        return us.value


def local_group(world):
    """An in-process all-reduce group for `world` HipOptimizer(testing=True) handles (tests of the sharded path on a one-GPU box)."""
    lib = _lib.hip_testing_lib()
    g = C.c_void_p()
    _lib.check(lib, lib.tsgo_local_group_create(world, C.byref(g)), "tsgo_local_group_create")
    return g


def free_local_group(group):
    _lib.hip_testing_lib().tsgo_local_group_destroy(group)


class GraphOptimizer:
    """Same call shape as python/optimizer/graph_optimizer.py:11-20: GraphOptimizer(graph).optimize(n)."""

    def __init__(self, graph, **kw):
        self.graph = graph
        self.kw = kw
        self.last = None

    def optimize(self, iterations, lr=0.2):
        """rules="cpp" (default): the C++ server's loop, whose step is fixed at 0.2 (remote/optimizer/OptimizerCpu.h:164).
        rules="python": the reference's own GraphOptimizer.optimize(iterations, lr) — damping lambda*I, any lr."""
        kw = dict(self.kw)
        if kw.get("rules", "cpp") in ("lm", "dogleg"):
            pass                                           # full steps: lr has no meaning
        elif kw.get("rules", "cpp") == "cpp":
            if lr != 0.2:
                raise ValueError("the remote optimizer's step is fixed at 0.2 (remote/optimizer/OptimizerCpu.h:164); pass rules=\"python\" for GraphOptimizer.optimize(iterations, lr)")
        else:
            kw["lr"] = lr
        arr = GraphArrays.from_optgraph(self.graph)
        opt = HipOptimizer(**kw)
        try:
            opt.set_graph(arr)
            self.last = opt.optimize(iterations)
            arr.write_back(self.graph, opt.vertices())
        finally:
            opt.close()
        return self.last
