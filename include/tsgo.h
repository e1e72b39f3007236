/* tsgo.h — C ABI of the MI355X-native pose-graph optimizer (libtsgo_hip.so / libtsgo_host.so).
 *
 * This is the drop-in boundary for ToySlam's remote `graph_optimizer` hot path.  The reference has
 * no FFI of its own: its optimizer sits behind the in-process C++ interfaces cited per entry point
 * below (paths relative to the ToySlam tree), fed by the TCP codec.  Every entry point takes plain
 * pointers and sizes, returns an int status (0 = ok, <0 = error, text via tsgo_last_error()), and
 * never throws across the boundary.
 *
 * libtsgo_hip.so  : everything here (device entry points need a gfx950 GPU; they fail loudly
 *                   without one — there is no CPU fallback).
 * libtsgo_host.so : the host-only entry points (codec, synthetic graphs, problem layout), so that
 *                   CPU-only tests can exercise the boundary logic.
 */
#ifndef TSGO_H
#define TSGO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the OptGraph as plain arrays ----------------------------------------------------------------
 * Mirrors the reference graph model: remote/graph/GraphCpu.h:12-59 (AddVertex/AddEdge/FixVertex),
 * vertex/VertexType.h:3-7 (Se2 = 0, Point2 = 1), edge/EdgeType.h:3-7 (Se2 = 0 "ODOM", Se2Point2 = 1
 * "LM"), python twin python/optimizer/opt_graph.py:7-18.
 *   v_pos  : 3 doubles per vertex: (x, y, theta) for Se2, (x, y, 0) for Point2
 *   e_type : 0 ODOM, 1 LM — the two the reference's wire format carries — and 2 = VIRTUAL LANDMARK MEASUREMENT, behind this ABI only
 *            (README.md:53 "Further development: ... Virtual Meas."; the reference keeps a sketch commented out,
 *            python/optimizer/edges2d.py:83-121): two Se2 vertices that observed the same physical point, no landmark vertex;
 *            residual e = T1 p1 - T2 p2 (2), Jacobians [I | dR1/dth p1] and -[I | dR2/dth p2], 2 x 2 diagonal information
 *            3 = POSE PRIOR and 4 = LANDMARK PRIOR, behind this ABI only too: unary edges (id2 must equal id1) that pull one vertex
 *            toward an absolute measurement m in the world frame (a GNSS fix, a surveyed point, a soft anchor); any number of them may
 *            sit on one vertex (summed in input order), also on a fixed one.  Pose prior on an Se2 vertex: e_t = R_m^T (t - t_m),
 *            e_th = atan2(sin(th - m_th), cos(th - m_th)) (the ODOM residual of an edge whose first pose is held at the origin),
 *            J = blockdiag(R_m^T, 1): H_pp += [[R_m diag(a0, a1) R_m^T, 0], [0, a2]], b_p -= J^T Omega_w e.  Landmark prior on a Point2
 *            vertex: e = l - m, J = I: D_l += Omega_w, b_l -= Omega_w e.  Omega_w = the class's robust weight (default Huber, 1.5) * diag(w), chi^2 += rho as
 *            for every edge; independent of odom_jacobian; damped and (at a fixed vertex) zeroed with the rest under rules = 1
 *   e_meas : 9 doubles per edge: ODOM = the 3x3 measurement row-major (EdgeSe2.h); LM = (range,
 *            bearing, 0...) (EdgeSe2Point2d.h:34-35); virtual landmark = (range1, bearing1, range2, bearing2, 0...): the point
 *            as seen from id1 and from id2; pose prior = (mx, my, m_theta, 0...); landmark prior = (mx, my, 0...)
 *   e_inf  : 3 doubles per edge: the diagonal of the information matrix (the wire format carries
 *            nothing else, DeserializeGraph.h:123-147); LM, virtual landmark and landmark prior use the first two
 *   fixed  : vertex ids given to FixVertex; a repeated id adds the gauge term once per occurrence
 *            (OptimizerCpu.h:132-138 iterates the vector) */
typedef struct tsgo_graph {
    int32_t n_vertices;
    const uint32_t* v_id;
    const uint32_t* v_type;
    const double* v_pos;
    int32_t n_edges;
    const uint32_t* e_type;
    const uint32_t* e_ids;   /* 2 per edge: id1, id2 */
    const double* e_meas;
    const double* e_inf;
    int32_t n_fixed;
    const uint32_t* fixed;
} tsgo_graph;

/* ---- optimizer -----------------------------------------------------------------------------------*/
typedef struct tsgo_optimizer tsgo_optimizer;

typedef struct tsgo_config {
    int32_t device;          /* HIP device ordinal */
    int32_t precision;       /* 64 (default, parity mode) or 32 */
    double pcg_rel_tol;      /* stop PCG when sqrt(r^T D^-1 r) <= tol * sqrt(b^T D^-1 b), D = the 3x3 block diagonal of the reduced pose
                                system (both preconditioners; the residual norm block-Jacobi PCG measures); default 1e-10 */
    int32_t pcg_max_iters;   /* cap per Gauss-Newton iteration; default 20000 */
    int32_t lanes_per_pose;  /* 0 = auto; 1, 2, 4 or 8 lanes cooperate on one pose row */
    int32_t lanes_per_lm;    /* 0 = auto */
    int32_t use_graphs;      /* how the PCG iterations are launched.  0: kernel by kernel (eager).  1: replayed from a captured hipGraph (from the
                                second tsgo_optimize on a structure on).  2 (default): eager while the host thread enqueues an iteration well
                                within the time the device needs to run it, replay once it has been seen not to.  Eager launches on one device
                                are paced by the first kernel of every iteration, which reports to pinned host memory; edge-sharded runs launch
                                eagerly whatever this says (RCCL calls sit between the kernels).  Same answers, bit for bit. */
    int32_t rank, world;     /* edge sharding: this process owns shard `rank` of `world` (default 0, 1) */
    int32_t verbose;
    int32_t preconditioner;  /* 1 (default): smoothed-aggregation multigrid V-cycle on the reduced pose system; 0: block-Jacobi on its
                                3x3 diagonal.  Edge-sharded runs (world > 1) take the same cycle: every rank builds the hierarchy's
                                patterns from the whole graph (host memory: a full-graph layout + the hierarchy on every rank), the level-0
                                blocks are all-reduced (rank 0 contributes the diagonal), everything below is computed redundantly. */
    int32_t xcd_map;         /* 1: workgroup -> slice map gives each XCD a contiguous eighth of the vertices; 0: round-robin */
    int32_t warm_start;      /* 0: PCG starts from zero.  m >= 1: from a prediction of this solve's pose delta made from the deltas of the last
                                (up to m, at most 5: a sixth delta is held only to measure order 5, and only measured orders are taken,
                                so values above 5 act as 5) Gauss-Newton iterations: order 1 is (1 - step) * the previous delta (the un-taken
                                remainder of the last step); order k continues the degree-(k-1) trend of delta_j / (1 - step)^j.  Below the
                                cap the engine takes, solve by solve, the order that would have predicted the previous delta best.
                                Default 6.  Same answer to pcg_rel_tol. */
    int32_t rules;           /* 0 (default): the loop of the C++ server, remote/optimizer/OptimizerCpu.h:80-180 (fixed step 0.2, plateau /
                                short-step / getting-worse stops, b untouched at fixed vertices).  1: the loop of the reference's in-process
                                Python optimizer, python/optimizer/graph_optimizer.py:20-92 — Levenberg-Marquardt-style damping H + lambda I
                                (lambda from 1e-3, x1.1 when chi^2 rose, /1.1 otherwise, within [1e-6, 10]; the `lambdaVal` the C++
                                declares and never uses, OptimizerCpu.h:70), step `lr`, b zeroed at fixed vertices, stop on ||lr dx|| < 1e-3 only.
                                2: Levenberg-Marquardt with step acceptance (no reference counterpart; the loop g2o and Ceres run).  One TRIAL =
                                linearise at x with H + lambda I (b zeroed at fixed vertices as under 1), solve (H + lambda I) d = b (PCG from
                                zero: warm_start is ignored, a full step leaves no remainder), take the FULL step x + d tentatively, evaluate the
                                robustified chi^2 there and decide by the gain ratio rho = (chi^2(x) - chi^2(x + d)) / pred, pred = b^T d +
                                lambda d^T d (the drop of the quadratic model: grad(sum rho) = -2 b exactly for every robust kernel of tsgo_set_robust, whose weight is
                                w = rho'; d^T H d = b^T d - lambda d^T d).
                                Accepted (rho > 0 and pred > 0): the step stays, lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2.  Rejected: the
                                estimates are restored bit for bit, lambda *= nu, nu *= 2, and the next trial linearises again at the restored
                                point.  lambda starts at lm_lambda0 (nu at 2) on every tsgo_optimize and stays within [1e-9, 1e9].  Trials count
                                against `iterations`; chi^2 never rises.  Stops: TSGO_STOP_CONVERGED after an accepted step with ||d|| < 1e-3 or
                                chi^2(x) - chi^2(x + d) <= lm_chi2_rel_tol * chi^2(x); TSGO_STOP_DAMPING when a rejection would push lambda past
                                1e9; TSGO_STOP_CAP; TSGO_STOP_SOLVER.  Meant to be run with odom_jacobian = 1: under the constant Jacobians the
                                model is wrong and the loop rejects often (and says so in steps_rejected).  precision = 32 and world > 1 are
                                refused by tsgo_create.
                                3: Powell's dogleg, the trust-region loop g2o and Ceres offer next to 2 (tsgo_set_dogleg below has the loop
                                and its parameters): H, b and chi^2 as under 2 with lambda = 0, one linearisation and one solve per ACCEPTED
                                step, and a rejected trial costs one step from the snapshot and one chi^2 pass.  lm_lambda0 and
                                lm_chi2_rel_tol are not read.  precision = 32 and world > 1 are refused by tsgo_create. */
    double lr;               /* rules = 1: the step scale `lr` of GraphOptimizer.optimize(iterations, lr) (slam_main.py passes 0.2); ignored by rules = 0 */
    int32_t odom_jacobian;   /* 0 (default): the reference's ODOM Jacobians, the constants A = -I, B = +I (remote/graph/edge/EdgeSe2.h:35-37;
                                parity).  1: the analytic Jacobians of the same residual under the reference's vertex update (SURVEY 8f
                                rank 4; README.md:53 "further development") — same fixed points, and pose graphs with loop closures, which
                                diverge under the constants ("Error is getting worse"), converge. */
    int32_t reuse_structure; /* 1 (default): tsgo_set_graph with the SAME vertex ids/types, edge list and fixed list as the graph the
                                handle already holds only refills estimates, measurements and weights (the reference re-creates
                                everything per message, remote/app/ConnectionHandler.h:18-21); 0: always rebuild.  Same results. */
    int32_t cycle_level0;    /* what the two level-0 products INSIDE the multigrid V-cycle read.  0 (default): the implicit Schur passes over the
                                slot tables (current with every linearisation; in an edge-sharded run each ends in an all-reduce).  1: the explicit
                                level-0 matrix of the hierarchy (replicated on every shard, as old as the hierarchy): no all-reduce inside the
                                cycle, a few per cent more PCG iterations; what bench.py --gpus N (N > 1) runs.  PCG's own product is always the
                                implicit one in `precision`.  Same answers. */
    int32_t cycle_storage;   /* 16 (default) or 32: the copies of the hierarchy's matrices that the V-cycle reads as nine half floats with a common
                                power-of-two exponent per 3x3 block (20 bytes) or as nine f32 (36 bytes).  PCG's own operator and every vector stay
                                in `precision`.  Same answers; a structure whose solves take more than 64 iterations (nearly singular systems) is
                                moved to 32 by the engine (tsgo_stats.cycle_storage_now). */
    int32_t warm_requests;   /* 0 (default): every tsgo_set_graph starts the solver from nothing, so a handle's results are bit-identical to a
                                fresh handle's.  1: the warm start's history (the pose deltas of the last Gauss-Newton iterations) survives
                                tsgo_set_graph — kept for the same structure, carried over by vertex id into a grown one, dropped at the first
                                solve when it does not fit the new estimates — for a front-end that resends the graph with the estimates it was
                                returned (python/slam_main.py:215-238; the reference re-creates everything per message,
                                remote/app/ConnectionHandler.h:18-21).  Same answer to pcg_rel_tol.  What graph_optimizer runs, per connection
                                (tsgo_reset_history). */
    double lm_lambda0;       /* rules = 2: the damping of the first trial of every tsgo_optimize call; default 1e-3 (where rules = 1 starts) */
    double lm_chi2_rel_tol;  /* rules = 2: an accepted step that lowered chi^2 by no more than this fraction of it ends the run (converged);
                                default 1e-6 */
} tsgo_config;

enum { TSGO_STOP_CAP = 0, TSGO_STOP_WORSE = 1, TSGO_STOP_PLATEAU = 2, TSGO_STOP_CONVERGED = 3, TSGO_STOP_SOLVER = 4,
       TSGO_STOP_DAMPING = 5 /* rules = 2: a rejected trial would have raised lambda past its upper bound */,
       TSGO_STOP_RADIUS = 6 /* rules = 3: a rejected trial left the trust-region radius below radius_min */ };

#define TSGO_MAX_TRACE 256
typedef struct tsgo_stats {
    int32_t iterations_run;              /* Gauss-Newton linearisations performed (rules = 2 and 3: trials) */
    int32_t stop_reason;                 /* TSGO_STOP_*; rules of OptimizerCpu.h:140-153,167-177 */
    double chi2[TSGO_MAX_TRACE];         /* robustified chi^2 at each linearisation (`err`, :117); the first TSGO_MAX_TRACE of them */
    int32_t pcg_iters[TSGO_MAX_TRACE];   /* PCG iterations of each solve (rules = 3: of the solve that trial ran, 0 for a trial that reused one;
                                            pcg_iters_total adds accordingly) */
    double last_delta_norm;              /* ||delta||_2 of the last solve (unscaled, :173) */
    double ms_total, ms_linearize, ms_solve, ms_update;   /* device time, hipEvent (rules = 3: a trial that reused a solve adds to ms_update alone) */
    double ms_setup;                     /* tsgo_set_graph: host layout build + upload, or the refill when the structure was reused */
    int32_t structure_reused;            /* 1 when the last tsgo_set_graph found the same structure and only refilled values */
    int32_t cycle_storage_now;           /* what the multigrid cycle of this structure reads now: 16 (packed halves) or 32 (f32: chosen by
                                            tsgo_config.cycle_storage, or by the engine after a solve of more than 64 iterations — a graph too
                                            ill-conditioned for 11-bit blocks); 0 with block-Jacobi */
    double lambda_last;                  /* rules = 1: the damping used by the last iteration */
    int64_t n_pose, n_lm, n_odom_edges, n_lm_edges;
    int64_t pcg_iters_total;
    int32_t pcg_fallbacks;               /* solves repeated with block-Jacobi after a multigrid breakdown */
    int32_t trace_len;                   /* entries of chi2[] / pcg_iters[] that are valid: min(iterations_run, TSGO_MAX_TRACE) */
    double chi2_last;                    /* chi^2 of the LAST linearisation (`Summary() error`, OptimizerCpu.h:182), also when the
                                            run is longer than the trace */
    int32_t history_carried;             /* tsgo_config.warm_requests: 1 when this run started from the solver history of the handle's previous
                                            request (kept in place or carried over by vertex id), 2 when it did and the first solve dropped it
                                            (it did not fit the new estimates), 0 otherwise */
    int32_t graph_replay;                /* 1 when this run replayed captured hipGraphs of the PCG iteration (tsgo_config.use_graphs), 0: eager launches */
    /* rules = 2 (all zero under rules 0 and 1).  Every trace of a rules = 2 run is PER TRIAL: chi2[it] is the chi^2 at the point trial `it`
     * linearised (it repeats after a rejection), lambda_last the damping of the last trial, iterations_run the number of trials.
     * rules = 3 fills the same fields per trial: chi2[it] is the chi^2 at the point trial `it` was taken from, steps_rejected, lm_gain, lm_pred
     * and lm_chi2_trial are as under rules = 2, lm_lambda[] and lambda_last stay 0; the radii and scalars are in tsgo_dogleg_trace. */
    int32_t steps_rejected;              /* trials whose step was rolled back */
    double lm_lambda[TSGO_MAX_TRACE];    /* damping of each trial */
    double lm_gain[TSGO_MAX_TRACE];      /* gain ratio rho of each trial (0 where pred = 0); accepted when > 0 with pred > 0 */
    double lm_pred[TSGO_MAX_TRACE];      /* predicted decrease b^T d + lambda d^T d of each trial */
    double lm_chi2_trial[TSGO_MAX_TRACE];/* robustified chi^2 at the trial point x + d: the chi2 of the next trial when the step was accepted */
} tsgo_stats;

/* Fills cfg with defaults. */
void tsgo_default_config(tsgo_config* cfg);

/* GPUs visible to this process (hipGetDeviceCount; 0 when none or on error): tsgo_config.device picks one of them per handle.  The
 * server's DEVICE=all spreads its engine pool over them (host/server.cpp); the reference has one device (GraphManager.h:73-122). */
int tsgo_device_count(void);

/* Replaces CreateOptimizer/CreateSolver/CreateGraph (remote/app/GraphManager.h:73-122): one handle
 * holds the device buffers and is reusable across requests. */
int tsgo_create(const tsgo_config* cfg, tsgo_optimizer** out);
void tsgo_destroy(tsgo_optimizer* opt);

/* Replaces the graph-builder policy Functions::CreateVertex/CreateEdge + graph->AddVertex/AddEdge/
 * FixVertex (remote/serialization/DeserializeGraphFuncCpu.h:14-38, DeserializeGraph.h:43,52,151,172)
 * and GraphGpu::ToDevice (remote/cuda/graph/GraphGpu.h:80-187).  Pointers are borrowed for the call. */
int tsgo_set_graph(tsgo_optimizer* opt, const tsgo_graph* g);

/* tsgo_config.warm_requests only: forget the solver history the handle holds, so that the NEXT tsgo_set_graph starts from nothing —
 * what a pool of handles calls when a handle goes to another client than the one whose requests built that history (the
 * reference creates a fresh optimizer per message, remote/app/ConnectionHandler.h:18-21: nothing of one client ever reaches another). */
void tsgo_reset_history(tsgo_optimizer* opt);

/* Robust kernels per edge class (no reference counterpart: the reference robustifies every edge by Huber with delta = 1.5,
 * remote/optimizer/OptimizerCpu.h:36-46,92, which is the default here).  All are functions of s = e^T Omega e, the unrobustified chi^2 of
 * the edge: rho(s) goes into chi^2, w = rho'(s) scales Omega.
 *   NONE            rho = s                                            w = 1
 *   HUBER(d)        rho = s if s <= d^2, else 2 d sqrt(s) - d^2         w = 1 if s <= d^2, else d / sqrt(s)
 *   CAUCHY(d)       rho = d^2 ln(1 + s / d^2)                          w = 1 / (1 + s / d^2)
 *   GEMAN_MCCLURE   rho = d^2 s / (d^2 + s)                            w = (d^2 / (d^2 + s))^2
 * tsgo_set_robust may be called any time after tsgo_create, before or after tsgo_set_graph, and takes effect at the next linearisation
 * (tsgo_linearize, tsgo_solve_step, tsgo_optimize under every `rules`, tsgo_marginals, tsgo_joint_marginals).  The setting belongs to the
 * handle: it survives tsgo_set_graph, whether the structure is rebuilt or reused, so it can be changed between two tsgo_optimize calls on
 * one structure (wide, then narrow) without a rebuild.  A call that changes anything makes the next linearisation rebuild the multigrid
 * hierarchy; the warm start's history stays (same answer to pcg_rel_tol).  precision 64 and 32.  A handle whose setting equals the default
 * runs the same device code, bit for bit, as one that was never given a setting.  Errors (< 0, text in tsgo_last_error): a NULL argument,
 * an unknown kernel id, a delta that is not finite or outside [1e-6, 1e6] on a class whose kernel uses one, a non-default setting on an
 * edge-sharded handle (world > 1).  A class is an edge TYPE: to robustify the loop closures and leave the odometry chain quadratic (both
 * type 0), or to trust one GNSS fix and doubt another, see tsgo_set_edge_robust below. */
enum { TSGO_ROBUST_NONE = 0, TSGO_ROBUST_HUBER = 1, TSGO_ROBUST_CAUCHY = 2, TSGO_ROBUST_GEMAN_MCCLURE = 3 };
typedef struct tsgo_robust {
    int32_t kernel[5];   /* indexed by tsgo_graph.e_type: 0 ODOM, 1 LM, 2 virtual landmark, 3 pose prior, 4 landmark prior */
    int32_t reserved;    /* 0 */
    double  delta[5];    /* width; ignored by NONE */
} tsgo_robust;
void tsgo_default_robust(tsgo_robust* r);                        /* host-only too: HUBER, 1.5 everywhere */
int tsgo_set_robust(tsgo_optimizer* opt, const tsgo_robust* r);
int tsgo_get_robust(tsgo_optimizer* opt, tsgo_robust* out);

/* Robust kernels per EDGE: a palette of at most TSGO_EDGE_ROBUST_MAX kernels and one byte per edge of the tsgo_graph the handle holds, in
 * input order (what g2o's per-edge setRobustKernel and GTSAM's per-factor noise model offer).  The usual call: leave
 * the odometry chain quadratic and robustify the closures, which tsgo_set_robust cannot say because both are type 0.
 *   entry_of_edge[e] == 0   the edge takes its class's kernel from tsgo_set_robust, looked up at every launch: a later tsgo_set_robust applies
 *   entry_of_edge[e] == k   (k >= 1) the edge takes entries[k - 1], whatever its class; kernel ids and width rules are tsgo_set_robust's
 * s = e^T Omega e is unchanged; rho and w = rho'(s) come from the edge's effective kernel.  An edge whose entry is NONE is exempt: rho = s
 * and w = 1 exactly.  The setting applies wherever a class kernel is evaluated: the linearisation under every `rules`, the chi^2-only pass
 * of rules 2 and 3, the g'Hg pass of rules 3, tsgo_linearize and tsgo_solve_step, tsgo_edge_report (per record; the class summaries stay
 * indexed by e_type and `downweighted` counts w < 1 as before), tsgo_marginals, tsgo_joint_marginals, tsgo_gate_edges (Sigma only; the
 * candidate itself is never robustified) and tsgo_sample_marginals, and the inner runs of tsgo_gnc.
 *   Clearing: n_entries == 0 with entry_of_edge == NULL and n_mask == 0.  An all-zero mask is the same as cleared (stats->active = 0), and
 *   tsgo_get_edge_robust then returns no entries and zeros.  A cleared handle runs the same device code, bit for bit, as one that was never
 *   given a per-edge setting.
 *   Lifetime: that of an edge-information edit, not of the handle: the next tsgo_set_graph, refill or rebuild, drops the setting, so a
 *   reused handle does what a fresh one does.  tsgo_set_robust, tsgo_set_edge_information, tsgo_init_estimates, tsgo_gnc and tsgo_optimize
 *   keep it.
 *   Solver state: the rule of tsgo_set_robust.  A call that changes anything makes the next linearisation build a fresh multigrid
 *   hierarchy; the warm start's history stays.
 * tsgo_get_edge_robust: the number of entries, the entries (entries_out has room for TSGO_EDGE_ROBUST_MAX; those past the count are zero)
 * and the byte of every edge.  precision 64 only.
 * Errors (< 0, text in tsgo_last_error; everything is validated before anything changes, the handle is exactly as before): a NULL handle;
 * no graph set; n_mask != n_edges; n_entries outside [0, TSGO_EDGE_ROBUST_MAX]; entries == NULL with n_entries > 0; entry_of_edge == NULL
 * with edges to read; an unknown kernel id; a delta that is not finite or outside [1e-6, 1e6] on an entry whose kernel uses one; an
 * entry_of_edge value above n_entries; precision = 32; an edge-sharded handle (world > 1); for the get call cap_edges < n_edges, or a NULL
 * output with something to return. */
#define TSGO_EDGE_ROBUST_MAX 15
typedef struct tsgo_edge_robust_entry {
    int32_t kernel;      /* TSGO_ROBUST_* */
    int32_t reserved;    /* 0 */
    double  delta;       /* width; ignored by NONE */
} tsgo_edge_robust_entry;
typedef struct tsgo_edge_robust_stats {
    int64_t edges_by_entry[TSGO_EDGE_ROBUST_MAX + 1];   /* [0] = edges left to their class, [k] = edges given entries[k - 1] */
    int64_t overridden_by_class[5];                     /* edges with a non-zero entry, per tsgo_graph.e_type */
    int32_t active, reserved;                           /* 1 when any edge has a non-zero entry */
    double  ms_total;
} tsgo_edge_robust_stats;
int tsgo_set_edge_robust(tsgo_optimizer* opt, int32_t n_entries, const tsgo_edge_robust_entry* entries,
                         const uint8_t* entry_of_edge /* 1 per edge of the tsgo_graph, input order */, int64_t n_mask,
                         tsgo_edge_robust_stats* stats /* may be NULL */);
int tsgo_get_edge_robust(tsgo_optimizer* opt, int32_t* n_entries_out, tsgo_edge_robust_entry* entries_out /* room for TSGO_EDGE_ROBUST_MAX */,
                         uint8_t* entry_of_edge_out, int64_t cap_edges);

/* Powell's dogleg trust-region loop, tsgo_config.rules = 3 (no reference counterpart).  The model is that of rules = 2 with lambda = 0:
 * chi^2(x + d) ~ chi^2 - 2 b^T d + d^T H d, with H, b and chi^2 from the linearisation of rules = 2 (b zeroed at fixed vertices, the gauge
 * term inside H; the handle's robust setting, odom_jacobian, virtual-landmark and prior edges apply), g = b the descent direction.
 *   per SOLVE (at the start and after every accepted step): linearise; solve H d_gn = b (PCG from zero: warm_start is ignored and nothing
 *     of a trial enters the solver history; a failed solve ends the run with TSGO_STOP_SOLVER); back-substitute the landmarks' part; four
 *     scalars, folded on the host in f64 from per-workgroup partials: gg = b^T b, gd = b^T d_gn, dd = |d_gn|^2, gHg = b^T H b (one pass
 *     over the edges: sum of w (J b)^T Omega (J b); H is never formed).  gg == 0: TSGO_STOP_CONVERGED with no step; the linearisation is
 *     recorded as a trial of kind 0 with zero step, pred and gain.
 *   per TRIAL with radius D, alpha = gg / gHg, n = sqrt(gg), the step d = c1 b + c2 d_gn:
 *     kind 0, Gauss-Newton   sqrt(dd) <= D                 c1 = 0, c2 = 1
 *     kind 2, gradient       else alpha n >= D             c1 = D / n, c2 = 0
 *     kind 1, dogleg         otherwise                     c1 = alpha (1 - beta), c2 = beta, beta in (0, 1) the positive root of
 *                            |alpha b + beta (d_gn - alpha b)| = D:  beta = (-h + sqrt(h^2 - a c)) / a  with  a = dd - 2 alpha gd + alpha^2 gg,
 *                            h = alpha gd - alpha^2 gg,  c = alpha^2 gg - D^2
 *     pred = 2 (c1 gg + c2 gd) - (c1^2 gHg + 2 c1 c2 gg + c2^2 gd) — the model's decrease 2 b^T d - d^T H d written with H d_gn = b, which
 *     holds to pcg_rel_tol, not exactly;  step_norm = |d| from the same scalars.  The step is applied FROM THE SNAPSHOT of the estimates
 *     taken at the solve (poses by the vertex update of rules = 2, landmarks by addition), chi^2 at the trial point comes from the chi^2-only
 *     pass of rules = 2, gain = (chi^2 - chi^2_trial) / pred (0 where pred == 0).  Accepted iff gain > 0 and pred > 0; a NaN rejects.
 *   radius, after every trial, in this order: !(gain >= 0.25) -> D = 0.25 step_norm; else gain > 0.75 and kind != 0 -> D = min(2 D,
 *     radius_max); else unchanged.
 *   after an accepted trial: TSGO_STOP_CONVERGED when step_norm < 1e-3 or chi^2 - chi^2_trial <= chi2_rel_tol chi^2; otherwise the next
 *     trial solves again.  After a rejected trial: the estimates are restored bit for bit; TSGO_STOP_RADIUS when the new D < radius_min;
 *     otherwise the next trial REUSES the linearisation, d_gn and the four scalars: no linearisation, no hierarchy work, no solve.
 * Trials count against `iterations` (TSGO_STOP_CAP).  Every tsgo_optimize call starts at radius0.  chi^2 never rises.
 * The parameters belong to the handle: they survive tsgo_set_graph and are read by rules = 3 only.  tsgo_set_dogleg returns an error (< 0,
 * text in tsgo_last_error, handle unchanged) for a NULL argument, a non-finite value, anything outside 0 < radius_min <= radius0 <=
 * radius_max, and chi2_rel_tol < 0. */
typedef struct tsgo_dogleg_params { double radius0, radius_min, radius_max, chi2_rel_tol; } tsgo_dogleg_params;
void tsgo_default_dogleg(tsgo_dogleg_params* p);                 /* host-only too: 1e4, 1e-9, 1e9, 1e-6 */
int tsgo_set_dogleg(tsgo_optimizer* opt, const tsgo_dogleg_params* p);
int tsgo_get_dogleg(tsgo_optimizer* opt, tsgo_dogleg_params* out);
typedef struct tsgo_dogleg_trace {      /* of the handle's LAST tsgo_optimize; all zero when that was not a rules = 3 run */
    int32_t trials, solves;             /* solves = linearise + solve pairs run; trials - solves = trials that reused one */
    int32_t kind[TSGO_MAX_TRACE], solved[TSGO_MAX_TRACE];   /* 0 / 1 / 2 as above; 1 when the trial ran its own solve */
    double  radius[TSGO_MAX_TRACE], step_norm[TSGO_MAX_TRACE], gg[TSGO_MAX_TRACE], gHg[TSGO_MAX_TRACE], gd[TSGO_MAX_TRACE], dd[TSGO_MAX_TRACE];
    double  radius_last;                /* the radius the next trial would have used */
} tsgo_dogleg_trace;
int tsgo_get_dogleg_trace(tsgo_optimizer* opt, tsgo_dogleg_trace* out);

/* Replaces IOptimizer<T>::Optimize(IGraph*) (remote/optimizer/IOptimizer.h:21; loop semantics of
 * OptimizerCpu.h:25-183) including ISolver<T>::Solve (remote/solver/ISolver.h:10).  The graph held by
 * the handle is updated in place. */
int tsgo_optimize(tsgo_optimizer* opt, int32_t iterations, tsgo_stats* stats);

/* Replaces GraphGpu::ToHost (remote/cuda/graph/GraphGpu.h:190-224) / the vertex read-out of
 * SerializeGraphFuncCpu::SerializeVertex (remote/serialization/SerializeGraphFuncCpu.h:10-41):
 * v_pos_out has 3 doubles per vertex in the order of tsgo_graph.v_id; theta = atan2(R10, R00).  A shard (world > 1)
 * writes every pose and the landmarks IT owns; the entries of the other shards' landmarks are left untouched. */
int tsgo_get_vertices(tsgo_optimizer* opt, double* v_pos_out);

/* Parity probes (no reference counterpart; they expose what OptimizerCpu.h:82-138 builds).
 * tsgo_linearize runs one linearisation at the current state and returns, per vertex in tsgo_graph
 * order: diag (9 doubles, the dense diagonal block of H incl. the gauge term, row-major, 2x2 blocks
 * use the leading 2x2) and grad (3 doubles, b = -J^T Omega_w e), plus chi2.
 * tsgo_solve_step additionally solves H delta = b and returns delta (3 doubles per vertex, unscaled)
 * without updating the vertices.
 * A solve that reaches tsgo_config.pcg_max_iters before it meets pcg_rel_tol returns -22, and what it had is still read out: delta_out
 * holds the iterate after pcg_max_iters vector updates (poses: x_k of the PCG started from zero on a handle without history; landmarks:
 * the back-substitution u - D_l^-1 W^T x_k of that pose part) and *pcg_iters_out equals the cap.  With the multigrid preconditioner on
 * packed cycle storage (cycle_storage = 16) a capped solve is first repeated on f32 copies of the cycle's operators, and the read-out is
 * the repeat's; cycle_storage = 32 solves once. */
int tsgo_linearize(tsgo_optimizer* opt, double* diag_out, double* grad_out, double* chi2_out);
int tsgo_solve_step(tsgo_optimizer* opt, double* delta_out, double* chi2_out, int32_t* pcg_iters_out);

/* Multi-GPU (one process per GPU).  Rank 0 calls tsgo_comm_unique_id and ships the 128 bytes to the
 * other ranks (any transport); every rank then calls tsgo_comm_init.  Collectives are RCCL. */
int tsgo_comm_unique_id(uint8_t id_out[128]);
int tsgo_comm_init(tsgo_optimizer* opt, const uint8_t id[128]);
/* One element through the all-reduce the solver uses (rank + 1 from every rank, world (world + 1) / 2 expected back) and the
 * communicator's own rank count (ncclCommCount) in *ranks_out (1 without a communicator).  The first collective is where a
 * missing peer shows — as a hang: callers run it under a watchdog (bench.py). */
int tsgo_comm_selftest(tsgo_optimizer* opt, int32_t* ranks_out);
/* Timing probe used by bench.py on more than one GPU: `reps` back-to-back all-reduces (sum) of n_elements numbers of the handle's
 * precision on the handle's communicator and stream — the call the solver makes after a sharded product (3 P + partials), after a
 * linearisation (18 P + partials) and after the level-0 blocks of a hierarchy build; *us_per_call = hipEvent time / reps.  Every rank
 * of the communicator must call it with the same arguments.  0 microseconds without a communicator. */
int tsgo_comm_time_allreduce(tsgo_optimizer* opt, int64_t n_elements, int32_t reps, double* us_per_call);
/* Timing probe used by bench.py: average device time (hipEvent, microseconds) of `reps` back-to-back
 * launches of one kernel on the handle's stream, and the algorithmic bytes one launch moves.
 * which: 0 schur_lm, 1 schur_pose, 2 cg_update, 3 lin_lm, 4 lin_pose, 5 one whole PCG iteration
 * (preconditioner application included), 6 the multigrid numeric setup of one GN iteration, 7 the chi^2-only evaluation pass of a
 * rules = 2 trial (a handle created with rules = 2; to be compared with 3 + 4, the linearisation it stands in for), 8 the summary-only pass
 * of tsgo_edge_report on the handle's graph (to be compared with 7, which reads the same tables), 9 the g^T H g pass of a rules = 3 solve
 * (a handle created with rules = 3, on which 7 runs too; to be compared with 7, which reads the same tables: 9 gathers the gradient of
 * both ends of every edge on top). */
int tsgo_time_kernel(tsgo_optimizer* opt, int32_t which, int32_t reps, double* us_per_launch, double* bytes_per_launch);

/* Timing probe for the multigrid V-cycle's coarse levels (bench.py's per-kernel table): for every explicit level below
 * level 0, the average time of one block-Jacobi smoothing sweep (k_bcsr_residual, hipEvent over `reps` back-to-back
 * launches), its algorithmic bytes (the level's 3x3 blocks + column indices once, three vectors and the diagonal
 * inverse) and how many such sweeps one V-cycle runs on that level.  Returns the number of levels written (<= cap). */
typedef struct tsgo_cycle_level {
    int64_t rows, blocks;            /* block rows / 3x3 blocks of the level's matrix */
    int32_t sweeps_per_cycle;        /* k_bcsr_residual launches per V-cycle on this level (smoothing + residual) */
    int32_t lanes_per_row;
    double us_per_sweep, bytes_per_sweep;
} tsgo_cycle_level;
int tsgo_cycle_probe(tsgo_optimizer* opt, int32_t reps, tsgo_cycle_level* out, int32_t cap);

/* In-situ timing of ONE multigrid-preconditioned PCG iteration, kernel by kernel (bench.py's `roofline`): `reps` iterations are
 * launched eagerly on the handle's stream with the stopping test disabled and a hipEvent recorded before every launch; an entry
 * is one kernel instantiation at one place of the iteration (name = kernel symbol without arguments, `where` = level / role).
 * us = average time from that launch's event to the next one's (the kernel in the cache state the solve leaves it in, plus
 * one kernel boundary); bytes = the algorithmic bytes one such launch moves (the byte models of DESIGN.md section 4).  Returns
 * the number of entries written (<= cap), in launch order; < 0 on error.  Block-Jacobi handles return their three kernels. */
typedef struct tsgo_prof_entry {
    char name[64];
    char where[32];
    int32_t launches_per_iteration;
    int32_t reserved;                    /* 0 */
    double us, bytes;
} tsgo_prof_entry;
int tsgo_profile_iteration(tsgo_optimizer* opt, int32_t reps, tsgo_prof_entry* out, int32_t cap);

/* Marginal covariances: the diagonal blocks of H^-1, H = the Gauss-Newton matrix of ONE linearisation at the handle's current
 * estimates (each class's robust weights, default Huber 1.5 (tsgo_set_robust); the gauge term once per occurrence in the fixed list, tsgo_config.odom_jacobian, virtual landmark edges;
 * NOT the rules = 1 damping).  Per queried vertex id, in query order, 9 doubles of cov_out: the 3x3 block of a pose, row-major, or the
 * 2x2 block of a landmark in the leading 2x2 (the other five entries 0); each block is symmetrised, (S + S^T) / 2.  A pose's block is
 * (S^-1)_ii of the reduced pose system S = Hpp - W D^-1 W^T, a landmark's D_l^-1 + Y_l^T S^-1 Y_l with Y_l = W_{:,l} D_l^-1: 3 k + 2 m
 * right-hand sides of S for k poses and m landmarks, solved a batch of columns per launch chain by PCG on the device with the handle's
 * preconditioner.  rel_tol <= 0: the handle's pcg_rel_tol; every column stops by that rule on its own.  Duplicate ids are allowed;
 * n_ids == 0 returns 0 and does nothing.  The estimates are not changed, and nothing the next tsgo_optimize reads is (DESIGN.md
 * section 11).  H includes the prior edges (types 3, 4): a graph anchored by a pose prior with w0, w1, w2 > 0 instead of a fixed vertex
 * gives covariances in the world frame.  Errors (< 0, text in tsgo_last_error): a NULL handle, no graph set, an unknown id, a graph with
 * neither a fixed vertex nor such a pose prior (H is singular), precision = 32, an edge-sharded handle (world > 1: not supported). */
typedef struct tsgo_marginal_stats {
    int32_t columns, batches, batch_width;       /* right-hand sides solved, launch chains run, columns per chain */
    int32_t pcg_iters_max;  int64_t pcg_iters_total;
    int32_t preconditioner;                      /* 1 multigrid, 0 block-Jacobi: what the batches ran */
    int32_t fallbacks;                           /* batches repeated with block-Jacobi after a cycle breakdown */
    double ms_total, ms_solve;
} tsgo_marginal_stats;
int tsgo_marginals(tsgo_optimizer* opt, const uint32_t* ids, int32_t n_ids, double rel_tol,
                   double* cov_out, tsgo_marginal_stats* stats /* may be NULL */);

/* Joint marginal covariance: the whole block of H^-1 (the same H as tsgo_marginals) over the queried vertices, cross blocks included
 * (pose-pose, pose-landmark, landmark-landmark).  Rows and columns are compact and in query order: a pose takes 3, a landmark 2, no
 * padding, so D = 3 (pose ids) + 2 (landmark ids).  cov_out is D x D doubles, row-major, symmetrised (C + C^T) / 2.  Two calls: with
 * cov_out == NULL the call writes D to *dim_out and solves nothing; then with cov_cap >= D * D (entries, not bytes).  dim_out may be
 * NULL when cov_out is not; if given it always receives D once the ids are resolved.  Duplicate ids give repeated rows; n_ids == 0
 * gives D = 0 and returns 0.  It solves the D columns of the query (3 unit columns per pose, the 2 columns of Y_l per landmark) a batch
 * at a time; every batch but the last is full.  The state rule of tsgo_marginals holds: nothing the next tsgo_optimize reads changes.
 * Errors (< 0): those of tsgo_marginals, cov_cap < D * D, and D > 8192 (a 512 MB result). */
int tsgo_joint_marginals(tsgo_optimizer* opt, const uint32_t* ids, int32_t n_ids, double rel_tol,
                         double* cov_out, int64_t cov_cap, int32_t* dim_out, tsgo_marginal_stats* stats /* may be NULL */);

/* Posterior samples and the marginal covariance of EVERY vertex: "how uncertain is the whole map?" for K solves
 * instead of the 3 P + 2 L columns tsgo_marginals would need.  Perturb-and-MAP: sample k solves H delta = b_k, the H of tsgo_marginals
 * exactly (one linearisation at the current estimates: the robust weights of tsgo_set_robust, gamma_v = 1e6 x occurrences of v in the fixed
 * list, the handle's odom_jacobian, virtual-landmark and prior edges, no rules = 1 damping), with
 *   b_k = sum over edges e of J_e^T eta_e  +  sqrt(gamma_v) n_v on every axis of every vertex with gamma_v > 0,
 *   eta_e,j = sqrt(a_j) n_j, a_j = w_e inf_j the robust-weighted information of the linearisation (a zero information gives 0),
 *   n = noise(seed, 0, e, k) for input edge e (its first 3 normals for types 0 and 3, 2 for types 1, 2 and 4),
 *   n = noise(seed, 1, v, k) for the gauge term of the vertex at position v of the tsgo_graph vertex arrays,
 * J_e = [A | B] the Jacobians that linearisation uses (ODOM: -I, +I under odom_jacobian = 0, the analytic ones under 1; LM: A = [-R^T |
 * (ppy, -ppx)], B = R^T; virtual landmark: A = [I | u1], B = -[I | u2]; pose prior: blockdiag(R_m^T, 1); landmark prior: I).  Cov(b) = H, so
 * delta ~ N(0, H^-1) exactly, and the second moments of K samples estimate every diagonal block of H^-1 with relative standard error
 * sqrt(2 / K) on a variance, whatever the correlations.
 *   noise(seed, tag, index, k): Philox4x32-10 with key (seed low 32 bits, seed high 32 bits) and counter (index, tag, k, 0); its words
 *   r0 .. r3 give four normals by Box-Muller in f64: u1 = (r0 + 0.5) / 2^32, u2 = (r1 + 0.5) / 2^32, n0 = sqrt(-2 ln u1) cos(2 pi u2),
 *   n1 = sqrt(-2 ln u1) sin(2 pi u2); (r2, r3) give n2, n3 the same way.  tsgo_sample_noise is that function on the host.
 * cov_out receives 9 doubles per vertex of the graph, in tsgo_graph vertex order, in the format of tsgo_marginals (a pose's 3x3 row-major,
 * a landmark's 2x2 in the leading 2x2, the other five entries 0): (1 / K) sum_k delta_k delta_k^T — the mean is known to be 0, so no
 * K - 1 — exactly symmetric.  samples_out (may be NULL) receives sample k of the vertex at position v at [(k V + v) 3]; a landmark's third
 * entry is 0.  rel_tol <= 0: the handle's pcg_rel_tol.  The same call twice gives the same bits; sample k depends on (seed, k, graph,
 * estimates, settings) only, not on n_samples or on its place in a batch; another seed gives other samples.  The state rule of
 * tsgo_marginals holds: nothing the next tsgo_optimize reads changes.
 * Errors (< 0, text in tsgo_last_error; everything is validated before anything is launched, the handle stays usable): those of
 * tsgo_marginals (NULL handle, no graph, neither a fixed vertex nor a full pose prior, precision = 32, world > 1); n_samples outside
 * [1, 65536]; cov_out == NULL or cap_vertices < n_vertices; samples_cap < n_samples * n_vertices * 3 when samples_out is given. */
typedef struct tsgo_sample_stats {
    int32_t samples, reserved;
    tsgo_marginal_stats solve;              /* columns = samples; batches, width, iterations, fallbacks, ms */
    double ms_total, ms_noise, ms_readout;  /* whole call; hipEvent time of the right-hand-side kernels / of the read-out kernels */
} tsgo_sample_stats;
int tsgo_sample_marginals(tsgo_optimizer* opt, int32_t n_samples, uint64_t seed, double rel_tol,
                          double* cov_out /* 9 per vertex, tsgo_graph order */, int64_t cap_vertices,
                          double* samples_out /* may be NULL: [n_samples][n_vertices][3] */, int64_t samples_cap,
                          tsgo_sample_stats* stats /* may be NULL */);
/* host-only too (libtsgo_host.so): the generator alone, for CPU tests */
void tsgo_sample_noise(uint64_t seed, uint32_t tag, uint32_t index, uint32_t sample,
                       uint32_t words_out[4] /* may be NULL */, double normals_out[4] /* may be NULL */);

/* Leverage of EVERY edge in the graph from posterior samples: "how much does the map rest on each edge?".  With
 * Sigma = H^-1, C_e = J_e Sigma J_e^T is the covariance of the predicted measurement of edge e and h_e = tr(Omega_a C_e), in [0, dof], its
 * leverage; dof - h_e is its redundancy.  An edge with h near dof cannot be checked by any residual test: the estimate follows it.
 * H, the Jacobians J_e = [A | B], the weights a = w inf (w the robust weight of the edge's effective kernel: its class's, tsgo_set_robust,
 * or its own, tsgo_set_edge_robust) and the samples delta_k are those of tsgo_sample_marginals for the same (seed, k): a call with the
 * same seed and n_samples sees bit for bit the delta_k that tsgo_sample_marginals stages in samples_out.  ODOM edges use the handle's
 * odom_jacobian (under 0 that is -I / +I, the J that built H; with another J the trace identity below would fail).  Per sample and edge
 * y = A delta_first + B delta_second (a prior edge: y = A delta), and the record of edge e, 8 doubles at rec_out[8 e] in the edge order of
 * the tsgo_graph, is (c00, c01, c02, c11, c12, c22, h, dof_a):
 *   C      = (1 / K) sum_k y y^T — the mean is 0, so no K - 1; for the dof-2 classes (LM, virtual landmark, landmark prior) c02 = c12 = c22 = 0 exactly
 *   h      = sum_j a_j C_jj
 *   dof_a  = the number of axes the class uses with a_j > 0.  An edge with zero information has h = 0 and dof_a = 0; its C is still reported.
 * dof_a - h may be slightly negative: that is sampling noise and it is not clamped.  A diagonal entry of C has relative standard error
 * sqrt(2 / K).  For a few edges exactly, hand them to tsgo_gate_edges as candidates with innov_out: it returns S = C + Omega^-1.
 * stats (folded on the host in f64, in input edge order, from the records): per edge class the count, the sum of h and the sum of dof_a;
 * h_gauge = sum over vertices of gamma_v tr(C_v), C_v = (1 / K) sum_k delta_v delta_v^T from the accumulators of the sampling path,
 * gamma_v = 1e6 x occurrences in the fixed list; trace = h_sum[0 .. 4] added in class order, + h_gauge, whose expectation is the number of
 * unknowns 3 P + 2 L (tr(H Sigma) = n; with the same samples it equals (1 / K) sum_k delta_k^T H delta_k up to rounding).
 * State rule, determinism and refusals are those of tsgo_sample_marginals: nothing the next tsgo_optimize reads changes; the same call
 * twice gives the same bits; precision = 64 and world == 1 only; a fixed vertex or a full pose prior is required; n_samples in [1, 65536];
 * plus rec_out == NULL and cap_edges < n_edges.  Everything is validated before anything is launched and the handle stays usable. */
typedef struct tsgo_leverage_stats {
    int32_t samples, reserved;
    int64_t edges[5];                       /* per tsgo_graph.e_type */
    double  h_sum[5], dof_sum[5];           /* sum of h_e, sum of dof_a, per class */
    double  h_gauge;                        /* sum over vertices of gamma_v tr(C_v) */
    double  trace;                          /* h_sum[0 .. 4] folded in class order, + h_gauge; expectation = unknowns */
    int64_t unknowns;                       /* 3 P + 2 L */
    tsgo_marginal_stats solve;              /* as tsgo_sample_stats.solve */
    double ms_total, ms_noise, ms_readout;  /* as tsgo_sample_stats; ms_readout includes the leverage kernels */
} tsgo_leverage_stats;
int tsgo_edge_leverage(tsgo_optimizer* opt, int32_t n_samples, uint64_t seed, double rel_tol,
                       double* rec_out /* 8 per edge, input order */, int64_t cap_edges,
                       tsgo_leverage_stats* stats /* may be NULL */);

/* Per-edge residual report: which edges the robust kernels down-weighted, and by how much (what g2o's per-edge chi2() and Ceres' residual
 * evaluation answer).  Everything is evaluated at the handle's CURRENT estimates under its current tsgo_set_robust setting, by the edge
 * functions every linearisation runs; odom_jacobian, rules, damping and the fixed list do not enter.  rec_out receives six doubles per edge,
 * in the edge order of the tsgo_graph the handle was given: (e0, e1, e2, s, rho, w).
 *   e    the residual (EdgeSe2.h, EdgeSe2Point2d.h and the extensions described at tsgo_graph.e_type); e2 = 0 for LM, virtual landmark and
 *        landmark prior edges; a virtual landmark edge reports T1 p1 - T2 p2
 *   s    sum_k inf_k e_k^2 with the RAW information diagonal: the unrobustified chi^2 of the edge
 *   rho  the class's kernel at s (what the edge adds to chi^2);  w = rho'(s), the scalar that multiplies Omega (1 at s = 0)
 * stats receives, per edge class, the count, how many edges have w < 1, the sums of s and rho and the worst edge (largest s; among equal
 * ones the lowest index), and chi2 = the robustified chi^2 (the five rho_sum added in class order: tsgo_linearize's up to summation order).
 * Either output may be NULL, not both.  rec_out == NULL is the summary-only mode a caller polls between tsgo_optimize calls: no per-edge
 * buffer is allocated on the device and none is copied back.  precision 64 and 32 (an f32 handle evaluates in f32; the records are
 * widened).  The state rule of tsgo_marginals holds: the estimates, the solver history and everything the next tsgo_optimize or
 * tsgo_linearize reads stay bit for bit what they were.  Errors (< 0, text in tsgo_last_error): a NULL handle, both outputs NULL, no graph
 * set, cap_edges < n_edges with rec_out given, an edge-sharded handle (world > 1: not supported). */
typedef struct tsgo_edge_class_summary {
    int64_t edges;          /* edges of this class in the graph */
    int64_t downweighted;   /* of them, those with w < 1 */
    double  s_sum, rho_sum; /* sum of s, sum of rho(s) */
    double  s_max;          /* largest s (0 when the class is empty) */
    int64_t s_max_edge;     /* its index in tsgo_graph edge order; ties: the lowest index; -1 when the class is empty */
} tsgo_edge_class_summary;
typedef struct tsgo_edge_report_stats {
    tsgo_edge_class_summary cls[5];   /* indexed by tsgo_graph.e_type */
    double chi2;                      /* sum of the five rho_sum, folded in class order */
    double ms_total;
} tsgo_edge_report_stats;
int tsgo_edge_report(tsgo_optimizer* opt, double* rec_out /* may be NULL */, int64_t cap_edges, tsgo_edge_report_stats* stats /* may be NULL */);

/* Gate candidate edges by Mahalanobis distance: should this loop closure, this landmark match, this GNSS fix go INTO the graph?  (What
 * tsgo_edge_report answers for the edges already in it.)  The n candidates come in the encoding of tsgo_graph (e_type, 2 ids, 9 e_meas,
 * 3 e_inf per candidate); they are not in the graph and are not added to it.  Everything is evaluated at the handle's current estimates:
 *   e      the residual of the edge function the linearisation runs for that type (0 ODOM, 1 LM, 2 virtual landmark, 3 pose prior,
 *          4 landmark prior with id2 == id1); s = e^T Omega e with the raw information diagonal: what tsgo_edge_report would say for the
 *          edge if it were in the graph.  Robust kernels are not applied to the candidate itself.
 *   J      = [A | B], the analytic Jacobians of that residual under the reference's vertex update.  ODOM candidates take the
 *          odom_jacobian = 1 Jacobians (tsgo_config) whatever the handle's setting: the constants -I / +I are not the derivative of
 *          anything.  LM: A = [-R^T | (ppy, -ppx)], B = R^T.  Virtual landmark and priors: as described at tsgo_graph.e_type.
 *   Sigma  the joint marginal of the candidate's one or two vertices, exactly the tsgo_joint_marginals block: the same H (the handle's
 *          robust weights, the gauge, the priors, the handle's odom_jacobian, no damping).
 *   S      = J Sigma J^T + Omega^-1, d2 = e^T S^-1 e, logdet = ln det S, dof = 3 for types 0 and 3, 2 for types 1, 2 and 4: d2 is
 *          chi^2-distributed with dof degrees of freedom when the candidate is consistent with the graph (accept at the 99 % quantile:
 *          11.345 for 3, 9.210 for 2).  A gate cannot reject what the graph's own uncertainty allows: after a long stretch of pure
 *          odometry Sigma is large and false closures pass.
 * rec_out receives 8 doubles per candidate, in input order: (e0, e1, e2, s, d2, dof, logdet, status); e2 = 0 where dof = 2.  status is 0,
 * or 1 when the Cholesky factorisation of S fails (S not positive definite): then d2 and logdet are NaN and stats->not_pd counts the
 * candidate.  innov_out (may be NULL) receives S, row-major in the leading dof x dof of 9 doubles per candidate, the rest 0, exactly
 * symmetric.  The distinct vertices of the candidates are solved once (3 columns a pose, 2 a landmark, however many candidates share
 * the vertex), a batch of columns per launch chain as tsgo_joint_marginals does, every batch but the last full: stats->solve.columns =
 * 3 (distinct poses) + 2 (distinct landmarks).  rel_tol <= 0: the handle's pcg_rel_tol.  A repeated call gives the same bits.  n == 0
 * returns 0 and solves nothing.  The state rule of tsgo_marginals holds: nothing the next tsgo_optimize reads changes.
 * Errors (< 0, text in tsgo_last_error; the candidates are validated completely before anything is launched, the handle stays usable):
 * those of tsgo_marginals (NULL handle, no graph, precision = 32, world > 1, neither a fixed vertex nor a full pose prior, an unknown
 * vertex id); an unknown e_type; a vertex of the wrong kind for the type (LM needs a pose, then a landmark); id1 == id2 on a binary type
 * or id1 != id2 on a unary one; an information entry on a used axis that is not finite and > 0 (Omega^-1 must exist); a non-invertible
 * ODOM measurement; n < 0 or n > 2^20 (the device holds 36 doubles per candidate); rec_out == NULL with n > 0. */
typedef struct tsgo_gate_stats {
    int32_t candidates, vertices;      /* candidates given; distinct vertices they touch */
    int32_t not_pd, reserved;          /* candidates whose innovation covariance was not positive definite (status = 1) */
    tsgo_marginal_stats solve;         /* the batched solve: columns, batches, batch_width, iterations, fallbacks, ms */
    double ms_total, ms_readout;       /* whole call; device time of the gate's own kernels (read-out after every batch, evaluation) */
} tsgo_gate_stats;
int tsgo_gate_edges(tsgo_optimizer* opt, int32_t n, const uint32_t* e_type, const uint32_t* e_ids, const double* e_meas, const double* e_inf, double rel_tol,
                    double* rec_out, double* innov_out /* 9 per candidate, may be NULL */, tsgo_gate_stats* stats /* may be NULL */);

/* Initial estimates from an odometry spanning tree (what g2o's computeInitialGuess and GTSAM's initializers offer):
 * the estimates that ODOMETRY ALONE implies, before the first tsgo_optimize, or as what tsgo_gate_edges and tsgo_edge_report judge closures
 * against.  Every other loop of the engine is a local method and needs a start near the optimum.
 *   The tree depends on the graph's structure and the mask only, never on information values.  An edge is usable when e_type == 0, id1 != id2
 *   and (odom_mask == NULL or odom_mask[e] != 0); the mask has one byte per edge of the graph (n_mask must equal n_edges; entries of non-ODOM
 *   edges are ignored); edge types 1-4 never enter the tree.  Breadth-first search from the fixed pose vertices (in order of first occurrence
 *   in the fixed list, depth 0, all in the FIFO queue at the start); a popped vertex scans its usable incident edges in increasing input edge
 *   index and an unvisited other endpoint becomes its child through that edge.  When the queue runs empty and poses remain unvisited, the
 *   unvisited pose with the lowest input vertex index becomes a root (it keeps its estimate: roots_free) and the search goes on.  Roots
 *   and fixed vertices are never written.
 *   TSGO_INIT_POSES: along a tree edge with measurement M (row-major 3x3), theta = atan2(M10, M00), t = (M02, M12); a child that is the edge's
 *   id2 gets T_child = T_parent o (t, theta), a child that is id1 gets T_parent o (t, theta)^-1: for a rigid M the edge's ODOM residual is
 *   zero afterwards.  The handle keeps M^-1, not M: (t, theta) is taken from M^-1 inverted back in f64 with its last row taken as (0, 0, 1),
 *   so a measurement that is not a rigid transform gets what that gives.  On the device: one record per pose, ceil(log2(depth_max + 1))
 *   pointer-jumping passes (no atomics, no host round trip), then the write exactly as a pose update writes (cos, sin of atan2(s, c)).
 *   TSGO_INIT_LANDMARKS (after the poses when both are asked for, from the current poses otherwise): every non-fixed landmark with at least one
 *   LM edge whose two information entries are both > 0 becomes the plain mean of t_pose + R_pose (r cos phi, r sin phi) over those edges;
 *   every other landmark stays bit for bit.
 * The call changes estimates: it leaves the solver as a tsgo_set_graph that only refills values does (no multigrid hierarchy is valid, and
 * the warm start's history is dropped even under warm_requests: a jump does not continue it); what belongs to the handle (tsgo_set_robust)
 * stays.  The same call twice gives the same bits, and the second changes none (the roots did not move).
 * Errors (< 0, text in tsgo_last_error; everything is validated before anything is launched, the handle stays usable): a NULL handle, no
 * graph set, `what` outside 0..3, n_mask != n_edges with a mask given, precision = 32, an edge-sharded handle (world > 1). */
typedef struct tsgo_init_stats {
    int64_t poses_set, landmarks_set;       /* estimates overwritten */
    int64_t roots_fixed, roots_free;        /* trees rooted at a fixed pose / at a free pose that kept its estimate */
    int64_t edges_usable, tree_edges;       /* ODOM edges the tree could use / did use (= poses_set when poses are set) */
    int64_t landmarks_unobserved;           /* non-fixed landmarks without a usable LM edge: left as they were */
    int32_t depth_max, rounds;              /* deepest tree node; composition passes run on the device (0 when poses are not set) */
    double ms_total, ms_tree, ms_device;    /* whole call; host tree build; hipEvent time of the kernels */
} tsgo_init_stats;
#define TSGO_INIT_POSES 1
#define TSGO_INIT_LANDMARKS 2
int tsgo_init_estimates(tsgo_optimizer* opt, int32_t what /* 0 = both */, const uint8_t* odom_mask /* may be NULL */,
                        int64_t n_mask, tsgo_init_stats* stats /* may be NULL */);

/* Edit edge weights in place on the device (g2o's edge `level`; what a caller-side IRLS, GNC or switchable-constraints loop needs per
 * round): replace the information diagonal of n edges of the graph the handle holds.
 *   edge_idx   positions in the edge arrays of the tsgo_graph the handle was given (the numbering of tsgo_edge_report), or NULL for "all
 *              edges in order" (then n must equal n_edges)
 *   e_inf      3 doubles per LISTED edge, in list order, the encoding of tsgo_graph.e_inf; the entry an edge's type does not use (the third
 *              of LM, virtual landmark and landmark prior edges) is ignored
 * After the call every table of the handle holds, bit for bit, what a same-structure tsgo_set_graph whose graph differs from the held one
 * only in those e_inf rows would hold: the stored value is (T)value in the handle's precision (64 and 32).  Nothing else on the device is
 * written: the estimates keep their bits, which a tsgo_set_graph (it takes them from the host, through cos / sin) cannot offer.  A zero
 * information is legal: the edge then contributes exactly nothing to H, b and chi^2, and tsgo_edge_report gives it s = 0, rho = 0, w = 1.
 * If the edits leave a vertex with no information at all, or the graph disconnected, the result is what tsgo_set_graph would make of that
 * graph: the caller's responsibility there and here.
 *   Solver state: the rule of tsgo_set_robust.  A call with n > 0 makes the next linearisation build a fresh multigrid hierarchy; the warm
 *   start's history and everything else the solver learnt stay, and so does the robust setting.  n == 0 returns 0 and changes nothing.
 *   Lifetime: the edit belongs to the values, not to the handle: the next tsgo_set_graph, refill or rebuild, replaces every weight with
 *   what it carries.
 * tsgo_get_edge_information: what the handle holds now, 3 doubles per edge in input order, widened from the handle's precision; an entry
 * the edge's type does not use comes back as 0.
 * Errors (< 0, text in tsgo_last_error; everything is validated before anything is uploaded or launched, the handle is exactly as before):
 * a NULL handle; no graph set; n < 0; e_inf == NULL with n > 0; edge_idx == NULL with n != n_edges (n > 0); an index outside [0, n_edges);
 * an index listed twice; an entry on an axis the edge's type uses that is not finite or is negative; an edge-sharded handle (world > 1),
 * for either call; cap_edges < n_edges or e_inf_out == NULL with edges to return (get). */
typedef struct tsgo_edge_info_stats {
    int64_t edges_listed;        /* n */
    int64_t edges_by_class[5];   /* of them, per tsgo_graph.e_type */
    int32_t maps_built;          /* 1 when this call built and uploaded the edge -> slot map of the structure, 0 when it was there */
    int32_t reserved;            /* 0 */
    double ms_total, ms_host, ms_device;   /* whole call; validation + map + staging; hipEvent time of the kernel */
} tsgo_edge_info_stats;
int tsgo_set_edge_information(tsgo_optimizer* opt, int64_t n, const int64_t* edge_idx /* may be NULL */, const double* e_inf,
                              tsgo_edge_info_stats* stats /* may be NULL */);
int tsgo_get_edge_information(tsgo_optimizer* opt, double* e_inf_out, int64_t cap_edges);

/* Edit vertices in place on the device (g2o's setFixed and setEstimate on a live optimizer): which vertices are fixed,
 * and the estimates of listed vertices, without a tsgo_set_graph — which would rebuild the layout for another fixed list and, as a refill,
 * drop every weight edit, the per-edge robust setting and the solver's history for other estimates.  Typical: move the anchor to the
 * current pose, so that tsgo_marginals and tsgo_gate_edges give uncertainty relative to the robot; freeze the old part of a map; release a
 * surveyed landmark; try a relocalisation hypothesis under tsgo_edge_report.
 * tsgo_set_fixed: count[i] is the multiplicity of ids[i] in the fixed list (NULL: 1 each); 0 releases the vertex, k >= 1 stands for k
 * occurrences (the gauge term is 1e6 per occurrence).  Unlisted vertices keep theirs.  The call writes (T)(1e6 * k) into the handle's two
 * gauge arrays and nothing else on the device: the estimates keep their bits.
 *   The canonical list: afterwards the handle's fixed list is the vertices with count > 0 in tsgo_graph vertex order, each repeated count
 *   times, and every reader sees it — the linearisation, tsgo_init_estimates (its breadth-first sources and the landmarks it leaves alone),
 *   and the "is H regular" check of tsgo_marginals, tsgo_joint_marginals, tsgo_gate_edges, tsgo_sample_marginals and tsgo_edge_leverage.  Every later call
 *   behaves, bit for bit where the same kernels see the same inputs, as a fresh handle given the same graph with that list.  Releasing
 *   every fixed vertex is legal: the result is what tsgo_set_graph makes of n_fixed = 0, and tsgo_marginals then refuses as it does there.
 *   Solver state: the rule of tsgo_set_edge_information.  The next linearisation builds a fresh multigrid hierarchy; the warm start's
 *   history, weight edits, the per-edge robust setting and the robust setting stay.  n == 0 returns 0 and changes nothing.
 *   Lifetime: that of an edit.  The next tsgo_set_graph installs the list it carries; whether it may reuse the structure is still decided
 *   against the list of the previous tsgo_set_graph, not against the edit.
 * tsgo_get_fixed: the multiplicities the handle holds now, one per vertex in tsgo_graph order (after a plain tsgo_set_graph: the
 * occurrences in its list).
 * tsgo_set_estimates: the listed vertices receive (x, y, theta) — 3 doubles per listed vertex, a landmark's third is ignored — exactly as
 * tsgo_set_graph writes them: a pose's record ((T)x, (T)y, (T)cos theta, (T)sin theta) and (T)theta with cos / sin taken on the host in
 * f64, a landmark's (T)x, (T)y.  ids == NULL: every vertex in order (n must equal n_vertices).  Every other estimate keeps its bits; fixed
 * vertices may be listed.  The call ends as tsgo_init_estimates does: the solver restarts as after a refill and the warm start's history
 * is dropped even under warm_requests.  Weight edits, robust settings and a tsgo_set_fixed stay.
 * Errors (< 0, text in tsgo_last_error; everything is validated before anything is staged or launched, the handle is exactly as before):
 * a NULL handle; no graph set; n < 0; ids == NULL with n > 0 (set_fixed) or with n != n_vertices (set_estimates); v_pos == NULL with n > 0;
 * an unknown id; an id listed twice; a count outside [0, 65535]; an estimate that is not finite on an axis the vertex uses; cap_vertices <
 * n_vertices or count_out == NULL with vertices to return (get); an edge-sharded handle (world > 1), for all three. */
typedef struct tsgo_vertex_edit_stats {
    int64_t listed, poses, landmarks;     /* vertices listed; of them Se2 / Point2 */
    int64_t fixed_now, released;          /* vertices of the graph with count > 0 after the call; set_fixed: listed vertices that went from > 0 to 0 */
    double ms_total, ms_host, ms_device;  /* whole call; validation + staging; hipEvent time of the kernel */
} tsgo_vertex_edit_stats;
int tsgo_set_fixed(tsgo_optimizer* opt, int64_t n, const uint32_t* ids, const int32_t* count /* may be NULL: 1 each */,
                   tsgo_vertex_edit_stats* stats /* may be NULL */);
int tsgo_get_fixed(tsgo_optimizer* opt, int32_t* count_out /* 1 per vertex, tsgo_graph order */, int64_t cap_vertices);
int tsgo_set_estimates(tsgo_optimizer* opt, int64_t n, const uint32_t* ids /* NULL: all vertices in order, n == n_vertices */,
                       const double* v_pos /* 3 per listed vertex */, tsgo_vertex_edit_stats* stats /* may be NULL */);

/* Graduated non-convexity with the truncated-least-squares surrogate (Yang, Antonante, Tzoumas, Carlone 2020; GTSAM's GncOptimizer with
 * known inliers): the outer loop for a graph whose start cannot be trusted, where an M-estimator of tsgo_set_robust
 * only helps near the optimum.  Every round re-evaluates every edge on the device, turns its squared residual into a weight in [0, 1] and
 * scatters weight * base information into the tables (what tsgo_edge_report, host arithmetic and tsgo_set_edge_information would do in
 * three calls and two transfers), then runs the handle's own tsgo_optimize.
 *   Base information: what the handle holds when the call starts (tsgo_get_edge_information).  s = sum_k base_k e_k^2 of an edge never
 *   depends on the weight the tables hold at that moment.  A dormant edge (base 0) has s = 0, w = 1 and stays dormant.
 *   Subject edges: barc2[e_type] > 0 and (subject == NULL or subject[e] != 0); n_mask must equal n_edges when a mask is given.  Every other
 *   edge is exempt (a known inlier): w = 1, and its information is never written.  Without known inliers nothing anchors the first rounds
 *   (all weights start small together): mask the edges that are trusted, typically the odometry chain.
 *   The loop: a probe pass finds q_max = max over subject edges of s / barc2[class].  2 q_max - 1 <= 0: nothing is written, rounds = 0,
 *   TSGO_GNC_ALL_INLIERS.  Otherwise mu = 1 / (2 q_max - 1), and each round
 *     reweights   q = s / barc2:  w = 1 when q <= mu / (mu + 1), w = 0 when q >= (mu + 1) / mu, else w = sqrt(mu (mu + 1) / q) - mu (f64, in
 *                 that form); the tables receive w * base_k on the axes the class uses;
 *     invalidates as tsgo_set_edge_information does (the next linearisation builds a fresh multigrid hierarchy; the history stays);
 *     optimises   tsgo_optimize(inner_iterations) under the handle's own rules, odom_jacobian and robust setting.  The call does NOT touch
 *                 the robust setting: textbook GNC is tsgo_set_robust with NONE on every class, set by the caller beforehand;
 *     stops       with TSGO_GNC_BINARY when every subject weight of this round was 0 or 1, with TSGO_GNC_SOLVER when the inner run ended
 *                 with TSGO_STOP_SOLVER, with TSGO_GNC_ROUNDS after rounds_max rounds; otherwise mu *= mu_step.
 *   keep_weights = 1: on return the tables hold w * base of the last round (a later tsgo_set_graph replaces them, as after an edit).
 *   keep_weights = 0: the base information is restored bit for bit; the estimates stay where the loop left them.
 * w_out (may be NULL) receives the last round's weight of every edge in input order, 1 for exempt edges (all 1 after ALL_INLIERS).
 * precision 64 only.  Errors (< 0, text in tsgo_last_error; everything is validated before anything is launched, the handle is exactly as
 * before): a NULL handle or params; no graph set; n_mask != n_edges with a mask given; cap_edges < n_edges with w_out given; mu_step not
 * finite or <= 1; rounds_max outside [1, TSGO_GNC_MAX_ROUNDS]; inner_iterations < 0; a barc2 that is not finite; keep_weights not 0 or 1;
 * no subject edge; precision = 32; an edge-sharded handle (world > 1). */
#define TSGO_GNC_MAX_ROUNDS 128
enum { TSGO_GNC_ALL_INLIERS = 0, TSGO_GNC_BINARY = 1, TSGO_GNC_ROUNDS = 2, TSGO_GNC_SOLVER = 3 };
typedef struct tsgo_gnc_params {
    double  barc2[5];           /* indexed by tsgo_graph.e_type: inlier threshold on s; <= 0: the class is exempt.  Defaults: the 99 % chi^2
                                   quantiles of tsgo_gate_edges, 11.345 for types 0 and 3 (3 dof), 9.210 for types 1, 2 and 4 (2 dof) */
    double  mu_step;            /* > 1; default 1.4 */
    int32_t rounds_max;         /* 1 .. TSGO_GNC_MAX_ROUNDS; default 64 */
    int32_t inner_iterations;   /* tsgo_optimize's `iterations` of every round; default 10.  0: the round reweights only */
    int32_t keep_weights;       /* 1 (default) or 0 */
    int32_t reserved;           /* 0 */
} tsgo_gnc_params;
typedef struct tsgo_gnc_stats {
    int32_t rounds, stop_reason;                          /* rounds run; TSGO_GNC_* */
    double  q_max;                                        /* of the probe pass */
    double  mu[TSGO_GNC_MAX_ROUNDS];                      /* per round: the control parameter, */
    double  cost[TSGO_GNC_MAX_ROUNDS];                    /* ... sum of w s over subject edges at the reweighting point, */
    double  chi2_inner[TSGO_GNC_MAX_ROUNDS];              /* ... tsgo_stats.chi2_last of the inner run (0 with inner_iterations = 0), */
    int32_t inner_iterations_run[TSGO_GNC_MAX_ROUNDS];    /* ... its iterations_run */
    int32_t inner_stop[TSGO_GNC_MAX_ROUNDS];              /* ... and stop_reason (TSGO_STOP_*), */
    int64_t n_zero[TSGO_GNC_MAX_ROUNDS], n_one[TSGO_GNC_MAX_ROUNDS], n_between[TSGO_GNC_MAX_ROUNDS];   /* ... subject weights = 0, = 1, in between */
    int64_t subject_by_class[5];                          /* subject edges per tsgo_graph.e_type */
    int64_t pcg_iters_total;                              /* over all inner runs */
    double  ms_total, ms_reweight, ms_inner;              /* whole call; hipEvent time of the reweighting passes (probe included); wall time of the inner runs */
} tsgo_gnc_stats;
void tsgo_default_gnc(tsgo_gnc_params* p);                /* host-only too */
int tsgo_gnc(tsgo_optimizer* opt, const tsgo_gnc_params* params, const uint8_t* subject /* may be NULL */, int64_t n_mask,
             double* w_out /* 1 per edge, may be NULL */, int64_t cap_edges, tsgo_gnc_stats* stats /* may be NULL */);

/* Max-mixture edges (Olson and Agarwal 2013; g2o's max-mixture edge types, GTSAM's mixture factors): "this measurement
 * is one of these alternatives" — a loop closure or its null hypothesis (the same mean, a very wide covariance), landmark A or landmark B,
 * a direct fix or a known multipath offset.  Every pass evaluates every alternative on the device, selects the likeliest of each group and
 * switches the others off in the tables (what tsgo_edge_report, host arithmetic per group and tsgo_set_edge_information would do in three
 * calls and two transfers), then runs the handle's own tsgo_optimize.  A local method: it finds the selection that is consistent with the
 * estimates it starts from (from an odometry-only start every closure looks false).
 *   Components: a group is a list of edges that are already in the graph, each with its own measurement and information (positions in
 *   the edge arrays of the tsgo_graph the handle was given, the numbering of tsgo_edge_report): group g is member_edge[group_off[g] ..
 *   group_off[g + 1]).  Exactly one member of a group is switched on at a time; the others are held at information 0, where an edge
 *   contributes exactly nothing (tsgo_set_edge_information).  An edge belongs to at most one group.  Edges in no group are never read for
 *   their weights and never written.
 *   Base information: what the handle holds when the call starts (tsgo_get_edge_information).  s_e = sum_k base_k e_k^2 of a member at the
 *   current estimates, under the NONE kernel and written term for term as tsgo_edge_report writes it, never depends on what the tables hold
 *   at that moment.
 *   Cost of member m (edge e): c_m = s_e + k_m with k_m = -(ln b_0 + ln b_1 [+ ln b_2]) - 2 log_weight_m over the axes the edge's type uses,
 *   in that order (k_m on the host in f64, c_m on the device in f64): -2 ln of the component's weighted Gaussian likelihood without its
 *   (2 pi) term, which is the same for every member because the members of a group must have the same number of axes.  A cost that is not
 *   finite counts as +infinity.
 *   Selection: the member with the smallest cost; the comparison is strict, so a tie goes to the lowest position in the group, and a group
 *   whose costs are all +infinity selects position 0.
 *   The loop: nothing is selected at first.  Pass r = 0, 1, ... evaluates the costs at the current estimates and selects; n_changed[r] is the
 *   number of groups whose selection differs from the previous pass's (in pass 0: every group), cost_sum[r] the sum of the winners' costs.
 *     no group changed (r > 0)   the call stops with TSGO_MIX_STABLE: nothing is written, the tables hold this selection already;
 *     otherwise                  the tables receive base for each winner and 0 for each loser on the axes the type uses, and the solver is
 *                                invalidated as tsgo_set_edge_information does (the next linearisation builds a fresh multigrid hierarchy; the
 *                                history and the robust settings stay);
 *     r == rounds_max            the call stops with TSGO_MIX_ROUNDS: rounds_max rounds did not settle the selection (the tables hold the
 *                                selection of this last pass, which no inner run has followed);
 *     otherwise                  round r ends with tsgo_optimize(inner_iterations) under the handle's own rules, odom_jacobian and robust
 *                                settings; an inner run that ends with TSGO_STOP_SOLVER stops the call with TSGO_MIX_SOLVER, an inner error
 *                                code (< 0) ends the call with that code at once.
 *   So passes = rounds + 1 unless the solver failed, and a call that settles reports TSGO_MIX_STABLE whatever rounds_max is.  With
 *   inner_iterations = 0 a round selects and scatters only; inner_iterations = 1 is Olson and Agarwal's form (a selection per
 *   linearisation).  selected_out (the position inside its group, one per group) and cost_out (one per member, as computed: a cost that
 *   is not finite is returned as it is) are those of the last pass.
 *   keep_selection = 1: on return the tables hold the last selection (a later tsgo_set_graph replaces it, as after an edit).
 *   keep_selection = 0: the base information is restored bit for bit; the estimates stay where the loop left them.
 * Deterministic: the same call from the same state gives the same bits.  n_groups == 0 returns 0 and does nothing.  precision 64 and
 * world == 1 only.  Errors (< 0, text in tsgo_last_error; everything is validated before anything of the handle is written, the handle is
 * exactly as before): a NULL handle or params; no graph set; n_groups < 0; group_off or member_edge NULL with groups to read; group_off[0]
 * != 0; a group_off that does not increase (every group has at least 1 member); a group above TSGO_MIX_MAX_MEMBERS; an edge index outside
 * the graph; an edge listed twice, in one group or in two; members of one group whose types differ in their number of axes (types 0 and 3
 * have 3; types 1, 2 and 4 have 2); a base information on a used axis that is not finite and > 0; a log_weight that is not finite;
 * rounds_max outside [1, TSGO_MIX_MAX_ROUNDS]; inner_iterations < 0; keep_selection not 0 or 1; cap_groups < n_groups with selected_out
 * given, cap_members < group_off[n_groups] with cost_out given; precision = 32; an edge-sharded handle (world > 1). */
#define TSGO_MIX_MAX_ROUNDS 128
#define TSGO_MIX_MAX_MEMBERS 64
enum { TSGO_MIX_STABLE = 0, TSGO_MIX_ROUNDS = 1, TSGO_MIX_SOLVER = 2 };
typedef struct tsgo_mixture_params {
    int32_t rounds_max;         /* 1 .. TSGO_MIX_MAX_ROUNDS; default 32 */
    int32_t inner_iterations;   /* tsgo_optimize's `iterations` of every round; default 5.  0: select and scatter only */
    int32_t keep_selection;     /* 1 (default) or 0 */
    int32_t reserved;           /* 0 */
} tsgo_mixture_params;
typedef struct tsgo_mixture_stats {
    int32_t rounds, passes;                                   /* rounds run (scatter and inner run); selection passes */
    int32_t stop_reason, reserved;                            /* TSGO_MIX_*; 0 */
    int64_t n_changed[TSGO_MIX_MAX_ROUNDS + 1];               /* per pass: groups whose selection moved, */
    double  cost_sum[TSGO_MIX_MAX_ROUNDS + 1];                /* ... sum of the winners' costs (workgroup partials folded in order) */
    double  chi2_inner[TSGO_MIX_MAX_ROUNDS + 1];              /* per round: tsgo_stats.chi2_last of the inner run (0 with inner_iterations = 0), */
    int32_t inner_iterations_run[TSGO_MIX_MAX_ROUNDS + 1];    /* ... its iterations_run */
    int32_t inner_stop[TSGO_MIX_MAX_ROUNDS + 1];              /* ... and stop_reason (TSGO_STOP_*) */
    int64_t groups, members, members_by_class[5];             /* n_groups; group_off[n_groups]; members per tsgo_graph.e_type */
    int64_t pcg_iters_total;                                  /* over all inner runs */
    double  ms_total, ms_select, ms_inner;                    /* whole call; hipEvent time of the two kernels over all passes; wall time of the inner runs */
} tsgo_mixture_stats;
void tsgo_default_mixture(tsgo_mixture_params* p);            /* host-only too */
int tsgo_max_mixture(tsgo_optimizer* opt, const tsgo_mixture_params* params, int64_t n_groups, const int64_t* group_off /* n_groups + 1 */,
                     const int64_t* member_edge /* group_off[n_groups] input edge indices */,
                     const double* log_weight /* one per member, may be NULL: 0 */,
                     int32_t* selected_out /* one per group, may be NULL */, int64_t cap_groups,
                     double* cost_out /* one per member, may be NULL */, int64_t cap_members,
                     tsgo_mixture_stats* stats /* may be NULL */);

const char* tsgo_last_error(void);

/* ---- host-only: wire codec (libtsgo_host.so and libtsgo_hip.so) ---------------------------------
 * Request payload = what python/remote/graph_to_bytes.py:32-67 writes and
 * remote/serialization/DeserializeGraph.h:18-173 reads (WITHOUT the 4-byte length prefix).
 * Response = what remote/serialization/SerializeGraph.h:17-71 + SerializeGraphFuncCpu.h:10-65 write
 * (WITH the u32 length prefix) and python/remote/bytes_to_graph.py:49-108 reads. */
typedef struct tsgo_wire_graph tsgo_wire_graph;
int tsgo_wire_decode(const uint8_t* payload, size_t len, tsgo_wire_graph** out);
/* The same into an existing handle (tsgo_wire_new, or one decoded before): its arrays keep their capacity, so a
 * connection that sends graph after graph (remote/app/ConnectionHandler.h:30-32) does not fault in ~2x the payload of
 * fresh pages per message.  On failure the handle stays valid but holds no graph. */
tsgo_wire_graph* tsgo_wire_new(void);
int tsgo_wire_decode_into(tsgo_wire_graph* w, const uint8_t* payload, size_t len);
void tsgo_wire_view(const tsgo_wire_graph* w, tsgo_graph* view);
/* Encodes the reply for the decoded request with vertex positions replaced by v_pos (3 doubles per
 * vertex, request order).  Two-call pattern: buf = NULL returns the size. */
int64_t tsgo_wire_encode_response(const tsgo_wire_graph* w, const double* v_pos, uint8_t* buf, size_t cap);
/* Encodes a REQUEST (client side; byte-identical to graph_to_bytes for the same OptGraph), prefix
 * included.  Two-call pattern. */
int64_t tsgo_wire_encode_request(const tsgo_graph* g, uint8_t* buf, size_t cap);
void tsgo_wire_free(tsgo_wire_graph* w);

/* ---- host-only: synthetic graphs (BASELINE.json configs 2-5; definition in DESIGN.md) ------------*/
typedef struct tsgo_synth_config {
    int64_t n_poses;
    int32_t lm_per_pose;        /* LM edges per pose (k nearest landmarks in range) */
    double lm_obs_target;       /* aimed observations per landmark (sets landmark density) */
    int32_t loop_closures;      /* extra ODOM edges between revisiting poses (config 5) */
    uint64_t seed;
} tsgo_synth_config;
typedef struct tsgo_synth tsgo_synth;
int tsgo_synth_create(const tsgo_synth_config* cfg, tsgo_synth** out);
void tsgo_synth_view(const tsgo_synth* s, tsgo_graph* view);
/* ground-truth vertex positions (3 doubles per vertex), for convergence checks */
const double* tsgo_synth_truth(const tsgo_synth* s);
void tsgo_synth_free(tsgo_synth* s);

/* ---- host-only: layout probe (tests of the SELL builder and of the shard planner) ---------------*/
typedef struct tsgo_layout_info {
    int64_t n_pose, n_lm_local, n_lm_total, n_lm_edges_local, n_odom_slots;
    int64_t rows_by_pose, rows_by_lm, rows_odom;      /* 64-lane rows incl. padding */
    int32_t lanes_per_pose, lanes_per_lm;
    int64_t lm_first, lm_last;                        /* landmark range owned (in landmark order of the graph) */
    int64_t pose_first, pose_last;                    /* pose range whose ODOM rows/gauge this shard owns */
} tsgo_layout_info;
int tsgo_layout_probe(const tsgo_graph* g, int32_t rank, int32_t world, int32_t lanes_per_pose,
                      int32_t lanes_per_lm, tsgo_layout_info* out);

/* ---- host-only: multigrid hierarchy probe (tests + setup timing) ------------------------------------*/
typedef struct tsgo_amg_info {
    int32_t n_levels;               /* matrices in the hierarchy, the dense coarsest one included */
    int64_t rows[8];                /* block rows per level (level 0 = poses) */
    int64_t blocks[8];              /* 3x3 blocks per level */
    int64_t p_blocks[8];            /* blocks of the prolongator leaving each level */
    int64_t schur_contribs;         /* landmark-pair terms summed into the explicit level-0 matrix */
    double ms_layout, ms_symbolic;  /* host time: slot tables / hierarchy patterns */
    int32_t agg_min[8], agg_max[8]; /* smallest / largest aggregate (in nodes of that level) leaving each level */
    uint64_t checksum;              /* FNV-1a over every slot table, numbering, pattern and gather list, in order: equal checksums
                                     * = the device would be handed the same bytes (the build must not depend on the thread count) */
} tsgo_amg_info;
int tsgo_amg_probe(const tsgo_graph* g, tsgo_amg_info* out);
/* The same for shard `rank` of `world` (edge-sharded runs replicate the hierarchy; only the level-0 contribution lists
 * are per shard): out->schur_contribs = landmark-pair terms THIS shard sums, *odom_contribs_out = its odometry terms.
 * Over all ranks both add up to the unsharded counts. */
int tsgo_amg_probe_shard(const tsgo_graph* g, int32_t rank, int32_t world, tsgo_amg_info* out, int64_t* odom_contribs_out);

/* ---- host-only: the spanning tree of tsgo_init_estimates alone ------------------------------------------
 * Per vertex in tsgo_graph order: the parent's position in the vertex arrays, the input edge that joins them (-1 for roots and for
 * landmarks) and the depth (0 for roots, -1 for landmarks); any output may be NULL.  stats receives roots_fixed, roots_free, edges_usable,
 * tree_edges, depth_max and rounds = ceil(log2(depth_max + 1)); its other fields are 0.  Reads v_id, v_type, e_type, e_ids and fixed only. */
int tsgo_init_tree(const tsgo_graph* g, const uint8_t* odom_mask, int64_t n_mask,
                   int32_t* parent_out, int32_t* edge_out, int32_t* depth_out, tsgo_init_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* TSGO_H */
