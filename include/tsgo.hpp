// tsgo.hpp — header-only C++ host side above the C ABI (tsgo.h), shaped like the reference's own in-process
// interfaces so that code written against ToySlam's classes reads the same:
//
//   reference (remote/…)                                        here (namespace tsgo)
//   graph/vertex/VertexType.h:3-7   enum class VertexType       VertexType { Se2 = 0, Point2 = 1 }
//   graph/edge/EdgeType.h:3-7       enum class EdgeType         EdgeType   { Se2 = 0, Se2Point2 = 1 }
//   graph/GraphCpu.h:15-28          AddVertex / AddEdge /       Graph::AddVertex / AddEdge / FixVertex
//                                   FixVertex                   (values instead of unique_ptr<BaseVertexCpu<T>>)
//   graph/GraphCpu.h:45-53          GetVertex(id)               Graph::GetVertex(id) -> (x, y, theta) / (x, y, 0)
//   optimizer/IOptimizer.h:10-26    IOptimizer(iterations,      OptimizerHip(iterations[, config]);
//                                   solver); Optimize(IGraph*)  Optimize(Graph*)  — graph mutated in place, errors
//                                                               printed and the call returns early (OptimizerCpu.h style)
//
// The solver argument of the reference's optimizers has no counterpart: the implicit-Schur PCG is part of the
// library (SolverEigen.h:20 is what it replaces).  Nothing here touches the device directly; link libtsgo_hip.so.
#pragma once

#include <cmath>
#include <cstdint>
#include <iostream>
#include <stdexcept>
#include <unordered_map>
#include <vector>

#include "tsgo.h"

namespace tsgo {

enum class VertexType : uint32_t { Se2 = 0, Point2 = 1 };
// 2, 3, 4: behind the C ABI only (include/tsgo.h), not in the reference's enum
enum class EdgeType : uint32_t { Se2 = 0, Se2Point2 = 1, Se2VirtualPoint2 = 2, Se2Prior = 3, Point2Prior = 4 };

class Graph {
public:
    // Se2: (x, y, theta); Point2: (x, y).  Same role as Functions::CreateVertex + GraphCpu::AddVertex
    // (remote/serialization/DeserializeGraphFuncCpu.h:14-25, GraphCpu.h:15-18).
    void AddVertex(unsigned id, VertexType type, double x, double y, double theta = 0.0) {
        if (index.count(id)) throw std::invalid_argument("AddVertex: duplicate vertex id");
        index[id] = v_id.size();
        v_id.push_back(id); v_type.push_back((uint32_t)type);
        v_pos.push_back(x); v_pos.push_back(y); v_pos.push_back(type == VertexType::Se2 ? theta : 0.0);
    }
    // ODOM edge: measurement = relative pose (x, y, theta) — the 3x3 transform of EdgeSe2.h:23-38 is built here as
    // remote/graph/Helper.h:6-19 does; information = its diagonal (the only form the wire carries, DeserializeGraph.h:123-147).
    void AddEdgeSe2(unsigned id1, unsigned id2, double mx, double my, double mtheta, double w0, double w1, double w2) {
        const double c = std::cos(mtheta), s = std::sin(mtheta);
        const double m[9] = {c, -s, mx, s, c, my, 0, 0, 1};
        push_edge(EdgeType::Se2, id1, id2, m, w0, w1, w2);
    }
    // LM edge: measurement = (range, bearing) (EdgeSe2Point2d.h:34-35); information = diag(w0, w1).
    void AddEdgeSe2Point2(unsigned id_pose, unsigned id_landmark, double range, double bearing, double w0, double w1) {
        const double m[9] = {range, bearing, 0, 0, 0, 0, 0, 0, 0};
        push_edge(EdgeType::Se2Point2, id_pose, id_landmark, m, w0, w1, 0.0);
    }
    // Virtual landmark measurement (README.md:53; python/optimizer/edges2d.py:83-121): the same physical point seen from two poses as
    // (range, bearing) each; information = diag(w0, w1).  No wire encoding exists for it.
    void AddEdgeVirtualLandmark(unsigned id_pose_1, unsigned id_pose_2, double range1, double bearing1, double range2, double bearing2, double w0, double w1) {
        const double m[9] = {range1, bearing1, range2, bearing2, 0, 0, 0, 0, 0};
        push_edge(EdgeType::Se2VirtualPoint2, id_pose_1, id_pose_2, m, w0, w1, 0.0);
    }
    // Pose prior (edge type 3): an absolute measurement (x, y, theta) of pose `id` in the world frame, information = diag(w0, w1, w2).
    void AddEdgePosePrior(unsigned id, double x, double y, double theta, double w0, double w1, double w2) {
        const double m[9] = {x, y, theta, 0, 0, 0, 0, 0, 0};
        push_edge(EdgeType::Se2Prior, id, id, m, w0, w1, w2);
    }
    // Landmark prior (edge type 4): an absolute position (x, y) of landmark `id`, information = diag(w0, w1).
    void AddEdgeLandmarkPrior(unsigned id, double x, double y, double w0, double w1) {
        const double m[9] = {x, y, 0, 0, 0, 0, 0, 0, 0};
        push_edge(EdgeType::Point2Prior, id, id, m, w0, w1, 0.0);
    }
    // generic form, same argument meaning as Functions::CreateEdge(type, id1, id2, meas, inf)
    // (DeserializeGraphFuncCpu.h:27-38): meas = 9 doubles row-major (ODOM) or (range, bearing, 0...) (LM)
    void AddEdge(EdgeType type, unsigned id1, unsigned id2, const double meas[9], const double inf_diag[3]) {
        push_edge(type, id1, id2, meas, inf_diag[0], inf_diag[1], inf_diag[2]);
    }
    void FixVertex(unsigned id) { fixed.push_back(id); }                                 // GraphCpu.h:25-28

    struct Position { double x, y, theta; };
    Position GetVertex(unsigned id) const {                                              // GraphCpu.h:45-53 (.at throws)
        const size_t i = index.at(id);
        return {v_pos[3 * i], v_pos[3 * i + 1], v_pos[3 * i + 2]};
    }
    size_t VertexCount() const { return v_id.size(); }
    size_t EdgeCount() const { return e_type.size(); }
    const std::vector<unsigned>& GetFixedVertices() const { return fixed; }              // GraphCpu.h:40-43

    tsgo_graph View() const {
        return tsgo_graph{(int32_t)v_id.size(), v_id.data(), v_type.data(), v_pos.data(), (int32_t)e_type.size(), e_type.data(),
                          e_ids.data(), e_meas.data(), e_inf.data(), (int32_t)fixed.size(), fixed.data()};
    }
    void SetPositions(const std::vector<double>& xyt) { v_pos = xyt; }

private:
    void push_edge(EdgeType type, unsigned id1, unsigned id2, const double* m, double w0, double w1, double w2) {
        e_type.push_back((uint32_t)type); e_ids.push_back(id1); e_ids.push_back(id2);
        e_meas.insert(e_meas.end(), m, m + 9);
        e_inf.push_back(w0); e_inf.push_back(w1); e_inf.push_back(w2);
    }
    std::vector<uint32_t> v_id, v_type, e_type, e_ids, fixed;
    std::vector<double> v_pos, e_meas, e_inf;
    std::unordered_map<unsigned, size_t> index;
};

class OptimizerHip {
public:
    explicit OptimizerHip(unsigned iterations, const tsgo_config* config = nullptr) : iterations(iterations) {
        tsgo_config c;
        if (config) c = *config; else tsgo_default_config(&c);
        if (tsgo_create(&c, &handle)) throw std::runtime_error(tsgo_last_error());     // no device: fails loudly, no CPU path
    }
    ~OptimizerHip() { tsgo_destroy(handle); }
    OptimizerHip(const OptimizerHip&) = delete;
    OptimizerHip& operator=(const OptimizerHip&) = delete;

    // IOptimizer<T>::Optimize(IGraph*) (IOptimizer.h:21): in place, no return value; the reference prints and returns
    // on errors (OptimizerCpu.h:28-33) and prints its stop reason and "Summary() error" (:146,:169,:175,:182).
    void Optimize(Graph* graph) {
        if (!graph) return;
        const tsgo_graph g = graph->View();
        if (tsgo_set_graph(handle, &g) || tsgo_optimize(handle, (int)iterations, &stats)) { std::cout << tsgo_last_error() << std::endl; return; }
        std::vector<double> out(graph->VertexCount() * 3);
        if (tsgo_get_vertices(handle, out.data())) { std::cout << tsgo_last_error() << std::endl; return; }
        graph->SetPositions(out);
        if (stats.stop_reason == TSGO_STOP_WORSE) std::cout << "Error is getting worse\n";
        if (stats.stop_reason == TSGO_STOP_PLATEAU) std::cout << "Plateau: NO MORE OPT\n";
        if (stats.stop_reason == TSGO_STOP_CONVERGED) std::cout << "CONVERGED\n";
        if (stats.stop_reason == TSGO_STOP_DAMPING) std::cout << "Damping at its upper bound: no step lowers the error\n";      // rules = 2 only
        if (stats.stop_reason == TSGO_STOP_RADIUS) std::cout << "Trust region at its lower bound: no step lowers the error\n";      // rules = 3 only
        const int last = stats.iterations_run > 0 ? (stats.iterations_run < TSGO_MAX_TRACE ? stats.iterations_run : TSGO_MAX_TRACE) - 1 : 0;
        std::cout << "Summary() error = " << stats.chi2[last] << std::endl;
    }
    const tsgo_stats& Stats() const { return stats; }
    // Optimises the graph the handle HOLDS (SetGraph) without handing it over again, so that what was set on it since — SetEdgeRobust,
    // SetEdgeInformation, InitEstimates, SetFixed, SetEstimates — stays in force; `graph` (the one given to SetGraph) receives the positions.  Throws on an error.
    void OptimizeHeld(Graph* graph) {
        if (tsgo_optimize(handle, (int)iterations, &stats)) throw std::runtime_error(tsgo_last_error());
        if (!graph) return;
        std::vector<double> out(graph->VertexCount() * 3);
        if (tsgo_get_vertices(handle, out.data())) throw std::runtime_error(tsgo_last_error());
        graph->SetPositions(out);
    }
    // rules = 2 (Levenberg-Marquardt, tsgo_config.rules): what the last Optimize did trial by trial — Stats().lm_lambda / lm_gain / lm_pred /
    // lm_chi2_trial, entries 0 .. Stats().trace_len - 1 — and how many of its steps were rolled back
    int StepsRejected() const { return stats.steps_rejected; }
    bool StepAccepted(int trial) const { return trial >= 0 && trial < stats.trace_len && stats.lm_gain[trial] > 0 && stats.lm_pred[trial] > 0; }
    // A config for that loop: the defaults with rules = 2 and the analytic ODOM Jacobians it is meant to run with.
    static tsgo_config LevenbergMarquardtConfig(double lambda0 = 1e-3, double chi2_rel_tol = 1e-6) {
        tsgo_config c; tsgo_default_config(&c);
        c.rules = 2; c.odom_jacobian = 1; c.lm_lambda0 = lambda0; c.lm_chi2_rel_tol = chi2_rel_tol;
        return c;
    }

    // rules = 3 (Powell's dogleg, tsgo_config.rules): a config for that loop — the defaults with rules = 3 and the analytic ODOM Jacobians — and
    // its parameters, which belong to the handle (tsgo_set_dogleg; DefaultDogleg() adjusted).  SetDogleg throws on an error (a non-finite value,
    // radii outside 0 < radius_min <= radius0 <= radius_max, chi2_rel_tol < 0).  DoglegTrace: what the last Optimize did trial by trial (kind,
    // solved, radius, step_norm and the four scalars; trials - solves of them reused a solve); StepsRejected / StepAccepted serve this loop too.
    static tsgo_config DoglegConfig() {
        tsgo_config c; tsgo_default_config(&c);
        c.rules = 3; c.odom_jacobian = 1;
        return c;
    }
    static tsgo_dogleg_params DefaultDogleg() { tsgo_dogleg_params p; tsgo_default_dogleg(&p); return p; }
    void SetDogleg(const tsgo_dogleg_params& params) {
        if (tsgo_set_dogleg(handle, &params)) throw std::runtime_error(tsgo_last_error());
    }
    tsgo_dogleg_params Dogleg() const {
        tsgo_dogleg_params p;
        if (tsgo_get_dogleg(handle, &p)) throw std::runtime_error(tsgo_last_error());
        return p;
    }
    tsgo_dogleg_trace DoglegTrace() const {
        tsgo_dogleg_trace t;
        if (tsgo_get_dogleg_trace(handle, &t)) throw std::runtime_error(tsgo_last_error());
        return t;
    }

    // Robust kernel of one edge class (tsgo_set_robust): kernel = TSGO_ROBUST_*, delta its width (ignored by TSGO_ROBUST_NONE); the other
    // classes keep what the handle has.  Takes effect at the next Optimize.  Throws on an error (unknown kernel, delta out of range).
    void SetRobust(EdgeType edge_class, int kernel, double delta = 1.5) {
        tsgo_robust r;
        if (tsgo_get_robust(handle, &r)) throw std::runtime_error(tsgo_last_error());
        r.kernel[(uint32_t)edge_class] = kernel; r.delta[(uint32_t)edge_class] = delta;
        SetRobust(r);
    }
    void SetRobust(const tsgo_robust& setting) {
        if (tsgo_set_robust(handle, &setting)) throw std::runtime_error(tsgo_last_error());
    }
    tsgo_robust Robust() const {
        tsgo_robust r;
        if (tsgo_get_robust(handle, &r)) throw std::runtime_error(tsgo_last_error());
        return r;
    }

    // Robust kernels per EDGE of the graph the handle holds (tsgo_set_edge_robust): a palette of at most TSGO_EDGE_ROBUST_MAX entries and
    // one byte per edge in input order — 0: the edge keeps its class's kernel (SetRobust), k >= 1: palette[k - 1] whatever the class; an
    // entry with TSGO_ROBUST_NONE exempts its edges (the odometry chain, a surveyed beacon).  An empty palette with an empty mask clears.
    // The setting goes with the next SetGraph / Optimize(&graph).  Throws on an error (a mask of the wrong length, a value above the
    // palette's size, an unknown kernel, precision 32).
    void SetEdgeRobust(const std::vector<tsgo_edge_robust_entry>& palette, const std::vector<uint8_t>& entry_of_edge, tsgo_edge_robust_stats* stats = nullptr) {
        if (tsgo_set_edge_robust(handle, (int32_t)palette.size(), palette.empty() ? nullptr : palette.data(), entry_of_edge.empty() ? nullptr : entry_of_edge.data(),
                                 (int64_t)entry_of_edge.size(), stats))
            throw std::runtime_error(tsgo_last_error());
    }
    // ... read back: the palette, and (if asked for) the byte of every one of the graph's n_edges edges
    std::vector<tsgo_edge_robust_entry> EdgeRobust(size_t n_edges, std::vector<uint8_t>* entry_of_edge = nullptr) const {
        std::vector<tsgo_edge_robust_entry> palette(TSGO_EDGE_ROBUST_MAX);
        std::vector<uint8_t> mask(n_edges);
        int32_t n = 0;
        if (tsgo_get_edge_robust(handle, &n, palette.data(), mask.data(), (int64_t)n_edges)) throw std::runtime_error(tsgo_last_error());
        palette.resize((size_t)n);
        if (entry_of_edge) entry_of_edge->swap(mask);
        return palette;
    }

    // Marginal covariances at the estimates of the last Optimize (tsgo_marginals): 9 doubles per id, row-major; a landmark's 2x2 block
    // in the leading 2x2.  Throws on an error (unknown id, no fixed vertex, no graph yet, precision 32).
    std::vector<double> Marginals(const std::vector<uint32_t>& ids) {
        std::vector<double> cov(ids.size() * 9);
        if (tsgo_marginals(handle, ids.data(), (int32_t)ids.size(), 0.0, cov.data(), nullptr)) throw std::runtime_error(tsgo_last_error());
        return cov;
    }

    // Joint marginal covariance of the vertices `ids` (tsgo_joint_marginals): D x D doubles, row-major, rows and columns in query order,
    // 3 per pose and 2 per landmark; *dim (if given) receives D.  Throws on an error (those of Marginals, and D > 8192).
    std::vector<double> JointMarginals(const std::vector<uint32_t>& ids, int* dim = nullptr) {
        int32_t d = 0;
        if (tsgo_joint_marginals(handle, ids.data(), (int32_t)ids.size(), 0.0, nullptr, 0, &d, nullptr)) throw std::runtime_error(tsgo_last_error());
        std::vector<double> cov((size_t)d * (size_t)d);
        if (d > 0 && tsgo_joint_marginals(handle, ids.data(), (int32_t)ids.size(), 0.0, cov.data(), (int64_t)cov.size(), &d, nullptr))
            throw std::runtime_error(tsgo_last_error());
        if (dim) *dim = d;
        return cov;
    }

    // Posterior samples and the marginal covariance of every vertex (tsgo_sample_marginals): 9 doubles per vertex of the graph last handed
    // to Optimize or SetGraph, in its vertex order, in the format of Marginals, estimated from n_samples perturb-and-MAP samples (relative
    // standard error sqrt(2 / n_samples) on a variance); *samples (if given) receives them, [n_samples][vertices][3].  Throws on an error
    // (those of Marginals, n_samples outside 1 .. 65536).
    std::vector<double> SampleMarginals(size_t n_vertices, int n_samples, uint64_t seed = 0, std::vector<double>* samples = nullptr, tsgo_sample_stats* stats = nullptr) {
        std::vector<double> cov(n_vertices * 9);
        if (samples) samples->assign((size_t)(n_samples > 0 ? n_samples : 0) * n_vertices * 3, 0.0);
        if (tsgo_sample_marginals(handle, n_samples, seed, 0.0, cov.data(), (int64_t)n_vertices, samples ? samples->data() : nullptr,
                                  samples ? (int64_t)samples->size() : 0, stats))
            throw std::runtime_error(tsgo_last_error());
        return cov;
    }

    // Leverage of every edge from posterior samples (tsgo_edge_leverage): eight doubles per edge of the graph last handed to Optimize or
    // SetGraph, in its edge order: (c00, c01, c02, c11, c12, c22, h, dof_a) — C = J Sigma J^T of the predicted measurement, h = tr(Omega_a C),
    // the number of weighted axes; the redundancy is dof_a - h.  Estimated from n_samples samples (relative standard error
    // sqrt(2 / n_samples) on a diagonal entry of C).  *stats (if given): the per-class sums and the trace.  Throws on an error (those of
    // SampleMarginals).
    std::vector<double> EdgeLeverage(size_t n_edges, int n_samples, uint64_t seed = 0, tsgo_leverage_stats* stats = nullptr) {
        std::vector<double> rec(n_edges * 8);
        double none[8];
        if (tsgo_edge_leverage(handle, n_samples, seed, 0.0, rec.empty() ? none : rec.data(), (int64_t)n_edges, stats)) throw std::runtime_error(tsgo_last_error());
        return rec;
    }

    // Per-edge residual report at the current estimates (tsgo_edge_report): six doubles per edge of the graph last handed to Optimize, in
    // its edge order: (e0, e1, e2, s, rho, w); *stats (if given) receives the per-class summary.  EdgeSummary: the summary alone (no per-edge
    // buffer anywhere).  Both throw on an error (no graph yet, an edge-sharded handle).
    std::vector<double> EdgeReport(tsgo_edge_report_stats* stats = nullptr) {
        tsgo_edge_report_stats s;
        if (tsgo_edge_report(handle, nullptr, 0, &s)) throw std::runtime_error(tsgo_last_error());
        int64_t n = 0;
        for (const tsgo_edge_class_summary& c : s.cls) n += c.edges;
        std::vector<double> rec((size_t)n * 6);
        if (tsgo_edge_report(handle, rec.empty() ? nullptr : rec.data(), n, &s)) throw std::runtime_error(tsgo_last_error());
        if (stats) *stats = s;
        return rec;
    }
    tsgo_edge_report_stats EdgeSummary() {
        tsgo_edge_report_stats s;
        if (tsgo_edge_report(handle, nullptr, 0, &s)) throw std::runtime_error(tsgo_last_error());
        return s;
    }

    // Mahalanobis gate of candidate edges (tsgo_gate_edges): the EDGES of `candidates` (its vertices are ignored; the ids refer to the
    // graph last handed to Optimize) against the joint marginal of their vertices.  Eight doubles per candidate, in its edge order:
    // (e0, e1, e2, s, d2, dof, logdet, status); *innovation (if given) receives S, 9 doubles per candidate.  Nothing is added to the graph.
    // Throws on an error (those of Marginals, a candidate that is not a valid edge of the graph's vertices).
    std::vector<double> GateEdges(const Graph& candidates, std::vector<double>* innovation = nullptr, tsgo_gate_stats* stats = nullptr) {
        const tsgo_graph c = candidates.View();
        std::vector<double> rec((size_t)c.n_edges * 8);
        if (innovation) innovation->assign((size_t)c.n_edges * 9, 0.0);
        if (tsgo_gate_edges(handle, c.n_edges, c.e_type, c.e_ids, c.e_meas, c.e_inf, 0.0, rec.data(), innovation ? innovation->data() : nullptr, stats))
            throw std::runtime_error(tsgo_last_error());
        return rec;
    }

    // Initial estimates from an odometry spanning tree (tsgo_init_estimates), for the graph last handed to Optimize or SetGraph: poses
    // composed along the tree from the fixed poses, landmarks as the mean of their observations.  what: TSGO_INIT_POSES | TSGO_INIT_LANDMARKS
    // (0 = both); odom_mask: empty = every ODOM edge may enter the tree, otherwise one byte per edge of the graph.  The graph's positions are
    // updated in place when `graph` is given.  Throws on an error (no graph yet, a mask of the wrong length, precision 32).
    tsgo_init_stats InitEstimates(Graph* graph = nullptr, int what = 0, const std::vector<uint8_t>& odom_mask = std::vector<uint8_t>()) {
        tsgo_init_stats s;
        if (tsgo_init_estimates(handle, what, odom_mask.empty() ? nullptr : odom_mask.data(), (int64_t)odom_mask.size(), &s)) throw std::runtime_error(tsgo_last_error());
        if (graph) {
            std::vector<double> out(graph->VertexCount() * 3);
            if (tsgo_get_vertices(handle, out.data())) throw std::runtime_error(tsgo_last_error());
            graph->SetPositions(out);
        }
        return s;
    }
    // Edit edge weights in place (tsgo_set_edge_information): `edges` are positions in the edge order of the graph last handed to Optimize or
    // SetGraph (the numbering of EdgeReport), `inf` three doubles per listed edge; an empty `edges` with 3 * EdgeCount values is "every edge
    // in order".  Zeros switch an edge off.  The estimates and the robust setting stay; the next Optimize(graph) or SetGraph replaces every
    // weight with what the graph carries.  EdgeInformation: what the handle holds now, three doubles per edge.  Both throw on an error (no
    // graph yet, an index out of range or listed twice, a negative or non-finite value, an edge-sharded handle).
    void SetEdgeInformation(const std::vector<int64_t>& edges, const std::vector<double>& inf, tsgo_edge_info_stats* stats = nullptr) {
        if (!edges.empty() && inf.size() != edges.size() * 3) throw std::runtime_error("SetEdgeInformation: three values per listed edge");
        if (tsgo_set_edge_information(handle, (int64_t)(inf.size() / 3), edges.empty() ? nullptr : edges.data(), inf.empty() ? nullptr : inf.data(), stats))
            throw std::runtime_error(tsgo_last_error());
    }
    std::vector<double> EdgeInformation() {
        tsgo_edge_report_stats s;
        if (tsgo_edge_report(handle, nullptr, 0, &s)) throw std::runtime_error(tsgo_last_error());
        int64_t n = 0;
        for (const tsgo_edge_class_summary& c : s.cls) n += c.edges;
        std::vector<double> inf((size_t)n * 3);
        if (tsgo_get_edge_information(handle, inf.empty() ? nullptr : inf.data(), n)) throw std::runtime_error(tsgo_last_error());
        return inf;
    }
    // Edit vertices in place (tsgo_set_fixed, tsgo_set_estimates) on the graph last handed to Optimize or SetGraph.  SetFixed: `counts` is the
    // multiplicity of each listed id in the fixed list (empty: 1 each; 0 releases), unlisted vertices keep theirs; Release: count 0 for the
    // listed ids; FixedCounts: what the handle holds now, one per vertex in the graph's vertex order.  SetEstimates: three doubles (x, y,
    // theta) per listed id, a landmark's third is ignored; an empty `ids` with 3 * VertexCount values is "every vertex in order".  The other
    // estimates, weight edits and robust settings stay; run OptimizeHeld afterwards — Optimize(graph) or SetGraph installs the list and the
    // positions the graph carries.  All throw on an error (no graph yet, an unknown id or one listed twice, a count outside [0, 65535], a
    // non-finite estimate, an edge-sharded handle).
    void SetFixed(const std::vector<uint32_t>& ids, const std::vector<int32_t>& counts = std::vector<int32_t>(), tsgo_vertex_edit_stats* stats = nullptr) {
        if (!counts.empty() && counts.size() != ids.size()) throw std::runtime_error("SetFixed: one count per listed id");
        if (tsgo_set_fixed(handle, (int64_t)ids.size(), ids.empty() ? nullptr : ids.data(), counts.empty() ? nullptr : counts.data(), stats))
            throw std::runtime_error(tsgo_last_error());
    }
    void Release(const std::vector<uint32_t>& ids, tsgo_vertex_edit_stats* stats = nullptr) { SetFixed(ids, std::vector<int32_t>(ids.size(), 0), stats); }
    std::vector<int32_t> FixedCounts(size_t n_vertices) const {
        std::vector<int32_t> counts(n_vertices);
        if (tsgo_get_fixed(handle, counts.empty() ? nullptr : counts.data(), (int64_t)n_vertices)) throw std::runtime_error(tsgo_last_error());
        return counts;
    }
    void SetEstimates(const std::vector<uint32_t>& ids, const std::vector<double>& xyt, tsgo_vertex_edit_stats* stats = nullptr) {
        if (!ids.empty() && xyt.size() != ids.size() * 3) throw std::runtime_error("SetEstimates: three values per listed id");
        if (tsgo_set_estimates(handle, (int64_t)(xyt.size() / 3), ids.empty() ? nullptr : ids.data(), xyt.empty() ? nullptr : xyt.data(), stats))
            throw std::runtime_error(tsgo_last_error());
    }
    // Graduated non-convexity, truncated least squares (tsgo_gnc), on the graph last handed to Optimize or SetGraph: rounds of on-device
    // reweighting and Optimize-style inner runs under the handle's own rules and robust setting (textbook GNC: SetRobust NONE on every
    // class first).  params: DefaultGnc() adjusted; subject: empty = every edge of a class with barc2 > 0, otherwise one byte per edge
    // (nonzero = may be down-weighted; the others are known inliers).  Returns the last round's weight of every edge (1 for exempt ones);
    // the graph's positions are updated in place when `graph` is given.  Throws on an error (no graph yet, a mask of the wrong length, a
    // parameter out of range, no subject edge, precision 32, an edge-sharded handle).
    static tsgo_gnc_params DefaultGnc() { tsgo_gnc_params p; tsgo_default_gnc(&p); return p; }
    std::vector<double> Gnc(const tsgo_gnc_params& params, const std::vector<uint8_t>& subject = std::vector<uint8_t>(), Graph* graph = nullptr,
                            tsgo_gnc_stats* stats = nullptr) {
        tsgo_edge_report_stats s;
        if (tsgo_edge_report(handle, nullptr, 0, &s)) throw std::runtime_error(tsgo_last_error());
        int64_t n = 0;
        for (const tsgo_edge_class_summary& c : s.cls) n += c.edges;
        std::vector<double> w((size_t)n, 1.0);
        if (tsgo_gnc(handle, &params, subject.empty() ? nullptr : subject.data(), (int64_t)subject.size(), w.empty() ? nullptr : w.data(), n, stats))
            throw std::runtime_error(tsgo_last_error());
        if (graph) {
            std::vector<double> out(graph->VertexCount() * 3);
            if (tsgo_get_vertices(handle, out.data())) throw std::runtime_error(tsgo_last_error());
            graph->SetPositions(out);
        }
        return w;
    }
    // Max-mixture edges (tsgo_max_mixture) on the graph last handed to Optimize or SetGraph: `groups` lists, per measurement, the input edge
    // indices of its alternatives; exactly one of each group is switched on (the cheapest at the current estimates), the others are held at
    // information 0, and rounds of selection and Optimize-style inner runs follow until no group changes.  params: DefaultMixture()
    // adjusted; log_weight: empty = 0, otherwise one value per member in the order of `groups`.  Returns the selected position of every
    // group; the graph's positions are updated in place when `graph` is given.  Throws on an error (no graph yet, an edge outside the
    // graph or listed twice, an empty or too long group, members of different dof, a member without information, a parameter out of
    // range, precision 32, an edge-sharded handle).
    static tsgo_mixture_params DefaultMixture() { tsgo_mixture_params p; tsgo_default_mixture(&p); return p; }
    std::vector<int32_t> MaxMixture(const tsgo_mixture_params& params, const std::vector<std::vector<int64_t>>& groups,
                                    const std::vector<double>& log_weight = std::vector<double>(), Graph* graph = nullptr, tsgo_mixture_stats* stats = nullptr) {
        std::vector<int64_t> off(1, 0), member;
        for (const std::vector<int64_t>& g : groups) { member.insert(member.end(), g.begin(), g.end()); off.push_back((int64_t)member.size()); }
        if (!log_weight.empty() && log_weight.size() != member.size()) throw std::runtime_error("MaxMixture: one log_weight per member");
        std::vector<int32_t> sel(groups.size());
        if (tsgo_max_mixture(handle, &params, (int64_t)groups.size(), off.data(), member.empty() ? nullptr : member.data(), log_weight.empty() ? nullptr : log_weight.data(),
                             sel.empty() ? nullptr : sel.data(), (int64_t)sel.size(), nullptr, 0, stats))
            throw std::runtime_error(tsgo_last_error());
        if (graph) {
            std::vector<double> out(graph->VertexCount() * 3);
            if (tsgo_get_vertices(handle, out.data())) throw std::runtime_error(tsgo_last_error());
            graph->SetPositions(out);
        }
        return sel;
    }
    // Hands the graph to the handle without optimising it (what InitEstimates, EdgeReport or GateEdges need before a first Optimize).
    void SetGraph(const Graph& graph) {
        const tsgo_graph g = graph.View();
        if (tsgo_set_graph(handle, &g)) throw std::runtime_error(tsgo_last_error());
    }

private:
    unsigned iterations;
    tsgo_optimizer* handle = nullptr;
    tsgo_stats stats{};
};

}  // namespace tsgo
