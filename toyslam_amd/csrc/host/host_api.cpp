// host_api.cpp — host-only C-ABI entry points that need no GPU (see include/tsgo.h).
#include "../../../include/tsgo.h"
#include "errors.h"
#include "problem.h"
#include "amg.h"
#include "init_tree.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>      // (this file is also compiled into the device library: TSGO_HD of tsgo_math.h then needs the runtime's attributes)
#endif
#include "../tsgo_math.h"         // noise(): philox4x32_10, box_muller
#include <algorithm>
#include <chrono>
#include <cstring>

extern "C" void tsgo_default_config(tsgo_config* c) {
    if (!c) return;
    c->device = 0; c->precision = 64; c->pcg_rel_tol = 1e-10; c->pcg_max_iters = 20000;
    c->lanes_per_pose = 0; c->lanes_per_lm = 0; c->use_graphs = 2; c->rank = 0; c->world = 1; c->verbose = 0; c->preconditioner = 1; c->xcd_map = 1; c->warm_start = 6; c->odom_jacobian = 0; c->reuse_structure = 1; c->rules = 0; c->lr = 0.2; c->cycle_level0 = 0; c->cycle_storage = 16; c->warm_requests = 0;
    c->lm_lambda0 = 1e-3; c->lm_chi2_rel_tol = 1e-6;
}

extern "C" void tsgo_default_robust(tsgo_robust* r) {
    if (!r) return;
    for (int k = 0; k < 5; ++k) { r->kernel[k] = TSGO_ROBUST_HUBER; r->delta[k] = 1.5; }
    r->reserved = 0;
}

extern "C" void tsgo_default_dogleg(tsgo_dogleg_params* p) {
    if (!p) return;
    p->radius0 = 1e4; p->radius_min = 1e-9; p->radius_max = 1e9; p->chi2_rel_tol = 1e-6;
}

extern "C" void tsgo_default_gnc(tsgo_gnc_params* p) {
    if (!p) return;
    static const double quantile99[5] = {11.345, 9.210, 9.210, 11.345, 9.210};      // chi^2, 3 dof (types 0, 3) and 2 dof (types 1, 2, 4)
    for (int k = 0; k < 5; ++k) p->barc2[k] = quantile99[k];
    p->mu_step = 1.4; p->rounds_max = 64; p->inner_iterations = 10; p->keep_weights = 1; p->reserved = 0;
}

extern "C" void tsgo_default_mixture(tsgo_mixture_params* p) {
    if (!p) return;
    p->rounds_max = 32; p->inner_iterations = 5; p->keep_selection = 1; p->reserved = 0;
}

extern "C" void tsgo_sample_noise(uint64_t seed, uint32_t tag, uint32_t index, uint32_t sample, uint32_t words_out[4], double normals_out[4]) {
    const tsgo::Philox4 p = tsgo::philox4x32_10(index, tag, sample, 0u, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32));
    if (words_out) for (int k = 0; k < 4; ++k) words_out[k] = p.r[k];
    if (normals_out) { tsgo::box_muller(p.r[0], p.r[1], normals_out[0], normals_out[1]); tsgo::box_muller(p.r[2], p.r[3], normals_out[2], normals_out[3]); }
}

extern "C" int tsgo_layout_probe(const tsgo_graph* g, int32_t rank, int32_t world, int32_t lanes_per_pose,
                                 int32_t lanes_per_lm, tsgo_layout_info* out) {
    if (!g || !out) return tsgo::set_error(-1, "tsgo_layout_probe: null argument");
    tsgo::Problem pr;
    tsgo::BuildOptions bo; bo.rank = rank; bo.world = world; bo.lanes_per_pose = lanes_per_pose; bo.lanes_per_lm = lanes_per_lm;
    const std::string err = tsgo::build_problem(*g, bo, pr);
    if (!err.empty()) return tsgo::set_error(-2, err);
    out->n_pose = pr.P; out->n_lm_local = pr.L; out->n_lm_total = pr.L_total; out->n_lm_edges_local = pr.n_lm_edges;
    int64_t od = 0; for (uint32_t e : pr.odom.edge) od += e != tsgo::kNoEdge;
    out->n_odom_slots = od;
    out->rows_by_pose = (int64_t)pr.by_pose.rows; out->rows_by_lm = (int64_t)pr.by_lm.rows; out->rows_odom = (int64_t)pr.odom.rows;
    out->lanes_per_pose = pr.by_pose.G; out->lanes_per_lm = pr.by_lm.G;
    out->lm_first = pr.lm_first; out->lm_last = pr.lm_last; out->pose_first = pr.pose_first; out->pose_last = pr.pose_last;
    return 0;
}

static int amg_probe(const tsgo_graph* g, int rank, int world, tsgo_amg_info* out, int64_t* odom_out) {
    std::memset(out, 0, sizeof(*out));
    tsgo::Problem pr; tsgo::BuildOptions bo; bo.rank = rank; bo.world = world;
    auto t0 = std::chrono::steady_clock::now();
    std::string err = tsgo::build_problem(*g, bo, pr);
    if (!err.empty()) return tsgo::set_error(-2, err);
    auto t1 = std::chrono::steady_clock::now();
    tsgo::AmgSym amg;
    err = world > 1 ? tsgo::build_amg_sharded(*g, pr, amg) : tsgo::build_amg(pr, amg);
    if (!err.empty()) return tsgo::set_error(-2, err);
    auto t2 = std::chrono::steady_clock::now();
    out->ms_layout = std::chrono::duration<double, std::milli>(t1 - t0).count();
    out->ms_symbolic = std::chrono::duration<double, std::milli>(t2 - t1).count();
    int n = 0;
    for (const auto& L : amg.levels) if (n < 8) {
        out->rows[n] = L.n; out->blocks[n] = L.A.nnz(); out->p_blocks[n] = L.P.nnz();
        std::vector<int> cnt(L.n_agg, 0);
        for (int a : L.agg) ++cnt[a];
        out->agg_min[n] = cnt.empty() ? 0 : *std::min_element(cnt.begin(), cnt.end());
        out->agg_max[n] = cnt.empty() ? 0 : *std::max_element(cnt.begin(), cnt.end());
        ++n;
    }
    if (n < 8) { out->rows[n] = amg.A_last.n_rows; out->blocks[n] = amg.A_last.nnz(); ++n; }
    out->n_levels = n;
    out->schur_contribs = (int64_t)amg.schur.slot_i.size();
    if (odom_out) *odom_out = (int64_t)amg.schur.od_slot.size();
    out->checksum = tsgo::amg_checksum(pr, amg);
    return 0;
}

extern "C" int tsgo_amg_probe(const tsgo_graph* g, tsgo_amg_info* out) {
    if (!g || !out) return tsgo::set_error(-1, "tsgo_amg_probe: null argument");
    return amg_probe(g, 0, 1, out, nullptr);
}

extern "C" int tsgo_amg_probe_shard(const tsgo_graph* g, int32_t rank, int32_t world, tsgo_amg_info* out, int64_t* odom_contribs_out) {
    if (!g || !out || world < 1 || rank < 0 || rank >= world) return tsgo::set_error(-1, "tsgo_amg_probe_shard: bad argument");
    return amg_probe(g, rank, world, out, odom_contribs_out);
}

extern "C" int tsgo_init_tree(const tsgo_graph* g, const uint8_t* odom_mask, int64_t n_mask, int32_t* parent_out, int32_t* edge_out, int32_t* depth_out,
                              tsgo_init_stats* stats) {
    if (!g) return tsgo::set_error(-1, "tsgo_init_tree: null argument");
    tsgo::InitTree t;
    const std::string err = tsgo::build_init_tree(*g, odom_mask, n_mask, t);
    if (!err.empty()) return tsgo::set_error(-2, "tsgo_init_tree: " + err);
    const size_t n = (size_t)g->n_vertices;
    if (parent_out && n) std::memcpy(parent_out, t.parent.data(), n * sizeof(int32_t));
    if (edge_out && n) std::memcpy(edge_out, t.edge.data(), n * sizeof(int32_t));
    if (depth_out && n) std::memcpy(depth_out, t.depth.data(), n * sizeof(int32_t));
    if (stats) {      // the tree's own counts; what only a device call knows stays 0
        std::memset(stats, 0, sizeof(*stats));
        stats->roots_fixed = t.roots_fixed; stats->roots_free = t.roots_free; stats->edges_usable = t.edges_usable; stats->tree_edges = t.tree_edges;
        stats->depth_max = t.depth_max; stats->rounds = t.rounds();
    }
    return 0;
}
