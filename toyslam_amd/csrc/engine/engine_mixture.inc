// engine/engine_mixture.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// tsgo_max_mixture.  Max-mixture edges (Olson and Agarwal 2013; DESIGN.md section 24): groups of alternative edges of which exactly one is
// switched on.  Per pass two launches (tsgo_mixture_kernels.h): k_mix_cost — the once-per-edge walk of tsgo_edge_walk.h, the cost of every
// member at the current estimates — and k_mix_select — a thread per group: the cheapest member, base to the winner and 0 to the others in
// the slots the edit knows.  Then the handle's own optimize().  Per pass one MixPartial per workgroup comes back; the selection and the
// costs cross the bus once, at the end.
//
// Buffers: the report's slot -> edge maps and the edit's edge -> slot map (StructureMaps) and one allocation that lives for the call — the
// base information (3 doubles per edge, taken with k_get_edge_inf; k_mix_members gathers the members' rows for the host, which checks them
// and makes the constants k: 24 B per member cross the bus, not 24 B per edge), member_of, k, the group arrays, the costs, the selection,
// the partials.  A handle that never calls tsgo_max_mixture launches what it launched before.
//
// State: a pass that moved a selection ends as tsgo_set_edge_information does (mem.hier_age = -1: the next linearisation builds a fresh
// hierarchy; the warm start's history and the robust settings stay); a pass that moved none wrote nothing and invalidates nothing.
// pri_p_w follows the pose priors' weights when the call returns.  An inner run that fails with an error code (< 0, not TSGO_STOP_SOLVER)
// ends the call with that code at once: the tables then hold the last selection, whatever keep_selection says.
    void launch_mix_cost(const MixArgs& ma) {
        if constexpr (sizeof(T) == 8) {
            if (report_lm_priors()) pick<1, 2, 4, 8>(pr.by_lm.G, [&](auto g) {
                launch(k_mix_cost_lm_prior<T, g>, nbL, tl, (const T*)lmrec, (const uint32_t*)maps.rep_pl_edge, lm_prior_args(), ma);
            });
            pick_edge_walk([&](auto g, auto general, auto pri) {
                launch(k_mix_cost<T, g, general, pri>, nbP, tp, to, (const T*)ps, (const T*)lmrec, maps.edge_maps(), pri ? pose_prior_args() : no_priors(), ma);
            });
        }
    }

    int max_mixture(const tsgo_mixture_params& p, int64_t n_groups, const int64_t* group_off, const int64_t* member_edge, const double* log_weight,
                    int32_t* selected_out, int64_t cap_groups, double* cost_out, int64_t cap_members, tsgo_mixture_stats* st_out) override {
        const auto wall0 = std::chrono::steady_clock::now();
        auto ms_since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
        const std::string nm = "tsgo_max_mixture";
        if (sizeof(T) != 8) return set_error(-1, nm + ": needs precision = 64");
        if (cfg.world > 1 || collective()) return set_error(-1, nm + ": edge-sharded handles (world > 1) are not supported");
        if (!have_graph_data) return set_error(-3, nm + ": no graph set");
        if (p.rounds_max < 1 || p.rounds_max > TSGO_MIX_MAX_ROUNDS) return set_error(-1, nm + ": rounds_max = " + std::to_string(p.rounds_max) + " is outside [1, " + std::to_string(TSGO_MIX_MAX_ROUNDS) + "]");
        if (p.inner_iterations < 0) return set_error(-1, nm + ": inner_iterations = " + std::to_string(p.inner_iterations) + " is negative");
        if (p.keep_selection != 0 && p.keep_selection != 1) return set_error(-1, nm + ": keep_selection = " + std::to_string(p.keep_selection) + " must be 0 or 1");
        if (n_groups < 0) return set_error(-1, nm + ": n_groups = " + std::to_string(n_groups) + " is negative");
        tsgo_mixture_stats s; std::memset(&s, 0, sizeof(s));
        if (n_groups == 0) { if (st_out) *st_out = s; return 0; }
        if (!group_off || !member_edge) return set_error(-1, nm + ": group_off or member_edge is NULL with n_groups = " + std::to_string(n_groups));
        // ---- the lists: everything is checked before anything of the handle is written ----
        const size_t E = structure.e_type.size();
        const std::vector<uint32_t>& type = structure.e_type;
        if (group_off[0] != 0) return set_error(-1, nm + ": group_off[0] = " + std::to_string(group_off[0]) + " must be 0");
        if (n_groups > (int64_t)E) return set_error(-1, nm + ": " + std::to_string(n_groups) + " groups but the graph has " + std::to_string(E) + " edges: an edge is listed twice (member_edge)");
        for (int64_t g = 0; g < n_groups; ++g) {
            const int64_t n = group_off[g + 1] - group_off[g];
            if (n < 1) return set_error(-1, nm + ": group_off[" + std::to_string(g + 1) + "] = " + std::to_string(group_off[g + 1]) + " is not above group_off[" + std::to_string(g) + "]: every group has at least 1 member");
            if (n > TSGO_MIX_MAX_MEMBERS) return set_error(-1, nm + ": group " + std::to_string(g) + " has " + std::to_string(n) + " members (group_off), above TSGO_MIX_MAX_MEMBERS = " + std::to_string(TSGO_MIX_MAX_MEMBERS));
        }
        const int64_t M = group_off[n_groups];
        if (selected_out && cap_groups < n_groups) return set_error(-1, nm + ": cap_groups " + std::to_string(cap_groups) + " is below n_groups = " + std::to_string(n_groups));
        if (cost_out && cap_members < M) return set_error(-1, nm + ": cap_members " + std::to_string(cap_members) + " is below the " + std::to_string(M) + " members listed");
        if (edit_stamp.size() != E || edit_call == 0xFFFFFFFFu) { edit_stamp.assign(E, 0u); edit_call = 0; }
        ++edit_call;
        for (int64_t g = 0; g < n_groups; ++g)
            for (int64_t m = group_off[g]; m < group_off[g + 1]; ++m) {
                const int64_t e = member_edge[m];
                if (e < 0 || e >= (int64_t)E) return set_error(-1, nm + ": member_edge[" + std::to_string(m) + "] = " + std::to_string(e) + " is outside [0, " + std::to_string(E) + ")");
                if (edit_stamp[(size_t)e] == edit_call) return set_error(-1, nm + ": edge " + std::to_string(e) + " is listed twice (member_edge[" + std::to_string(m) + "]): an edge belongs to at most one group");
                edit_stamp[(size_t)e] = edit_call;
                const int64_t first = member_edge[group_off[g]];
                if (edit_axes(type[(size_t)e]) != edit_axes(type[(size_t)first]))
                    return set_error(-1, nm + ": member_edge[" + std::to_string(m) + "] = " + std::to_string(e) + " (type " + std::to_string(type[(size_t)e]) + ") and edge " + std::to_string(first) + " (type " +
                                             std::to_string(type[(size_t)first]) + ") of group " + std::to_string(g) + " differ in their degrees of freedom");
                if (log_weight && !std::isfinite(log_weight[m])) return set_error(-2, nm + ": log_weight[" + std::to_string(m) + "] = " + std::to_string(log_weight[m]) + " must be finite");
                ++s.members_by_class[type[(size_t)e]];
            }
        s.groups = n_groups; s.members = M;
        if constexpr (sizeof(T) == 8) {
            HIP_OK(hipSetDevice(cfg.device));
            if (int rc = report_prepare()) return rc;
            if (int rc = edit_prepare(nm)) return rc;
            const int nbG = grid_for((int)n_groups);
            CallScratch scratch; EventPair te;
            double *base_d = nullptr, *mb_d = nullptr, *k_d = nullptr, *cost_d = nullptr; uint32_t *member_of_d = nullptr, *off_d = nullptr, *edge_d = nullptr; int32_t* sel_d = nullptr; MixPartial* part_d = nullptr;
            scratch.want(&base_d, 24 * E); scratch.want(&mb_d, 24 * (size_t)M); scratch.want(&k_d, 8 * (size_t)M); scratch.want(&cost_d, 8 * (size_t)M); scratch.want(&member_of_d, 4 * E);
            scratch.want(&off_d, 4 * (size_t)(n_groups + 1)); scratch.want(&edge_d, 4 * (size_t)M); scratch.want(&sel_d, 4 * (size_t)n_groups); scratch.want(&part_d, (size_t)nbG * sizeof(MixPartial));
            if (int rc = scratch.commit()) return rc;
            if (int rc = te.create()) return rc;
            // ---- the lists go up; the base information is read out as tsgo_get_edge_information reads it and the members' rows come back
            // (reads of the tables and writes of this call's buffers: the handle is still as before) ----
            std::vector<uint32_t> off_host((size_t)n_groups + 1), edge_host((size_t)M);
            for (int64_t g = 0; g <= n_groups; ++g) off_host[(size_t)g] = (uint32_t)group_off[g];
            for (int64_t m = 0; m < M; ++m) edge_host[(size_t)m] = (uint32_t)member_edge[m];
            HIP_OK(hipMemcpyAsync(off_d, off_host.data(), 4 * off_host.size(), hipMemcpyHostToDevice, stream));
            HIP_OK(hipMemcpyAsync(edge_d, edge_host.data(), 4 * (size_t)M, hipMemcpyHostToDevice, stream));
            HIP_OK(hipMemsetAsync(member_of_d, 0xFF, 4 * E, stream));                // kNoMember
            HIP_OK(hipMemsetAsync(sel_d, 0xFF, 4 * (size_t)n_groups, stream));      // kMixNone
            launch(k_get_edge_inf<T>, grid_for((int)E), (int)E, (const uint32_t*)maps.edit_map, (const uint8_t*)maps.edit_cls, edit_tables(), base_d);
            launch(k_mix_members, grid_for((int)M), (int)M, (const uint32_t*)edge_d, (const double*)base_d, member_of_d, mb_d);
            HIP_OK(hipGetLastError());
            std::vector<double> mb(3 * (size_t)M), k_host((size_t)M);
            if (int rc = copy_sync(mb.data(), mb_d, 24 * (size_t)M, hipMemcpyDeviceToHost)) return rc;
            for (int64_t m = 0; m < M; ++m) {
                const size_t e = (size_t)member_edge[m];
                double ln = 0.0;
                for (int a = 0; a < edit_axes(type[e]); ++a) {
                    const double b = mb[3 * (size_t)m + a];
                    if (!(std::isfinite(b) && b > 0)) return set_error(-2, nm + ": the information of member_edge[" + std::to_string(m) + "] = " + std::to_string(e) + " on axis " + std::to_string(a) + " is " + std::to_string(b) + ": a member's base information must be finite and > 0");
                    ln = a == 0 ? std::log(b) : ln + std::log(b);
                }
                k_host[(size_t)m] = -ln - 2.0 * (log_weight ? log_weight[m] : 0.0);
            }
            if (int rc = copy_sync(k_d, k_host.data(), 8 * (size_t)M, hipMemcpyHostToDevice)) return rc;
            const MixArgs ma{member_of_d, base_d, k_d, cost_d};
            const MixGroups mg{(int)n_groups, off_d, edge_d, cost_d, base_d, maps.edit_cls, maps.edit_map, sel_d};
            std::vector<MixPartial> hp((size_t)nbG);
            s.stop_reason = TSGO_MIX_ROUNDS;
            for (int r = 0;; ++r) {
                // ---- pass r: costs, selection, scatter; the partials folded in workgroup order ----
                HIP_OK(hipEventRecord(te[0], stream));
                launch_mix_cost(ma);
                launch(k_mix_select<T>, nbG, mg, edit_tables(), part_d);
                HIP_OK(hipGetLastError());
                HIP_OK(hipEventRecord(te[1], stream));
                HIP_OK(hipMemcpyAsync(hp.data(), part_d, hp.size() * sizeof(MixPartial), hipMemcpyDeviceToHost, stream));
                HIP_OK(hipStreamSynchronize(stream));
                { float ms = 0; HIP_OK(hipEventElapsedTime(&ms, te[0], te[1])); s.ms_select += ms; }
                double changed = 0.0, cost_sum = 0.0;
                for (const MixPartial& q : hp) { changed += q.changed; cost_sum += q.cost_sum; }
                s.n_changed[r] = (int64_t)changed; s.cost_sum[r] = cost_sum; s.passes = r + 1;
                if (changed == 0.0) { s.stop_reason = TSGO_MIX_STABLE; break; }      // (r > 0: pass 0 moves every group) nothing was written
                mem.hier_age = -1;      // the weights may move wholesale: the next linearisation builds a fresh hierarchy
                if (r == p.rounds_max) break;
                bool solver_failed = false;
                if (p.inner_iterations > 0) {
                    const auto t0 = std::chrono::steady_clock::now();
                    tsgo_stats in;
                    if (int rc = optimize(p.inner_iterations, &in)) return rc;
                    s.ms_inner += ms_since(t0);
                    s.chi2_inner[r] = in.chi2_last; s.inner_iterations_run[r] = in.iterations_run; s.inner_stop[r] = in.stop_reason;
                    s.pcg_iters_total += in.pcg_iters_total;
                    solver_failed = in.stop_reason == TSGO_STOP_SOLVER;
                }
                s.rounds = r + 1;
                if (solver_failed) { s.stop_reason = TSGO_MIX_SOLVER; break; }
            }
            // ---- the selection and the costs go to the host once; what mirrors weights there follows; keep_selection = 0 puts the base back ----
            std::vector<int32_t> sel((size_t)n_groups);
            if (int rc = copy_sync(sel.data(), sel_d, 4 * (size_t)n_groups, hipMemcpyDeviceToHost)) return rc;
            if (selected_out) std::copy(sel.begin(), sel.end(), selected_out);
            if (cost_out) { if (int rc = copy_sync(cost_out, cost_d, 8 * (size_t)M, hipMemcpyDeviceToHost)) return rc; }
            if (p.keep_selection == 0) {
                launch(k_mix_restore<T>, grid_for((int)M), (int)M, mg, edit_tables());
                HIP_OK(hipGetLastError());
                HIP_OK(hipStreamSynchronize(stream));
                mem.hier_age = -1;
            } else if (s.members_by_class[kClassPosePrior] > 0) {
                const std::vector<uint32_t>& loc = edges(nm)->loc;      // built by edit_prepare at the latest
                for (int64_t g = 0; g < n_groups; ++g)
                    for (int64_t m = group_off[g]; m < group_off[g + 1]; ++m) {
                        const size_t e = (size_t)member_edge[m];
                        if (type[e] != kClassPosePrior) continue;
                        const size_t k = loc[2 * e];      // which prior record the member is
                        for (int a = 0; a < 3 && 3 * k + a < pri_p_w.size(); ++a) pri_p_w[3 * k + a] = m - group_off[g] == sel[(size_t)g] ? mb[3 * (size_t)m + a] : 0.0;
                    }
            }
            s.ms_total = ms_since(wall0);
            if (st_out) *st_out = s;
            return 0;
        } else return set_error(-1, nm + ": needs precision = 64");
    }
