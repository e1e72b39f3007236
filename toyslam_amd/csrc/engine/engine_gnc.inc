// engine/engine_gnc.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// tsgo_gnc.  Graduated non-convexity with the truncated-least-squares surrogate (DESIGN.md section 18): per round ONE pass of
// k_gnc_reweight (tsgo_gnc_kernels.h; the once-per-edge walk of tsgo_edge_walk.h) — evaluate, weight, scatter into the slots the edit knows —
// then the handle's own optimize().  Per round one GncPartial per workgroup comes back; the weights cross the bus once, at the end, and
// only when the caller asks for them or a pose prior's host mirror needs them.
//
// Buffers: the report's slot -> edge maps and the edit's edge -> slot map (StructureMaps: built by the first call that needs them, kept
// by a refill) and one allocation that lives for the call — the base information (3 doubles per edge, taken with k_get_edge_inf), this
// round's weights, the subject bytes, the partials.  A handle that never calls tsgo_gnc launches what it launched before.
//
// State: every round ends as tsgo_set_edge_information does (mem.hier_age = -1: the next linearisation builds a fresh hierarchy; the
// warm start's history and the robust setting stay), pri_p_w follows the pose priors' weights when the call returns.
// An inner run that fails with an error code (< 0, not TSGO_STOP_SOLVER) ends the call with that code at once: the tables then hold the
// last round's weights, whatever keep_weights says.
    void launch_gnc_pass(bool probe, const GncArgs& ga, GncPartial* part) {
        if constexpr (sizeof(T) == 8) {
            pick<0, 1>(probe ? 1 : 0, [&](auto pb) {
                if (report_lm_priors()) pick<1, 2, 4, 8>(pr.by_lm.G, [&](auto g) {
                    launch(k_gnc_reweight_lm_prior<T, g, pb>, nbL, tl, (const T*)lmrec, (const uint32_t*)maps.rep_pl_edge, part + nbP, lm_prior_args(), ga, edit_tables());
                });
                pick_edge_walk([&](auto g, auto general, auto pri) {
                    launch(k_gnc_reweight<T, g, general, pri, pb>, nbP, tp, to, (const T*)ps, (const T*)lmrec, maps.edge_maps(), part, pri ? pose_prior_args() : no_priors(), ga, edit_tables());
                });
            });
        }
    }

    int gnc(const tsgo_gnc_params& p, const uint8_t* subject, int64_t n_mask, double* w_out, int64_t cap_edges, tsgo_gnc_stats* st_out) override {
        const auto wall0 = std::chrono::steady_clock::now();
        auto ms_since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
        const std::string nm = "tsgo_gnc";
        if (sizeof(T) != 8) return set_error(-1, nm + ": needs precision = 64");
        if (cfg.world > 1 || collective()) return set_error(-1, nm + ": edge-sharded handles (world > 1) are not supported");
        if (!have_graph_data) return set_error(-3, nm + ": no graph set");
        const size_t E = structure.e_type.size();
        if (subject && n_mask != (int64_t)E) return set_error(-1, nm + ": n_mask = " + std::to_string(n_mask) + " but the graph has " + std::to_string(E) + " edges (one byte per edge)");
        if (w_out && cap_edges < (int64_t)E) return set_error(-1, nm + ": cap_edges " + std::to_string(cap_edges) + " is below n_edges = " + std::to_string(E));
        if (!(std::isfinite(p.mu_step) && p.mu_step > 1.0)) return set_error(-1, nm + ": mu_step = " + std::to_string(p.mu_step) + " must be finite and > 1");
        if (p.rounds_max < 1 || p.rounds_max > TSGO_GNC_MAX_ROUNDS) return set_error(-1, nm + ": rounds_max = " + std::to_string(p.rounds_max) + " is outside [1, " + std::to_string(TSGO_GNC_MAX_ROUNDS) + "]");
        if (p.inner_iterations < 0) return set_error(-1, nm + ": inner_iterations = " + std::to_string(p.inner_iterations) + " is negative");
        if (p.keep_weights != 0 && p.keep_weights != 1) return set_error(-1, nm + ": keep_weights = " + std::to_string(p.keep_weights) + " must be 0 or 1");
        for (int c = 0; c < kEdgeClasses; ++c)
            if (!std::isfinite(p.barc2[c])) return set_error(-1, nm + ": barc2[" + std::to_string(c) + "] must be finite (<= 0 exempts the class)");
        tsgo_gnc_stats s; std::memset(&s, 0, sizeof(s));
        int64_t n_subject = 0;
        for (size_t e = 0; e < E; ++e) {
            const uint32_t c = structure.e_type[e];
            if (c < (uint32_t)kEdgeClasses && p.barc2[c] > 0 && (!subject || subject[e] != 0)) { ++s.subject_by_class[c]; ++n_subject; }
        }
        if (n_subject == 0) return set_error(-1, nm + ": no subject edge (every class has barc2 <= 0, or the mask leaves none)");
        if constexpr (sizeof(T) == 8) {
            HIP_OK(hipSetDevice(cfg.device));
            if (int rc = report_prepare()) return rc;
            if (int rc = edit_prepare(nm)) return rc;
            const size_t n_part = (size_t)nbP + (report_lm_priors() ? (size_t)nbL : 0);
            CallScratch scratch; EventPair te;
            double *base_d = nullptr, *w_d = nullptr; uint8_t* subject_d = nullptr; GncPartial* part_d = nullptr;
            scratch.want(&base_d, 24 * E); scratch.want(&w_d, 8 * E); scratch.want(&part_d, n_part * sizeof(GncPartial));
            if (subject) scratch.want(&subject_d, E);
            if (int rc = scratch.commit()) return rc;
            if (int rc = te.create()) return rc;
            if (subject) HIP_OK(hipMemcpyAsync(subject_d, subject, E, hipMemcpyHostToDevice, stream));
            launch(k_get_edge_inf<T>, grid_for((int)E), (int)E, (const uint32_t*)maps.edit_map, (const uint8_t*)maps.edit_cls, edit_tables(), base_d);
            HIP_OK(hipGetLastError());
            GncArgs ga{};
            for (int c = 0; c < kEdgeClasses; ++c) ga.barc2[c] = p.barc2[c];
            ga.base = base_d; ga.subject = subject_d; ga.cls = maps.edit_cls; ga.map = maps.edit_map; ga.w_buf = w_d;
            std::vector<GncPartial> hp(n_part);
            // one pass and its partials, folded in workgroup order (the landmark priors' behind the main pass's)
            struct Fold { double q_max, cost; int64_t zero, one, between; };
            auto pass = [&](bool probe, double mu, Fold& sum) -> int {
                ga.mu = mu;
                HIP_OK(hipEventRecord(te[0], stream));
                launch_gnc_pass(probe, ga, part_d);
                HIP_OK(hipGetLastError());
                HIP_OK(hipEventRecord(te[1], stream));
                HIP_OK(hipMemcpyAsync(hp.data(), part_d, n_part * sizeof(GncPartial), hipMemcpyDeviceToHost, stream));
                HIP_OK(hipStreamSynchronize(stream));
                { float ms = 0; HIP_OK(hipEventElapsedTime(&ms, te[0], te[1])); s.ms_reweight += ms; }
                sum = Fold{0.0, 0.0, 0, 0, 0};
                for (const GncPartial& q : hp) { sum.q_max = std::max(sum.q_max, q.q_max); sum.cost += q.cost; sum.zero += q.n_zero; sum.one += q.n_one; sum.between += q.n_between; }
                return 0;
            };
            Fold sum;
            if (int rc = pass(true, -1.0, sum)) return rc;
            s.q_max = sum.q_max;
            auto finish = [&]() {
                s.ms_total = ms_since(wall0);
                if (st_out) *st_out = s;
                return 0;
            };
            if (!(2.0 * s.q_max - 1.0 > 0.0)) {      // every subject edge is an inlier at full weight already: nothing is written
                s.rounds = 0; s.stop_reason = TSGO_GNC_ALL_INLIERS;
                if (w_out) std::fill(w_out, w_out + E, 1.0);
                return finish();
            }
            const std::vector<double> pri_base = pri_p_w;      // the pose priors' base information, record order
            double mu = 1.0 / (2.0 * s.q_max - 1.0);
            s.stop_reason = TSGO_GNC_ROUNDS;
            for (int r = 0; r < p.rounds_max; ++r) {
                if (int rc = pass(false, mu, sum)) return rc;
                mem.hier_age = -1;      // the weights may move wholesale: the next linearisation builds a fresh hierarchy
                s.mu[r] = mu; s.cost[r] = sum.cost; s.n_zero[r] = sum.zero; s.n_one[r] = sum.one; s.n_between[r] = sum.between;
                s.rounds = r + 1;
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
                if (solver_failed) { s.stop_reason = TSGO_GNC_SOLVER; break; }
                if (sum.between == 0) { s.stop_reason = TSGO_GNC_BINARY; break; }
                mu *= p.mu_step;
            }
            // ---- the weights go to the host once; what mirrors weights there follows; keep_weights = 0 puts the base back ----
            const bool pose_priors_subject = s.subject_by_class[kClassPosePrior] > 0 && p.keep_weights == 1;
            std::vector<double> w_host;
            double* w_dst = w_out;
            if (!w_dst && pose_priors_subject) { w_host.resize(E); w_dst = w_host.data(); }
            if (w_dst) { if (int rc = copy_sync(w_dst, w_d, 8 * E, hipMemcpyDeviceToHost)) return rc; }
            if (p.keep_weights == 0) {
                launch(k_set_edge_inf<T>, grid_for((int)E), (int)E, (const int64_t*)nullptr, (const double*)base_d, (const uint32_t*)maps.edit_map, (const uint8_t*)maps.edit_cls, edit_tables());
                HIP_OK(hipGetLastError());
                HIP_OK(hipStreamSynchronize(stream));
                mem.hier_age = -1;
            } else if (pose_priors_subject) {
                for (size_t k = 0; k < pr.prior_p_edge.size() && 3 * k + 2 < pri_p_w.size(); ++k)
                    for (int m = 0; m < 3; ++m) pri_p_w[3 * k + m] = w_dst[pr.prior_p_edge[k]] * pri_base[3 * k + m];
            }
            return finish();
        } else return set_error(-1, nm + ": needs precision = 64");
    }
