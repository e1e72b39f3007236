// engine/engine_gate.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body, after
// engine_marginals.inc): tsgo_gate_edges.  K candidate edges, not in the graph, are tested against the joint marginal of their vertices:
// d2 = e^T S^-1 e, S = J Sigma J^T + Omega^-1 (DESIGN.md section 15).
//
// The distinct vertices of the candidates are solved once, 3 columns a pose and 2 a landmark, through mb_for_batches exactly as mb_run_joint
// does (full_batches: every batch but the last full, columns may straddle batches).  After a batch only the candidates that have a vertex among its
// columns get work: the unchanged k_mb_joint gives the rows of those candidates' vertices against the batch's columns, k_gate_scatter
// places them in sig[K][6][6] (tsgo_gate_kernels.h).  A vertex's columns lie in at most two batches, so a candidate is visited at most four
// times: the read-out is O(K + columns) whatever the number of batches.  The per-batch lists are built on the host and uploaded once;
// between batches nothing is copied to the host but the PCG state mb_solve reads; k_gate_eval runs once and its records are copied back once.
//
// State rule: that of tsgo_marginals (mb_guarded).  Everything is validated before anything is launched.
    static constexpr int kGateMaxCandidates = 1 << 20;

    struct GatePlan {
        std::vector<MbQuery> verts;              // distinct vertices in order of first appearance
        std::vector<MbColumn> all;               // their columns (mb_run_joint's `all`)
        std::vector<int> col0;                   // first column of every distinct vertex
        std::vector<int> cand_v;                 // 2 per candidate: distinct-vertex numbers (equal for a unary type)
        std::vector<GateCand<T>> cands;
    };

    // the candidate arrays -> plan.cands, or an error; qs = the 2 n resolved ids of mb_queries
    int gate_validate(int n, const uint32_t* e_type, const uint32_t* e_ids, const double* e_meas, const double* e_inf, const std::vector<MbQuery>& qs,
                      GatePlan& plan) {
        const std::string nm("tsgo_gate_edges: candidate ");
        plan.cands.resize((size_t)n);
        for (int k = 0; k < n; ++k) {
            const uint32_t t = e_type[k];
            const std::string who = nm + std::to_string(k);
            if (t >= (uint32_t)kEdgeClasses) return set_error(-1, who + " has unknown edge type " + std::to_string(t));
            const MbQuery a = qs[2 * (size_t)k], b = qs[2 * (size_t)k + 1];
            const uint32_t id1 = e_ids[2 * (size_t)k], id2 = e_ids[2 * (size_t)k + 1];
            const bool unary = t == (uint32_t)kClassPosePrior || t == (uint32_t)kClassLmPrior;
            if (unary && id1 != id2) return set_error(-1, who + " is a prior: it must give the same vertex id twice");
            if (!unary && id1 == id2) return set_error(-1, who + " joins vertex " + std::to_string(id1) + " to itself");
            if (a.kind != gate_slot_kind((int)t, 0) || b.kind != gate_slot_kind((int)t, unary ? 0 : 1)) {
                static const char* want[] = {"must join two Se2 vertices", "must join an Se2 vertex to a Point2 vertex", "must join two Se2 vertices",
                                             "must sit on an Se2 vertex", "must sit on a Point2 vertex"};
                return set_error(-1, who + " (type " + std::to_string(t) + ") " + want[t]);
            }
            const double* m = e_meas + 9 * (size_t)k;
            const double* w = e_inf + 3 * (size_t)k;
            const int dof = (t == (uint32_t)kClassOdom || t == (uint32_t)kClassPosePrior) ? 3 : 2;
            for (int j = 0; j < dof; ++j)
                if (!(std::isfinite(w[j]) && w[j] > 0)) return set_error(-1, who + ": information entry " + std::to_string(j) + " must be finite and > 0 (Omega^-1 enters S)");
            GateCand<T>& c = plan.cands[(size_t)k];
            c = GateCand<T>{};
            c.type = (int)t; c.i0 = a.idx; c.i1 = b.idx;
            for (int j = 0; j < dof; ++j) c.w[j] = (T)w[j];
            if (t == (uint32_t)kClassOdom) {
                double inv[9];
                if (!invert3(m, inv)) return set_error(-1, who + " has a singular measurement matrix");
                for (int j = 0; j < 6; ++j) c.m[j] = (T)inv[j];
            } else if (t == (uint32_t)kClassLm) {
                double v[LM_PLANES]; lm_static(m, w, v);
                c.m[0] = (T)v[LM_ZX]; c.m[1] = (T)v[LM_ZY];
            } else if (t == (uint32_t)kClassVlm) {
                double v[9]; vlm_static(m, w, 0, v);
                for (int j = 0; j < 4; ++j) c.m[j] = (T)v[j];
            } else if (t == (uint32_t)kClassPosePrior) {
                double v[PRI_POSE_REC]; prior_static(t, m, w, v);
                c.m[0] = (T)v[PRI_MX]; c.m[1] = (T)v[PRI_MY]; c.m[2] = (T)v[PRI_C]; c.m[3] = (T)v[PRI_S];
            } else {
                double v[PRI_LM_REC]; prior_static(t, m, w, v);
                c.m[0] = (T)v[PRL_MX]; c.m[1] = (T)v[PRL_MY];
            }
            for (int j = 0; j < 6; ++j)
                if (!std::isfinite((double)c.m[j])) return set_error(-1, who + " has a measurement that is not finite");
        }
        // distinct vertices
        std::vector<int> of_pose((size_t)pr.P, -1), of_lm((size_t)std::max(pr.L, 1), -1);
        plan.cand_v.resize(2 * (size_t)n);
        for (size_t q = 0; q < qs.size(); ++q) {
            int& slot = qs[q].kind == 0 ? of_pose[(size_t)qs[q].idx] : of_lm[(size_t)qs[q].idx];
            if (slot < 0) {
                slot = (int)plan.verts.size();
                plan.verts.push_back(qs[q]);
                plan.col0.push_back((int)plan.all.size());
                const int need = qs[q].kind == 0 ? 3 : 2;
                for (int j = 0; j < need; ++j) plan.all.push_back(MbColumn{qs[q].kind, qs[q].idx, j, 0});
            }
            plan.cand_v[q] = slot;
        }
        return 0;
    }

    template <int NV> int gate_run(const GatePlan& plan, double tol, double* rec_out, double* innov_out, tsgo_gate_stats& gs) {
        const int K = (int)plan.cands.size(), D = (int)plan.all.size();
        // the per-batch lists: items (k_mb_joint) and jobs (k_gate_scatter) of every batch, one after the other (host/batch_plan.h)
        const GateLists gl = gate_batch_lists(plan.verts, plan.col0, plan.cand_v, NV);
        // ---- device memory of the call ----
        MbBuf B;
        if (int rc = mb_alloc(B, NV)) return rc;
        CallScratch gate; EventPair re;
        MbColumn* items_d = nullptr; GateJob* jobs_d = nullptr; GateCand<T>* cands_d = nullptr;
        double *sig_d = nullptr, *slice_d = nullptr, *rec_d = nullptr, *innov_d = nullptr;
        gate.want(&items_d, std::max<size_t>(gl.items.size(), 1) * sizeof(MbColumn));
        gate.want(&jobs_d, std::max<size_t>(gl.jobs.size(), 1) * sizeof(GateJob));
        gate.want(&cands_d, (size_t)K * sizeof(GateCand<T>));
        gate.want(&sig_d, (size_t)K * kGateSig * sizeof(double));
        gate.want(&slice_d, (size_t)gl.max_rows * NV * sizeof(double));
        gate.want(&rec_d, (size_t)K * kGateRec * sizeof(double));
        if (innov_out) gate.want(&innov_d, (size_t)K * 9 * sizeof(double));
        if (int rc = gate.commit()) return rc;
        if (!gl.items.empty()) HIP_OK(hipMemcpyAsync(items_d, gl.items.data(), gl.items.size() * sizeof(MbColumn), hipMemcpyHostToDevice, stream));
        if (!gl.jobs.empty()) HIP_OK(hipMemcpyAsync(jobs_d, gl.jobs.data(), gl.jobs.size() * sizeof(GateJob), hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemcpyAsync(cands_d, plan.cands.data(), (size_t)K * sizeof(GateCand<T>), hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemsetAsync(sig_d, 0, (size_t)K * kGateSig * sizeof(double), stream));
        // device time of the read-out: one event pair, read after the NEXT batch's solve has synchronised the stream (no wait of its own)
        if (int rc = re.create()) return rc;
        double ms_read = 0; bool pending = false;
        auto collect = [&]() -> int { if (pending) { float t = 0; HIP_OK(hipEventElapsedTime(&t, re[0], re[1])); ms_read += t; pending = false; } return 0; };
        if (int rc = mb_for_batches<NV>(B, plan.all, full_batches(D, NV), tol, gs.solve, [&](int b, int, int) -> int {
            if (int rc = collect()) return rc;
            const int i0 = gl.item_off[(size_t)b], n_items = gl.item_off[(size_t)b + 1] - i0, j0 = gl.job_off[(size_t)b], n_jobs = gl.job_off[(size_t)b + 1] - j0;
            HIP_OK(hipEventRecord(re[0], stream));
            launch_wave(k_mb_joint<T, NV>, n_items, tl, pr.by_lm.G, (const T*)ps, (const T*)lmrec, (const MbColumn*)(items_d + i0), (const MbColumn*)B.cols, (const T*)B.x, slice_d);
            HIP_OK(hipGetLastError());
            launch(k_gate_scatter<T, NV>, grid_for(n_jobs * NV), n_jobs, (const GateJob*)(jobs_d + j0), (const GateCand<T>*)cands_d, (const MbColumn*)B.cols, (const double*)slice_d, sig_d);
            HIP_OK(hipGetLastError());
            HIP_OK(hipEventRecord(re[1], stream));
            pending = true;
            return 0;
        })) return rc;
        HIP_OK(hipStreamSynchronize(stream));
        if (int rc = collect()) return rc;
        HIP_OK(hipEventRecord(re[0], stream));
        launch(k_gate_eval<T>, grid_for(K), K, (const GateCand<T>*)cands_d, (const T*)ps, (const T*)lmrec, (const double*)sig_d, rec_d, innov_d);
        HIP_OK(hipGetLastError());
        HIP_OK(hipEventRecord(re[1], stream));
        pending = true;
        HIP_OK(hipMemcpyAsync(rec_out, rec_d, (size_t)K * kGateRec * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (innov_out) HIP_OK(hipMemcpyAsync(innov_out, innov_d, (size_t)K * 9 * sizeof(double), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        if (int rc = collect()) return rc;
        gs.ms_readout = ms_read;
        return 0;
    }

    int gate_edges(int n, const uint32_t* e_type, const uint32_t* e_ids, const double* e_meas, const double* e_inf, double rel_tol, double* rec_out,
                   double* innov_out, tsgo_gate_stats* st_out) override {
        const auto wall0 = std::chrono::steady_clock::now();
        tsgo_gate_stats gs; std::memset(&gs, 0, sizeof(gs));
        if (n < 0 || n > kGateMaxCandidates) return set_error(-1, "tsgo_gate_edges: n = " + std::to_string(n) + " is outside 0 .. " + std::to_string(kGateMaxCandidates));
        if (cfg.world > 1) return set_error(-1, "tsgo_gate_edges: edge-sharded handles (world > 1) are not supported");      // (before a graph is set too)
        std::vector<MbQuery> qs;
        if (int rc = mb_queries("tsgo_gate_edges", e_ids, 2 * n, !rec_out, qs)) return rc;
        if (n == 0) { if (st_out) *st_out = gs; return 0; }
        if (!e_type || !e_meas || !e_inf) return set_error(-1, "tsgo_gate_edges: bad argument");
        if constexpr (sizeof(T) == 8) {
            GatePlan plan;
            if (int rc = gate_validate(n, e_type, e_ids, e_meas, e_inf, qs, plan)) return rc;
            gs.candidates = n; gs.vertices = (int)plan.verts.size();
            const double tol = rel_tol > 0 ? rel_tol : cfg.pcg_rel_tol;
            if (int rc = mb_compute([&](auto nv) { return gate_run<nv>(plan, tol, rec_out, innov_out, gs); })) return rc;
            for (int k = 0; k < n; ++k) gs.not_pd += rec_out[(size_t)k * kGateRec + 7] != 0.0;
            gs.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
            gs.solve.ms_total = gs.ms_total;
            if (st_out) *st_out = gs;
            return 0;
        } else return set_error(-1, "tsgo_gate_edges: needs precision = 64");      // (mb_queries has refused an f32 handle already)
    }
