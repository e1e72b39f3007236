// engine/engine_gate.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body, after
// engine_marginals.inc): tsgo_gate_edges.  K candidate edges, not in the graph, are tested against the joint marginal of their vertices:
// d2 = e^T S^-1 e, S = J Sigma J^T + Omega^-1 (DESIGN.md section 15).
//
// The distinct vertices of the candidates are solved once, 3 columns a pose and 2 a landmark, through mb_batch exactly as mb_run_joint
// does (every batch but the last full, columns may straddle batches).  After a batch only the candidates that have a vertex among its
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
        tsgo_marginal_stats& s = gs.solve;
        const int K = (int)plan.cands.size(), V = (int)plan.verts.size(), D = (int)plan.all.size();
        const int nb = (D + NV - 1) / NV;
        // ---- the per-batch lists: items (k_mb_joint) and jobs (k_gate_scatter) of every batch, one after the other ----
        std::vector<int> v_off((size_t)V + 1, 0), v_cand;      // candidates of every distinct vertex (a unary candidate once)
        auto second = [&](int k) { return plan.cand_v[2 * (size_t)k + 1] != plan.cand_v[2 * (size_t)k]; };
        for (int k = 0; k < K; ++k) { ++v_off[(size_t)plan.cand_v[2 * (size_t)k] + 1]; if (second(k)) ++v_off[(size_t)plan.cand_v[2 * (size_t)k + 1] + 1]; }
        for (int v = 0; v < V; ++v) v_off[(size_t)v + 1] += v_off[(size_t)v];
        v_cand.resize((size_t)v_off[(size_t)V]);
        {
            std::vector<int> fill(v_off.begin(), v_off.end() - 1);
            for (int k = 0; k < K; ++k) { v_cand[(size_t)fill[(size_t)plan.cand_v[2 * (size_t)k]]++] = k; if (second(k)) v_cand[(size_t)fill[(size_t)plan.cand_v[2 * (size_t)k + 1]]++] = k; }
        }
        std::vector<MbColumn> items;
        std::vector<GateJob> jobs;
        std::vector<int> item_off((size_t)nb + 1, 0), job_off((size_t)nb + 1, 0), rows_of((size_t)nb, 0);
        std::vector<int> cand_stamp((size_t)K, -1), vert_stamp((size_t)V, -1), vert_row((size_t)V, 0);
        int max_rows = 1;
        for (int b = 0, v_lo = 0; b < nb; ++b) {
            const int j0 = b * NV, j1 = std::min(D, j0 + NV);
            while (plan.col0[(size_t)v_lo] + (plan.verts[(size_t)v_lo].kind == 0 ? 3 : 2) <= j0) ++v_lo;      // first vertex with a column >= j0
            int rows = 0;
            auto row_of = [&](int v) {
                if (vert_stamp[(size_t)v] != b) {
                    vert_stamp[(size_t)v] = b; vert_row[(size_t)v] = rows;
                    items.push_back(MbColumn{plan.verts[(size_t)v].kind, plan.verts[(size_t)v].idx, rows, 0});
                    rows += plan.verts[(size_t)v].kind == 0 ? 3 : 2;
                }
                return vert_row[(size_t)v];
            };
            for (int v = v_lo; v < V && plan.col0[(size_t)v] < j1; ++v)
                for (int q = v_off[(size_t)v]; q < v_off[(size_t)v + 1]; ++q) {
                    const int k = v_cand[(size_t)q];
                    if (cand_stamp[(size_t)k] == b) continue;
                    cand_stamp[(size_t)k] = b;
                    const int r0 = row_of(plan.cand_v[2 * (size_t)k]), r1 = row_of(plan.cand_v[2 * (size_t)k + 1]);
                    jobs.push_back(GateJob{k, r0, r1, 0});
                }
            item_off[(size_t)b + 1] = (int)items.size(); job_off[(size_t)b + 1] = (int)jobs.size();
            rows_of[(size_t)b] = rows; max_rows = std::max(max_rows, rows);
        }
        // ---- device memory of the call ----
        MbBuf B; char* base = nullptr; char* gbase = nullptr;
        struct Free { char*& b; ~Free() { if (b) (void)hipFree(b); } } fr{base}, fg{gbase};
        if (int rc = mb_alloc(B, NV, &base)) return rc;
        MbColumn* items_d = nullptr; GateJob* jobs_d = nullptr; GateCand<T>* cands_d = nullptr;
        double *sig_d = nullptr, *slice_d = nullptr, *rec_d = nullptr, *innov_d = nullptr;
        {
            std::vector<std::pair<void**, size_t>> want;
            want.push_back({(void**)&items_d, std::max<size_t>(items.size(), 1) * sizeof(MbColumn)});
            want.push_back({(void**)&jobs_d, std::max<size_t>(jobs.size(), 1) * sizeof(GateJob)});
            want.push_back({(void**)&cands_d, (size_t)K * sizeof(GateCand<T>)});
            want.push_back({(void**)&sig_d, (size_t)K * kGateSig * sizeof(double)});
            want.push_back({(void**)&slice_d, (size_t)max_rows * NV * sizeof(double)});
            want.push_back({(void**)&rec_d, (size_t)K * kGateRec * sizeof(double)});
            if (innov_out) want.push_back({(void**)&innov_d, (size_t)K * 9 * sizeof(double)});
            size_t total = 0;
            for (auto& w : want) total += (w.second + 255) & ~size_t(255);
            HIP_OK(hipMalloc((void**)&gbase, total));
            size_t off = 0;
            for (auto& w : want) { *w.first = gbase + off; off += (w.second + 255) & ~size_t(255); }
        }
        if (!items.empty()) HIP_OK(hipMemcpyAsync(items_d, items.data(), items.size() * sizeof(MbColumn), hipMemcpyHostToDevice, stream));
        if (!jobs.empty()) HIP_OK(hipMemcpyAsync(jobs_d, jobs.data(), jobs.size() * sizeof(GateJob), hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemcpyAsync(cands_d, plan.cands.data(), (size_t)K * sizeof(GateCand<T>), hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemsetAsync(sig_d, 0, (size_t)K * kGateSig * sizeof(double), stream));
        // device time of the read-out: one event pair, read after the NEXT batch's solve has synchronised the stream (no wait of its own)
        hipEvent_t re[2] = {nullptr, nullptr};
        struct FreeEv { hipEvent_t* e; ~FreeEv() { for (int k = 0; k < 2; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } fe{re};
        HIP_OK(hipEventCreate(&re[0])); HIP_OK(hipEventCreate(&re[1]));
        double ms_read = 0; bool pending = false;
        auto collect = [&]() -> int { if (pending) { float t = 0; HIP_OK(hipEventElapsedTime(&t, re[0], re[1])); ms_read += t; pending = false; } return 0; };
        s.batch_width = NV;
        s.preconditioner = amg_on ? 1 : 0;
        float ms = 0;
        for (int b = 0; b < nb; ++b) {
            const int j0 = b * NV, nc = std::min(NV, D - j0);
            std::vector<MbColumn> cols(kMbMaxWidth, MbColumn{-1, 0, 0, 0});
            std::copy(plan.all.begin() + j0, plan.all.begin() + j0 + nc, cols.begin());
            HIP_OK(hipMemcpyAsync(B.cols, cols.data(), cols.size() * sizeof(MbColumn), hipMemcpyHostToDevice, stream));
            if (int rc = mb_batch<NV>(B, tol, s, &ms)) return rc;
            if (int rc = collect()) return rc;
            const int n_items = item_off[(size_t)b + 1] - item_off[(size_t)b], n_jobs = job_off[(size_t)b + 1] - job_off[(size_t)b];
            HIP_OK(hipEventRecord(re[0], stream));
            hipLaunchKernelGGL((k_mb_joint<T, NV>), dim3((unsigned)n_items), dim3(64), 0, stream, tl, pr.by_lm.G, (const T*)ps, (const T*)lmrec,
                               (const MbColumn*)(items_d + item_off[(size_t)b]), (const MbColumn*)B.cols, (const T*)B.x, slice_d);
            HIP_OK(hipGetLastError());
            launch(k_gate_scatter<T, NV>, grid_for(n_jobs * NV), n_jobs, (const GateJob*)(jobs_d + job_off[(size_t)b]), (const GateCand<T>*)cands_d,
                   (const MbColumn*)B.cols, (const double*)slice_d, sig_d);
            HIP_OK(hipGetLastError());
            HIP_OK(hipEventRecord(re[1], stream));
            pending = true;
            s.columns += nc;
        }
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
        s.ms_solve = ms;
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
            const int rc = mb_guarded([&]() -> int {
                if (int r = mb_prepare()) return r;
                return pick<1, 16, 8>(marginal_width(), [&](auto nv) { return gate_run<nv>(plan, tol, rec_out, innov_out, gs); });
            });
            if (rc) return rc;
            for (int k = 0; k < n; ++k) gs.not_pd += rec_out[(size_t)k * kGateRec + 7] != 0.0;
            gs.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
            gs.solve.ms_total = gs.ms_total;
            if (st_out) *st_out = gs;
            return 0;
        } else return set_error(-1, "tsgo_gate_edges: needs precision = 64");      // (mb_queries has refused an f32 handle already)
    }
