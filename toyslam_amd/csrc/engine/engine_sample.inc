// engine/engine_sample.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body, after
// engine_marginals.inc and engine_report.inc): tsgo_sample_marginals.  K posterior samples delta_k ~ N(0, H^-1) by perturb-and-MAP and the
// diagonal blocks of H^-1 of EVERY vertex from their second moments (DESIGN.md section 19): K solves instead of 3 P + 2 L.
//
// The fourth reader of the batched solve (mb_for_batches), and the first whose right-hand side is not a list of unit columns: per batch of
// NV samples k_smp_rhs_lm / k_smp_rhs_pose (tsgo_sample_kernels.h) write b_p - W D^-1 b_l into the batch's r, handed to mb_solve as its
// right-hand-side callable, so that the block-Jacobi repeat after a breakdown rebuilds it.  After the solve k_mb_schur_lm gives
// t = Y^T X and the two accumulation kernels add the batch's live columns, in order, to the call's accumulators; the batches run in
// order, so the sums — and with them cov_out — are the same bits on every call.
//
// State rule: that of tsgo_marginals (mb_guarded).  The slot -> edge maps and the vertex positions go to the device BEFORE the snapshot
// (they are bump-allocated behind what the graph owns and belong to the structure, as the report's maps do); every other buffer is
// call-scoped.  Everything is validated before anything is launched.
    static constexpr int kSampleMax = 65536;

    int sample_prepare() {
        if (maps.smp_ready) return 0;
        if (!edges("tsgo_sample_marginals")) return -30;      // every map entry is an input edge (host/structure_index.h)
        if (int rc = report_prepare()) return rc;              // by_pose, odom and the two prior lists: the report's maps
        if (int rc = upload_u32m(&maps.smp_lm_edge, pr.by_lm.edge)) return rc;
        auto upload_int = [&](int** out, const std::vector<int>& v) -> int {
            if (int rc = dalloc(out, v.size())) return rc;
            if (!v.empty()) { if (int rc = copy_sync(*out, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice)) return rc; }
            return 0;
        };
        if (int rc = upload_int(&maps.smp_pose_vertex, pr.pose_vertex)) return rc;
        if (int rc = upload_int(&maps.smp_lm_vertex, pr.lm_vertex)) return rc;
        maps.smp_ready = true;
        return 0;
    }

    // the right-hand side of one batch: samples k0 .. k0 + nc - 1 (columns past nc: zero)
    template <int NV> void launch_sample_rhs(MbBuf& B, T* u, uint64_t seed, int k0, int nc) {
        constexpr int CH = NV == 1 ? 1 : 4;
        const SampleBatch sb{SampleSeed{(uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32)}, k0, nc, NV};
        if (tl.n_slices > 0) pick<1, 2, 4, 8>(pr.by_lm.G, [&](auto g) { pick<2, 1>(rk(), [&](auto rk) {      // (RK 1 serves the default setting too; listed last: what pick falls back to)
            launch(k_smp_rhs_lm<T, g, CH, rk>, nbL, tl, (const T*)ps, (const T*)lmrec, (const uint32_t*)maps.smp_lm_edge, (const uint32_t*)maps.rep_pl_edge,
                   (const int*)maps.smp_lm_vertex, (const T*)gauge_l, pr.has_priors ? lm_prior_args() : no_priors(), robust_args(), sb, u);
        }); });
        pick<1, 2, 4, 8>(pr.by_pose.G, [&](auto g) { pick<2, 1>(rk(), [&](auto rk) {
            launch(k_smp_rhs_pose<T, g, CH, rk>, nbP, tp, to, (const T*)ps, (const T*)lmrec, (const uint32_t*)maps.rep_lm_edge, (const uint32_t*)maps.rep_od_edge,
                   (const uint32_t*)maps.rep_pp_edge, (const int*)maps.smp_pose_vertex, (const T*)gauge_p, (const T*)u,
                   pr.has_priors ? pose_prior_args() : no_priors(), robust_args(), odom_analytic_flag(), sb, B.r);
        }); });
    }

    // The batch driver of both sampling calls (right-hand side, solve, breakdown repeat, the vertex accumulators): tsgo_sample_marginals
    // and tsgo_edge_leverage (engine_leverage.inc) differ in the read-out hook alone — more(B, u, nc) enqueues what a call adds behind
    // the two accumulation kernels of a solved batch, inside the read-out's event pair.
    template <int NV, typename More> int sample_run(int K, uint64_t seed, double tol, double* cov, double* samples, tsgo_sample_stats& ss, More&& more) {
        const int P = pr.P, L = pr.L;
        const size_t V = (size_t)pr.n_vertices;
        MbBuf B;
        if (int rc = mb_alloc(B, NV)) return rc;
        CallScratch sm; EventPair en, er;
        T *u = nullptr, *acc_p = nullptr, *acc_l = nullptr; double* stage = nullptr;
        sm.want(&u, (size_t)std::max(L, 1) * NV * 2 * sizeof(T));
        sm.want(&acc_p, (size_t)std::max(P, 1) * 6 * sizeof(T));
        sm.want(&acc_l, (size_t)std::max(L, 1) * 3 * sizeof(T));
        if (samples) sm.want(&stage, (size_t)NV * std::max<size_t>(V, 1) * 3 * sizeof(double));
        if (int rc = sm.commit()) return rc;
        HIP_OK(hipMemsetAsync(sm.base, 0, sm.total, stream));      // (the staged entries of a vertex that is neither a pose nor a landmark stay 0)
        if (int rc = en.create()) return rc;
        if (int rc = er.create()) return rc;
        // device time of the right-hand-side and read-out kernels: one event pair each, read once the stream has been synchronised behind them
        // (by the batch's solve, or at the end)
        double ms_noise = 0, ms_read = 0; bool pend_n = false, pend_r = false;
        auto collect = [&](EventPair& e, bool& pending, double& acc) -> int { if (pending) { float t = 0; HIP_OK(hipEventElapsedTime(&t, e[0], e[1])); acc += t; pending = false; } return 0; };
        const std::vector<MbColumn> all((size_t)K, MbColumn{2, 0, 0, 0});      // kind 2: a sample column (nothing reads B.cols here)
        if (int rc = mb_for_batches<NV>(B, all, full_batches(K, NV), tol, ss.solve,
            [&](int j0, int nc) -> int {
                if (pend_n) { HIP_OK(hipEventSynchronize(en[1])); }      // a repeat of the batch: the first build's events have completed (mb_solve waited on the stream)
                if (int rc = collect(en, pend_n, ms_noise)) return rc;
                HIP_OK(hipEventRecord(en[0], stream));
                launch_sample_rhs<NV>(B, u, seed, j0, nc);
                HIP_OK(hipGetLastError());
                HIP_OK(hipEventRecord(en[1], stream));
                pend_n = true;
                return 0;
            },
            [&](int, int j0, int nc) -> int {
                if (int rc = collect(en, pend_n, ms_noise)) return rc;
                if (int rc = collect(er, pend_r, ms_read)) return rc;
                HIP_OK(hipEventRecord(er[0], stream));
                mb_lm<NV>(B.x, B.t, B.zero);      // t = Dl^-1 W^T X = Y^T X
                launch(k_smp_acc_pose<T>, grid_for(P), P, NV, nc, (const T*)B.x, (const int*)maps.smp_pose_vertex, (int64_t)V, acc_p, stage);
                if (L > 0) launch(k_smp_acc_lm<T>, grid_for(L), L, NV, nc, (const T*)u, (const T*)B.t, (const int*)maps.smp_lm_vertex, (int64_t)V, acc_l, stage);
                more(B, (const T*)u, nc);
                HIP_OK(hipGetLastError());
                HIP_OK(hipEventRecord(er[1], stream));
                pend_r = true;
                // (stream order keeps the next batch's read-out behind this copy)
                if (samples) HIP_OK(hipMemcpyAsync(samples + (size_t)j0 * V * 3, stage, (size_t)nc * V * 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
                return 0;
            })) return rc;
        std::vector<T> hp((size_t)P * 6), hl((size_t)L * 3);
        if (P > 0) HIP_OK(hipMemcpyAsync(hp.data(), acc_p, hp.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
        if (L > 0) HIP_OK(hipMemcpyAsync(hl.data(), acc_l, hl.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        if (int rc = collect(en, pend_n, ms_noise)) return rc;
        if (int rc = collect(er, pend_r, ms_read)) return rc;
        // (1 / K) sum delta delta^T: the mean is known to be 0
        std::fill(cov, cov + 9 * V, 0.0);
        const double inv = 1.0 / (double)K;
        for (int i = 0; i < P; ++i) {
            const T* a = hp.data() + (size_t)i * 6;
            double* o = cov + 9 * (size_t)pr.pose_vertex[(size_t)i];
            const double m[6] = {(double)a[0] * inv, (double)a[1] * inv, (double)a[2] * inv, (double)a[3] * inv, (double)a[4] * inv, (double)a[5] * inv};
            o[0] = m[0]; o[1] = m[1]; o[2] = m[2]; o[3] = m[1]; o[4] = m[3]; o[5] = m[4]; o[6] = m[2]; o[7] = m[4]; o[8] = m[5];
        }
        for (int l = 0; l < L; ++l) {
            const T* a = hl.data() + (size_t)l * 3;
            double* o = cov + 9 * (size_t)pr.lm_vertex[(size_t)l];
            o[0] = (double)a[0] * inv; o[1] = (double)a[1] * inv; o[3] = o[1]; o[4] = (double)a[2] * inv;
        }
        ss.ms_noise = ms_noise; ss.ms_readout = ms_read;
        return 0;
    }

    // what both sampling calls refuse about the handle and n_samples
    int sample_refusals(const std::string& nm, int n_samples) {
        if (sizeof(T) != 8) return set_error(-1, nm + ": needs precision = 64 (with the gauge, cond(H) is about 2e7: f32 samples would be noise)");
        if (cfg.world > 1 || collective()) return set_error(-1, nm + ": edge-sharded handles (world > 1) are not supported");
        if (!have_graph_data) return set_error(-3, nm + ": no graph set");
        if (!mb_anchored()) return set_error(-1, nm + ": sampling needs a fixed vertex or a full pose prior (without one H is singular)");
        if (n_samples < 1 || n_samples > kSampleMax) return set_error(-1, nm + ": n_samples = " + std::to_string(n_samples) + " is outside 1 .. " + std::to_string(kSampleMax));
        return 0;
    }

    int sample_marginals(int n_samples, uint64_t seed, double rel_tol, double* cov, int64_t cap_vertices, double* samples, int64_t samples_cap,
                         tsgo_sample_stats* st_out) override {
        const auto wall0 = std::chrono::steady_clock::now();
        const std::string nm("tsgo_sample_marginals");
        tsgo_sample_stats ss; std::memset(&ss, 0, sizeof(ss));
        if (int rc = sample_refusals(nm, n_samples)) return rc;
        const int64_t V = pr.n_vertices;
        if (!cov) return set_error(-1, nm + ": bad argument (cov_out is NULL)");
        if (cap_vertices < V) return set_error(-1, nm + ": cap_vertices " + std::to_string(cap_vertices) + " is below n_vertices = " + std::to_string(V));
        if (samples && samples_cap < (int64_t)n_samples * V * 3)
            return set_error(-1, nm + ": samples_cap " + std::to_string(samples_cap) + " is below n_samples * n_vertices * 3 = " + std::to_string((int64_t)n_samples * V * 3));
        if constexpr (sizeof(T) == 8) {
            HIP_OK(hipSetDevice(cfg.device));
            if (int rc = sample_prepare()) return rc;
            const double tol = rel_tol > 0 ? rel_tol : cfg.pcg_rel_tol;
            if (int rc = mb_compute([&](auto nv) { return sample_run<nv>(n_samples, seed, tol, cov, samples, ss, [](MbBuf&, const T*, int) {}); })) return rc;
            ss.samples = n_samples;
            ss.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
            ss.solve.ms_total = ss.ms_total;
            if (st_out) *st_out = ss;
            return 0;
        } else return 0;
    }
