// engine/engine_leverage.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body, after
// engine_sample.inc): tsgo_edge_leverage.  C_e = J_e H^-1 J_e^T and h_e = tr(Omega_a C_e) of EVERY input edge from the K posterior
// samples of tsgo_sample_marginals (DESIGN.md section 23): E [(J_e delta)(J_e delta)^T] = J_e H^-1 J_e^T, so the K solves that give every
// vertex's covariance give every edge's too.
//
// The call IS the sampling call with one more read-out: sample_run (engine_sample.inc) builds the right-hand sides, solves and repeats a
// batch after a breakdown exactly as for tsgo_sample_marginals — the same delta_k, bit for bit — and its hook enqueues k_lev_acc and
// k_lev_acc_lm_prior (tsgo_leverage_kernels.h) behind k_smp_acc_pose / k_smp_acc_lm of every solved batch.  Those two stay: the gauge
// term's share of the trace, h_gauge = sum_v gamma_v tr(C_v), comes from their sums.  acc is [E][8] numbers, call-scoped and zeroed; one
// copy brings it back, the host scales the seven sums by 1 / K and folds the stats in f64 in input edge order from the records.
//
// State rule, determinism and refusals: those of tsgo_sample_marginals (mb_guarded; everything is validated before anything is launched).
    template <int NV> void launch_leverage(const LevBatch<T>& lb) {
        if (report_lm_priors()) pick<1, 2, 4, 8>(pr.by_lm.G, [&](auto g) { pick<2, 1>(rk(), [&](auto rk) {      // (RK 1 serves the default setting too, as in launch_sample_rhs)
            launch(k_lev_acc_lm_prior<T, g, rk>, nbL, tl, (const T*)lmrec, (const uint32_t*)maps.rep_pl_edge, lm_prior_args(), robust_args(), lb);
        }); });
        pick_edge_walk([&](auto g, auto general, auto pri) { pick<2, 1>(rk(), [&](auto rk) {
            launch(k_lev_acc<T, g, general, pri, rk>, nbP, tp, to, (const T*)ps, (const T*)lmrec, maps.edge_maps(), pri ? pose_prior_args() : no_priors(), robust_args(),
                   odom_analytic_flag(), lb);
        }); });
    }

    template <int NV> int leverage_run(int K, uint64_t seed, double tol, double* rec_out, size_t E, std::vector<double>& cov, tsgo_sample_stats& ss) {
        CallScratch lev; T* acc = nullptr;
        lev.want(&acc, std::max<size_t>(E, 1) * 8 * sizeof(T));
        if (int rc = lev.commit()) return rc;
        HIP_OK(hipMemsetAsync(lev.base, 0, lev.total, stream));
        if (int rc = sample_run<NV>(K, seed, tol, cov.data(), nullptr, ss, [&](MbBuf& B, const T* u, int nc) {
                launch_leverage<NV>(LevBatch<T>{NV, nc, (const T*)B.x, u, (const T*)B.t, acc});
            })) return rc;
        if constexpr (sizeof(T) == sizeof(double)) {
            if (E > 0) HIP_OK(hipMemcpyAsync(rec_out, acc, E * 8 * sizeof(double), hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
        }
        return 0;
    }

    int edge_leverage(int n_samples, uint64_t seed, double rel_tol, double* rec_out, int64_t cap_edges, tsgo_leverage_stats* st_out) override {
        const auto wall0 = std::chrono::steady_clock::now();
        const std::string nm("tsgo_edge_leverage");
        tsgo_sample_stats ss; std::memset(&ss, 0, sizeof(ss));
        if (int rc = sample_refusals(nm, n_samples)) return rc;
        const size_t E = structure.e_type.size(), V = (size_t)pr.n_vertices;
        if (!rec_out) return set_error(-1, nm + ": bad argument (rec_out is NULL)");
        if (cap_edges < (int64_t)E) return set_error(-1, nm + ": cap_edges " + std::to_string(cap_edges) + " is below n_edges = " + std::to_string(E));
        if constexpr (sizeof(T) == 8) {
            HIP_OK(hipSetDevice(cfg.device));
            if (int rc = sample_prepare()) return rc;
            const double tol = rel_tol > 0 ? rel_tol : cfg.pcg_rel_tol;
            std::vector<double> cov(9 * std::max<size_t>(V, 1));
            if (int rc = mb_compute([&](auto nv) { return leverage_run<nv>(n_samples, seed, tol, rec_out, E, cov, ss); })) return rc;
            const double inv = 1.0 / (double)n_samples;
            for (size_t e = 0; e < E; ++e)
                for (int m = 0; m < 7; ++m) rec_out[8 * e + m] *= inv;
            if (st_out) {
                tsgo_leverage_stats s; std::memset(&s, 0, sizeof(s));
                s.samples = n_samples;
                for (size_t e = 0; e < E; ++e) {
                    const uint32_t c = structure.e_type[e];
                    s.edges[c] += 1; s.h_sum[c] += rec_out[8 * e + 6]; s.dof_sum[c] += rec_out[8 * e + 7];
                }
                // gamma_v tr(C_v): poses, then landmarks, in internal order
                for (int i = 0; i < pr.P; ++i) { const double* o = cov.data() + 9 * (size_t)pr.pose_vertex[(size_t)i]; s.h_gauge += (double)pr.gauge_p[(size_t)i] * (o[0] + o[4] + o[8]); }
                for (int l = 0; l < pr.L; ++l) { const double* o = cov.data() + 9 * (size_t)pr.lm_vertex[(size_t)l]; s.h_gauge += (double)pr.gauge_l[(size_t)l] * (o[0] + o[4]); }
                for (int c = 0; c < kEdgeClasses; ++c) s.trace += s.h_sum[c];
                s.trace += s.h_gauge;
                s.unknowns = 3 * (int64_t)pr.P + 2 * (int64_t)pr.L;
                s.solve = ss.solve;
                s.ms_noise = ss.ms_noise; s.ms_readout = ss.ms_readout;
                s.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
                s.solve.ms_total = s.ms_total;
                *st_out = s;
            }
            return 0;
        } else return 0;
    }
