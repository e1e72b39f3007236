// engine/engine_probes.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// timing probes behind tsgo_cycle_probe / tsgo_profile_iteration / tsgo_time_kernel.
    void probe_sweep(int lprA, size_t level, const T* omega) {      // one smoothing sweep on the level's own vectors, in their type
        const CgState<T>* s0 = st[0];
        DevLevel<T>& L = lv[level];
#ifdef TSGO_TESTING
        if (cyc64) { launch_sweep<1>("", level, lprA, (const T*)L.r, (const T*)L.z, (T*)L.z2, omega, s0); return; }
#endif
        launch_sweep<1>("", level, lprA, (const CV<T>*)L.r, (const CV<T>*)L.z, (CV<T>*)L.z2, omega, s0);
    }
    int cycle_probe(int reps, tsgo_cycle_level* out, int cap) override {
        if (!have_graph_data) return set_error(-3, "tsgo_cycle_probe: no graph set");
        HIP_OK(hipSetDevice(cfg.device));
        if (!amg_on) return 0;
        double chi2;
        if (int rc = do_linearize(&chi2)) return rc;      // a built hierarchy; state slot 0 says "not done"
        int n = 0;
        for (size_t l = 1; l < lv.size() && n < cap; ++l, ++n) {
            DevLevel<T>& L = lv[l];
            const int lprA = lanes_for_sweep((double)L.nnzA / std::max(1, L.n), L.n);
            for (int pass = 0; pass < 2; ++pass) {
                const int m = pass == 0 ? 3 : reps;
                HIP_OK(hipEventRecord(ev[0], stream));
                for (int k = 0; k < m; ++k)
                    probe_sweep(lprA, l, (const T*)(omega_dev + l));
                HIP_OK(hipEventRecord(ev[1], stream));
                HIP_OK(hipEventSynchronize(ev[1]));
                if (pass == 1) { float ms = 0; HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1])); out[n].us_per_sweep = 1e3 * ms / m; }
            }
            out[n].rows = L.n; out[n].blocks = L.nnzA; out[n].lanes_per_row = lprA;
            out[n].sweeps_per_cycle = 2 * nu_at(l);         // (nu - 1) pre-sweeps + the residual + nu post-sweeps
            out[n].bytes_per_sweep = bytes_sweep(L);
        }
        return n;
    }

    struct TolGuard { double& tol; double keep; ~TolGuard() { tol = keep; } };      // puts cfg.pcg_rel_tol back on every way out of a probe that zeroes it
    // One PCG iteration kernel by kernel, in situ: `reps` iterations launched eagerly, the stopping test disabled, an event before
    // every launch (PF()).  Entry k of the result = the k-th launch of an iteration, averaged over the iterations.
    int profile_iteration(int reps, tsgo_prof_entry* out, int cap) override {
        if (!have_graph_data) return set_error(-3, "tsgo_profile_iteration: no graph set");
        HIP_OK(hipSetDevice(cfg.device));
        double chi2;
        if (int rc = do_linearize(&chi2)) return rc;      // valid operands, a built hierarchy; state slot 0 says "not done"
        TolGuard tol_guard{cfg.pcg_rel_tol, cfg.pcg_rel_tol};
        cfg.pcg_rel_tol = 0;
        reps = std::max(2, reps + (reps & 1));           // whole pairs: the state ring has two slots
        for (int j = 0; j < 4; ++j) if (int rc = launch_iteration(j & 1)) return rc;        // warm caches and clocks
        // Eager launches + event records are host-bound (~7 us each against kernels of 4-15 us): the stream is first blocked by a
        // kernel that waits kProfBlockMs on the constant-rate clock, the host enqueues everything behind it, and the device then
        // runs the queue back to back — what a hipGraph replay of the same iterations does.
        hipLaunchKernelGGL(k_wait_ms, dim3(1), dim3(64), 0, stream, (int)(kProfBlockUsPerLaunch * 40.0 * reps / 1000.0) + 2);
        prof_n = 0; prof_on = true;
        int rc = 0;
        for (int j = 0; j < reps && rc == 0; ++j) rc = launch_iteration(j & 1);
        PF(0, "", "end");
        prof_on = false;
        HIP_OK(hipStreamSynchronize(stream));
        if (rc) return rc;
        const size_t marks = prof_n - 1;
        if (marks == 0 || marks % (size_t)reps != 0) return set_error(-30, "tsgo_profile_iteration: the iterations did not launch the same kernels");
        const size_t per = marks / (size_t)reps;
        const int n = (int)std::min<size_t>(per, (size_t)cap);
        for (int k = 0; k < n; ++k) {
            double sum = 0;
            for (int j = 0; j < reps; ++j) {
                float ms = 0;
                HIP_OK(hipEventElapsedTime(&ms, prof[(size_t)j * per + k].e, prof[(size_t)j * per + k + 1].e));
                sum += ms;
            }
            const ProfMark& m = prof[k];
            std::memset(&out[k], 0, sizeof(out[k]));
            std::snprintf(out[k].name, sizeof(out[k].name), "%s", m.name);
            std::snprintf(out[k].where, sizeof(out[k].where), "%s", m.where);
            out[k].launches_per_iteration = 1; out[k].us = 1e3 * sum / reps; out[k].bytes = m.bytes;
        }
        cfg.pcg_rel_tol = tol_guard.keep;
        if (int rc2 = do_linearize(&chi2)) return rc2;   // leave a consistent state behind
        return n;
    }

    // which: 0 schur_lm, 1 schur_pose, 2 cg_update, 3 lin_lm, 4 lin_pose, 5 one whole PCG iteration, 6 multigrid setup, 7 the chi^2-only pass (rules = 2),
    // 8 the summary-only pass of tsgo_edge_report (engine_report.inc; reads what 7 reads plus the slot -> edge maps)
    int time_kernel(int which, int reps, double* us, double* bytes) override {
        if (!have_graph_data) return set_error(-3, "tsgo_time_kernel: no graph set");
        HIP_OK(hipSetDevice(cfg.device));
        double chi2;
        if (int rc = do_linearize(&chi2)) return rc;      // valid operands; state slot 0 says "not done"
        const double s = sizeof(T);
        const double El = (double)pr.n_lm_edges, P = pr.P, L = pr.L;
        const double od = od_slots_live(), b_lm = bytes_schur_lm(false), b_pose = bytes_schur_pose(false);
        const double b_upd = P * (3 + 3 + 6 + 4 * 3 * 2 - 3) * s;   // sz, z in; minv in; r p q x in+out (x,r,p,q), z out
        const double b_linlm = El * (4 + 4 * s + 4 * s) + P * 4 * s + L * (2 + 5 + 3) * s;
        const double b_linpose = El * (4 + 4 * s + 4 * s) + L * 7 * s + P * (4 + 18) * s + od * (4 + 9 * s + 3 * s);
        // whole iterations are timed with the stopping test disabled: a converged solve turns every kernel into an early exit
        TolGuard tol_guard{cfg.pcg_rel_tol, cfg.pcg_rel_tol};
        if (which == 5) cfg.pcg_rel_tol = 0;
        if (which == 8) {
            if (cfg.world > 1 || collective()) return set_error(-1, "tsgo_time_kernel: 8 (the edge report's pass): edge-sharded handles (world > 1) are not supported");
            if (int rc = report_prepare()) return rc;
        }
        if (which == 9) {
            if (!dogleg_rules()) return set_error(-1, "tsgo_time_kernel: 9 (the g'Hg pass) needs a handle created with rules = 3");
            if (int rc = report_prepare()) return rc;
            launch_dl_gradient();      // the gradient vectors of this linearisation (x and dl are whatever the last solve left: only the dots read them)
        }
        for (int pass = 0; pass < 2; ++pass) {
            const int n = pass == 0 ? 3 : reps;
            HIP_OK(hipEventRecord(ev[0], stream));
            for (int k = 0; k < n; ++k) {
                switch (which) {
                    case 0: launch_schur_lm(0, false, nullptr, ""); break;
                    case 1: launch_schur_pose(0, false, (const T*)nullptr, (T*)nullptr, false, false, ""); break;
                    case 2: {   // state slot 1 is never written here, slot 0 stays "iters = 0, not done"
                        const T tol2 = (T)0;
                        hipLaunchKernelGGL((k_cg_update<T>), dim3(nbC), dim3(kBlock), 0, stream, pr.P, nbP, (const CgState<T>*)st[0], (const T*)(sbuf + (size_t)pr.P * 3), (const T*)gpart[0], nbC,
                                           (const T*)sbuf, gpart[1], st[1], minv, r, p, q, x, zc, tol2, 1 << 30, (const T*)one_dev);
                        break;
                    }
                    case 3: launch_lin_lm(); break;
                    case 4: launch_lin_pose_only(); break;
                    case 7: if (!trial_rules()) return set_error(-1, "tsgo_time_kernel: 7 (the chi^2-only pass) needs a handle created with rules = 2 (or 3)"); launch_chi2(lm_red); break;
                    case 9: launch_ghg(dl_red + (size_t)3 * dl_nb()); break;
                    case 8: launch_edge_report(nullptr); break;
                    case 6: if (amg_on) { if (int rc = launch_amg_setup()) return rc; } break;
                    default: if (int rc = launch_iteration(0)) return rc; if (int rc = launch_iteration(1)) return rc; break;
                }
            }
            HIP_OK(hipEventRecord(ev[1], stream));
            HIP_OK(hipEventSynchronize(ev[1]));
            if (pass == 1) {
                float ms = 0;
                HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1]));
                const double per = which == 5 ? 2.0 * n : (double)n;
                *us = 1e3 * ms / per;
            }
        }
        cfg.pcg_rel_tol = tol_guard.keep;
        const double tab[10] = {b_lm, b_pose, b_upd, b_linlm, b_linpose, (amg_on ? 3.0 : 1.0) * (b_lm + b_pose) + b_upd, 0.0, bytes_chi2(), which == 8 ? bytes_report(false) : 0.0,
                                which == 9 ? bytes_ghg() : 0.0};
        *bytes = tab[std::min(std::max(which, 0), 9)];
        // leave a consistent state behind
        return do_linearize(&chi2);
    }
