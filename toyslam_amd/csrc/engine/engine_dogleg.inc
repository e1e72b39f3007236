// engine/engine_dogleg.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// rules = 3, Powell's dogleg trust-region loop (include/tsgo.h: tsgo_config.rules, tsgo_set_dogleg, tsgo_get_dogleg_trace; DESIGN.md section 20).
//
// One linearisation (lambda = 0, b zeroed at fixed vertices) and one solve give the Gauss-Newton step; every trial until a step is
// accepted is a combination c1 g + c2 d_gn of it and the gradient, applied from the snapshot of rules = 2 (k_lm_state) and judged by the
// chi^2-only pass (k_chi2).  A rejection shrinks the radius and costs one step kernel and one chi^2 pass: no linearisation, no hierarchy
// work, no solve.  Kernels: tsgo_dogleg_kernels.h.  The host steps around the launches are the ones rules 0 to 2 take (engine_solve.inc:
// fetch_partials, sum_partials, begin_trial, note_linearisation / note_trial / accepted, end_step_timing; engine_launch.inc: launch_backsub).
    // ---- what belongs to the HANDLE (tsgo_hip.hip lists the lifetimes): the parameters survive tsgo_set_graph; the trace is the last tsgo_optimize's
    tsgo_dogleg_params dogleg = default_dogleg();
    tsgo_dogleg_trace dl_trace{};
    static tsgo_dogleg_params default_dogleg() { tsgo_dogleg_params p; tsgo_default_dogleg(&p); return p; }
    int set_dogleg(const tsgo_dogleg_params& p) override { dogleg = p; return 0; }
    void get_dogleg(tsgo_dogleg_params* out) const override { *out = dogleg; }
    void get_dogleg_trace(tsgo_dogleg_trace* out) const override { *out = dl_trace; }

    // ---- per graph (null unless rules = 3; engine_graph.inc): the gradient as dense vectors and the partials of a solve's four scalars,
    // dl_red = [ g'g (dl_nb) | g'd (dl_nb) | d'd (dl_nb) | g'Hg, classes 0 .. 3 (nbP) | g'Hg, landmark priors (nbL) ]
    T *dl_gp = nullptr, *dl_gl = nullptr, *dl_red = nullptr;
    int dl_nb() const { return grid_for(std::max(pr.P, pr.L)); }
    size_t dl_red_size() const { return (size_t)3 * dl_nb() + nbP + std::max(nbL, 1); }
    int dl_alloc() {
        if (int rc = dalloc(&dl_gp, (size_t)pr.P * 3)) return rc;
        if (int rc = dalloc(&dl_gl, (size_t)std::max(pr.L, 1) * 2)) return rc;
        return dalloc(&dl_red, dl_red_size());
    }
    // g'Hg by the once-per-edge walk (tsgo_time_kernel 9 too): nbP partials at `out`, the landmark priors' nbL behind them
    // (f64 instantiations only: tsgo_create refuses rules = 3 with precision = 32, and the f32 engine launches none of the three)
    static constexpr bool kDoglegKernels = std::is_same<T, double>::value;
    void launch_ghg(T* out) {
        if constexpr (kDoglegKernels) launch_ghg_f64(out);
    }
    void launch_ghg_f64(T* out) {
        if (report_lm_priors()) pick<1, 2, 4, 8>(pr.by_lm.G, [&](auto g) { pick_rk([&](auto rk) {
            launch(k_dl_ghg_lm_prior<T, g, rk>, nbL, tl, (const T*)lmrec, (const uint32_t*)maps.rep_pl_edge, (const T*)dl_gl, out + nbP, lm_prior_args(), robust_args());
        }); });
        pick_edge_walk([&](auto g, auto general, auto pri) { pick_rk([&](auto rk) {
            launch(k_dl_ghg<T, g, general, pri, rk>, nbP, tp, to, (const T*)ps, (const T*)lmrec, maps.edge_maps(), (const T*)dl_gp, (const T*)dl_gl, out, general ? odom_analytic_flag() : 0,
                   pri ? pose_prior_args() : no_priors(), robust_args());
        }); });
    }
    void launch_dl_gradient() {
        if constexpr (kDoglegKernels) launch(k_dl_gradient<T>, dl_nb(), pr.P, pr.L, (const T*)part, (const T*)lmrec, (const T*)x, (const T*)dl, dl_gp, dl_gl, dl_red);
    }
    // what the edge report's summary pass reads without its class partials, one number per workgroup out, and the gradient: the walking
    // pose's own, a landmark's per LM edge, the neighbour's per evaluated pose-pose slot
    double bytes_ghg() {
        const double v = sizeof(T);
        return bytes_report(false) - (double)(nbP * kEdgeClasses + (report_lm_priors() ? nbL : 0)) * sizeof(ReportPartial<T>) + (double)(nbP + (report_lm_priors() ? nbL : 0)) * v +
               pr.P * 3.0 * v + (double)pr.n_lm_edges * 2.0 * v + od_slots_live() * 3.0 * v + (report_lm_priors() ? pr.L * 2.0 * v : 0.0);
    }

    // What a solve leaves for its trials: the snapshot, d_gn (x, and dl by the back-substitution with step 0, as solve_step does), the
    // gradient vectors and the four scalars.  Nothing enters the warm start's history.
    struct DoglegScalars { double gg = 0, gd = 0, dd = 0, ghg = 0; };
    int dl_after_solve(DoglegScalars* out) {
        begin_trial();
        launch_backsub<1>(T(0), npart + nbC, T(0), nullptr);
        launch_dl_gradient();
        launch_ghg(dl_red + (size_t)3 * dl_nb());
        const int nb = dl_nb(), nlp = report_lm_priors() ? nbL : 0;
        const T* h = nullptr;
        if (int rc = fetch_partials(dl_red, (size_t)3 * nb + nbP + nlp, &h)) return rc;
        out->gg = sum_partials(h, 0, nb); out->gd = sum_partials(h, (size_t)nb, nb); out->dd = sum_partials(h, (size_t)2 * nb, nb);
        out->ghg = sum_partials(h, (size_t)3 * nb, nbP) + sum_partials(h, (size_t)3 * nb + nbP, nlp);
        return 0;
    }
    // the trial step from the snapshot and chi^2 there, one report
    int dl_trial(double c1, double c2, double* chi2_trial, hipEvent_t after) {
        if constexpr (kDoglegKernels) launch(k_dl_step<T>, dl_nb(), pr.P, pr.L, (T)c1, (T)c2, (const T*)dl_gp, (const T*)x, (const T*)dl_gl, (const T*)dl, (const T*)snap_ps, (const T*)snap_lm, ps, theta, lmrec);
        launch_chi2(lm_red);
        const T* h = nullptr;
        if (int rc = fetch_partials(lm_red, (size_t)nbP, &h, after)) return rc;
        *chi2_trial = sum_partials(h, 0, nbP);
        return 0;
    }

    // The loop.  need_solve: at the start and after every accepted step; a rejected trial leaves the linearisation, d_gn and the scalars
    // in place for the next one.  Step timing (end_step_timing): a trial that reused a solve recorded evc[2] and evc[3] alone and adds to
    // ms_update alone.
    int dogleg_loop(int iterations, tsgo_stats& s) {
        if (int rc = report_prepare()) return rc;      // the slot -> edge maps of the once-per-edge walk
        tsgo_dogleg_trace& tr = dl_trace;
        double radius = dogleg.radius0, err = 0;
        DoglegScalars q;
        bool need_solve = true;
        lambda = 0;
        tr.radius_last = radius;
        for (int it = 0; it < iterations; ++it) {
            const bool traced = it < TSGO_MAX_TRACE, solved = need_solve;
            int cg = 0;
            if (solved) {
                int fail = 0;
                HIP_OK(hipEventRecord(evc[0], stream));
                if (int rc = do_linearize(&err)) return rc;
                HIP_OK(hipEventRecord(evc[1], stream));
                if (int rc = do_solve(&cg, &fail)) return rc;
                s.pcg_iters_total += cg;
                if (fail != 0) {
                    note_linearisation(s, it, err);
                    if (traced) { s.pcg_iters[it] = cg; tr.solved[it] = 1; tr.radius[it] = radius; }
                    tr.trials = it + 1; ++tr.solves;
                    s.stop_reason = TSGO_STOP_SOLVER;
                    break;
                }
                if (int rc = dl_after_solve(&q)) return rc;
                ++tr.solves;
                need_solve = false;
            }
            HIP_OK(hipEventRecord(evc[2], stream));
            note_linearisation(s, it, err);
            tr.trials = it + 1;
            if (traced) {
                s.pcg_iters[it] = cg;
                tr.solved[it] = solved ? 1 : 0; tr.radius[it] = radius; tr.gg[it] = q.gg; tr.gHg[it] = q.ghg; tr.gd[it] = q.gd; tr.dd[it] = q.dd;
            }
            if (q.gg == 0) {      // a stationary point: no step (kind 0, zero step, pred and gain)
                if (traced) s.lm_chi2_trial[it] = err;
                s.last_delta_norm = 0;
                if (reports()) HIP_OK(hipEventRecord(evc[3], stream));      // (no trial closes this set)
                if (int rc = end_step_timing(s, solved)) return rc;
                s.stop_reason = TSGO_STOP_CONVERGED;
                break;
            }
            // the step: Gauss-Newton inside the region, else the gradient step to the boundary, else the dogleg between the Cauchy point and d_gn
            const double n = std::sqrt(q.gg), alpha = q.gg / q.ghg;
            int kind; double c1, c2;
            if (std::sqrt(q.dd) <= radius) { kind = 0; c1 = 0; c2 = 1; }
            else if (alpha * n >= radius) { kind = 2; c1 = radius / n; c2 = 0; }
            else {
                const double a = q.dd - 2 * alpha * q.gd + alpha * alpha * q.gg, h = alpha * q.gd - alpha * alpha * q.gg, c = alpha * alpha * q.gg - radius * radius;
                const double beta = (-h + std::sqrt(h * h - a * c)) / a;
                kind = 1; c1 = alpha * (1 - beta); c2 = beta;
            }
            // pred = 2 b'd - d'Hd with H d_gn = b (true to pcg_rel_tol): b'H d_gn = g'g, d_gn'H d_gn = g'd_gn
            const double pred = 2 * (c1 * q.gg + c2 * q.gd) - (c1 * c1 * q.ghg + 2 * c1 * c2 * q.gg + c2 * c2 * q.gd);
            const double step_norm = std::sqrt(c1 * c1 * q.gg + 2 * c1 * c2 * q.gd + c2 * c2 * q.dd);
            double trial = 0;
            if (int rc = dl_trial(c1, c2, &trial, step_end_event())) return rc;
            if (int rc = end_step_timing(s, solved)) return rc;
            const double gain = note_trial(s, it, err, pred, trial);
            s.last_delta_norm = step_norm;
            if (traced) { tr.kind[it] = kind; tr.step_norm[it] = step_norm; }
            if (!(gain >= 0.25)) radius = 0.25 * step_norm;
            else if (gain > 0.75 && kind != 0) radius = std::min(2 * radius, dogleg.radius_max);
            tr.radius_last = radius;
            if (accepted(gain, pred)) {
                if (step_norm < kDeltaTol || err - trial <= dogleg.chi2_rel_tol * err) { s.stop_reason = TSGO_STOP_CONVERGED; break; }
                need_solve = true;
            } else {
                if (int rc = lm_restore()) return rc;
                ++s.steps_rejected;
                if (!(radius >= dogleg.radius_min)) { s.stop_reason = TSGO_STOP_RADIUS; break; }
            }
        }
        return flush_step_timing(s);
    }
