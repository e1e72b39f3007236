// engine/engine_solve.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// the Gauss-Newton loop: linearise, warm start, PCG (bursts, hipGraph replay, paced eager launches), back-substitution and update, stop rules.
// (rules = 3, the dogleg loop, is engine_dogleg.inc; tsgo_optimize below picks the loop.)
    int capture_cg_graph() {
        hipGraph_t graph = nullptr;
        HIP_OK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        for (int j = 0; j < chunk(); ++j) if (int rc = launch_iteration(j & 1)) return rc;     // never collective: no RCCL call is captured
        HIP_OK(hipStreamEndCapture(stream, &graph));
        HIP_OK(hipGraphInstantiate(&cg_graph, graph, nullptr, nullptr, 0));
        HIP_OK(hipGraphDestroy(graph));
        return 0;
    }

    // The host's side of a step report (k_report): polls the report word until it holds `seq`, with do_solve_paced's pause / yield pattern
    // and its 30 s limit — an error return, never an endless wait.  The partials are then in rep_data().
    int wait_report(uint64_t seq) {
        const auto w0 = std::chrono::steady_clock::now();
        long spins = 0;
        while (__atomic_load_n(h_rep, __ATOMIC_ACQUIRE) < seq) {
            __builtin_ia32_pause();
            if ((spins & 0x3f) == 0x3f) std::this_thread::yield();
            if ((++spins & 0xfffff) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count() > 30.0)
                return set_error(-20, "step report: the device stopped reporting (30 s without a report)");
        }
        return 0;
    }
    // The most partials one fetch brings back: the report buffer and the copy path's pinned destination (h_scratch) are both sized by it.
    size_t partials_max() const { return std::max({(size_t)nbP, (size_t)nbC + nbL, trial_rules() ? lm_red_size() : (size_t)0, dogleg_rules() ? dl_red_size() : (size_t)0}); }
    // n partials at src to the host, *h.  Step reports: the report is launched here, unless the caller `sent` it earlier in the chain
    // (do_linearize), and `after`, a step's closing event, is recorded right behind it.  Otherwise copy + synchronise into h_scratch.
    int fetch_partials(const T* src, size_t n, const T** h, hipEvent_t after = nullptr, uint64_t sent = 0) {
        if (reports()) {
            const uint64_t rseq = sent ? sent : launch_report(src, n);
            if (after) HIP_OK(hipEventRecord(after, stream));
            if (int rc = wait_report(rseq)) return rc;
            *h = rep_data();
        } else {
            HIP_OK(hipMemcpyAsync(h_scratch, src, sizeof(T) * n, hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            *h = h_scratch;
        }
        return 0;
    }
    // ... and their sum: in double, ascending from `from`
    static double sum_partials(const T* h, size_t from, int count) { double v = 0; for (int k = 0; k < count; ++k) v += (double)h[from + k]; return v; }
    // one linearisation; chi2 on the host
    int do_linearize(double* chi2) {
        launch_lin();
        if (int rc = allreduce(part, (size_t)pr.P * 18 + nbP)) return rc;
        // Step reports: the chi^2 partials are final here (k_lin_pose wrote them; nothing below touches them).  Ahead of a paced solve the
        // report leaves now: the host's wait at the end of this function is then over while k_pose_finalize, or a hierarchy build, still runs,
        // and the solve's first launches queue up behind them.  Ahead of a burst or a replay it leaves at the end of the chain, so that the
        // host goes on when the stream is empty, as it does after a copy + synchronise: those paths time their solves by the wall clock
        // (do_solve_once: dev_us_per_iter) and must keep seeing the solve alone.
        const T* chi_part = part + (size_t)pr.P * 18;
        const uint64_t early = reports() && paced() ? launch_report(chi_part, (size_t)nbP) : 0;
        launch_finalize();
        if (amg_on) {
            // The Galerkin hierarchy is a preconditioner, not the operator: level 0 (the Schur products, its diagonal
            // inverse) is always the current linearisation, the coarse matrices may lag.  They are rebuilt when they
            // have served hier_max_age solves or the last solve took kHierSlack iterations more than the first one did.
            // ... and a young graph's linearisations move faster than a hierarchy ages (Huber weights switch by the thousand in the first
            // steps from a front-end's estimates: 22 / 23 / 30 iterations on one hierarchy where fresh ones take 22 / 19 / 18 at 100k poses):
            // the first kYoungLins linearisations of a graph share a hierarchy between two at most (profiles/r03z_early_iterations.txt)
            const int max_age = mem.n_lins < kYoungLins ? std::min(hier_max_age, kYoungMaxAge) : hier_max_age;
            ++mem.n_lins;
            const bool refresh = mem.hier_age < 0 || mem.hier_age >= max_age || mem.iters_last > mem.iters_fresh + hier_slack || mem.iters_last > kHierFreshAbove;
            if (refresh) {
                if (int rc = rebuild_hierarchy()) return rc;
                if (mem.lin_count++ % kRhoEvery == 0) {
                    if (int rc = estimate_damping()) return rc;
                    if (int rc = launch_bottom_setup()) return rc;      // the dense bottom operator holds the last level's damping
                    launch_finalize();        // zc = omega_0 Minv r with the fresh omega_0
                }
            }
        }
        const T* h = nullptr;
        if (int rc = fetch_partials(chi_part, (size_t)nbP, &h, nullptr, early)) return rc;
        *chi2 = sum_partials(h, 0, nbP);
        return 0;
    }

    // PCG; if the multigrid-preconditioned solve breaks down (indefinite preconditioner), the solve is
    // repeated from the same right-hand side with the block-Jacobi preconditioner.
    bool inject_armed = false;
    // Warm start (cfg.warm_start): the Gauss-Newton update takes kStepScale of the solved delta, so (1 - kStepScale) of it
    // is still to go at the next linearisation.  x0 = that remainder, r = b~ - S x0 (one extra product), and the stopping
    // rule keeps measuring against the right-hand side: gamma0 is scaled by (b^T D^-1 b) / (r0^T D^-1 r0).
    // the highest order launch_warm allows, and how many orders have an error to choose by
    void warm_orders(int& n_max, int& n_tested) const {
        n_max = std::max(1, std::min({mem.n_prev, (int)cfg.warm_start, kMaxWarm}));
        n_tested = std::min(mem.n_tested, n_max);
    }
    int launch_warm() {
        // x0 = the un-taken remainder of the previous step, (1 - step) d1, at order 1; higher orders continue the trend of the last
        // deltas as well (order 2: (1 - step) (d1 + c1) with c1 = d1 - (1 - step) d2, what the last step added over ITS prediction).
        // cfg.warm_start caps the order; below the cap the kernel takes the order that would have predicted the last delta best
        // (k_save_x measured every order then): high orders win once the iteration is smooth (50 iterations at 100 k poses:
        // 849 PCG iterations at order 2, 724 at order 6) and lose while Huber weights still switch (profiles/r03w_warm_start_order.txt).
        WarmTerms<T> w{};
        warm_coefficients(w);
        for (int j = 0; j < kMaxWarm; ++j) w.v[j] = hist[j];
        warm_orders(w.n_max, w.n_tested);
        w.errpart = warm_err; w.nb_err = nbC;
        launch_pack_x(w, warm_order_dev);
        if (int rc = launch_matvec(0)) return rc;
        hipLaunchKernelGGL((k_warm_residual<T>), dim3(nbC), dim3(kBlock), 0, stream, pr.P, (const T*)sbuf, (const T*)minv, r, zc, (const T*)(amg_on ? omega_dev : one_dev), npart, amg_on && low_cycle ? zc32 : (float*)nullptr);
        hipLaunchKernelGGL((k_warm_scale<T>), dim3(1), dim3(kBlock), 0, stream, nbC, (const T*)gpart[0], (const T*)npart, amg_on ? (T*)nullptr : gpart[0], gscale_dev,
                           amg_on ? st[0] : (CgState<T>*)nullptr, (T)(cfg.pcg_rel_tol * cfg.pcg_rel_tol));
        return 0;
    }
    // The two steps the rungs of do_solve's ladder are made of: the hierarchy rebuilt for the current linearisation (age 0 BEFORE the solve that
    // follows, which files its count under that age), and the solve repeated from the plain right-hand side (stagnation, 3, is a breakdown, 1).
    int rebuild_hierarchy() { if (int rc = launch_amg_setup()) return rc; mem.hier_age = 0; return 0; }
    int solve_again(int* iters, int* fail) {
        launch_finalize();
        if (int rc = do_solve_once(iters, fail)) return rc;
        if (*fail == 3) *fail = 1;
        return 0;
    }
    int do_solve(int* iters, int* fail) {
        const bool warmed = cfg.warm_start && mem.have_prev && step_scale() < 1.0;      // a full step (rules = 1, lr = 1) leaves no remainder to start from
        if (warmed) { if (int rc = launch_warm()) return rc; }
        if (warmed && mem.carried) {
            // The history is the previous REQUEST's: it continues this one only if the client sent back the estimates it was
            // returned.  k_warm_scale leaves b'D^-1 b / r0'D^-1 r0, or 1 when the start is no better than zero: then the history
            // is dropped and the solve starts cold (every shard reads the same all-reduced numbers and decides alike).
            T gs = 0;
            if (int rc = copy_sync(&gs, gscale_dev, sizeof(T), hipMemcpyDeviceToHost)) return rc;
            if (!(gs > T(1))) { launch_finalize(); mem.have_prev = false; mem.n_prev = 0; mem.n_tested = 0; ++n_carry_dropped; mem.n_lins = 1; }      // ... and the graph is a young one after all
        }
        mem.carried = false;
        if (int rc = do_solve_once(iters, fail)) return rc;
        if (solve_timing && warmed) {
            int order = 0; T gs = 0; std::vector<T> e((size_t)kMaxWarm * nbC);
            if (int rc = copy_sync(&order, warm_order_dev, sizeof(int), hipMemcpyDeviceToHost)) return rc;
            if (int rc = copy_sync(&gs, gscale_dev, sizeof(T), hipMemcpyDeviceToHost)) return rc;
            if (int rc = copy_sync(e.data(), warm_err, e.size() * sizeof(T), hipMemcpyDeviceToHost)) return rc;
            std::fprintf(stderr, "[tsgo] warm start: order %d of %d tested, b'D^-1 b / r0'D^-1 r0 = %.3e, %d PCG iterations; prediction errors of the last delta:", order, mem.n_tested, (double)gs, *iters);
            for (int m = 0; m < mem.n_tested; ++m) { double s = 0; for (int k = 0; k < nbC; ++k) s += (double)e[(size_t)m * nbC + k]; std::fprintf(stderr, " %.3e", s); }
            std::fprintf(stderr, "\n");
        }
        if (say_env && *fail != 0) {      // what the device state says about a solve that failed
            CgState<T> hs;
            if (int rc = copy_sync(&hs, st[0], sizeof(hs), hipMemcpyDeviceToHost)) return rc;
            double gamma = 0, delta = 0;
            if (amg_on) {      // the partials the failing k_cg_step read are still in place (it returned before writing anything)
                std::vector<T> pz((size_t)nbP), pd((size_t)nbP);
                if (int rc = copy_sync(pz.data(), rzpart, pz.size() * sizeof(T), hipMemcpyDeviceToHost)) return rc;
                if (int rc = copy_sync(pd.data(), sbuf + (size_t)pr.P * 3, pd.size() * sizeof(T), hipMemcpyDeviceToHost)) return rc;
                for (int k = 0; k < nbP; ++k) { gamma += (double)pz[(size_t)k]; delta += (double)pd[(size_t)k]; }
            }
            const double beta = hs.gamma_old != T(0) ? gamma / (double)hs.gamma_old : 0.0;
            std::fprintf(stderr, "[tsgo] solve failed: fail %d after %d iterations (%s preconditioner, %s start, hierarchy age %d): gamma_old %.6e alpha_old %.6e gamma0 %.6e | now gamma = r'z %.6e, delta = z'Sz %.6e, beta %.4e, delta - beta gamma / alpha_old = %.6e\n", *fail, *iters,
                         amg_on ? "multigrid" : "block-Jacobi", warmed ? "warm" : "cold", mem.hier_age, (double)hs.gamma_old, (double)hs.alpha_old, (double)hs.gamma0, gamma, delta, beta,
                         delta - beta * gamma / (double)hs.alpha_old);
        }
        if (*fail == 3 && amg_on) *fail = 1;          // stagnation under the multigrid cycle (mapped after the trace above, which prints 3)
        // ---- The ladder: a multigrid solve that broke down (fail 1) is repeated on a hierarchy rebuilt under the next remedy, rung by rung.
        // Rung 1, packed -> f32: the only rung a solve that SUCCEEDED takes too (by its iteration count); only a failed one is repeated.
        if (amg_on && mem.cy16 && (*fail != 0 || *iters > kPackedCycleMaxIters)) {
            // Packed half floats round every block of the cycle's operators to 11 bits.  A coarse operator of a nearly singular
            // system (an odometry-only chain under the analytic Jacobians: a 24k-link beam) is a difference of large entries; at
            // that precision it stops being positive definite and the solve breaks down or crawls (20 000 iterations where the
            // f32 copies need 1 500; profiles/r03k_hard_chain.txt).  Such a graph shows itself by its iteration count: from here
            // on its cycle reads f32 copies (until the next tsgo_set_graph), and a solve that failed is repeated with them.
            mem.cy16 = false; ++n_cycle_f32_switches;
            if (cg_graph) { (void)hipGraphExecDestroy(cg_graph); cg_graph = nullptr; optimize_calls_on_tables = 1; }     // it holds the packed kernels; re-captured at the next tsgo_optimize
            if (say_env) std::fprintf(stderr, "[tsgo] %d PCG iterations (fail %d) with the packed cycle format: this structure's cycle switches to f32 copies\n", *iters, *fail);
            if (int rc = rebuild_hierarchy()) return rc;
            mem.iters_fresh = 0;
            if (*fail != 0) { if (int rc = solve_again(iters, fail)) return rc; }
        }
        const int age_used = mem.hier_age;
        if (amg_on) { mem.iters_last = *iters; if (mem.hier_age == 0) mem.iters_fresh = *iters; if (mem.hier_age >= 0) ++mem.hier_age; }      // (the solve that stands so far; the rungs below book their own)
        if (*fail == 1 && amg_on && age_used > 0) {
            // Rung 2, stale hierarchy (its solve is booked as a fresh hierarchy's first whether it succeeded or not).  The hierarchy that failed
            // was built for an earlier linearisation (the lag rule).  Before giving the multigrid cycle up for this solve, build it for THIS one
            // and solve again: on beam-like odometry chains (analytic Jacobians) a lagged hierarchy can be indefinite where a fresh one takes
            // 1 400 iterations and block-Jacobi does not finish in 20 000.
            ++n_hier_retries;
            if (int rc = rebuild_hierarchy()) return rc;
            if (int rc = solve_again(iters, fail)) return rc;
            mem.iters_last = *iters; mem.iters_fresh = *iters; mem.hier_age = 1;
        }
        // Rungs 3 and 4, diagonal shifts (skipped under the injection hook; a shift already in force is not repeated; booked only on success).
        // Still broken down (r^T M^-1 r < 0) on a hierarchy built for THIS linearisation, in f32 copies: its level-0 matrix is S rounded to f32, and
        // where the smooth bending modes of several hundred thousand poses carry 1e-6 per pose that rounding can leave it, its Galerkin products
        // and the cycle INDEFINITE (a 372k-pose graph: 15 500 block-Jacobi iterations per solve, profiles/r04p_indefinite_cycle_f32_hierarchy.txt).
        // The hierarchy's copy of S gets its diagonal raised by 1e-6, then 1e-5, of itself: positive definite again, at some more PCG iterations
        // (42-63 where an f64 hierarchy takes 25-34).  The raise holds until the next tsgo_set_graph, refill or new structure alike (a refilled
        // handle does what a fresh one does): a structure that needs it pays the failed solve again on every request.
        for (const double shift : {1e-6, 1e-5}) {
            if (!(*fail == 1 && amg_on) || hook_inject_amg_failure) break;
            if (mem.hier_shift >= shift) continue;
            mem.hier_shift = shift; ++n_hier_shifts;
            if (say_env) std::fprintf(stderr, "[tsgo] multigrid cycle indefinite on a fresh hierarchy: its level-0 matrix gets its diagonal raised by %.0e from here on\n", shift);
            if (int rc = rebuild_hierarchy()) return rc;
            if (int rc = solve_again(iters, fail)) return rc;
            if (*fail == 0) { mem.iters_last = *iters; mem.iters_fresh = *iters; mem.hier_age = 1; }
        }
        // test hook: TSGO_INJECT_AMG_FAILURE=1 treats the first multigrid solve of every tsgo_optimize call as broken down, so that the
        // block-Jacobi repeat below runs on a graph where the cycle is perfectly healthy (tests/test_gpu_parity.py)
        if (hook_inject_amg_failure && amg_on && inject_armed) { inject_armed = false; *fail = 1; }
        if (*fail == 1 && amg_on) {      // Last rung, block-Jacobi: cycle and replay are set aside for this one solve
            ++n_fallbacks;
            mem.hier_age = -1;                               // whatever went wrong, start from a fresh hierarchy next time
            const bool keep = amg_on; hipGraphExec_t g = cg_graph;
            amg_on = false; cg_graph = nullptr;          // eager block-Jacobi launches
            launch_finalize();
            const int rc = do_solve_once(iters, fail);
            amg_on = keep; cg_graph = g;
            return rc;
        }
        return 0;
    }
    // Eager launches, one device, multigrid cycle: the host thread stays ONE iteration ahead of the device instead of predicting a burst.
    // The gate (first kernel) of every iteration writes to pinned host memory that it has run and what it saw; the host enqueues
    // iteration j + 1 when the gate of iteration j has run (90 us of launches against the 217 us the device then spends on j) and
    // stops at the first gate that reports `done`.  What is wasted past convergence is the rest of that one iteration (29 kernels that
    // exit at once, 43 us) instead of the two or three a predicted burst over-provisions, an under-provisioned burst (the device idle
    // while the host enqueues more: 0.4 ms) cannot happen, and the iteration count and failure flag arrive with the report: the stream is
    // not drained at the end of the solve — the back-substitution queues up behind the last exits (profiles/r03z_paced_eager.txt).
    int do_solve_paced(int* iters, int* fail) {
        uint64_t* hw = reinterpret_cast<uint64_t*>(h_flag);
        if (paced_base > 0x70000000u) {      // (wrap-around: once per 4e9 iterations) nothing may be in flight when the numbering restarts
            HIP_OK(hipStreamSynchronize(stream));
            paced_base = 0; __atomic_store_n(hw, (uint64_t)0, __ATOMIC_SEQ_CST);
        }
        const uint32_t base = paced_base;
        const bool timing = solve_timing;
        const auto w0 = std::chrono::steady_clock::now();
        auto since = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - w0).count(); };
        int launched = 0, seen_last = 0; long spins = 0;
        double t_last_gate = 0;        // when the newest gate was seen (or the last launch made): a healthy long solve keeps moving this
        double t_first_gate = -1;      // when the first gate of this solve was seen
        uint64_t w = 0;
        for (;;) {
            w = __atomic_load_n(hw, __ATOMIC_ACQUIRE);      // seq << 32 | done << 31 | fail << 28 | iterations completed (k_iter_gate)
            const int32_t rel = (int32_t)((uint32_t)(w >> 32) - base);
            const int seen = rel > 0 ? (int)rel : 0;          // reports of earlier solves count as "nothing seen yet"
            if (seen != seen_last) { seen_last = seen; t_last_gate = since(); if (t_first_gate < 0) t_first_gate = t_last_gate; }
            if (seen > 0 && ((w >> 31) & 1)) break;
            if (launched - seen < pace_lead) {
                if (launched > cfg.pcg_max_iters + 4) { paced_base = base + (uint32_t)launched; return set_error(-20, "PCG did not terminate"); }
                if (int rc = launch_iteration(launched & 1, (int)(base + (uint32_t)launched + 1u))) { paced_base = base + (uint32_t)launched + 1u; return rc; }
                ++launched; spins = 0; t_last_gate = since();
            } else {
                __builtin_ia32_pause();
                if ((spins & 0x3f) == 0x3f) std::this_thread::yield();      // the device needs ~120 us before the next iteration has to be on its way: other threads may have the core
                if ((++spins & 0xfffff) == 0 && since() - t_last_gate > 30e6) { paced_base = base + (uint32_t)launched; return set_error(-20, "PCG: the device stopped reporting (30 s without a gate)"); }
            }
        }
        paced_base = base + (uint32_t)launched;
        solve_done((int)(w & 0x0fffffffu), (int)((w >> 28) & 7), iters, fail);
        // Under step reports the linearisation's last kernels, or a hierarchy build, may still have been running when this solve was enqueued:
        // its time per iteration is counted from its first gate (n iterations lie between the first gate and the one that reports `done`)
        const double wall = since() - (reports() && t_first_gate > 0 ? t_first_gate : 0.0);
        if (timing) std::fprintf(stderr, "[tsgo] solve (paced): %d iterations launched, done reported after %d at %.0f us\n", launched, *iters, wall);
        // a host that cannot stay ahead shows as iterations that take longer than the burst path measured: then the handle goes over to replay
        if (cfg.use_graphs == 2 && *iters >= 8 && !*fail && mem.ref_us_per_iter > 0 && !hook_force_paced) {
            if (wall / *iters > 1.3 * mem.ref_us_per_iter) { if (++mem.n_paced_slow >= 3) host_slow = true; } else mem.n_paced_slow = 0;
        }
        return 0;
    }
    // (only where the structure's first solves showed a host with room to spare: on a 150-pose graph an iteration is 20 kernels at the floor, 74 us,
    // and waiting for a gate before enqueueing the next iteration would expose the host's 60 us every time: use_graphs = 0 keeps the predicted burst there)
    bool paced() const {
        if (!amg_on || cg_graph || collective() || cfg.use_graphs == 1 || prof_on || h_flag == nullptr) return false;
        if (hook_force_paced) return true;       // test hook (TSGO_TESTING builds): the paced path from the first solve on
        return mem.n_decided >= kDecideSolves && 2 * mem.n_slow_seen <= kDecideSolves && !host_slow;
    }

    void solve_done(int n, int failed, int* iters, int* fail) {      // what every solve ends with: the caller's verdict, the next burst's predictors
        *iters = n; *fail = failed;
        mem.predicted_cg = n;
        if (amg_on && mem.hier_age >= 0 && mem.hier_age < kAgeSlots) mem.iters_by_age[mem.hier_age] = failed ? 0 : n;
    }
    // PCG until the device state says done.  The state ring is at slot 0 on entry and on exit.
    int do_solve_once(int* iters, int* fail) {
        if (paced()) return do_solve_paced(iters, fail);
        int launched = 0;
        const int ch = chunk();
        // chunks before the first look at the device state.  An iteration past convergence costs ~40 us (its kernels exit
        // at once), a look costs about as much plus an idle gap: under the multigrid cycle, where counts move by one or
        // two between solves, the burst aims one iteration past the prediction (a solve on a fresh hierarchy is predicted
        // by the last fresh one, an aged one by the previous solve + 1); block-Jacobi counts are in the thousands and
        // drift, so that burst stops at 90 %.
        // Under the lag rule the counts repeat from one hierarchy to the next (15 15 16 17 | 15 15 16 17 at 100k poses): the best
        // predictor of a solve is the solve of the same age on the previous hierarchy.
        const int by_age = (amg_on && mem.hier_age >= 0 && mem.hier_age < kAgeSlots) ? mem.iters_by_age[mem.hier_age] : 0;
        const int pred = amg_on ? (by_age > 0 ? by_age : (mem.hier_age == 0 && mem.iters_fresh > 0 ? mem.iters_fresh : mem.predicted_cg + 1)) : mem.predicted_cg;
        int burst = amg_on ? std::max(1, (pred + 1 + ch - 1) / ch) : std::max(1, (int)(0.9 * pred) / ch);
        const bool timing = solve_timing;
        const auto w0 = std::chrono::steady_clock::now();
        auto since = [&] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - w0).count(); };
        for (;;) {
            for (int b = 0; b < burst; ++b) {
                if (cg_graph) HIP_OK(hipGraphLaunch(cg_graph, stream));
                else for (int j = 0; j < ch; ++j) if (int rc = launch_iteration(j & 1)) return rc;
                launched += ch;
            }
            const double t_enq = since();
            if (timing) std::fprintf(stderr, "[tsgo] solve: %d chunk(s) enqueued at %.0f us", burst, t_enq);
            if (!cg_graph && amg_on && burst >= 4 && dev_us_per_iter > 0) {      // an eager burst of >= 8 iterations: was the host well ahead of the device?
                const double host_us_per_iter = t_enq / (burst * ch);
                const double share = host_us_per_iter / dev_us_per_iter;
                if (mem.n_decided < kDecideSolves) {      // the structure's first solves settle it (within a bench's warm-up, a request's first iterations): no flip in mid-run
                    mem.n_slow_seen += share > kHostSlowFraction;
                    if (++mem.n_decided == kDecideSolves && 2 * mem.n_slow_seen > kDecideSolves) host_slow = true;
                } else if (share > 0.95) { if (++mem.n_host_slow >= 3) host_slow = true; } else mem.n_host_slow = 0;      // later only outright starvation (a profiler attached, cores taken away)
            }
            if (cg_graph) replayed = true;
            burst = 1;
            HIP_OK(hipMemcpyAsync(h_state, st[0], sizeof(CgState<T>), hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            if (timing) std::fprintf(stderr, ", drained at %.0f us (iters %d done %d)\n", since(), h_state->iters, h_state->done);
            if (h_state->done) break;
            if (launched > cfg.pcg_max_iters + 2 * ch) return set_error(-20, "PCG did not terminate");
        }
        if (amg_on && h_state->iters >= 4 && !h_state->fail) { dev_us_per_iter = since() / h_state->iters; if (!cg_graph) mem.ref_us_per_iter = mem.ref_us_per_iter > 0 ? std::min(mem.ref_us_per_iter, dev_us_per_iter) : dev_us_per_iter; }      // (an upper bound: the solve's wall time over its iterations)
        solve_done(h_state->iters, h_state->fail, iters, fail);
        return 0;
    }

    // The solved delta in x enters the warm start's history (k_save_x; fused: k_save_update, which also takes the step): the oldest buffer
    // takes it, the orders that can be tested on it leave their prediction errors in warm_err, and the three counters move.  (Also what
    // tsgo_testing_warm_start plants a history with, engine_testing.inc.)
    void record_delta(bool fused, T step) {
        std::rotate(hist, hist + kMaxWarm - 1, hist + kMaxWarm);      // the oldest buffer takes this delta; hist[1..] are the deltas before it
        WarmTerms<T> w{};
        warm_coefficients(w);
        for (int j = 0; j + 1 < kMaxWarm; ++j) w.v[j] = hist[j + 1];
        w.n_max = std::min({mem.n_prev, (int)cfg.warm_start, kMaxWarm - 1});      // orders that can be tested on this delta
        if (fused) launch_save_update(w, hist[0], warm_err, step);
        else launch_save_x(w, hist[0], warm_err);
        mem.n_tested = w.n_max; mem.have_prev = true; mem.n_prev = std::min(mem.n_prev + 1, kMaxWarm);
    }
    // ... or the solved delta enters nothing (a probe, a trial's full step): k_pack_x without a history, and the history is forgotten
    void forget_warm_history() {
        launch_pack_x(WarmTerms<T>{}, (int*)nullptr);
        mem.have_prev = false; mem.n_prev = 0; mem.n_tested = 0;
    }

    // landmarks: dl = u - Dl^-1 W^T x (+ optional update); poses: update.  Returns ||delta_p||^2 (identical on every
    // rank: pose vectors are replicated) and THIS rank's ||delta_l||^2 (landmark deltas are shard-local).
    // Step reports (one-shard handles): a step that is taken runs k_save_x and k_pose_update as ONE launch in front of the landmark pass (which
    // reads zc and lmrec, neither ps nor theta), the partials come back through k_report, and `after` (the step's closing event) is recorded behind it.
    int do_backsub_update(T step, double* np2_out, double* nl2_local_out, hipEvent_t after = nullptr) {
        const bool fused = reports() && step != T(0);
        if (step != T(0)) record_delta(fused, step);
        else forget_warm_history();      // a probe (step 0) leaves nothing to carry over
        launch_backsub<1>(step, npart + nbC, T(0), nullptr);
        if (!fused) hipLaunchKernelGGL((k_pose_update<T>), dim3(nbC), dim3(kBlock), 0, stream, pr.P, x, ps, theta, step, npart);
        const int nl = lm_nl();
        const T* h = nullptr;
        if (int rc = fetch_partials(npart, (size_t)(nbC + nl), &h, after)) return rc;
        *np2_out = sum_partials(h, 0, nbC); *nl2_local_out = sum_partials(h, (size_t)nbC, nl);
        return 0;
    }
    // Sum of the ranks' landmark-delta norms.  The stop rule ||delta|| < 1e-3 (OptimizerCpu.h:173) can only fire when the
    // pose part alone is already below the tolerance, and the pose part is known on every rank: this collective runs
    // when that happens and once at the end of tsgo_optimize for the reported norm, not once per iteration.
    int landmark_norm_allreduce(double* nl2) {
        if (!collective()) return 0;
        T* d = npart;         // one-element device scratch (its partials were consumed by do_backsub_update)
        T v = (T)*nl2;
        HIP_OK(hipMemcpyAsync(d, &v, sizeof(T), hipMemcpyHostToDevice, stream));
        if (int rc = allreduce(d, 1)) return rc;
        HIP_OK(hipMemcpyAsync(&v, d, sizeof(T), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        *nl2 = (double)v;
        return 0;
    }

    // ---- rules = 2: Levenberg-Marquardt with step acceptance (include/tsgo.h: tsgo_config.rules; DESIGN.md section 12) ----
    static constexpr double kLmLambdaMin = 1e-9, kLmLambdaMax = 1e9;
    int lm_nl() const { return tl.n_slices > 0 ? nbL : 0; }
    size_t lm_red_size() const { return (size_t)2 * (nbC + std::max(nbL, 1)) + nbP; }
    // The tentative full step of a trial and everything the decision needs, in one chain of launches and ONE fetch: snapshot of the
    // estimates, back-substitution + update with step 1 (the landmarks' predicted decrease in the same pass, k_schur_lm<.., 2>; the poses'
    // in k_pose_update_lm), chi^2 at the trial point (k_chi2).  Nothing of the step enters the warm start's history: a full step leaves
    // no remainder to start from, and a rejected one must leave nothing at all.
    int do_lm_step(double lam, double* np2, double* nl2, double* pred, double* chi2_trial, hipEvent_t after = nullptr) {
        const int nl = lm_nl();
        T* norm_p = lm_red; T* norm_l = lm_red + nbC; T* pred_p = norm_l + nl; T* pred_l = pred_p + nbC; T* chi = pred_l + nl;
        begin_trial();      // (under step reports too the trial keeps its own kernels: k_pack_x takes no history and k_pose_update_lm reads the gradient as well)
        launch_backsub<2>(T(1), norm_l, (T)lam, pred_l);
        launch(k_pose_update_lm<T>, nbC, pr.P, (const T*)x, ps, theta, (const T*)part, (T)lam, norm_p, pred_p);
        launch_chi2(chi);
        const T* h = nullptr;
        if (int rc = fetch_partials(lm_red, (size_t)2 * (nbC + nl) + nbP, &h, after)) return rc;
        *np2 = sum_partials(h, 0, nbC); *nl2 = sum_partials(h, (size_t)nbC, nl);
        *pred = sum_partials(h, (size_t)nbC + nl, nbC) + sum_partials(h, (size_t)2 * nbC + nl, nl);
        *chi2_trial = sum_partials(h, (size_t)2 * (nbC + nl), nbP);
        return 0;
    }
    // A trial (rules 2 and 3) starts from a snapshot of the estimates, which lm_restore puts back, and leaves nothing in the warm start's history
    void begin_trial() {
        launch(k_lm_state<T, 0>, grid_for(std::max(pr.P, pr.L)), pr.P, pr.L, ps, theta, lmrec, snap_ps, snap_theta, snap_lm);
        forget_warm_history();
    }
    int lm_restore() {
        launch(k_lm_state<T, 1>, grid_for(std::max(pr.P, pr.L)), pr.P, pr.L, ps, theta, lmrec, snap_ps, snap_theta, snap_lm);
        return 0;
    }
    // What every loop files per linearisation and per trial (the trial's gain ratio is returned), and the acceptance test of rules 2 and 3
    static void note_linearisation(tsgo_stats& s, int it, double err) {
        if (it < TSGO_MAX_TRACE) s.chi2[it] = err;
        s.chi2_last = err;
        s.iterations_run = it + 1; s.trace_len = std::min(it + 1, TSGO_MAX_TRACE);
    }
    static double note_trial(tsgo_stats& s, int it, double err, double pred, double trial) {
        const double gain = pred != 0 ? (err - trial) / pred : 0.0;
        if (it < TSGO_MAX_TRACE) { s.lm_pred[it] = pred; s.lm_chi2_trial[it] = trial; s.lm_gain[it] = gain; }
        return gain;
    }
    static bool accepted(double gain, double pred) { return gain > 0 && pred > 0; }      // (a NaN anywhere fails both tests: rejected)
    // A step that ran no linearisation and no solve (solved = false: a dogleg trial that reused a solve) recorded e[2] and e[3] alone
    int add_step_times(hipEvent_t* e, bool solved, tsgo_stats& s) {
        float ms = 0;
        if (solved) {
            HIP_OK(hipEventElapsedTime(&ms, e[0], e[1])); s.ms_linearize += ms;
            HIP_OK(hipEventElapsedTime(&ms, e[1], e[2])); s.ms_solve += ms;
        }
        HIP_OK(hipEventElapsedTime(&ms, e[2], e[3])); s.ms_update += ms;
        return 0;
    }
    // evc[0..2] stand before a step's linearisation, solve and update.  Copy + synchronise: closes the update, waits, adds the device times.
    // Step reports: evc[3] already stands behind the report the host has seen (fetch_partials: `after`), and no second wait is
    // spent on it: the set is read at the end of the NEXT step, when its events lie a whole step back in the stream, while that step
    // records the other set; the last step's set is read by flush_step_timing, once per tsgo_optimize.
    hipEvent_t step_end_event() const { return reports() ? evc[3] : (hipEvent_t) nullptr; }
    int end_step_timing(tsgo_stats& s, bool solved = true) {
        if (!reports()) {
            HIP_OK(hipEventRecord(evc[3], stream));
            HIP_OK(hipEventSynchronize(evc[3]));
            return add_step_times(evc, solved, s);
        }
        if (ev_pending) { if (int rc = add_step_times(ev_pending, pending_solved, s)) return rc; }
        ev_pending = evc; pending_solved = solved; evc = evc == ev ? ev_b : ev;
        return 0;
    }
    int flush_step_timing(tsgo_stats& s) {
        hipEvent_t* e = ev_pending;
        ev_pending = nullptr; evc = ev;
        if (!e) return 0;
        HIP_OK(hipEventSynchronize(e[3]));      // (it stands right behind a report that has arrived)
        return add_step_times(e, pending_solved, s);
    }
    // The loop.  One trial = linearise (H + lambda I, b zeroed at fixed vertices), solve, tentative full step, decide; a rejected trial is
    // followed by a fresh linearisation at the restored point: lambda is baked into the landmark inverses and the pose diagonals.
    int lm_loop(int iterations, tsgo_stats& s) {
        double lam = std::min(std::max(cfg.lm_lambda0, kLmLambdaMin), kLmLambdaMax), nu = 2;
        for (int it = 0; it < iterations; ++it) {
            double err = 0;
            HIP_OK(hipEventRecord(evc[0], stream));
            lambda = lam;
            if (int rc = do_linearize(&err)) return rc;
            HIP_OK(hipEventRecord(evc[1], stream));
            const bool traced = it < TSGO_MAX_TRACE;
            note_linearisation(s, it, err);
            if (traced) s.lm_lambda[it] = lam;
            s.lambda_last = lam;
            int cg = 0, fail = 0;
            if (int rc = do_solve(&cg, &fail)) return rc;
            HIP_OK(hipEventRecord(evc[2], stream));
            if (traced) s.pcg_iters[it] = cg;
            s.pcg_iters_total += cg;
            if (fail != 0) { s.stop_reason = TSGO_STOP_SOLVER; break; }
            double np2 = 0, nl2 = 0, pred = 0, trial = 0;
            if (int rc = do_lm_step(lam, &np2, &nl2, &pred, &trial, step_end_event())) return rc;
            if (int rc = end_step_timing(s)) return rc;
            s.last_delta_norm = std::sqrt(np2 + nl2);
            const double gain = note_trial(s, it, err, pred, trial);
            if (accepted(gain, pred)) {
                const double t = 2 * gain - 1;
                lam = std::min(std::max(lam * std::max(1.0 / 3.0, 1 - t * t * t), kLmLambdaMin), kLmLambdaMax); nu = 2;
                if (s.last_delta_norm < kDeltaTol || err - trial <= cfg.lm_chi2_rel_tol * err) { s.stop_reason = TSGO_STOP_CONVERGED; break; }
            } else {
                if (int rc = lm_restore()) return rc;
                ++s.steps_rejected;
                if (lam * nu > kLmLambdaMax) { s.stop_reason = TSGO_STOP_DAMPING; break; }
                lam *= nu; nu *= 2;
            }
        }
        return flush_step_timing(s);
    }

    // rules 0 and 1: Gauss-Newton with the reference's stop rules (OptimizerCpu.h:80-180 / graph_optimizer.py:24-92)
    int gn_loop(int iterations, tsgo_stats& s) {
        double prevErr = -1; int penalty = 0;
        bool nl2_whole = true;        // sharded: last_delta_norm holds every rank's landmark part (see landmark_norm_allreduce)
        double np2_last = 0, nl2_last = 0;
        // rules = 1 (graph_optimizer.py:24-31): lambda starts at 1e-3 on every call
        const double lam_max = 1e1, lam_min = 1e-6, lam_fac = 1.1;
        double lam = 1e-3;
        const double step = step_scale();
        for (int it = 0; it < iterations; ++it) {
            double err = 0;
            HIP_OK(hipEventRecord(evc[0], stream));
            if (py_rules()) {
                // lambda follows the chi^2 of THIS linearisation (:41-42), which the linearisation itself needs: it is run with the
                // value a non-increasing chi^2 gives (the common case) and repeated with the other one when chi^2 did rise
                lambda = std::max(lam / lam_fac, lam_min);
                if (int rc = do_linearize(&err)) return rc;
                if (prevErr > -1 && err > prevErr) { lambda = std::min(lam * lam_fac, lam_max); if (int rc = do_linearize(&err)) return rc; }
                lam = lambda; s.lambda_last = lam;
            } else {
                lambda = 0;
                if (int rc = do_linearize(&err)) return rc;
            }
            HIP_OK(hipEventRecord(evc[1], stream));
            note_linearisation(s, it, err);
            if (!py_rules()) {
                if (prevErr > 0 && err > prevErr) {                          // OptimizerCpu.h:140-153
                    if (++penalty > 2) { s.stop_reason = TSGO_STOP_WORSE; break; }
                } else penalty = 0;
            }
            int cg = 0, fail = 0;
            if (int rc = do_solve(&cg, &fail)) return rc;
            HIP_OK(hipEventRecord(evc[2], stream));
            if (it < TSGO_MAX_TRACE) s.pcg_iters[it] = cg;
            s.pcg_iters_total += cg;
            if (fail != 0) { s.stop_reason = TSGO_STOP_SOLVER; break; }       // breakdown, or pcg_max_iters reached without convergence: no step is taken
            double np2 = 0, nl2 = 0;
            if (int rc = do_backsub_update((T)step, &np2, &nl2, step_end_event())) return rc;   // :159-165 / graph_optimizer.py:66-75
            if (int rc = end_step_timing(s)) return rc;
            nl2_whole = !collective();
            const bool last = it + 1 == iterations;
            const bool plateau = !py_rules() && std::fabs(err - prevErr) < kPlateauTol;
            // the norm the stop rule looks at: ||delta|| (OptimizerCpu.h:173) or ||lr * dx|| (graph_optimizer.py:66,90)
            const double norm_scale = py_rules() ? step : 1.0;
            if (collective() && (last || plateau || norm_scale * norm_scale * np2 < kDeltaTol * kDeltaTol)) {      // every rank takes this branch or none does
                if (int rc = landmark_norm_allreduce(&nl2)) return rc;
                nl2_whole = true;
            }
            s.last_delta_norm = norm_scale * std::sqrt(np2 + nl2);
            np2_last = np2; nl2_last = nl2;
            if (plateau) { s.stop_reason = TSGO_STOP_PLATEAU; break; }                                  // :167-171
            if (nl2_whole && s.last_delta_norm < kDeltaTol) { s.stop_reason = TSGO_STOP_CONVERGED; break; }   // :173-177 / py :90-92
            prevErr = err;                                                                              // :179 / py :44
        }
        if (!nl2_whole) {             // the loop ended before its last update's landmark norm was summed (worse / solver stop)
            if (int rc = landmark_norm_allreduce(&nl2_last)) return rc;
            s.last_delta_norm = (py_rules() ? step : 1.0) * std::sqrt(np2_last + nl2_last);
        }
        return flush_step_timing(s);
    }

    int optimize(int iterations, tsgo_stats* out) override {
        if (!have_graph_data) return set_error(-3, "tsgo_optimize: no graph set");
        HIP_OK(hipSetDevice(cfg.device));
        // use_graphs 1: the PCG iterations are replayed from a captured hipGraph (from the second tsgo_optimize on these tables on).  2
        // (default): eager launches while the host thread enqueues an iteration in well under the time the device takes to run it
        // (3 us per launch against 7 on an EPYC 9575F: eager is then 1-3 % FASTER than the replay and steadier, profiles/r03z_eager_vs_graph.txt);
        // a host that cannot keep that distance (busy cores, a slow clock, a profiler; or a graph of 10k poses, whose iteration the device runs in 99 us)
        // is noticed by do_solve_once and the handle goes over to replay.
        if (hook_force_host_slow) host_slow = true;      // test hook (TSGO_TESTING builds)
        const bool want_graph = cfg.use_graphs == 1 || (cfg.use_graphs == 2 && (host_slow || !amg_on));      // (block-Jacobi PCG is two short kernels per iteration, thousands of times: always replayed)
        if (want_graph && !collective() && !cg_graph && optimize_calls_on_tables >= 1) { if (int rc = capture_cg_graph()) return rc; }
        inject_armed = true;
        ++optimize_calls_on_tables;
        tsgo_stats s; std::memset(&s, 0, sizeof(s));
        s.n_pose = pr.P; s.n_lm = pr.L_total; s.n_odom_edges = pr.n_odom_edges_total; s.n_lm_edges = pr.n_lm_edges_total;
        s.ms_setup = ms_setup; s.structure_reused = last_set_reused ? 1 : 0;
        const int fallbacks0 = n_fallbacks, dropped0 = n_carry_dropped;
        const bool started_carried = mem.carried;
        replayed = false;
        ev_pending = nullptr; evc = ev;      // (a call that ended in an error may have left a set unread)
        s.stop_reason = TSGO_STOP_CAP;
        const auto wall0 = std::chrono::steady_clock::now();
        std::memset(&dl_trace, 0, sizeof(dl_trace));      // of the handle's LAST tsgo_optimize: all zero unless dogleg_loop fills it
        if (int rc = dogleg_rules() ? dogleg_loop(iterations, s) : (lm_rules() ? lm_loop(iterations, s) : gn_loop(iterations, s))) return rc;
        s.pcg_fallbacks = n_fallbacks - fallbacks0;
        s.history_carried = started_carried ? (n_carry_dropped > dropped0 ? 2 : 1) : 0;
        s.graph_replay = replayed ? 1 : 0;
        s.cycle_storage_now = amg_on ? (mem.cy16 ? 16 : 32) : 0;
        s.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        if (out) *out = s;
        return 0;
    }

    int get_vertices(double* out) override {
        if (!have_graph_data) return set_error(-3, "tsgo_get_vertices: no graph set");
        HIP_OK(hipSetDevice(cfg.device));
        const int P = pr.P, L = pr.L;
        std::vector<T> hp((size_t)P * 4), hl((size_t)std::max(L, 1) * kLmRec);
        { if (int rc_ = copy_sync(hp.data(), ps, hp.size() * sizeof(T), hipMemcpyDeviceToHost)) return rc_; }
        if (L) { if (int rc_ = copy_sync(hl.data(), lmrec, (size_t)L * kLmRec * sizeof(T), hipMemcpyDeviceToHost)) return rc_; }
        for (int i = 0; i < P; ++i) {
            const int v = pr.pose_vertex[i];
            out[3 * (size_t)v] = hp[4 * (size_t)i]; out[3 * (size_t)v + 1] = hp[4 * (size_t)i + 1];
            out[3 * (size_t)v + 2] = std::atan2((double)hp[4 * (size_t)i + 3], (double)hp[4 * (size_t)i + 2]);   // SerializeGraphFuncCpu.h:28
        }
        for (int l = 0; l < L; ++l) {
            const int v = pr.lm_vertex[l];
            out[3 * (size_t)v] = hl[(size_t)l * kLmRec]; out[3 * (size_t)v + 1] = hl[(size_t)l * kLmRec + 1]; out[3 * (size_t)v + 2] = 0;
        }
        return 0;
    }

    int linearize(double* diag, double* grad, double* chi2) override {
        if (!have_graph_data) return set_error(-3, "tsgo_linearize: no graph set");
        HIP_OK(hipSetDevice(cfg.device));
        if (int rc = do_linearize(chi2)) return rc;
        const int P = pr.P, L = pr.L;
        std::vector<T> hpart((size_t)P * 18), hl((size_t)std::max(L, 1) * kLmRec);
        { if (int rc_ = copy_sync(hpart.data(), part, hpart.size() * sizeof(T), hipMemcpyDeviceToHost)) return rc_; }
        if (L) { if (int rc_ = copy_sync(hl.data(), lmrec, (size_t)L * kLmRec * sizeof(T), hipMemcpyDeviceToHost)) return rc_; }
        std::memset(diag, 0, sizeof(double) * 9 * (size_t)pr.n_vertices);
        std::memset(grad, 0, sizeof(double) * 3 * (size_t)pr.n_vertices);
        for (int i = 0; i < P; ++i) {
            const T* o = &hpart[(size_t)i * 18];
            double* d = diag + 9 * (size_t)pr.pose_vertex[i]; double* g = grad + 3 * (size_t)pr.pose_vertex[i];
            d[0] = o[0]; d[1] = d[3] = o[1]; d[2] = d[6] = o[2]; d[4] = o[3]; d[5] = d[7] = o[4]; d[8] = o[5];
            g[0] = o[6]; g[1] = o[7]; g[2] = o[8];
        }
        for (int l = 0; l < L; ++l) {
            const T* o = &hl[(size_t)l * kLmRec];
            double ixx = o[2], ixy = o[3], iyy = o[4], dxx, dxy, dyy;
            inv_sym2<double>(ixx, ixy, iyy, dxx, dxy, dyy);       // Dl = (Dl^-1)^-1
            double* d = diag + 9 * (size_t)pr.lm_vertex[l]; double* g = grad + 3 * (size_t)pr.lm_vertex[l];
            d[0] = dxx; d[1] = d[3] = dxy; d[4] = dyy;
            g[0] = dxx * o[5] + dxy * o[6]; g[1] = dxy * o[5] + dyy * o[6];
        }
        return 0;
    }

    int solve_step(double* delta, double* chi2, int* iters) override {
        if (!have_graph_data) return set_error(-3, "tsgo_solve_step: no graph set");
        HIP_OK(hipSetDevice(cfg.device));
        if (int rc = do_linearize(chi2)) return rc;
        int cg = 0, fail = 0;
        if (int rc = do_solve(&cg, &fail)) return rc;
        if (iters) *iters = cg;
        // back-substitute with step 0: state untouched (theta is re-derived from the same cos/sin)
        double np2 = 0, nl2 = 0;
        if (int rc = do_backsub_update((T)0, &np2, &nl2)) return rc;
        const int P = pr.P, L = pr.L;
        std::vector<T> hx((size_t)P * 3), hd((size_t)std::max(L, 1) * 2);
        { if (int rc_ = copy_sync(hx.data(), x, hx.size() * sizeof(T), hipMemcpyDeviceToHost)) return rc_; }
        if (L) { if (int rc_ = copy_sync(hd.data(), dl, (size_t)L * 2 * sizeof(T), hipMemcpyDeviceToHost)) return rc_; }
        std::memset(delta, 0, sizeof(double) * 3 * (size_t)pr.n_vertices);
        for (int i = 0; i < P; ++i) for (int k = 0; k < 3; ++k) delta[3 * (size_t)pr.pose_vertex[i] + k] = hx[(size_t)i * 3 + k];
        for (int l = 0; l < L; ++l) for (int k = 0; k < 2; ++k) delta[3 * (size_t)pr.lm_vertex[l] + k] = hd[(size_t)l * 2 + k];
        return fail == 1 ? set_error(-21, "PCG breakdown") : (fail != 0 ? set_error(-22, "PCG did not converge within pcg_max_iters") : 0);
    }

