// engine/engine_launch.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// kernel launches: linearisation, Schur products, the hierarchy's numeric set-up, the V-cycle, one PCG iteration; byte models of the in-situ profiler.
    // ---- in-situ profiler (tsgo_profile_iteration): an event before every launch of an eagerly launched iteration ----
    struct ProfMark { hipEvent_t e; char name[64]; char where[32]; double bytes; };
    std::vector<ProfMark> prof; size_t prof_n = 0; bool prof_on = false;
    template <typename U> static const char* tname_of() { return sizeof(U) == 8 ? "double" : "float"; }      // (every vector type is one of the two)
    static const char* tname() { return tname_of<T>(); }
    // PF(bytes, where, kernel, template arguments ...): a mark in front of a launch.  The name is the kernel symbol as rocprofv3 prints it, e.g.
    // "k_schur_lm<double, 4, 0, 1>" (kernel_name(), tsgo_hip.hip), formatted from the template arguments of the launch next to it.
    // The arguments (byte models, labels, names) are evaluated only while a profile is being taken
#define PF(...) do { if (prof_on) pf(__VA_ARGS__); } while (0)
    template <typename... A> void pf(double bytes, const char* where, const char* kernel, const A&... targs) {
        if (!prof_on) return;
        if (prof_n == prof.size()) { ProfMark m{}; if (hipEventCreate(&m.e) != hipSuccess) { prof_on = false; return; } prof.push_back(m); }
        ProfMark& m = prof[prof_n++];
        std::snprintf(m.name, sizeof(m.name), "%s", kernel_name(kernel, targs...).c_str());
        std::snprintf(m.where, sizeof(m.where), "%s", where); m.bytes = bytes;
        (void)hipEventRecord(m.e, stream);
    }
    // a kernel on the engine's stream, kBlock threads per workgroup.  Every argument is listed: a kernel's default arguments do not travel
    // with its address
    template <typename... P, typename... A> void launch(void (*kernel)(P...), int grid, A&&... args) {
        kernel<<<dim3(grid), dim3(kBlock), 0, stream>>>(std::forward<A>(args)...);
    }
    // ... one wavefront (64 threads) per workgroup: the right-hand-side and read-out kernels of the batched solve (__launch_bounds__(64))
    template <typename... P, typename... A> void launch_wave(void (*kernel)(P...), int grid, A&&... args) {
        kernel<<<dim3(grid), dim3(64), 0, stream>>>(std::forward<A>(args)...);
    }
    // A table kernel with an argument head (tsgo_kernels.h, "Argument heads"): the walked table's row offsets, slice and vertex counts and
    // the grid's eighth under the XCD map go first, as plain arguments; `args` continue the head and then list everything else
    template <typename... P, typename... A> void launch_table(void (*kernel)(P...), int grid, const Table<T>& tb, A&&... args) {
        launch(kernel, grid, tb.row_off, tb.n_slices, tb.n_vertices, xcd8(tb.xcd, grid), std::forward<A>(args)...);
    }
    static int xcd8(int xcd, int grid) { return xcd ? grid / 8 : 0; }      // what the kernels' xcd8 argument takes: gridDim.x / 8, or 0 for round-robin
    std::string lvl(const char* role, size_t l) const { return std::string(role) + " L" + std::to_string(l); }
    // algorithmic bytes of the table kernels (DESIGN.md section 4) and of the block-row kernels of the cycle
    double od_slots_live() { if (od_live < 0) { od_live = 0; for (uint32_t e : pr.odom.edge) od_live += e != kNoEdge; } return od_live; }
    double bytes_schur_lm(bool low) const { const double s = low ? 4 : sizeof(T), v = sizeof(T); return (double)pr.n_lm_edges * (4 + 4 * s) + pr.P * 5.0 * v + pr.L * 5.0 * v; }
    double bytes_schur_pose(bool low) { const double s = low ? 4 : sizeof(T), v = sizeof(T); return (double)pr.n_lm_edges * (4 + 4 * s) + pr.L * 2.0 * v + pr.P * 14.0 * v + od_slots_live() * (4 + 6 * v); }
    // (fine vectors of level 0 are T, every other cycle vector cv_bytes())
    double bytes_sweep(const DevLevel<T>& L) const { return (double)L.nnzA * (4.0 * cyw() + 4) + (double)L.n * (3 * 3 * cv_bytes() + 9 * sizeof(H) + 4); }
    double bytes_transfer(const DevLevel<T>& L, int vecs_fine, bool fine_is_l0 = false) const {
        return (double)L.nnzP * (4.0 * cyw() + 4) + (double)L.n * 3 * (fine_is_l0 ? sizeof(T) : cv_bytes()) * vecs_fine + (double)L.n_agg * (3 * cv_bytes() + 4);
    }

    // ---- launches --------------------------------------------------------------------------------
    // damping of the current linearisation (rules = 1, graph_optimizer.py:24-43; 0 under the cpu/eigen rules) and the step the update takes
    double lambda = 0;
    bool py_rules() const { return cfg.rules == 1; }
    bool lm_rules() const { return cfg.rules == 2; }      // Levenberg-Marquardt with step acceptance (engine_solve.inc: lm_loop)
    bool dogleg_rules() const { return cfg.rules == 3; }  // Powell's dogleg (engine_dogleg.inc: dogleg_loop)
    bool trial_rules() const { return lm_rules() || dogleg_rules(); }      // full steps taken tentatively: snapshot, chi^2-only pass, b zeroed at fixed vertices
    // pose-pose slots in general form (tsgo_math.h: eight dynamic planes per slot): analytic ODOM Jacobians, or a graph that holds
    // virtual landmark measurements (edge type 2) — the kernels' OJ = 1 instantiations
    bool oj() const { return cfg.odom_jacobian == 1 || pr.has_vlm; }
    int odom_analytic_flag() const { return cfg.odom_jacobian == 1 ? 1 : 0; }
    double step_scale() const { return trial_rules() ? 1.0 : (py_rules() ? cfg.lr : kStepScale); }
    // a graph with priors (edge types 3, 4) takes the PRI = 1 instantiations; one without launches exactly what it did before priors existed
    PriorArgs<T> pose_prior_args() const { return PriorArgs<T>{pri_p_off, pri_p, pri_lchi, tl.n_slices > 0 ? nbL : 0}; }
    PriorArgs<T> lm_prior_args() const { return PriorArgs<T>{pri_l_off, pri_l, pri_lchi, 0}; }
    static PriorArgs<T> no_priors() { return PriorArgs<T>{nullptr, nullptr, nullptr, 0}; }
    static GateArgs<T> no_gate() { return GateArgs<T>{nullptr, nullptr, nullptr, 0, T(0), nullptr, 0}; }
    // Robust kernels per edge class (tsgo_set_robust): belongs to the HANDLE (it survives tsgo_set_graph; tsgo_hip.hip lists the lifetimes), read by every launch that
    // robustifies.  A setting equal to the default takes the RK = 0 instantiations — the compile-time Huber, exactly what was launched
    // before the setting existed; anything else the RK = 1 ones, which read kind and width from the by-value argument below.  While a
    // per-edge setting is active (tsgo_set_edge_robust, engine_edge_robust.inc; f64 handles only) the RK = 2 ones, which also read a byte per
    // slot, record or edge and the palette behind the pointers at the argument's end.
    tsgo_robust robust = default_robust();
    static tsgo_robust default_robust() { tsgo_robust r; tsgo_default_robust(&r); return r; }
    static bool same_robust(const tsgo_robust& a, const tsgo_robust& b) {
        for (int k = 0; k < kEdgeClasses; ++k)
            if (a.kernel[k] != b.kernel[k] || (a.kernel[k] != TSGO_ROBUST_NONE && a.delta[k] != b.delta[k])) return false;      // NONE ignores its width
        return true;
    }
    int rk() const { return er.active ? 2 : (same_robust(robust, default_robust()) ? 0 : 1); }
    // pick_rk(f): f(RK) for this handle; the RK = 2 kernels are instantiated for double alone
    template <typename F> void pick_rk(F&& f) {
        if constexpr (sizeof(T) == 8) pick<0, 1, 2>(rk(), std::forward<F>(f));
        else pick<0, 1>(rk(), std::forward<F>(f));
    }
    RobustArgs<T> robust_args() const {
        RobustArgs<T> a{};
        for (int k = 0; k < kEdgeClasses; ++k) { a.kind[k] = robust.kernel[k]; a.delta[k] = (T)robust.delta[k]; }
        if (er.active) { a.pal = maps.er_pal; a.by_lm = maps.er_lm; a.by_pose = maps.er_pose; a.odom = maps.er_od; a.pose_prior = maps.er_pp; a.lm_prior = maps.er_pl; a.edge = maps.er_edge; }
        return a;
    }
    int set_robust(const tsgo_robust& r) override {
        if (!same_robust(r, default_robust()) && cfg.world > 1)
            return set_error(-1, "tsgo_set_robust: a non-default robust kernel is not supported on an edge-sharded handle (world > 1)");
        if (!same_robust(r, robust)) mem.hier_age = -1;      // the weights may move wholesale: the next linearisation builds a fresh hierarchy
        robust = r; robust.reserved = 0;
        return 0;
    }
    void get_robust(tsgo_robust* out) const override { *out = robust; }
    void launch_lin() {
        launch_lin_lm();
        launch_lin_pose_only();
    }
    void launch_lin_lm() {              // (tsgo_time_kernel too)
        const int zf = (py_rules() || trial_rules()) ? 1 : 0;
        if (tl.n_slices == 0) return;
        pick<1, 2, 4, 8>(pr.by_lm.G, [&](auto g) { pick<0, 1>(pr.has_priors, [&](auto pri) { pick_rk([&](auto rk) {
            launch_table(k_lin_lm<T, g, pri, rk>, nbL, tl, zf, lmrec, (const T*)ps, (const T*)gauge_l, ninv, tl, (T)lambda, pri ? lm_prior_args() : no_priors(), robust_args());
        }); }); });
    }
    void launch_lin_pose_only() {       // (tsgo_time_kernel too)
        const int zf = (py_rules() || trial_rules()) ? 1 : 0;
        pick<1, 2, 4, 8>(pr.by_pose.G, [&](auto g) { pick<0, 1>(oj(), [&](auto general) { pick<0, 1>(pr.has_priors, [&](auto pri) { pick_rk([&](auto rk) {
            launch_table(k_lin_pose<T, g, general, pri, rk>, nbP, tp, zf, (const T*)ps, (const T*)lmrec, to.row_off, (const T*)gauge_p, tp, to, pr.pose_first, pr.pose_last, part,
                         part + (size_t)pr.P * 18, (T)lambda, general ? odom_analytic_flag() : 0, pri ? pose_prior_args() : no_priors(), robust_args());
        }); }); }); });
    }
    // rules = 2: robustified chi^2 at the current estimates, nbP partials into `out` (tsgo_lm_kernels.h; tsgo_time_kernel 7 too).  One launch,
    // and one more in front of it on a graph with priors (the landmark priors' partials, which k_chi2<.., 1> folds as k_lin_pose<.., 1> does)
    void launch_chi2(T* out) {
        if (pr.has_priors && tl.n_slices > 0) pick<1, 2, 4, 8>(pr.by_lm.G, [&](auto g) { pick_rk([&](auto rk) {
            launch(k_chi2_lm_prior<T, g, rk>, nbL, tl, (const T*)lmrec, lm_prior_args(), robust_args());
        }); });
        pick<1, 2, 4, 8>(pr.by_pose.G, [&](auto g) { pick<0, 1>(oj(), [&](auto general) { pick<0, 1>(pr.has_priors, [&](auto pri) { pick_rk([&](auto rk) {
            launch(k_chi2<T, g, general, pri, rk>, nbP, tp, to, (const T*)ps, (const T*)lmrec, out, pri ? pose_prior_args() : no_priors(), robust_args());
        }); }); }); });
    }
    // (LM slot: index, zx zy w0 w1, 16 B of the landmark record; pose-pose slot: its index, and at the first endpoint nine planes + the neighbour's record)
    double bytes_chi2() { const double v = sizeof(T); return (double)pr.n_lm_edges * (4 + 6 * v) + pr.P * 4.0 * v + od_slots_live() * (4 + 6.5 * v) + nbP * v; }
    void launch_finalize() {
        hipLaunchKernelGGL((k_pose_finalize<T>), dim3(nbC), dim3(kBlock), 0, stream, pr.P, part, ps, dp, minv, r, p, q, x, zc, gpart[0], st[0], (const T*)(amg_on ? omega_dev : one_dev), gscale_dev, amg_on && low_cycle ? zc32 : (float*)nullptr);
    }
    // S * (vector in zc) -> sbuf, dot partials behind it.  low: read the f32 copy of the slot planes (the two
    // products inside the multigrid cycle; never the product PCG itself takes).
    // Edge-sharded runs: every rank's passes cover its own landmarks (and the ODOM rows / diagonal blocks of its own
    // poses), so what lands in sbuf is a PARTIAL product and partial dots: one all-reduce of [3P | nbP] makes both whole
    // on every rank.  (r, z) partials are computed redundantly from replicated vectors and need no reduction.
    int launch_matvec(int slot, bool with_rz = false, bool low = false, const GateArgs<T>* gate = nullptr, bool post_smooth = false, bool as_residual = false) {
        const char* wh = low ? "in-cycle product" : (with_rz ? "PCG product" : "product");
        launch_schur_lm(slot, low, low ? gate : nullptr, wh);
        launch_schur_pose(slot, low, (const T*)(!low && with_rz ? r : nullptr), rzpart, low && post_smooth, low && as_residual, wh);
        return allreduce(sbuf, (size_t)pr.P * 3 + nbP);
    }
    // the two passes of a product (tsgo_time_kernel too).  The f32 operands, the gate and the epilogue go with LOW = 1 alone
    void launch_schur_lm(int slot, bool low, const GateArgs<T>* gate, const char* wh) {
        pick<1, 2, 4, 8>(pr.by_lm.G, [&](auto g) { pick<0, 1>(low, [&](auto lo) {
            PF(bytes_schur_lm(lo) + (gate ? 2.0 * nbC * sizeof(T) : 0.0), gate ? "stopping rule + in-cycle product" : wh, "k_schur_lm", tname(), g, 0, lo);
            const GateArgs<T> ga = lo && gate ? *gate : no_gate();      // the head carries the state once: the gate's own where there is one (launch_iteration: st[slot])
            if (tl.n_slices > 0) launch_table(k_schur_lm<T, g, 0, lo>, nbL, tl, ga.st ? ga.n : 0, ga.st ? ga.st : st[slot], (const T*)ninv, ga.rdr_part, ga.bpart, tl, (const T*)zc, lmrec, tvec,
                                              T(0), dl, npart, lo ? (const float*)zc32 : nullptr, lo ? tvec32 : nullptr, ga, T(0), (T*)nullptr);
        }); });
    }
    // The landmark pass as the back-substitution: dl = u - Dl^-1 W^T x, the update by `step`, |dl|^2 partials at norm_out (MODE 1: do_backsub_update,
    // dl_after_solve); MODE 2 (do_lm_step) also leaves the landmarks' predicted decrease under lam at pred_out
    template <int MODE> void launch_backsub(T step, T* norm_out, T lam, T* pred_out) {
        if (tl.n_slices > 0) pick<1, 2, 4, 8>(pr.by_lm.G, [&](auto g) {
            launch_table(k_schur_lm<T, g, MODE, 0>, nbL, tl, 0, st[0], (const T*)ninv, (const T*)nullptr, (const T*)nullptr, tl, (const T*)zc, lmrec, tvec, step, dl, norm_out, (const float*)nullptr, (float*)nullptr, no_gate(), lam,
                         pred_out);
        });
    }
    void launch_schur_pose(int slot, bool low, const T* rvec, T* rz_part, bool post_smooth, bool as_residual, const char* wh) {
        pick<1, 2, 4, 8>(pr.by_pose.G, [&](auto g) { pick<0, 1>(low, [&](auto lo) { pick<0, 1>(oj(), [&](auto general) {
            PF(bytes_schur_pose(lo) + (post_smooth ? pr.P * (6 + 3 + 3 + 3) * (double)sizeof(T) : 0.0), post_smooth ? "in-cycle product + post-smoothing L0" : wh, "k_schur_pose", tname(), g, lo, general);
            const T* pm_ = post_smooth ? (const T*)minv : (const T*)nullptr;      // the level-0 post-smoothing in this pass's epilogue (k_schur_pose)
            const T* pr_ = (post_smooth || as_residual) ? (const T*)r : (const T*)nullptr;      // ... or sbuf = r - S z (as_residual: the cycle's first product)
            launch_table(k_schur_pose<T, g, lo, general>, nbP, tp, (const CgState<T>*)st[slot], (const T*)zc, lo ? (const float*)zc32 : nullptr, to.row_off, tp, to, (const T*)tvec, (const T*)dp,
                         pr.pose_first, pr.pose_last, sbuf, sbuf + (size_t)pr.P * 3, rvec, rz_part, lo ? (const float*)tvec32 : nullptr, pm_, pr_, lo ? (const T*)omega_dev : nullptr, lo ? zc : nullptr);
        }); }); });
    }
    // the warm start's two kernels: what they read of `w` before their first vector load goes in their plain heads (and is read from there alone)
    void launch_pack_x(const WarmTerms<T>& w, int* order_out) {
        hipLaunchKernelGGL((k_pack_x<T>), dim3(nbC), dim3(kBlock), 0, stream, pr.P, w.n_max, w.n_tested, w.nb_err, w.errpart, x, zc, order_out, w);
    }
    void launch_save_x(const WarmTerms<T>& w, T* xsave, T* errpart) {
        hipLaunchKernelGGL((k_save_x<T>), dim3(nbC), dim3(kBlock), 0, stream, pr.P, w.n_max, (const T*)x, zc, xsave, errpart, w);
    }
    // k_save_x and k_pose_update in one launch (do_backsub_update under step reports)
    void launch_save_update(const WarmTerms<T>& w, T* xsave, T* errpart, T step) {
        hipLaunchKernelGGL((k_save_update<T>), dim3(nbC), dim3(kBlock), 0, stream, pr.P, w.n_max, (const T*)x, zc, xsave, errpart, ps, theta, step, npart, w);
    }
    // Step reports: one-shard handles, unless TSGO_STEP_DRAINS=1 asks for copy + synchronise (host/knobs.h)
    bool reports() const { return !step_drains && !collective() && h_rep != nullptr; }
    // n partials at src -> the pinned report buffer, then the next sequence number into its word (k_report); wait_report(the number returned) is the host's side
    uint64_t launch_report(const T* src, size_t n) {
        const uint64_t seq = ++rep_seq;
        hipLaunchKernelGGL((k_report<T>), dim3(1), dim3(kBlock), 0, stream, (int)n, src, rep_data(), reinterpret_cast<unsigned long long*>(h_rep), (unsigned long long)seq);
        return seq;
    }
    static int grid_for(int n, int per_thread_lanes = 1) { return std::max(1, (int)(((size_t)n * per_thread_lanes + kBlock - 1) / kBlock)); }

    // One Galerkin product from its pair lists (TRANS 0: T = A P; 1: A_next = P^T T, upper blocks): a lane per output block, or 8 / 16 / 64 lanes
    // sharing one where the average list is long
    template <int TRANS> void launch_pair_gemm(double avg_pairs, int n_out, const int* ptr, const int* px, const int* py, const H* X, const H* Y, H* out, const int* upper) {
        if (avg_pairs > kMediumPairList)
            pick<8, 16, 64>(avg_pairs > kVeryLongPairList ? 64 : (avg_pairs > kLongPairList ? 16 : 8), [&](auto lpb) {
                launch(k_pair_gemm_wave<T, TRANS, lpb>, grid_for(n_out, lpb), n_out, ptr, px, py, X, Y, out, upper);
            });
        else launch(k_pair_gemm<T, TRANS>, grid_for((n_out + kPairBlocksPerWave - 1) / kPairBlocksPerWave, 64), n_out, ptr, px, py, X, Y, out, upper);
    }

    // numeric multigrid setup for the current linearisation (after lin + finalize)
    int launch_amg_setup() {
        DevLevel<T>& L0 = lv[0];
        // sharded: off-diagonal blocks are partial sums over this rank's landmarks and ODOM rows; the diagonal (from the
        // all-reduced linearisation partials, identical everywhere) is contributed by rank 0 alone; one all-reduce
        // makes level 0 whole and identical on every rank, everything below it is then computed redundantly
        const int n_sum = n_upper0 >= 0 ? n_upper0 : L0.nnzA;
        hipLaunchKernelGGL((k_schur_blocks<T>), dim3(grid_for(n_sum)), dim3(kBlock), 0, stream, n_sum, L0.A_row, L0.A_col, sc_ptr, sc_si, sc_sk,
                           sc_optr, sc_os, tp, (const T*)to.dyn, to.slots, (const T*)lmrec, (const T*)ps, (const T*)part, L0.A, pr.rank == 0 ? 1 : 0,
                           to.idx, oj() ? 1 : 0, (const int*)(n_upper0 >= 0 ? upper0 : nullptr), (const int*)(n_upper0 >= 0 ? lower0 : nullptr), (T)mem.hier_shift);
        if (int rc = allreduce_h(L0.A, (size_t)L0.nnzA * 9)) return rc;
        if (explicit0) pick<0, 1>(mem.cy16, [&](auto pk) { launch(k_to_planes<T, pk>, grid_for(L0.n, 8), L0.n, (const int*)L0.A_ptr, (const H*)L0.A, L0.Apm); });
        for (size_t l = 0; l < lv.size(); ++l) {
            DevLevel<T>& L = lv[l];
            H* Anext = l + 1 < lv.size() ? lv[l + 1].A : A_last;
            hipLaunchKernelGGL((k_block_inv<T>), dim3(grid_for(L.n)), dim3(kBlock), 0, stream, L.n, L.diag, (const H*)L.A, L.Dinv);
            pick<0, 1>(mem.cy16, [&](auto pk) {
                launch(k_prolongator<T, pk>, grid_for(L.nnzP), L.nnzP, L.P_row, L.p_self, L.ps_ptr, L.ps_x, L.ps_y, (const H*)L.A, (const H*)L.Dinv, (const T*)L.rel, (T)kProlongOmega, L.P,
                       L.p_to_r, L.Rv, (const int*)L.P_ptr, (const int*)L.P_col, (const int*)L.R_ptr, L.Ppm, L.Rpm);
            });
            launch_pair_gemm<0>(L.pairs_T, L.nnzT, L.ts_ptr, L.ts_x, L.ts_y, (const H*)L.A, (const H*)L.P, L.Tv, (const int*)nullptr);
            launch_pair_gemm<1>(L.pairs_A, L.n_upper, L.as_ptr, L.as_x, L.as_y, (const H*)L.P, (const H*)L.Tv, Anext, (const int*)L.as_upper);
            {   // the mirrored blocks of the next level's matrix and, in the same pass, its cycle-format copy (the last one, the dense level's, has none)
                const bool packed_next = l + 1 < lv.size();
                const int* rows_next = packed_next ? (const int*)lv[l + 1].A_row : (const int*)nullptr;
                const int* ptr_next = packed_next ? (const int*)lv[l + 1].A_ptr : (const int*)nullptr;
                uint32_t* pm_next = packed_next ? lv[l + 1].Apm : (uint32_t*)nullptr;
                pick<0, 1>(mem.cy16, [&](auto pk) { launch(k_mirror_pack<T, pk>, grid_for(L.nnzNext), L.nnzNext, (const int*)L.as_mirror, Anext, rows_next, ptr_next, pm_next); });
            }
        }
        hipLaunchKernelGGL((k_dense_inverse<T>), dim3(1), dim3(kDenseThreads), 0, stream, nb_last, last_ptr, last_col, (const H*)A_last, inv_last);
        return launch_bottom_setup();
    }

    static double blocks_per_row(int nnz, int n_rows) { return (double)nnz / std::max(1, n_rows); }      // what lanes_for / lanes_for_sweep take
    static int lanes_for(double avg_row) {
        return avg_row <= 4 ? 4 : (avg_row <= 12 ? 8 : (avg_row <= 40 ? 32 : 64));
    }
    // Block-row sweeps (k_bcsr_residual): on the big levels (thousands of rows: every wave slot of the device is taken more
    // than once) a lane should carry two to four blocks, not one — 16 lanes per row at 28 and at 67 blocks per row measured
    // 8.7 / 5.6 us against 9.3 / 6.2 us with 32 / 64 lanes; the small levels are one wave round either way and want the
    // shortest chain, i.e. many lanes (profiles/r02h_lanes_per_row.txt).
    static int lanes_for_sweep(double avg_row, int n_rows) {
        if (n_rows >= 4096 && avg_row > 12) return 16;
        return lanes_for(avg_row);
    }
    // grids of the block-row kernels: levels with at least kXcdMinBlocks workgroups are rounded up to a multiple of 8 and take the XCD-aware
    // workgroup map (block_row(), tsgo_block_row.h): the surplus workgroups clamp to the last row and write nothing
    static constexpr int kXcdMinBlocks = 64;
    bool lpr_xcd = true;       // research: TSGO_LPR_XCD=0 keeps the round-robin map everywhere
    int lpr_grid(int n_rows, int lanes, int* xcd) const {
        int g = grid_for(n_rows, lanes);
        *xcd = (lpr_xcd && g >= kXcdMinBlocks) ? 1 : 0;
        return *xcd ? 8 * ((g + 7) / 8) : g;
    }
    // A block-row kernel with `lpr` lanes per row over the cycle-format copies: f(LPR, PK, grid, xcd), PK = packed half (1) or f32 (0) blocks
    template <typename F> void pick_block_row(int lpr, int n_rows, F&& f) {
        pick<4, 8, 16, 32, 64>(lpr, [&](auto lanes) { pick<0, 1>(mem.cy16, [&](auto pk) {
            int xcd = 0;
            const int grid = lpr_grid(n_rows, lanes, &xcd);
            f(lanes, pk, grid, xcd);
        }); });
    }
    // a block-row sweep over the cycle-format copy of a level's matrix (MODE 0 residual, 1 smoothing sweep); role: the profiler's label
    template <int MODE, typename V> void launch_sweep(const char* role, size_t level, int lpr, const V* rhs, const V* cur, V* out, const T* omega, const CgState<T>* s) {
        DevLevel<T>& L = lv[level];
        pick_block_row(lpr, L.n, [&](auto lanes, auto pk, int grid, int xcd) {
            PF(bytes_sweep(L), lvl(role, level).c_str(), "k_bcsr_residual", tname(), lanes, MODE, 1, pk, tname_of<V>());
            launch(k_bcsr_residual<T, lanes, MODE, 1, pk, V>, grid, L.n, xcd8(xcd, grid), s, L.A_ptr, L.A_col, (const void*)L.Apm, cur, rhs, (const H*)L.Dinv, out, omega);
        });
    }
    // restriction of level `level` (SUB 1: of va - vb, two fine vectors), with the first pre-sweep of the level below where dinv_next is given
    template <int SUB, typename VI, typename VO> void launch_restrict(size_t level, int lpr, const VI* va, const VI* vb, VO* rc, const H* dinv_next, VO* z_next, const T* omega, const CgState<T>* s) {
        DevLevel<T>& L = lv[level];
        pick_block_row(lpr, L.n_agg, [&](auto lanes, auto pk, int grid, int xcd) {
            PF(bytes_transfer(L, SUB ? 2 : 1, level == 0), lvl("restrict from", level).c_str(), "k_restrict", tname(), lanes, SUB, pk, tname_of<VI>(), tname_of<VO>());
            launch(k_restrict<T, lanes, SUB, pk, VI, VO>, grid, L.n_agg, xcd8(xcd, grid), s, L.R_ptr, L.R_col, (const uint32_t*)L.Rpm, va, vb, rc, dinv_next, z_next, omega);
        });
    }
    template <typename VE, typename VZ> void launch_prolong(size_t level, const VE* e, VZ* z, int zs, const CgState<T>* s) {
        DevLevel<T>& L = lv[level];
        float* z32 = (level == 0 && low_cycle && !explicit0) ? zc32 : (float*)nullptr;      // level 0 prolongs into the pose records: keep their f32 copy current
        pick_block_row(lanes_for(blocks_per_row(L.nnzP, L.n)), L.n, [&](auto lanes, auto pk, int grid, int xcd) {
            PF(bytes_transfer(L, 2, level == 0), lvl("prolong into", level).c_str(), "k_prolong_add", tname(), lanes, pk, tname_of<VE>(), tname_of<VZ>());
            launch(k_prolong_add<T, lanes, pk, VE, VZ>, grid, L.n, xcd8(xcd, grid), s, L.P_ptr, L.P_col, (const uint32_t*)L.Ppm, e, z, zs, z32);
        });
    }

    // Damping of the block-Jacobi smoother per level from a power iteration on D^-1 A (12 steps): the V-cycle
    // is a symmetric positive definite preconditioner only while omega * rho(D^-1 A) < 2, and smoothed Galerkin
    // matrices reach rho = 2.1 ... 3.4 (measured on the CPU twin).  omega = min(1, 1.6 / (1.05 rho)).
    int estimate_damping() {
        const size_t nl = lv.size();
        for (size_t l = 0; l < nl; ++l) {
            DevLevel<T>& L = lv[l];
            T* a = pw_a; T* b = pw_b;      // (sized for level 0: every level fits; the power iteration runs in T)
            const int n3 = L.n * 3;
            hipLaunchKernelGGL((k_seed_vector<T>), dim3(grid_for(n3)), dim3(kBlock), 0, stream, n3, a);
            const int lprA = lanes_for(blocks_per_row(L.nnzA, L.n));
            for (int it = 0; it < kRhoSteps; ++it) {
                pick<4, 8, 16, 32, 64>(lprA, [&](auto lanes) {     // the block-indexed matrix (PM = 0): level 0 has no cycle-format copy
                    launch(k_bcsr_residual<T, lanes, 2, 0>, grid_for(L.n, lanes), L.n, 0, (const CgState<T>*)st[0], L.A_ptr, L.A_col, (const void*)L.A, (const T*)a, (const T*)a, (const H*)L.Dinv, b, (const T*)omega_dev);
                });
                std::swap(a, b);
            }
            // a = v_K, b = v_{K-1}
            hipLaunchKernelGGL((k_norm2<T>), dim3(kRhoBlocks), dim3(kBlock), 0, stream, n3, (const T*)a, rho_part + (2 * l) * kRhoBlocks);
            hipLaunchKernelGGL((k_norm2<T>), dim3(kRhoBlocks), dim3(kBlock), 0, stream, n3, (const T*)b, rho_part + (2 * l + 1) * kRhoBlocks);
        }
        HIP_OK(hipMemcpyAsync(h_rho, rho_part, sizeof(T) * 2 * nl * kRhoBlocks, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        std::vector<T> om(16, (T)kSmootherOmega);
        for (size_t l = 0; l < nl; ++l) {
            double nk = 0, nk1 = 0;
            for (int k = 0; k < kRhoBlocks; ++k) { nk += (double)h_rho[(2 * l) * kRhoBlocks + k]; nk1 += (double)h_rho[(2 * l + 1) * kRhoBlocks + k]; }
            double w = kSmootherOmega;
            if (nk1 > 0 && nk > 0 && std::isfinite(nk) && std::isfinite(nk1)) {
                const double rho = 1.05 * std::sqrt(nk / nk1);
                w = std::min(1.0, 1.6 / rho);
            }
            om[l] = (T)w; omega_host[l] = w;
        }
        if (say_env) { std::fprintf(stderr, "[tsgo] smoother damping per level:"); for (size_t l = 0; l < nl; ++l) std::fprintf(stderr, " %.3f", omega_host[l]); std::fprintf(stderr, "\n"); }
        HIP_OK(hipMemcpyAsync(omega_dev, om.data(), 16 * sizeof(T), hipMemcpyHostToDevice, stream));
        HIP_OK(hipStreamSynchronize(stream));
        return 0;
    }

    // zc[.][0..2] = V(1,1)-cycle(r).  On entry zc already holds the level-0 pre-smoothing Minv r
    // (written by pose_finalize / k_cg_step).  Level l >= 1 keeps r, z (pre-smoothed by the restriction
    // above it), res and the post-smoothed result z2.
    // tsgo_config.cycle_level0 = 1: the two products inside the cycle read the EXPLICIT level-0 matrix of the hierarchy
    // (lagged with it, hub landmarks truncated, f32) instead of the implicit Schur passes — no all-reduce in a sharded run
    bool explicit0 = false;
    int launch_cycle_product(int slot, const GateArgs<T>* gate = nullptr, bool post_smooth = false, bool as_residual = false) {
        if (!explicit0) return launch_matvec(slot, false, low_cycle, gate, post_smooth, as_residual);
        DevLevel<T>& L = lv[0];
        pick_block_row(lanes_for_sweep(blocks_per_row(L.nnzA, L.n), L.n), L.n, [&](auto lanes, auto pk, int grid, int xcd) {
            PF(bytes_sweep(L), "in-cycle product (explicit)", "k_bcsr_apply", tname(), lanes, pk);
            launch(k_bcsr_apply<T, lanes, pk>, grid, L.n, xcd8(xcd, grid), (const CgState<T>*)st[slot], L.A_ptr, L.A_col, (const uint32_t*)L.Apm, (const T*)zc, kPoseRec, sbuf);
        });
        return 0;
    }
    // the dense level alone: z = inv_last r, one workgroup
    template <typename V> void launch_dense_solve(const V* rhs, V* z, const CgState<T>* s) {
        PF((double)nb_last * 3 * nb_last * 3 * sizeof(T), "dense solve", "k_dense_apply", tname(), tname_of<V>());
        hipLaunchKernelGGL((k_dense_apply<T, V>), dim3(1), dim3(kBlock), 0, stream, nb_last * 3, (const T*)inv_last, rhs, z, s);
    }
    // the cycle's vectors below level 0 are V (CV<T>; T under cyc64, testing builds only)
    int launch_vcycle(int slot, const GateArgs<T>* gate = nullptr) {
#ifdef TSGO_TESTING
        if (cyc64) return launch_vcycle_v<T>(slot, gate);
#endif
        return launch_vcycle_v<CV<T>>(slot, gate);
    }
    template <typename V> int launch_vcycle_v(int slot, const GateArgs<T>* gate) {
        auto v = [](void* q) { return static_cast<V*>(q); };
        auto cv = [](void* q) { return static_cast<const V*>(q); };
        const CgState<T>* s = st[slot];
        const size_t nl = lv.size();              // explicit levels 0 .. nl-1, dense level below
        // the cycle's first product leaves the residual r - S z itself (pose pass epilogue) where it reads f32 copies and needs no all-reduce:
        // the restriction then gathers ONE fine vector per block instead of two
        const bool res_fused = fuse_post_smooth && !explicit0 && low_cycle && !collective();
        if (int rc = launch_cycle_product(slot, gate, false, res_fused)) return rc;
        {
            DevLevel<T>& L = lv[0];
            const int lpr = lanes_for(blocks_per_row(L.nnzP, L.n_agg));
            const H* dnext = (bottom_dense && nl == 2) ? (const H*)nullptr : (nl > 1 ? (const H*)lv[1].Dinv : (const H*)nullptr);      // (nl == 3 with the factored level: lv[1] keeps its pre-sweep)
            if (nl > 1 && res_fused) launch_restrict<0>(0, lpr, (const T*)sbuf, (const T*)sbuf, v(lv[1].r), dnext, v(lv[1].z), (const T*)(omega_dev + 1), s);
            else if (nl > 1) launch_restrict<1>(0, lpr, (const T*)r, (const T*)sbuf, v(lv[1].r), dnext, v(lv[1].z), (const T*)(omega_dev + 1), s);
        }
        // coarse levels: V(nu,nu) with nu = coarse_sweeps block-Jacobi sweeps (the first pre-sweep comes fused
        // with the restriction above).  The current iterate alternates between L.z and L.z2; it ends in L.z2.
        const bool dense_bottom = bottom_dense && nl > 1;      // the last explicit level's whole cycle is one dense product (k_bottom_apply) ...
        const bool dense_tail2 = dense_bottom && tail2;        // ... and the level above it two launches (t = E^T r, k_tail_up)
        const size_t first_dense = dense_tail2 ? nl - 2 : (dense_bottom ? nl - 1 : nl);      // levels from here down run no sweeps of their own
        for (size_t l = 1; l < std::min(nl, first_dense); ++l) {
            DevLevel<T>& L = lv[l];
            const int nu = nu_at(l);
            const int lprA = lanes_for_sweep(blocks_per_row(L.nnzA, L.n), L.n);
            V* cur = v(L.z); V* oth = v(L.z2);
            for (int sw = 1; sw < nu; ++sw) {
                launch_sweep<1>("pre-sweep", l, lprA, cv(L.r), (const V*)cur, oth, (const T*)(omega_dev + l), s);
                std::swap(cur, oth);
            }
            launch_sweep<0>("residual", l, lprA, cv(L.r), (const V*)cur, v(L.res), (const T*)(omega_dev + l), s);
            if (l + 1 < nl) {
                const int lpr = lanes_for(blocks_per_row(L.nnzP, L.n_agg));
                const bool no_presmooth = dense_bottom && !dense_tail2 && l + 2 == nl;      // the dense bottom operator pre-smooths by itself (the factored level wants z1 = W r)
                launch_restrict<0>(l, lpr, cv(L.res), cv(L.res), v(lv[l + 1].r), no_presmooth ? (const H*)nullptr : (const H*)lv[l + 1].Dinv, v(lv[l + 1].z), (const T*)(omega_dev + l + 1), s);
            }
        }
        // iterate of level l after the down pass: L.z when nu is odd, L.z2 when even
        auto down_iter = [&](DevLevel<T>& L, int nu) { return v((nu % 2) ? L.z : L.z2); };
        auto down_other = [&](DevLevel<T>& L, int nu) { return v((nu % 2) ? L.z2 : L.z); };
        if (dense_tail2) {       // levels nl-2 and nl-1 at once: z2 = 2 z1 - W A z1 + G (E^T r), z1 = W r left by the restriction into nl-2
            DevLevel<T>& L = lv[nl - 2];
            const int n3 = L.n * 3, nd = lv[nl - 1].n * 3;
            PF((double)n3 * nd * sizeof(float) + (double)(n3 + nd) * cv_bytes(), lvl("t = E^T r of", nl - 2).c_str(), "k_rowdot_wg", tname(), tname_of<V>());
            hipLaunchKernelGGL((k_rowdot_wg<T, V>), dim3(nd), dim3(kBlock), 0, stream, nd, n3, (const float*)tail_Etf, cv(L.r), v(tail_t), s);
            pick<0, 1>(mem.cy16, [&](auto pk) {
                PF(bytes_sweep(L) + (double)n3 * nd * sizeof(float), lvl("cycles of", nl - 2).c_str(), "k_tail_up", tname(), pk, tname_of<V>());
                launch(k_tail_up<T, pk, V>, L.n, L.n, nd, s, (const int*)L.A_ptr, (const float*)tail_Gf, cv(tail_t), (const int*)L.A_col, (const uint32_t*)L.Apm, cv(L.z), (const H*)L.Dinv, (const T*)(omega_dev + nl - 2), v(L.z2));
            });
        } else if (dense_bottom) {      // z2 = B r: pre-sweep, coarse correction through the dense inverse and post-sweep of the last explicit level at once
            DevLevel<T>& L = lv[nl - 1];
            const int n3 = L.n * 3;
            PF((double)n3 * n3 * sizeof(float) + 2.0 * n3 * cv_bytes(), lvl("whole cycle of", nl - 1).c_str(), "k_bottom_apply", tname(), tname_of<V>());
            hipLaunchKernelGGL((k_bottom_apply<T, V>), dim3(grid_for(n3, 64)), dim3(kBlock), 0, stream, n3, n3, (const float*)bot_Bf, cv(L.r), v(L.z2), s);
        } else if (nl > 1 && lv[nl - 1].n * 4 <= kDenseThreads) {   // bottom: restrict + dense inverse + prolong in one workgroup, on the last explicit level
            DevLevel<T>& L = lv[nl - 1];
            PF(2.0 * L.nnzP * (9 * sizeof(H) + 4) + (double)nb_last * 3 * nb_last * 3 * sizeof(T) + L.n * 6.0 * cv_bytes(), lvl("restrict + dense solve + prolong", nl - 1).c_str(), "k_coarse_tail", tname(), tname_of<V>());
            hipLaunchKernelGGL((k_coarse_tail<T, V>), dim3(1), dim3(kDenseThreads), 0, stream, L.n, L.n_agg, L.R_ptr, L.R_col, (const H*)L.Rv, L.P_ptr, L.P_col, (const H*)L.P,
                               cv(L.res), (const T*)inv_last, down_iter(L, nu_at(nl - 1)), s);
        } else if (nl > 1) {   // a last explicit level too long for the one-workgroup kernel (4 lanes per row): the same three steps as launches
            DevLevel<T>& L = lv[nl - 1];
            launch_restrict<0>(nl - 1, 8, cv(L.res), cv(L.res), v(r_last), (const H*)nullptr, (V*)nullptr, (const T*)one_dev, s);
            launch_dense_solve(cv(r_last), v(z_last), s);
            launch_prolong(nl - 1, cv(z_last), down_iter(L, nu_at(nl - 1)), 3, s);
        } else {        // only level 0 above the dense level: residual r - S z is restricted from (r, sbuf)
            DevLevel<T>& L = lv[0];
            if (res_fused) launch_restrict<0>(0, 8, (const T*)sbuf, (const T*)sbuf, v(r_last), (const H*)nullptr, (V*)nullptr, (const T*)one_dev, s);
            else launch_restrict<1>(0, 8, (const T*)r, (const T*)sbuf, v(r_last), (const H*)nullptr, (V*)nullptr, (const T*)one_dev, s);
            launch_dense_solve(cv(r_last), v(z_last), s);
        }
        for (size_t l = nl - 1; l >= 1; --l) {
            DevLevel<T>& L = lv[l];
            if (l >= first_dense) continue;      // a dense level's result is in its z2 already
            const int nu = nu_at(l);
            V* cur = down_iter(L, nu); V* oth = down_other(L, nu);
            if (l + 1 < nl) launch_prolong(l, cv(lv[l + 1].z2), cur, 3, s);
            const int lprA = lanes_for_sweep(blocks_per_row(L.nnzA, L.n), L.n);
            for (int sw = 0; sw < nu; ++sw) {
                launch_sweep<1>("post-sweep", l, lprA, cv(L.r), (const V*)cur, oth, (const T*)(omega_dev + l), s);
                std::swap(cur, oth);
            }
            // nu post-sweeps after nu-1 pre-swaps: the result sits in L.z2 for every nu (odd+odd / even+even swaps)
        }
        launch_prolong(0, nl > 1 ? cv(lv[1].z2) : cv(z_last), zc, kPoseRec, s);
        // level-0 post-smoothing zc += omega Minv (r - S zc): in the epilogue of the product's pose pass where that pass reads f32 copies and its
        // result needs no all-reduce (one shard), else a launch of its own
        const bool fuse_post = fuse_post_smooth && !explicit0 && low_cycle && !collective();
        if (int rc = launch_cycle_product(slot, nullptr, fuse_post)) return rc;
        if (!fuse_post) {
            PF(pr.P * (6 + 3 + 3 + 3 + 3) * (double)sizeof(T), "post-smoothing L0", "k_smooth0", tname(), 1);
            hipLaunchKernelGGL((k_smooth0<T, 1>), dim3(nbC), dim3(kBlock), 0, stream, pr.P, (const T*)minv, (const T*)r, (const T*)sbuf, zc, (const T*)omega_dev, s);
        }
        return 0;
    }
    void launch_cg_step(int slot) {
        const T tol2 = (T)(cfg.pcg_rel_tol * cfg.pcg_rel_tol);
        const T* dots = sbuf + (size_t)pr.P * 3; const T* rzs = rzpart; int n_part = nbP;
        if (nbP > kFoldAbove) {       // a million poses: fold the partials once instead of in every workgroup of k_cg_step
            PF(2.0 * nbP * sizeof(T), "partials of the two dot products folded", "k_fold_partials", tname());
            hipLaunchKernelGGL((k_fold_partials<T>), dim3(kFoldOut, 2), dim3(kBlock), 0, stream, nbP, dots, rzs, fold_part);
            dots = fold_part; rzs = fold_part + kFoldOut; n_part = kFoldOut;
        }
        const bool ask_first = nbC <= kAskFirstAbove;      // one round of workgroups: every operand asked for before the first wait (tsgo_amg_kernels.h)
        PF(pr.P * (3 + 3 + 6 + 4 * 3 * 2) * (double)sizeof(T), "vector step + pre-smoothing L0", ask_first ? "k_cg_step" : "k_cg_step_rounds", tname());
        hipLaunchKernelGGL((ask_first ? k_cg_step<T> : k_cg_step_rounds<T>), dim3(nbC), dim3(kBlock), 0, stream, pr.P, (const T*)sbuf, dots, rzs, n_part,
                           (const CgState<T>*)st[slot], st[slot ^ 1], r, p, q, x, zc, (const T*)minv, (const T*)omega_dev, tol2, cfg.pcg_max_iters, (const T*)gscale_dev, kAmgStallIter, (T)kAmgStallRatio,
                           npart, low_cycle && !explicit0 ? zc32 : (float*)nullptr);
    }
    // one PCG iteration reading state slot `slot`, writing slot^1
    int launch_iteration(int slot, int seq = 0) {      // seq > 0: the gate reports to the host thread (do_solve_paced)
        if (amg_on) {
            // the stopping rule: in workgroup 0 of the cycle's first product (f32-copy landmark pass) where that is the iteration's first
            // launch, else its own one-workgroup kernel
            const GateArgs<T> ga{st[slot], (const T*)npart, (const T*)gpart[0], nbC, (T)(cfg.pcg_rel_tol * cfg.pcg_rel_tol), seq > 0 ? h_flag : (int*)nullptr, seq};
            const bool fold = fold_gate && !explicit0 && low_cycle && tl.n_slices > 0;
            if (!fold) {
                PF(2.0 * nbC * sizeof(T), "stopping rule", "k_iter_gate", tname());
                hipLaunchKernelGGL((k_iter_gate<T>), dim3(1), dim3(kBlock), 0, stream, ga.st, ga.rdr_part, ga.bpart, ga.n, ga.tol2, ga.host_flag, ga.seq);
            }
            if (int rc = launch_vcycle(slot, fold ? &ga : nullptr)) return rc;
            if (int rc = launch_matvec(slot, true)) return rc;
            launch_cg_step(slot);
        } else {
            if (int rc = launch_matvec(slot)) return rc;
            launch_cg_update(slot);
        }
        return 0;
    }
    int chunk() const {
        return amg_on ? kChunkAmg : kChunk;
    }
    void launch_cg_update(int slot) {
        const T tol2 = (T)(cfg.pcg_rel_tol * cfg.pcg_rel_tol);
        PF(pr.P * (3 + 3 + 6 + 4 * 3 * 2) * (double)sizeof(T), "vector step", "k_cg_update", tname());
        hipLaunchKernelGGL((k_cg_update<T>), dim3(nbC), dim3(kBlock), 0, stream, pr.P, nbP, (const CgState<T>*)st[slot], (const T*)(sbuf + (size_t)pr.P * 3), (const T*)gpart[slot], nbC,
                           (const T*)sbuf, gpart[slot ^ 1], st[slot ^ 1], minv, r, p, q, x, zc, tol2, cfg.pcg_max_iters, (const T*)gscale_dev);
    }
