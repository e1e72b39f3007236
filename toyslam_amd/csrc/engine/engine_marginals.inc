// engine/engine_marginals.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// tsgo_marginals and tsgo_joint_marginals.  The diagonal blocks (or the whole joint block) of H^-1 for a list of vertices, from NV columns
// of S X = B at a time (tsgo_marginal_kernels.h): a pose takes its three unit columns, a landmark the two columns of Y_l = W_{:,l} Dl^-1
// (DESIGN.md section 11).
//
// State rule: the call linearises at the current estimates (lambda = 0) and builds a fresh hierarchy IN the handle's own buffers, so
// before it touches anything it copies every byte of the handle's device slabs aside and afterwards copies them back (plus the two host
// fields these launches write: lambda and the smoother damping per level).  Everything the next tsgo_optimize reads is then what it
// was, bit for bit; nothing of the solver's memory (Engine::mem: hierarchy age, warm-start history, cycle storage, ...) is touched.
    // Columns per launch chain (research: TSGO_MARGINAL_WIDTH = 1, 8 or 16).  Measured at config 3 (profiles/r06_marginals_timing.jsonl):
    // under the multigrid cycle 16 columns solve 264 columns/s against 139 at 8 and 24 at 1; block-Jacobi batches (thousands of short
    // iterations) run 0.19 ms per iteration at 8 columns and 0.47 at 16, so they take 8.
    int marginal_width() const {
        const int w = TSGO_RESEARCH_INT("TSGO_MARGINAL_WIDTH", amg_on ? 16 : 8);
        return w <= 1 ? 1 : (w <= 8 ? 8 : 16);
    }
    static constexpr int kMbChunkMg = 4, kMbChunkBj = 32;      // iterations enqueued between two looks at the batch's state

    struct MbBuf {
        CallScratch mem;      // everything below lies in it (mb_alloc) and goes with it
        T *x = nullptr, *r = nullptr, *z = nullptr, *p = nullptr, *q = nullptr, *s0 = nullptr, *t = nullptr;
        T *dpart = nullptr, *gpart = nullptr, *fd = nullptr, *fg = nullptr;
        MbState<T>* st[2] = {nullptr, nullptr};
        MbColumn *cols = nullptr, *items = nullptr;
        double* out = nullptr;
        int* zero = nullptr;
        std::vector<T*> lb, lz, lz2, lres;      // per level >= 1: right-hand side, iterate (two), residual
        T *b_last = nullptr, *z_last = nullptr;
        std::vector<T*> lfinal;                 // where each level's post-smoothed iterate ended (mb_cycle)
        int nbV = 0;
    };

    // ---- launches ----
    template <int NV> void mb_lm(const T* v, T* t, const int* stop) {
        if (tl.n_slices == 0) return;
        pick<1, 2, 4, 8>(pr.by_lm.G, [&](auto g) { launch(k_mb_schur_lm<T, g, NV>, nbL, tl, v, (const T*)ps, (const T*)ninv, t, stop); });
    }
    // S v (MODE 0: + partials of v^T S v; 2: without) or rvec - S v (MODE 1), all NV columns
    template <int NV, int MODE> void mb_product(MbBuf& B, const T* v, T* out, const T* rvec, const int* stop) {
        mb_lm<NV>(v, B.t, stop);
        pick<1, 2, 4, 8>(pr.by_pose.G, [&](auto g) { pick<0, 1>(oj(), [&](auto general) {
            launch(k_mb_schur_pose<T, g, general, NV, MODE>, nbP, tp, to, v, B.t, (const T*)ps, (const T*)dp, out, rvec, B.dpart, stop);
        }); });
    }
    template <int NV, int MODE> void mb_bsr(int n, const int* ptr, const int* col, const H* M, const T* x, const T* b, const H* dinv, const T* omega, T* out, const int* stop) {
        launch(k_mb_bsr<T, NV, MODE>, grid_for(n * NV), n, ptr, col, M, x, b, dinv, omega, out, stop);
    }
    // z = V-cycle(r) on the handle's hierarchy, NV columns: level 0 with the implicit Schur passes and Minv (one sweep per side), the levels
    // below with their block-indexed matrices (nu_at(l) block-Jacobi sweeps per side), the coarsest one through its dense inverse.  Same
    // number of sweeps on both sides and R = P^T: a symmetric preconditioner.
    template <int NV> void mb_cycle(MbBuf& B, const T* r, T* z, const int* stop) {
        const int P = pr.P;
        const size_t nl = lv.size();
        const int gv = grid_for(P * NV);
        launch(k_mb_smooth0<T, NV, 0>, gv, P, (const T*)minv, (const T*)omega_dev, r, (const T*)nullptr, z, stop);
        mb_product<NV, 1>(B, z, B.s0, r, stop);
        mb_bsr<NV, 2>(lv[0].n_agg, lv[0].R_ptr, lv[0].R_col, (const H*)lv[0].Rv, B.s0, nullptr, nullptr, nullptr, nl > 1 ? B.lb[1] : B.b_last, stop);
        for (size_t l = 1; l < nl; ++l) {
            DevLevel<T>& L = lv[l];
            const int nu = nu_at(l);
            T* cur = B.lz[l]; T* oth = B.lz2[l];
            mb_bsr<NV, 1>(L.n, L.A_ptr, L.A_col, (const H*)L.A, nullptr, B.lb[l], (const H*)L.Dinv, omega_dev + l, cur, stop);
            for (int sw = 1; sw < nu; ++sw) { mb_bsr<NV, 1>(L.n, L.A_ptr, L.A_col, (const H*)L.A, cur, B.lb[l], (const H*)L.Dinv, omega_dev + l, oth, stop); std::swap(cur, oth); }
            mb_bsr<NV, 0>(L.n, L.A_ptr, L.A_col, (const H*)L.A, cur, B.lb[l], nullptr, nullptr, B.lres[l], stop);
            mb_bsr<NV, 2>(L.n_agg, L.R_ptr, L.R_col, (const H*)L.Rv, B.lres[l], nullptr, nullptr, nullptr, l + 1 < nl ? B.lb[l + 1] : B.b_last, stop);
            B.lfinal[l] = cur;
        }
        launch(k_mb_dense<T, NV>, grid_for(nb_last * NV), nb_last, (const T*)inv_last, (const T*)B.b_last, B.z_last, stop);
        for (size_t l = nl - 1; l >= 1; --l) {
            DevLevel<T>& L = lv[l];
            const int nu = nu_at(l);
            T* cur = B.lfinal[l]; T* oth = cur == B.lz[l] ? B.lz2[l] : B.lz[l];
            mb_bsr<NV, 3>(L.n, L.P_ptr, L.P_col, (const H*)L.P, l + 1 < nl ? B.lfinal[l + 1] : B.z_last, nullptr, nullptr, nullptr, cur, stop);
            for (int sw = 0; sw < nu; ++sw) { mb_bsr<NV, 1>(L.n, L.A_ptr, L.A_col, (const H*)L.A, cur, B.lb[l], (const H*)L.Dinv, omega_dev + l, oth, stop); std::swap(cur, oth); }
            B.lfinal[l] = cur;
        }
        mb_bsr<NV, 3>(lv[0].n, lv[0].P_ptr, lv[0].P_col, (const H*)lv[0].P, nl > 1 ? B.lfinal[1] : B.z_last, nullptr, nullptr, nullptr, z, stop);
        mb_product<NV, 2>(B, z, B.s0, nullptr, stop);
        launch(k_mb_smooth0<T, NV, 1>, gv, P, (const T*)minv, (const T*)omega_dev, r, (const T*)B.s0, z, stop);
    }

    // The right-hand side of the three readers whose columns are unit columns (B.cols): what mb_for_batches passes unless told otherwise
    template <int NV> auto mb_unit_rhs(MbBuf& B) {
        return [this, &B](int, int) -> int {
            HIP_OK(hipMemsetAsync(B.r, 0, (size_t)pr.P * NV * 3 * sizeof(T), stream));
            launch_wave(k_mb_rhs<T, NV>, 1, tl, pr.by_lm.G, (const T*)ps, (const T*)lmrec, (const MbColumn*)B.cols, B.r);
            return 0;
        };
    }
    // PCG on one batch: X = S^-1 B, column by column; rhs() writes B into B.r (every entry, or zeroes it first), so that a repeat of the
    // batch rebuilds it.  out: the batch and its largest / summed iterations counted in s, and whether any column broke down (1) or ran
    // out of iterations (2).
    template <int NV, typename Rhs> int mb_solve(MbBuf& B, bool mg, double tol, tsgo_marginal_stats& s, int* fail_out, Rhs&& rhs) {
        const int P = pr.P;
        const size_t vb = (size_t)P * NV * 3 * sizeof(T);
        HIP_OK(hipMemsetAsync(B.x, 0, vb, stream));
        if (int rc = rhs()) return rc;
        const int gv = grid_for(P * NV);
        // z = M^-1 r (the cycle, or Minv inside k_mb_dots) and the partials of r^T z, folded
        auto precondition = [&](const int* stop) {
            if (mg) {
                mb_cycle<NV>(B, B.r, B.z, stop);
                launch(k_mb_dots<T, NV, 0>, gv, P, (const T*)B.r, B.z, (const T*)minv, B.gpart, stop);
            } else launch(k_mb_dots<T, NV, 1>, gv, P, (const T*)B.r, B.z, (const T*)minv, B.gpart, stop);
            launch(k_mb_fold<T>, 1, gv, 2 * NV, (const T*)B.gpart, B.fg, stop);
        };
        precondition(B.zero);
        launch(k_mb_start<T, NV>, gv, P, (const T*)B.fg, (const T*)B.z, B.p, B.st[0]);
        const T tol2 = (T)(tol * tol);
        const int chunk = mg ? kMbChunkMg : kMbChunkBj;
        MbState<T> hs;
        int launched = 0;
        for (;;) {
            for (int j = 0; j < chunk; ++j, ++launched) {
                const int k = launched & 1;
                const int* stop = reinterpret_cast<const int*>(B.st[k]);      // MbState::all_done
                mb_product<NV, 0>(B, B.p, B.q, nullptr, stop);
                launch(k_mb_fold<T>, 1, nbP, NV, (const T*)B.dpart, B.fd, stop);
                launch(k_mb_alpha<T, NV>, gv, P, (const T*)B.fd, (const MbState<T>*)B.st[k], (const T*)B.p, (const T*)B.q, B.x, B.r);
                precondition(stop);
                launch(k_mb_beta<T, NV>, gv, P, (const T*)B.fd, (const T*)B.fg, (const MbState<T>*)B.st[k], B.st[k ^ 1], (const T*)B.z, B.p, tol2, cfg.pcg_max_iters);
            }
            HIP_OK(hipMemcpyAsync(&hs, B.st[launched & 1], sizeof(hs), hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            if (hs.all_done) break;
            if (launched > cfg.pcg_max_iters + 2 * chunk) return set_error(-20, "tsgo_marginals: PCG did not terminate");
        }
        ++s.batches; *fail_out = 0;
        for (int c = 0; c < NV; ++c) { s.pcg_iters_max = std::max(s.pcg_iters_max, hs.col[c].iters); s.pcg_iters_total += hs.col[c].iters; *fail_out = std::max(*fail_out, hs.col[c].fail); }
        return 0;
    }

    int mb_alloc(MbBuf& B, int NV) {
        B.nbV = grid_for(pr.P * NV);
        CallScratch& m = B.mem;
        const size_t pv = (size_t)pr.P * NV * 3 * sizeof(T);
        for (T** v : {&B.x, &B.r, &B.z, &B.p, &B.q, &B.s0}) m.want(v, pv);
        m.want(&B.t, (size_t)std::max(pr.L, 1) * NV * 2 * sizeof(T));
        m.want(&B.dpart, (size_t)nbP * NV * sizeof(T));
        m.want(&B.gpart, (size_t)B.nbV * 2 * NV * sizeof(T));
        m.want(&B.fd, (size_t)NV * sizeof(T));
        m.want(&B.fg, (size_t)2 * NV * sizeof(T));
        for (MbState<T>** v : {&B.st[0], &B.st[1]}) m.want(v, sizeof(MbState<T>));
        for (MbColumn** v : {&B.cols, &B.items}) m.want(v, (size_t)kMbMaxWidth * sizeof(MbColumn));
        m.want(&B.out, (size_t)kMbMaxWidth * 9 * sizeof(double));
        m.want(&B.zero, 4 * sizeof(int));
        const size_t nl = amg_on ? lv.size() : 0;
        B.lb.assign(nl, nullptr); B.lz.assign(nl, nullptr); B.lz2.assign(nl, nullptr); B.lres.assign(nl, nullptr); B.lfinal.assign(nl, nullptr);
        for (size_t l = 1; l < nl; ++l)
            for (T** v : {&B.lb[l], &B.lz[l], &B.lz2[l], &B.lres[l]}) m.want(v, (size_t)lv[l].n * NV * 3 * sizeof(T));
        if (amg_on) for (T** v : {&B.b_last, &B.z_last}) m.want(v, (size_t)nb_last * NV * 3 * sizeof(T));
        if (int rc = m.commit()) return rc;
        HIP_OK(hipMemsetAsync(m.base, 0, m.total, stream));
        return 0;
    }

    // the batches of one query list: queries are packed whole (3 columns a pose, 2 a landmark) into batches of NV columns
    template <int NV> int mb_run(const std::vector<MbQuery>& qs, double tol, double* cov, tsgo_marginal_stats& s) {
        MbBuf B;
        if (int rc = mb_alloc(B, NV)) return rc;
        const QueryBatches pl = whole_query_batches(qs, NV);
        if (pl.narrow) return mb_run_narrow<NV>(B, qs, tol, cov, s);      // NV < 3: columns one by one
        return mb_for_batches<NV>(B, pl.all, pl.ranges, tol, s, [&](int b, int, int) -> int {
            const size_t q0 = (size_t)pl.q_off[(size_t)b], n = (size_t)pl.q_off[(size_t)b + 1] - q0;
            HIP_OK(hipMemcpyAsync(B.items, pl.items.data() + q0, n * sizeof(MbColumn), hipMemcpyHostToDevice, stream));
            std::vector<double> o(n * 9);
            launch_wave(k_mb_extract<T, NV>, 1, tl, pr.by_lm.G, (int)n, (const T*)ps, (const T*)lmrec, (const MbColumn*)B.items, (const T*)B.x, B.out);
            HIP_OK(hipMemcpyAsync(o.data(), B.out, o.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            for (size_t k = 0; k < n; ++k) mb_store(o.data() + 9 * k, cov + 9 * (q0 + k));
            return 0;
        });
    }
    // Every reader of the batched solve.  For each range (j0, nc) of `all`: the columns go to B.cols (padded to kMbMaxWidth with "none"),
    // mb_batch solves them (and ends with the one host synchronisation of a batch), after(b, j0, nc) reads X out of B.x with the copies and waits it needs.
    // rhs(j0, nc): the batch's right-hand side (mb_solve); the overload without one takes the unit columns of B.cols (mb_unit_rhs).
    template <int NV, typename After>
    int mb_for_batches(MbBuf& B, const std::vector<MbColumn>& all, const BatchRanges& ranges, double tol, tsgo_marginal_stats& s, After&& after) {
        return mb_for_batches<NV>(B, all, ranges, tol, s, mb_unit_rhs<NV>(B), after);
    }
    template <int NV, typename Rhs, typename After>
    int mb_for_batches(MbBuf& B, const std::vector<MbColumn>& all, const BatchRanges& ranges, double tol, tsgo_marginal_stats& s, Rhs&& rhs, After&& after) {
        s.batch_width = NV; s.preconditioner = amg_on ? 1 : 0;
        float ms = 0;
        for (size_t b = 0; b < ranges.size(); ++b) {
            const int j0 = ranges[b].first, nc = ranges[b].second;
            std::vector<MbColumn> cols(kMbMaxWidth, MbColumn{-1, 0, 0, 0});
            std::copy(all.begin() + j0, all.begin() + j0 + nc, cols.begin());
            HIP_OK(hipMemcpyAsync(B.cols, cols.data(), cols.size() * sizeof(MbColumn), hipMemcpyHostToDevice, stream));
            if (int rc = mb_batch<NV>(B, tol, s, &ms, [&]() -> int { return rhs(j0, nc); })) return rc;
            if (int rc = after((int)b, j0, nc)) return rc;
            s.columns += nc;
        }
        s.ms_solve = ms;
        return 0;
    }
    static void mb_store(const double* m, double* out) {      // (Sigma + Sigma^T) / 2
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) out[3 * a + b] = 0.5 * (m[3 * a + b] + m[3 * b + a]);
    }
    // one batch: the handle's preconditioner, repeated with block-Jacobi after a breakdown of the cycle
    template <int NV, typename Rhs> int mb_batch(MbBuf& B, double tol, tsgo_marginal_stats& s, float* ms_acc, Rhs&& rhs) {
        HIP_OK(hipEventRecord(ev[0], stream));
        int fail = 0;
        if (int rc = mb_solve<NV>(B, amg_on, tol, s, &fail, rhs)) return rc;
        if (fail == 1 && amg_on) {
            ++s.fallbacks; s.preconditioner = 0;
            if (int rc = mb_solve<NV>(B, false, tol, s, &fail, rhs)) return rc;
        }
        HIP_OK(hipEventRecord(ev[1], stream));
        HIP_OK(hipEventSynchronize(ev[1]));
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        *ms_acc += ms;
        if (fail == 1) return set_error(-21, "tsgo_marginals: PCG breakdown");
        if (fail != 0) return set_error(-22, "tsgo_marginals: PCG did not converge within pcg_max_iters");
        return 0;
    }
    // width 1 (the research baseline): every column a batch of its own.  A query's three / two solves are gathered on the host into a
    // [P][need][3] block; after the last of them the block goes back and is read out with the same kernel
    template <int NV> int mb_run_narrow(MbBuf& B, const std::vector<MbQuery>& qs, double tol, double* cov, tsgo_marginal_stats& s) {
        const int P = pr.P;
        std::vector<MbColumn> all; std::vector<size_t> query_of;
        for (size_t q = 0; q < qs.size(); ++q)
            for (int k = 0; k < mb_columns_of(qs[q].kind); ++k) { all.push_back(MbColumn{qs[q].kind, qs[q].idx, k, 0}); query_of.push_back(q); }
        std::vector<T> xall, col((size_t)P * NV * 3);
        return mb_for_batches<NV>(B, all, full_batches((int)all.size(), 1), tol, s, [&](int, int j, int) -> int {
            const size_t q = query_of[(size_t)j];
            const int need = mb_columns_of(qs[q].kind), k = all[(size_t)j].comp;
            if (k == 0) xall.assign((size_t)P * need * 3, T(0));
            HIP_OK(hipMemcpyAsync(col.data(), B.x, col.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            for (int i = 0; i < P; ++i) for (int m = 0; m < 3; ++m) xall[((size_t)i * need + k) * 3 + m] = col[(size_t)i * NV * 3 + m];
            if (k + 1 < need) return 0;
            CallScratch xs; T* xd = nullptr;
            xs.want(&xd, xall.size() * sizeof(T));
            if (int rc = xs.commit()) return rc;
            HIP_OK(hipMemcpyAsync(xd, xall.data(), xall.size() * sizeof(T), hipMemcpyHostToDevice, stream));
            MbColumn it{qs[q].kind, qs[q].idx, 0, 0};
            HIP_OK(hipMemcpyAsync(B.items, &it, sizeof(it), hipMemcpyHostToDevice, stream));
            double o[9];
            pick<3, 2>(need, [&](auto w) { launch_wave(k_mb_extract<T, w>, 1, tl, pr.by_lm.G, 1, (const T*)ps, (const T*)lmrec, (const MbColumn*)B.items, (const T*)xd, B.out); });
            HIP_OK(hipMemcpyAsync(o, B.out, sizeof(o), hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            mb_store(o, cov + 9 * q);
            return 0;
        });
    }

    // ONE linearisation at the current estimates, without damping, and a hierarchy built for it (both entry points)
    int mb_prepare() {
        lambda = 0;
        launch_lin();
        launch_finalize();
        if (amg_on) {
            if (int rc = launch_amg_setup()) return rc;
            if (int rc = estimate_damping()) return rc;
            if (int rc = launch_bottom_setup()) return rc;
        }
        return 0;
    }

    // the whole call between the snapshot and the restore (mb_guarded): the linearisation, then run(the batch width, as a constant)
    template <typename F> int mb_compute(F&& run) {
        return mb_guarded([&]() -> int { if (int rc = mb_prepare()) return rc; return pick<1, 16, 8>(marginal_width(), run); });
    }

    // The shell both entry points share.  mb_queries: the handle's checks and the id -> (pose | landmark, index) map (`name` prefixes
    // the errors; out_null: the caller's output pointer is missing where it is required).  n_ids == 0 returns 0 with qs empty before
    // the fixed-vertex check.
    // H is regular: a fixed vertex, or a pose prior on every axis (which anchors H to the world frame)
    bool mb_anchored() const {
        bool fixed = false;
        for (double g : pr.gauge_p) fixed |= g > 0;
        for (double g : pr.gauge_l) fixed |= g > 0;
        return fixed || has_full_pose_prior();
    }
    int mb_queries(const char* name, const uint32_t* ids, int n_ids, bool out_null, std::vector<MbQuery>& qs) {
        const std::string nm(name);
        qs.clear();
        if (sizeof(T) != 8) return set_error(-1, nm + ": needs precision = 64 (with the gauge, cond(H) is about 2e7: f32 marginals would be noise)");
        if (collective()) return set_error(-1, nm + ": edge-sharded handles (world > 1) are not supported");
        if (!have_graph_data) return set_error(-3, nm + ": no graph set");
        if (n_ids < 0 || (n_ids > 0 && (!ids || out_null))) return set_error(-1, nm + ": bad argument");
        if (n_ids == 0) return 0;
        if (!mb_anchored()) return set_error(-1, nm + ": marginals need a fixed vertex (without one H is singular)");
        qs.resize((size_t)n_ids);
        const VertexIndex& vi = vertices();
        for (int k = 0; k < n_ids; ++k) {
            const int v = vi.ids.find(ids[k]);
            if (v < 0 || vi.of[(size_t)v].kind < 0) { qs.clear(); return set_error(-1, nm + ": unknown vertex id " + std::to_string(ids[k])); }
            qs[(size_t)k] = vi.of[(size_t)v];
        }
        return 0;
    }
    // mb_guarded: run(), a callable of the prepared handle, between the snapshot of every device byte the handle owns and its restore
    // (see the top of this file)
    template <typename F> int mb_guarded(F&& run) {
        HIP_OK(hipSetDevice(cfg.device));
        size_t total = 0;
        for (const Slab& sl : slabs) total += sl.used;
        CallScratch aside; char* snap = nullptr;
        aside.want(&snap, std::max<size_t>(total, 1));
        if (int rc = aside.commit()) return rc;
        auto copy_slabs = [&](bool back) -> int {      // aside, or back
            size_t off = 0;
            for (const Slab& sl : slabs) { if (sl.used) { const hipError_t e = hipMemcpyAsync(back ? sl.base : snap + off, back ? snap + off : sl.base, sl.used, hipMemcpyDeviceToDevice, stream); HIP_OK(e); } off += sl.used; }
            return 0;
        };
        if (int rc = copy_slabs(false)) return rc;
        const double lambda0 = lambda;
        const std::vector<double> omega0 = omega_host;
        const int rc = run();
        lambda = lambda0; omega_host = omega0;
        const std::string err = rc ? std::string(tsgo_last_error()) : std::string();
        if (int rc2 = copy_slabs(true)) return rc2;
        const hipError_t es = hipStreamSynchronize(stream);
        HIP_OK(es);
        if (rc) return set_error(rc, err);
        return 0;
    }

    int marginals(const uint32_t* ids, int n_ids, double rel_tol, double* cov, tsgo_marginal_stats* st_out) override {
        const auto wall0 = std::chrono::steady_clock::now();
        tsgo_marginal_stats s; std::memset(&s, 0, sizeof(s));
        std::vector<MbQuery> qs;
        if (int rc = mb_queries("tsgo_marginals", ids, n_ids, !cov, qs)) return rc;
        if (n_ids == 0) { if (st_out) *st_out = s; return 0; }
        const double tol = rel_tol > 0 ? rel_tol : cfg.pcg_rel_tol;
        if (int rc = mb_compute([&](auto nv) { return mb_run<nv>(qs, tol, cov, s); })) return rc;
        s.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        if (st_out) *st_out = s;
        return 0;
    }

    // ---- tsgo_joint_marginals: the whole D x D block of H^-1 over the queried vertices (DESIGN.md section 11) ----
    static constexpr int64_t kJointMaxDim = 8192;      // D x D doubles: 512 MB
    // Every query column in order (3 a pose, 2 a landmark: row = column = its place in the compact D), NV per batch: every batch but the
    // last is full, and a query's columns may straddle two batches.  After each batch k_mb_joint writes the [D][NV] slice of the result
    // (one host synchronisation), which lands in columns j0 .. j0 + nc of cov.  At the end cov = (C + C^T) / 2.
    template <int NV> int mb_run_joint(const std::vector<MbQuery>& qs, int D, double tol, double* cov, tsgo_marginal_stats& s) {
        MbBuf B;
        if (int rc = mb_alloc(B, NV)) return rc;
        const size_t nq = qs.size();
        std::vector<MbColumn> items(nq), all;
        all.reserve((size_t)D);
        for (size_t q = 0; q < nq; ++q) {
            items[q] = MbColumn{qs[q].kind, qs[q].idx, (int)all.size(), 0};
            for (int k = 0; k < mb_columns_of(qs[q].kind); ++k) all.push_back(MbColumn{qs[q].kind, qs[q].idx, k, 0});
        }
        CallScratch joint; MbColumn* items_d = nullptr; double* out_d = nullptr;
        joint.want(&items_d, nq * sizeof(MbColumn));
        joint.want(&out_d, (size_t)D * NV * sizeof(double));
        if (int rc = joint.commit()) return rc;
        HIP_OK(hipMemcpyAsync(items_d, items.data(), nq * sizeof(MbColumn), hipMemcpyHostToDevice, stream));
        std::vector<double> o((size_t)D * NV);
        if (int rc = mb_for_batches<NV>(B, all, full_batches(D, NV), tol, s, [&](int, int j0, int nc) -> int {
            launch_wave(k_mb_joint<T, NV>, (int)nq, tl, pr.by_lm.G, (const T*)ps, (const T*)lmrec, (const MbColumn*)items_d, (const MbColumn*)B.cols, (const T*)B.x, out_d);
            HIP_OK(hipGetLastError());
            HIP_OK(hipMemcpyAsync(o.data(), out_d, o.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
            HIP_OK(hipStreamSynchronize(stream));
            for (int r = 0; r < D; ++r)
                for (int c = 0; c < nc; ++c) cov[(size_t)r * D + j0 + c] = o[(size_t)r * NV + c];
            return 0;
        })) return rc;
        for (int r = 0; r < D; ++r)
            for (int c = 0; c < r; ++c) {
                const double v = 0.5 * (cov[(size_t)r * D + c] + cov[(size_t)c * D + r]);
                cov[(size_t)r * D + c] = v; cov[(size_t)c * D + r] = v;
            }
        return 0;
    }

    int joint_marginals(const uint32_t* ids, int n_ids, double rel_tol, double* cov, int64_t cov_cap, int* dim_out, tsgo_marginal_stats* st_out) override {
        const auto wall0 = std::chrono::steady_clock::now();
        tsgo_marginal_stats s; std::memset(&s, 0, sizeof(s));
        std::vector<MbQuery> qs;
        if (int rc = mb_queries("tsgo_joint_marginals", ids, n_ids, false, qs)) return rc;
        int64_t D = 0;
        for (const MbQuery& q : qs) D += q.kind == 0 ? 3 : 2;
        if (dim_out) *dim_out = (int)std::min<int64_t>(D, INT32_MAX);
        if (D > kJointMaxDim) return set_error(-1, "tsgo_joint_marginals: D = " + std::to_string(D) + " rows exceed " + std::to_string(kJointMaxDim));
        if (!cov) {
            if (!dim_out) return set_error(-1, "tsgo_joint_marginals: bad argument (cov_out and dim_out both NULL)");
            if (st_out) *st_out = s;
            return 0;
        }
        if (cov_cap < D * D) return set_error(-1, "tsgo_joint_marginals: cov_cap " + std::to_string(cov_cap) + " is below D^2 = " + std::to_string(D * D));
        if (D == 0) { if (st_out) *st_out = s; return 0; }
        const double tol = rel_tol > 0 ? rel_tol : cfg.pcg_rel_tol;
        const int Di = (int)D;
        if (int rc = mb_compute([&](auto nv) { return mb_run_joint<nv>(qs, Di, tol, cov, s); })) return rc;
        s.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        if (st_out) *st_out = s;
        return 0;
    }
