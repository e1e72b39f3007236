// engine/engine_hierarchy.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// the multigrid hierarchy on the device: pattern upload, symbolic products (tsgo_sym_kernels.h), the dense bottom operators' set-up.
    static std::vector<int> rows_of(const BlockCsr& m) {
        std::vector<int> r(m.col.size());
        for (int i = 0; i < m.n_rows; ++i) for (int a = m.ptr[i]; a < m.ptr[i + 1]; ++a) r[a] = i;
        return r;
    }
    // The hierarchy's patterns are built by a host thread (host/amg.cpp) while this thread uploads state and slot tables —
    // and then the finished parts of the hierarchy itself: the contribution lists of level 0 as soon as they exist, every
    // level as soon as it is complete (a level's gather lists are tens of MB of pageable memory: their copies hide behind
    // the symbolic work on the next level).  Sharded runs remap the lists after the build and upload everything at the end.
    std::thread amg_builder;
    std::string amg_builder_error;
    std::mutex amg_mu; std::condition_variable amg_cv;
    bool amg_schur_ready = false, amg_finished = false; int amg_levels_ready = 0;
    bool device_products = true;     // research switch TSGO_HOST_PRODUCTS=1: every pair list on the host, as rounds 1-2
    int sym_decline = 0;             // test hook TSGO_SYM_DECLINE (bits): the device builders behave as if a row had overflowed their LDS tables —
                                     // 1: level 0, 2: T = A P of every level, 4: A' = R T of every odd level — so that the hand-back to the host runs
    void start_amg_builder(const tsgo_graph& g) {
        amg_schur_ready = amg_finished = false; amg_levels_ready = 0;
        amg_builder = std::thread([this, &g] {      // g is borrowed for the whole tsgo_set_graph call, which joins this thread
            const auto t0 = std::chrono::steady_clock::now();
            (void)hipSetDevice(cfg.device);
            t_builder_stream = stream2;
            AmgProgress pg;
            pg.schur_ready = [this] { { std::lock_guard<std::mutex> l(amg_mu); amg_schur_ready = true; } amg_cv.notify_all(); };
            pg.level_ready = [this](int n) { { std::lock_guard<std::mutex> l(amg_mu); amg_levels_ready = n; } amg_cv.notify_all(); };
            if (device_products && pr.world == 1)
                pg.schur = [this](const SchurCsr& in, BlockCsr& A0, std::vector<int>& sc_ptr_h, std::vector<int>& sc_od_ptr_h, std::string& err) -> bool {
                    bool accepted = false;
                    if (run_device_schur(in, A0, sc_ptr_h, sc_od_ptr_h, &accepted)) { err = last_error(); return false; }
                    return accepted;
                };
            if (device_products && pr.world == 1)
                pg.products = [this](int level, AmgLevel& L, BlockCsr& A_next, std::string& err) -> bool {       // on THIS thread, on its own stream
                    bool accepted = false;
                    if (level < 0 || level >= (int)lv.size()) return false;
                    if (run_device_products(level, L, A_next, &accepted)) { err = last_error(); return false; }
                    return accepted;
                };
            amg_builder_error = pr.world > 1 ? build_amg_sharded(g, pr, amg) : build_amg(pr, amg, &pg);
            ms_amg_symbolic = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            t_builder_stream = nullptr;
            { std::lock_guard<std::mutex> l(amg_mu); amg_finished = true; }
            amg_cv.notify_all();
        });
    }
    template <typename A> int upload_i32(int** out, const std::vector<int, A>& v) {
        if (int rc = dalloc(out, v.size())) return rc;
        if (!v.empty()) { if (int rc_ = copy_sync(*out, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice)) return rc_; }
        return 0;
    }
#define UP(dst, vec) if (int rc = upload_i32(&dst, vec)) return rc
    int upload_schur_lists() {
        if (schur_dev) return 0;
        UP(sc_ptr, amg.schur.ptr); UP(sc_optr, amg.schur.od_ptr);
        if (int rc = upload_u32m(&sc_si, amg.schur.slot_i)) return rc;
        if (int rc = upload_u32m(&sc_sk, amg.schur.slot_k)) return rc;
        if (int rc = upload_u32m(&sc_os, amg.schur.od_slot)) return rc;
        return 0;
    }
    int upload_level(size_t l) {
        const AmgLevel& L = amg.levels[l]; DevLevel<T>& D = lv[l];
        D.n = L.n; D.n_agg = L.n_agg; D.nnzA = L.A.nnz(); D.nnzP = L.P.nnz();
        if (!D.patterns_up) { UP(D.A_ptr, L.A.ptr); UP(D.A_col, L.A.col); UP(D.P_ptr, L.P.ptr); UP(D.P_col, L.P.col); UP(D.R_ptr, L.R.ptr); UP(D.R_col, L.R.col); UP(D.r_to_p, L.r_to_p); }
        UP(D.A_row, rows_of(L.A)); UP(D.diag, L.diag);
        UP(D.P_row, rows_of(L.P)); UP(D.p_self, L.p_self);
        UP(D.ps_ptr, L.p_src.ptr); UP(D.ps_x, L.p_src.x); UP(D.ps_y, L.p_src.y);
        { std::vector<int> inv(L.r_to_p.size()); for (size_t k = 0; k < inv.size(); ++k) inv[L.r_to_p[k]] = (int)k; UP(D.p_to_r, inv); }
        if (!D.products_dev) {       // the host built the two pair-list products (sharded runs, TSGO_HOST_PRODUCTS, a row too dense for the device tables)
            D.nnzT = L.T.nnz(); D.nnzNext = (int)L.a_src.ptr.size() - 1;
            D.pairs_T = (double)L.t_src.x.size() / std::max(1, D.nnzT); D.pairs_A = (double)L.a_src.x.size() / std::max<double>(1, (double)std::count(L.a_mirror.begin(), L.a_mirror.end(), -1));
            UP(D.ts_ptr, L.t_src.ptr); UP(D.ts_x, L.t_src.x); UP(D.ts_y, L.t_src.y); UP(D.T_ptr, L.T.ptr); UP(D.T_col, L.T.col);
            UP(D.as_ptr, L.a_src.ptr); UP(D.as_x, L.a_src.x); UP(D.as_y, L.a_src.y); UP(D.as_mirror, L.a_mirror);
            { std::vector<int> up; for (int b = 0; b < (int)L.a_mirror.size(); ++b) if (L.a_mirror[b] < 0) up.push_back(b); D.n_upper = (int)up.size(); UP(D.as_upper, up); }
        }
        if (int rc = upload_T(&D.rel, L.rel.data(), L.rel.size())) return rc;
        if (int rc = dalloc(&D.A, (size_t)D.nnzA * 9)) return rc;
        if (int rc = dalloc(&D.Dinv, (size_t)D.n * 9)) return rc;
        if (int rc = dalloc(&D.P, (size_t)D.nnzP * 9)) return rc;
        if (int rc = dalloc(&D.Rv, (size_t)D.nnzP * 9)) return rc;
        if (int rc = dalloc(&D.Tv, (size_t)D.nnzT * 9)) return rc;
        // sized for the f32 form (9 words per block): a handle that finds its graph too ill-conditioned for the packed halves
        // switches the cycle's copies to f32 in place (do_solve)
        if (int rc = dalloc(&D.Ppm, (size_t)D.nnzP * kCyWordsF32)) return rc;
        if (int rc = dalloc(&D.Rpm, (size_t)D.nnzP * kCyWordsF32)) return rc;
        if (l == 0 && explicit0) { if (int rc = dalloc(&D.Apm, (size_t)D.nnzA * kCyWordsF32)) return rc; }
        if (l > 0) {
            if (int rc = dalloc(&D.Apm, (size_t)D.nnzA * kCyWordsF32)) return rc;
            if (int rc = valloc(&D.r, (size_t)D.n * 3)) return rc;
            if (int rc = valloc(&D.z, (size_t)D.n * 3)) return rc;
            if (int rc = valloc(&D.res, (size_t)D.n * 3)) return rc;
            if (int rc = valloc(&D.z2, (size_t)D.n * 3)) return rc;
        }
        return 0;
    }
    // Level 0 on the device (tsgo_sym_kernels.h: k_s0_count / k_s0_fill): the pattern of the explicit Schur complement and, per block, the
    // pairs of LM-edge slots and the odometry slots it is summed from.  The pattern and the list offsets go back to the host builder (the
    // aggregation weighs a coupling by its number of contributions); the lists stay here.
    int run_device_schur(const SchurCsr& in, BlockCsr& A0, std::vector<int>& sc_ptr_h, std::vector<int>& sc_od_ptr_h, bool* accepted) {
        *accepted = false;
        const auto t0 = std::chrono::steady_clock::now();
        const int P = in.P;
        int *pp_ptr, *pp_lm, *obs_ptr, *obs_pose, *od_ptr, *od_col; uint32_t *pp_slot, *obs_slot, *od_slot;
        UP(pp_ptr, in.pp_ptr); UP(pp_lm, in.pp_lm); UP(obs_ptr, in.obs_ptr); UP(obs_pose, in.obs_pose); UP(od_ptr, in.od_ptr); UP(od_col, in.od_col);
        if (int rc = upload_u32m(&pp_slot, in.pp_slot)) return rc;
        if (int rc = upload_u32m(&obs_slot, in.obs_slot)) return rc;
        if (int rc = upload_u32m(&od_slot, in.od_slot)) return rc;
        int *d, *m, *mo, *zptr, *poff, *ooff, *flags;
        if (int rc = dalloc(&d, (size_t)P)) return rc;
        if (int rc = dalloc(&m, (size_t)P)) return rc;
        if (int rc = dalloc(&mo, (size_t)P)) return rc;
        if (int rc = dalloc(&zptr, (size_t)P + 1)) return rc;
        if (int rc = dalloc(&poff, (size_t)P + 1)) return rc;
        if (int rc = dalloc(&ooff, (size_t)P + 1)) return rc;
        if (int rc = dalloc(&flags, 4)) return rc;
        if (int rc = fill_zero(flags, 4 * sizeof(int))) return rc;
        launch_s0_count(cs(), P, pp_ptr, pp_lm, obs_ptr, obs_pose, od_ptr, od_col, in.max_pair_degree, d, m, mo, flags);
        launch_sym_scan(cs(), P, d, zptr);
        launch_sym_scan(cs(), P, m, poff);
        launch_sym_scan(cs(), P, mo, ooff);
        int h4[4];
        HIP_OK(hipMemcpyAsync(&h4[0], zptr + P, sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipMemcpyAsync(&h4[1], poff + P, sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipMemcpyAsync(&h4[2], ooff + P, sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipMemcpyAsync(&h4[3], flags, sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipStreamSynchronize(cs()));
        if (h4[3] || (sym_decline & 1)) return 0;      // a pose couples to too many others for the LDS tables: the host builds level 0
        const int nnz = h4[0], n_pairs = h4[1], n_od = h4[2];
        int* zcol = nullptr;
        if (int rc = dalloc(&zcol, (size_t)nnz)) return rc;
        if (int rc = dalloc(&sc_ptr, (size_t)nnz + 1)) return rc;
        if (int rc = dalloc(&sc_optr, (size_t)nnz + 1)) return rc;
        if (int rc = dalloc(&sc_si, (size_t)n_pairs)) return rc;
        if (int rc = dalloc(&sc_sk, (size_t)n_pairs)) return rc;
        if (int rc = dalloc(&sc_os, (size_t)n_od)) return rc;
        launch_s0_fill(cs(), P, pp_ptr, pp_lm, pp_slot, obs_ptr, obs_pose, obs_slot, od_ptr, od_col, od_slot, in.max_pair_degree, zptr, poff, ooff, zcol, sc_ptr, sc_optr, sc_si, sc_sk,
                       sc_os);
        HIP_OK(hipMemcpyAsync(sc_ptr + nnz, &n_pairs, sizeof(int), hipMemcpyHostToDevice, cs()));
        HIP_OK(hipMemcpyAsync(sc_optr + nnz, &n_od, sizeof(int), hipMemcpyHostToDevice, cs()));
        A0.n_rows = A0.n_cols = P;
        A0.ptr.resize((size_t)P + 1); A0.col.resize((size_t)nnz); sc_ptr_h.resize((size_t)nnz + 1); sc_od_ptr_h.resize((size_t)nnz + 1);
        HIP_OK(hipMemcpyAsync(A0.ptr.data(), zptr, ((size_t)P + 1) * sizeof(int), hipMemcpyDeviceToHost, cs()));
        if (nnz) HIP_OK(hipMemcpyAsync(A0.col.data(), zcol, (size_t)nnz * sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipMemcpyAsync(sc_ptr_h.data(), sc_ptr, ((size_t)nnz + 1) * sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipMemcpyAsync(sc_od_ptr_h.data(), sc_optr, ((size_t)nnz + 1) * sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipStreamSynchronize(cs()));
        schur_dev = true;
        *accepted = true;
        ms_device_products += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    }
    // One level's two pair-list products on the device (tsgo_sym_kernels.h): T = A P with its lists, A' = R T (upper blocks
    // listed, lower ones mirrored) with its lists; the pattern of A' goes back to the host builder, which needs it for the next
    // level.  *accepted = false: a row was too dense for the LDS tables — the host builds this level's lists itself.
    double ms_device_products = 0;
    int run_device_products(int l, AmgLevel& L, BlockCsr& A_next, bool* accepted) {
        *accepted = false;
        const auto t0 = std::chrono::steady_clock::now();
        DevLevel<T>& D = lv[l];
        UP(D.A_ptr, L.A.ptr); UP(D.A_col, L.A.col); UP(D.P_ptr, L.P.ptr); UP(D.P_col, L.P.col); UP(D.R_ptr, L.R.ptr); UP(D.R_col, L.R.col); UP(D.r_to_p, L.r_to_p);
        D.patterns_up = true;
        const int n = L.n, na = L.n_agg;
        int *d = nullptr, *m = nullptr, *tptr = nullptr, *tpoff = nullptr, *flags = nullptr;
        if (int rc = dalloc(&d, (size_t)std::max(n, na))) return rc;
        if (int rc = dalloc(&m, (size_t)std::max(n, na))) return rc;
        if (int rc = dalloc(&tptr, (size_t)n + 1)) return rc;
        if (int rc = dalloc(&tpoff, (size_t)n + 1)) return rc;
        if (int rc = dalloc(&flags, 4)) return rc;
        if (int rc = fill_zero(flags, 4 * sizeof(int))) return rc;
        int h3[3];
        // ---- T = A P
        launch_sym_count<0>(cs(), n, D.A_ptr, D.A_col, D.P_ptr, D.P_col, d, m, flags);
        launch_sym_scan(cs(), n, d, tptr);
        launch_sym_scan(cs(), n, m, tpoff);
        HIP_OK(hipMemcpyAsync(&h3[0], tptr + n, sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipMemcpyAsync(&h3[1], tpoff + n, sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipMemcpyAsync(&h3[2], flags, sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipStreamSynchronize(cs()));
        if (h3[2] || (sym_decline & 2)) return 0;      // declined
        const int nnzT = h3[0], pairsT = h3[1];
        int* tcol = nullptr;
        if (int rc = dalloc(&tcol, (size_t)nnzT)) return rc;
        if (int rc = dalloc(&D.ts_ptr, (size_t)nnzT + 1)) return rc;
        if (int rc = dalloc(&D.ts_x, (size_t)pairsT)) return rc;
        if (int rc = dalloc(&D.ts_y, (size_t)pairsT)) return rc;
        launch_sym_fill<0>(cs(), n, D.A_ptr, D.A_col, nullptr, D.P_ptr, D.P_col, tptr, tpoff, tcol, D.ts_ptr, D.ts_x, D.ts_y, nullptr);
        HIP_OK(hipMemcpyAsync(D.ts_ptr + nnzT, &pairsT, sizeof(int), hipMemcpyHostToDevice, cs()));
        // ---- A' = R T, upper blocks listed
        int *zptr = nullptr, *zpoff = nullptr, *nup = nullptr, *uoff = nullptr;
        if (int rc = dalloc(&zptr, (size_t)na + 1)) return rc;
        if (int rc = dalloc(&zpoff, (size_t)na + 1)) return rc;
        if (int rc = dalloc(&nup, (size_t)na)) return rc;
        if (int rc = dalloc(&uoff, (size_t)na + 1)) return rc;
        launch_sym_count<1>(cs(), na, D.R_ptr, D.R_col, tptr, tcol, d, m, flags + 1);
        launch_sym_scan(cs(), na, d, zptr);
        launch_sym_scan(cs(), na, m, zpoff);
        HIP_OK(hipMemcpyAsync(&h3[0], zptr + na, sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipMemcpyAsync(&h3[1], zpoff + na, sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipMemcpyAsync(&h3[2], flags + 1, sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipStreamSynchronize(cs()));
        if (h3[2] || ((sym_decline & 4) && (l & 1))) { D.ts_ptr = D.ts_x = D.ts_y = nullptr; return 0; }       // declined (the slab bytes of T's lists are lost until the next structure)
        const int nnzN = h3[0], pairsA = h3[1];
        int* zcol = nullptr;
        if (int rc = dalloc(&zcol, (size_t)nnzN)) return rc;
        if (int rc = dalloc(&D.as_ptr, (size_t)nnzN + 1)) return rc;
        if (int rc = dalloc(&D.as_x, (size_t)pairsA)) return rc;
        if (int rc = dalloc(&D.as_y, (size_t)pairsA)) return rc;
        if (int rc = dalloc(&D.as_mirror, (size_t)nnzN)) return rc;
        if (int rc = dalloc(&D.as_upper, (size_t)nnzN)) return rc;
        launch_sym_fill<1>(cs(), na, D.R_ptr, D.R_col, D.r_to_p, tptr, tcol, zptr, zpoff, zcol, D.as_ptr, D.as_x, D.as_y, nup);
        HIP_OK(hipMemcpyAsync(D.as_ptr + nnzN, &pairsA, sizeof(int), hipMemcpyHostToDevice, cs()));
        launch_sym_scan(cs(), na, nup, uoff);
        launch_sym_mirror(cs(), na, zptr, zcol, uoff, D.as_mirror, D.as_upper, flags + 2);
        A_next.n_rows = A_next.n_cols = na;
        A_next.ptr.resize((size_t)na + 1); A_next.col.resize((size_t)nnzN);
        HIP_OK(hipMemcpyAsync(A_next.ptr.data(), zptr, ((size_t)na + 1) * sizeof(int), hipMemcpyDeviceToHost, cs()));
        if (nnzN) HIP_OK(hipMemcpyAsync(A_next.col.data(), zcol, (size_t)nnzN * sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipMemcpyAsync(&h3[0], uoff + na, sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipMemcpyAsync(&h3[1], flags + 2, sizeof(int), hipMemcpyDeviceToHost, cs()));
        HIP_OK(hipStreamSynchronize(cs()));
        if (h3[1]) return set_error(-2, "tsgo_set_graph: the Galerkin pattern is not structurally symmetric");
        D.n_upper = h3[0]; D.nnzT = nnzT; D.nnzNext = nnzN; D.T_ptr = tptr; D.T_col = tcol;
        D.pairs_T = (double)pairsT / std::max(1, nnzT); D.pairs_A = (double)pairsA / std::max(1, D.n_upper);
        D.products_dev = true;
        *accepted = true;
        ms_device_products += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    }
    int upload_amg() {
        size_t done = 0; bool schur_done = false;
        if (pr.world == 1) {                     // consume what the builder has finished while it works on the rest
            for (;;) {
                int ready; bool schur, fin;
                {
                    std::unique_lock<std::mutex> l(amg_mu);
                    amg_cv.wait(l, [&] { return amg_finished || (int)done < amg_levels_ready || (!schur_done && amg_schur_ready); });
                    ready = amg_levels_ready; schur = amg_schur_ready; fin = amg_finished;
                }
                if (fin) break;                  // whatever is left is uploaded after the join (and errors are looked at there)
                if (schur && !schur_done) { if (int rc = upload_schur_lists()) return rc; schur_done = true; }
                for (; (int)done < ready; ++done) if (int rc = upload_level(done)) return rc;
            }
        }
        if (amg_builder.joinable()) amg_builder.join();
        if (!amg_builder_error.empty()) return set_error(-2, "tsgo_set_graph: " + amg_builder_error);
        if (amg.levels.size() > 16) return set_error(-2, "tsgo_set_graph: too many multigrid levels");
        if (!schur_done) { if (int rc = upload_schur_lists()) return rc; }
        for (; done < amg.levels.size(); ++done) if (int rc = upload_level(done)) return rc;
        lv.resize(amg.levels.size());
        UP(last_ptr, amg.A_last.ptr); UP(last_col, amg.A_last.col);
        nb_last = amg.A_last.n_rows; nnz_last = amg.A_last.nnz();
        if (nb_last * 3 > kDenseMax) return set_error(-2, "tsgo_set_graph: coarsest multigrid level too large");
        if (int rc = dalloc(&A_last, (size_t)nnz_last * 9)) return rc;
        if (int rc = dalloc(&inv_last, (size_t)nb_last * 3 * nb_last * 3)) return rc;
        if (int rc = valloc(&r_last, (size_t)nb_last * 3)) return rc;
        if (int rc = valloc(&z_last, (size_t)nb_last * 3)) return rc;
        if (int rc = dalloc(&rzpart, (size_t)nbP)) return rc;
        if (int rc = dalloc(&fold_part, (size_t)2 * kFoldOut)) return rc;
        if (int rc = dalloc(&omega_dev, 16)) return rc;
        if (int rc = dalloc(&pw_a, (size_t)pr.P * 3)) return rc;
        if (int rc = dalloc(&pw_b, (size_t)pr.P * 3)) return rc;
        if (int rc = dalloc(&rho_part, 16 * 2 * kRhoBlocks)) return rc;
        if (h_rho) (void)hipHostFree(h_rho);
        HIP_OK(hipHostMalloc((void**)&h_rho, sizeof(T) * 16 * 2 * kRhoBlocks));
        {   // S is symmetric: k_schur_blocks sums the blocks on and above the diagonal, the others are mirrored (half of the set-up's most
            // expensive gather: 137 us per hierarchy build at 100k poses)
            DevLevel<T>& L0 = lv[0];
            int *nup = nullptr, *uoff = nullptr, *flag = nullptr;
            n_upper0 = -1;
            if (int rc = dalloc(&nup, (size_t)L0.n)) return rc;
            if (int rc = dalloc(&uoff, (size_t)L0.n + 1)) return rc;
            if (int rc = dalloc(&flag, 4)) return rc;
            if (int rc = dalloc(&mirror0, (size_t)L0.nnzA)) return rc;
            if (int rc = dalloc(&upper0, (size_t)L0.nnzA)) return rc;
            if (int rc = fill_zero(flag, 4 * sizeof(int))) return rc;
            launch_count_upper(cs(), L0.n, L0.A_ptr, L0.A_col, nup);
            launch_sym_scan(cs(), L0.n, nup, uoff);
            launch_sym_mirror(cs(), L0.n, L0.A_ptr, L0.A_col, uoff, mirror0, upper0, flag);
            if (int rc = dalloc(&lower0, (size_t)L0.nnzA)) return rc;
            HIP_OK(hipMemsetAsync(lower0, 0xff, sizeof(int) * (size_t)L0.nnzA, cs()));
            launch_invert_mirror(cs(), L0.nnzA, mirror0, lower0);
            int h2[2] = {0, 0};
            HIP_OK(hipMemcpyAsync(&h2[0], uoff + L0.n, sizeof(int), hipMemcpyDeviceToHost, cs()));
            HIP_OK(hipMemcpyAsync(&h2[1], flag, sizeof(int), hipMemcpyDeviceToHost, cs()));
            HIP_OK(hipStreamSynchronize(cs()));
            if (!h2[1]) n_upper0 = h2[0];      // (a pattern that is not structurally symmetric — it always is — keeps every block summed)
        }
        // the bottom of the cycle as one dense operator (tsgo_amg_kernels.h: k_bottom_*): the last explicit level when it is small enough
        // and runs V(1,1); and the level above it in factored form (k_tail_*) when that one is small too
        const size_t nl = lv.size();
        bottom_dense = nl >= 2 && lv.back().n * 4 <= kDenseThreads && nb_last > 0 && nu_at(nl - 1) == 1;
        tail2 = bottom_dense && nl >= 3 && lv[nl - 2].n <= kSmallLevelRows && nu_at(nl - 2) == 1 && (size_t)lv[nl - 2].n * 3 * (size_t)lv.back().n * 3 <= (size_t(4) << 20);
        if (bottom_dense) {
            const size_t n3 = (size_t)lv.back().n * 3, nd = (size_t)nb_last * 3;
            if (int rc = dalloc(&bot_S, n3 * n3)) return rc;
            if (int rc = dalloc(&bot_B, n3 * n3)) return rc;
            if (int rc = dalloc(&bot_P, n3 * nd)) return rc;
            if (int rc = dalloc(&bot_E, n3 * nd)) return rc;
            if (int rc = dalloc(&bot_F, n3 * nd)) return rc;
            if (int rc = dalloc(&bot_Bf, n3 * n3)) return rc;
        }
        if (tail2) {
            const size_t n3 = (size_t)lv[nl - 2].n * 3, nd = (size_t)lv.back().n * 3;
            if (int rc = dalloc(&tail_Ef, n3 * nd)) return rc;
            if (int rc = dalloc(&tail_Etf, n3 * nd)) return rc;
            if (int rc = dalloc(&tail_Gf, n3 * nd)) return rc;
            if (int rc = valloc(&tail_t, nd)) return rc;
        }
        return 0;
    }
    int n_upper0 = -1; int *mirror0 = nullptr, *upper0 = nullptr, *lower0 = nullptr;      // level 0: blocks on / above the diagonal, and the mirror of every block below it
    bool bottom_dense = false, tail2 = false;
    T *bot_S = nullptr, *bot_B = nullptr, *bot_P = nullptr, *bot_E = nullptr, *bot_F = nullptr; float* bot_Bf = nullptr;
    void* tail_t = nullptr; float *tail_Ef = nullptr, *tail_Etf = nullptr, *tail_Gf = nullptr;
    // B = W + S W + E C E^T of the last explicit level (after k_dense_inverse, and again whenever the level's damping changes), then
    // E = P - W (A P) and G = E B of the level above it
    int launch_bottom_setup() {
        if (!bottom_dense) return 0;
        auto tiles = [](int n) { return (unsigned)((n + 15) / 16); };
        {
            DevLevel<T>& L = lv.back();
            const int n3 = L.n * 3, nd = nb_last * 3;
            const T* om = omega_dev + (lv.size() - 1);
            HIP_OK(hipMemsetAsync(bot_S, 0, sizeof(T) * (size_t)n3 * n3, stream));
            HIP_OK(hipMemsetAsync(bot_P, 0, sizeof(T) * (size_t)n3 * nd, stream));
            hipLaunchKernelGGL((k_bottom_scatter<T>), dim3(grid_for(L.nnzA + L.nnzP)), dim3(kBlock), 0, stream, L.nnzA, (const int*)L.A_row, (const int*)L.A_col, (const H*)L.A, (const H*)L.Dinv, om,
                               L.nnzP, (const int*)L.P_row, (const int*)L.P_col, (const H*)L.P, n3, nd, bot_S, bot_P);
            hipLaunchKernelGGL((k_small_gemm<T, 0>), dim3(tiles(nd), tiles(n3)), dim3(256), 0, stream, n3, nd, n3, (const T*)bot_S, n3, (const T*)bot_P, nd, bot_E, nd);          // E = S P
            hipLaunchKernelGGL((k_small_gemm<T, 0>), dim3(tiles(nd), tiles(n3)), dim3(256), 0, stream, n3, nd, nd, (const T*)bot_E, nd, (const T*)inv_last, nd, bot_F, nd);      // F = E C
            hipLaunchKernelGGL((k_small_gemm<T, 1>), dim3(tiles(n3), tiles(n3)), dim3(256), 0, stream, n3, n3, nd, (const T*)bot_F, nd, (const T*)bot_E, nd, bot_B, n3);         // G = F E^T
            hipLaunchKernelGGL((k_bottom_finish<T>), dim3(grid_for(n3 * n3)), dim3(kBlock), 0, stream, n3, (const T*)bot_S, (const H*)L.Dinv, om, (const T*)bot_B, bot_Bf, (T*)nullptr);
        }
        if (tail2) {
            DevLevel<T>& L = lv[lv.size() - 2];
            const int n3 = L.n * 3, nd = lv.back().n * 3;
            const T* om = omega_dev + (lv.size() - 2);
            HIP_OK(hipMemsetAsync(tail_Ef, 0, sizeof(float) * (size_t)n3 * nd, stream));
            hipLaunchKernelGGL((k_scatter_blocks<T>), dim3(grid_for(L.nnzP)), dim3(kBlock), 0, stream, L.nnzP, (const int*)L.P_row, (const int*)L.P_col, (const H*)L.P, nd, tail_Ef);
            hipLaunchKernelGGL((k_tail_E<T>), dim3(grid_for(L.n, 64)), dim3(kBlock), 0, stream, L.n, (const int*)L.T_ptr, (const int*)L.T_col, (const H*)L.Tv, (const H*)L.Dinv, om, nd, tail_Ef);      // E = P - W (A P)
            hipLaunchKernelGGL(k_gemm_f32, dim3((nd + 63) / 64, (n3 + 31) / 32), dim3(256), 0, stream, n3, nd, nd, (const float*)tail_Ef, nd, (const float*)bot_Bf, nd, tail_Gf, nd);      // G = E B
            hipLaunchKernelGGL(k_transpose_f32, dim3(grid_for(n3 * nd)), dim3(kBlock), 0, stream, n3, nd, (const float*)tail_Ef, tail_Etf);
        }
        return 0;
    }
#undef UP

