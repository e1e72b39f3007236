// engine/engine_testing.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body, TSGO_TESTING builds only):
// tsgo_testing_apply (include/tsgo_testing.h): the operators PCG applies, column by column, with the launches the solver itself makes;
// tsgo_testing_warm_start: what the PCG warm start decides and writes (at the end of this file).
//
// State rule: as tsgo_marginals — the call runs between mb_guarded's snapshot of every device byte the handle owns and its restore, on
// ONE linearisation at the current estimates with a hierarchy built for it (mb_prepare): no counter of the solver moves, and everything
// the next tsgo_optimize reads is what it was, bit for bit.
    // a vector in graph pose order (3 per pose) into the pose records zc (and their f32 copy): the records keep their cos / sin
    int ta_load_zc(const std::vector<int>& of_graph, const double* in, std::vector<T>& h, std::vector<float>& h32) {
        const int P = pr.P;
        for (int i = 0; i < P; ++i)
            for (int k = 0; k < 3; ++k) { const T v = (T)in[3 * (size_t)of_graph[i] + k]; h[(size_t)i * kPoseRec + k] = v; h32[(size_t)i * kPoseRec + k] = (float)v; }
        HIP_OK(hipMemcpyAsync(zc, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemcpyAsync(zc32, h32.data(), h32.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        return 0;
    }
    int ta_load_r(const std::vector<int>& of_graph, const double* in, std::vector<T>& h3) {
        const int P = pr.P;
        for (int i = 0; i < P; ++i) for (int k = 0; k < 3; ++k) h3[(size_t)i * 3 + k] = (T)in[3 * (size_t)of_graph[i] + k];
        HIP_OK(hipMemcpyAsync(r, h3.data(), h3.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        return 0;
    }
    template <int NV> int ta_batched(const std::vector<int>& of_graph, const double* in, double* out, int n_cols) {
        const int P = pr.P;
        MbBuf B;
        if (int rc = mb_alloc(B, NV)) return rc;
        std::vector<T> h((size_t)P * NV * 3, T(0));
        for (int c = 0; c < n_cols; ++c)
            for (int i = 0; i < P; ++i) for (int k = 0; k < 3; ++k) h[((size_t)i * NV + c) * 3 + k] = (T)in[(size_t)c * 3 * P + 3 * (size_t)of_graph[i] + k];
        HIP_OK(hipMemcpyAsync(B.r, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        mb_cycle<NV>(B, B.r, B.z, B.zero);      // B.zero: no column is stopped
        HIP_OK(hipMemcpyAsync(h.data(), B.z, h.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        for (int c = 0; c < n_cols; ++c)
            for (int i = 0; i < P; ++i) for (int k = 0; k < 3; ++k) out[(size_t)c * 3 * P + 3 * (size_t)of_graph[i] + k] = (double)h[((size_t)i * NV + c) * 3 + k];
        return 0;
    }
    // internal pose -> its place among the graph's poses (vertex order)
    std::vector<int> ta_of_graph() const {
        const int P = pr.P;
        std::vector<int> rank_of_vertex((size_t)pr.n_vertices, -1), of_graph((size_t)P);
        { std::vector<char> is_pose((size_t)pr.n_vertices, 0); for (int i = 0; i < P; ++i) is_pose[(size_t)pr.pose_vertex[i]] = 1;
          int k = 0; for (int v = 0; v < pr.n_vertices; ++v) if (is_pose[(size_t)v]) rank_of_vertex[(size_t)v] = k++; }
        for (int i = 0; i < P; ++i) of_graph[(size_t)i] = rank_of_vertex[(size_t)pr.pose_vertex[i]];
        return of_graph;
    }
    int ta_run(int which, const double* in, double* out, int n_cols) {
        if (int rc = mb_prepare()) return rc;      // state slot 0 says "not done"
        const int P = pr.P;
        const std::vector<int> of_graph = ta_of_graph();
        if (which == 3) return pick<1, 16, 8>(marginal_width(), [&](auto nv) { return ta_batched<nv>(of_graph, in, out, n_cols); });
        std::vector<T> hz((size_t)P * kPoseRec), h3((size_t)P * 3); std::vector<float> hz32((size_t)P * kPoseRec);
        { if (int rc = copy_sync(hz.data(), zc, hz.size() * sizeof(T), hipMemcpyDeviceToHost)) return rc; }
        { if (int rc = copy_sync(hz32.data(), zc32, hz32.size() * sizeof(float), hipMemcpyDeviceToHost)) return rc; }
        for (int c = 0; c < n_cols; ++c) {
            const double* x_in = in + (size_t)c * 3 * P; double* y = out + (size_t)c * 3 * P;
            const bool from_sbuf = which != 2;
            if (which == 0) {
                if (int rc = ta_load_zc(of_graph, x_in, hz, hz32)) return rc;
                if (int rc = launch_matvec(0, true)) return rc;
            } else if (which == 1) {
                if (int rc = ta_load_zc(of_graph, x_in, hz, hz32)) return rc;
                if (int rc = launch_cycle_product(0)) return rc;
            } else {
                // zc (and zc32) = omega_0 Minv r as k_cg_step / k_pose_finalize leave them: k_warm_residual with S x0 = 0 is that arithmetic
                if (int rc = ta_load_r(of_graph, x_in, h3)) return rc;
                HIP_OK(hipMemsetAsync(sbuf, 0, sizeof(T) * (size_t)P * 3, stream));
                launch(k_warm_residual<T>, nbC, P, (const T*)sbuf, (const T*)minv, r, zc, (const T*)(amg_on ? omega_dev : one_dev), npart, amg_on && low_cycle ? zc32 : (float*)nullptr);
                if (amg_on) { if (int rc = launch_vcycle(0)) return rc; }
            }
            if (from_sbuf) {
                if (int rc = copy_sync(h3.data(), sbuf, h3.size() * sizeof(T), hipMemcpyDeviceToHost)) return rc;
                for (int i = 0; i < P; ++i) for (int k = 0; k < 3; ++k) y[3 * (size_t)of_graph[i] + k] = (double)h3[(size_t)i * 3 + k];
            } else {
                if (int rc = copy_sync(hz.data(), zc, hz.size() * sizeof(T), hipMemcpyDeviceToHost)) return rc;
                for (int i = 0; i < P; ++i) for (int k = 0; k < 3; ++k) y[3 * (size_t)of_graph[i] + k] = (double)hz[(size_t)i * kPoseRec + k];
            }
        }
        return 0;
    }
    int testing_apply(int which, const double* in, double* out, int n_cols) override {
        if (!have_graph_data) return set_error(-3, "tsgo_testing_apply: no graph set");
        if (collective()) return set_error(-1, "tsgo_testing_apply: edge-sharded handles (world > 1) are not supported");
        if (which < 0 || which > 3 || n_cols < 0 || (n_cols > 0 && (!in || !out))) return set_error(-1, "tsgo_testing_apply: bad argument");
        if (which == 1 && !amg_on) return set_error(-1, "tsgo_testing_apply: a block-Jacobi handle has no in-cycle product");
        if (which == 3 && (!amg_on || sizeof(T) != 8)) return set_error(-1, "tsgo_testing_apply: the batched cycle needs a multigrid handle with precision = 64");
        if (which == 3 && n_cols > marginal_width()) return set_error(-1, "tsgo_testing_apply: more columns than the batch is wide");
        if (n_cols == 0) return 0;
        return mb_guarded([&] { return ta_run(which, in, out, n_cols); });
    }

    // ---- tsgo_testing_warm_start (include/tsgo_testing.h): what the warm start decides and writes, read out of the handle ----
    // a device vector of 3 per pose -> graph pose order, widened
    int tw_read(const std::vector<int>& of_graph, const T* dev, std::vector<T>& h3, double* out) {
        if (!out) return 0;
        if (int rc = copy_sync(h3.data(), dev, h3.size() * sizeof(T), hipMemcpyDeviceToHost)) return rc;
        for (int i = 0; i < pr.P; ++i) for (int k = 0; k < 3; ++k) out[3 * (size_t)of_graph[i] + k] = (double)h3[(size_t)i * 3 + k];
        return 0;
    }
    int tw_sum(const T* dev, int n, double* out) {
        std::vector<T> h((size_t)n);
        if (int rc = copy_sync(h.data(), dev, h.size() * sizeof(T), hipMemcpyDeviceToHost)) return rc;
        double s = 0;
        for (int k = 0; k < n; ++k) s += (double)h[(size_t)k];
        *out = s;
        return 0;
    }
    int tw_run(int n_plant, const double* plant, int fused, tsgo_testing_warm_out* out) {
        const int P = pr.P;
        const std::vector<int> of_graph = ta_of_graph();
        std::vector<T> h3((size_t)P * 3);
        if (n_plant > 0) {      // forget, then record every delta as the loops do (the linearisation below comes after, as in a Gauss-Newton step)
            mem.have_prev = false; mem.n_prev = 0; mem.n_tested = 0; mem.carried = false;
            for (int d = 0; d < n_plant; ++d) {
                const double* in = plant + (size_t)d * 3 * P;
                for (int i = 0; i < P; ++i) for (int k = 0; k < 3; ++k) h3[(size_t)i * 3 + k] = (T)in[3 * (size_t)of_graph[i] + k];
                if (int rc = copy_sync(x, h3.data(), h3.size() * sizeof(T), hipMemcpyHostToDevice)) return rc;
                record_delta(fused != 0, T(0));
            }
        }
        if (int rc = mb_prepare()) return rc;
        const bool warmed = cfg.warm_start && mem.have_prev && step_scale() < 1.0;      // do_solve's test
        int n_max = 0, n_tested = 0;
        warm_orders(n_max, n_tested);
        out->warmed = warmed ? 1 : 0; out->n_prev = mem.n_prev; out->n_tested = n_tested; out->n_max = n_max; out->carried = mem.carried ? 1 : 0;
        if (int rc = tw_read(of_graph, r, h3, out->b)) return rc;
        if (!warmed) return 0;
        if (int rc = tw_sum(gpart[0], nbC, &out->bdb)) return rc;      // (block-Jacobi: k_warm_scale overwrites these partials with r0's)
        if (int rc = launch_warm()) return rc;
        if (int rc = copy_sync(&out->order, warm_order_dev, sizeof(int), hipMemcpyDeviceToHost)) return rc;
        if (amg_on) {
            CgState<T> hs;
            if (int rc = copy_sync(&hs, st[0], sizeof(hs), hipMemcpyDeviceToHost)) return rc;
            out->done = hs.done;
        }
        for (int m = 0; m < n_tested; ++m) { if (int rc = tw_sum(warm_err + (size_t)m * nbC, nbC, &out->err[m])) return rc; }
        T gs = 0;
        if (int rc = copy_sync(&gs, gscale_dev, sizeof(T), hipMemcpyDeviceToHost)) return rc;
        out->scale = (double)gs;
        if (int rc = tw_sum(npart, nbC, &out->rdr)) return rc;
        if (out->hist) for (int j = 0; j < mem.n_prev; ++j) { if (int rc = tw_read(of_graph, hist[j], h3, out->hist + (size_t)j * 3 * P)) return rc; }
        if (int rc = tw_read(of_graph, x, h3, out->x0)) return rc;
        return tw_read(of_graph, r, h3, out->r0);
    }
    int testing_warm_start(int n_plant, const double* plant, int fused, tsgo_testing_warm_out* out) override {
        if (collective() || cfg.world > 1) return set_error(-1, "tsgo_testing_warm_start: edge-sharded handles (world > 1) are not supported");
        if (!have_graph_data) return set_error(-3, "tsgo_testing_warm_start: no graph set");
        if (!out || n_plant < 0 || n_plant > 12 || (n_plant > 0 && !plant) || (fused != 0 && fused != 1)) return set_error(-1, "tsgo_testing_warm_start: bad argument");
        out->warmed = out->n_prev = out->n_tested = out->n_max = out->order = out->done = out->carried = 0;
        for (double& e : out->err) e = 0;
        out->scale = out->bdb = out->rdr = 0;
        // mb_guarded restores the device; the host's side of the history is put back here: the counters and which buffer is the newest
        const SolverMemory mem0 = mem;
        T* hist0[kMaxWarm];
        std::copy(hist, hist + kMaxWarm, hist0);
        const int rc = mb_guarded([&] { return tw_run(n_plant, plant, fused, out); });
        mem = mem0;
        std::copy(hist0, hist0 + kMaxWarm, hist);
        return rc;
    }
