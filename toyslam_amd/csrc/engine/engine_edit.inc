// engine/engine_edit.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// tsgo_set_edge_information / tsgo_get_edge_information.  The information diagonal of listed edges is scattered, as (T)value, into every
// place the handle keeps it (tsgo_edit_kernels.h, DESIGN.md section 17): afterwards every table holds, bit for bit, what the refill of a
// same-structure tsgo_set_graph with those e_inf rows would hold, and nothing else on the device has been written — the estimates keep
// their bits.
//
// State: the rule of tsgo_set_robust.  The weights may move wholesale, so the next linearisation builds a fresh multigrid hierarchy
// (mem.hier_age = -1); the warm start's history and everything else the solver learnt stay, and a captured PCG hipGraph stays valid (it
// reads the planes through the same pointers).  Host state that mirrors weights follows: pri_p_w (has_full_pose_prior).
//
// The edge -> slot map (two words per input edge and the edge's class as a byte, tsgo_edit_kernels.h) is the structure index's EdgeSlots
// (host/structure_index.h), checked there; it goes to the device at the first call on a structure and lives where the report maps live
// (StructureMaps, tsgo_hip.hip): bump-allocated behind what the graph owns, kept by a refill, dropped where set_graph releases the slabs.
// With it comes one device buffer of 32 B per edge that receives a call's list and values in ONE transfer from the pinned staging buffer
// (the dense form fills 24 B per edge of it) and holds the read-out of the get call.  A handle that never edits pays nothing.
    std::vector<uint32_t> edit_stamp;          // [E] the call that last listed the edge (duplicate check in O(n))
    uint32_t edit_call = 0;

    static int edit_axes(uint32_t type) { return type == kClassOdom || type == kClassPosePrior ? 3 : 2; }      // entries of e_inf the class uses
    EditTables<T> edit_tables() { return EditTables<T>{st_p, tp.slots, st_l, tl.slots, st_o, to.slots, pri_p, pri_l}; }

    int edit_prepare(const std::string& nm) {
        if (maps.edit_ready) return 0;
        const EdgeSlots* es = edges(nm);
        if (!es) return -30;
        const size_t E = es->cls.size();
        if (int rc = upload_u32m(&maps.edit_map, es->loc)) return rc;
        if (int rc = dalloc(&maps.edit_cls, E)) return rc;
        if (E) { if (int rc = copy_sync(maps.edit_cls, es->cls.data(), E, hipMemcpyHostToDevice)) return rc; }
        if (int rc = dalloc(&maps.edit_buf, 32 * std::max<size_t>(E, 1))) return rc;
        maps.edit_ready = true;
        return 0;
    }

    int set_edge_information(int64_t n, const int64_t* idx, const double* inf, tsgo_edge_info_stats* st_out) override {
        const auto wall0 = std::chrono::steady_clock::now();
        auto ms_since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count(); };
        const std::string nm = "tsgo_set_edge_information";
        if (cfg.world > 1 || collective()) return set_error(-1, nm + ": edge-sharded handles (world > 1) are not supported");
        if (!have_graph_data) return set_error(-3, nm + ": no graph set");
        if (n < 0) return set_error(-1, nm + ": n = " + std::to_string(n) + " is negative");
        tsgo_edge_info_stats s; std::memset(&s, 0, sizeof(s));
        if (n == 0) { s.ms_total = ms_since(); if (st_out) *st_out = s; return 0; }
        const size_t E = structure.e_type.size();
        if (!inf) return set_error(-1, nm + ": e_inf is NULL with n = " + std::to_string(n));
        if (!idx && n != (int64_t)E) return set_error(-1, nm + ": edge_idx is NULL (all edges in order) but n = " + std::to_string(n) + " and the graph has " + std::to_string(E) + " edges");
        // ---- everything is validated before anything is staged, uploaded or launched ----
        const std::vector<uint32_t>& type = structure.e_type;
        auto bad_value = [&](size_t i, size_t e) -> int {      // the first used axis of listed edge i that is not finite or is negative, -1 when none
            for (int m = 0; m < edit_axes(type[e]); ++m) { const double v = inf[3 * i + m]; if (!(std::isfinite(v) && v >= 0)) return m; }
            return -1;
        };
        auto value_error = [&](size_t i, size_t e, int m) {
            return set_error(-2, nm + ": e_inf[" + std::to_string(3 * i + m) + "] = " + std::to_string(inf[3 * i + m]) + " (edge " + std::to_string(e) + ", type " + std::to_string(type[e]) +
                                     ") must be finite and >= 0");
        };
        if (idx) {
            if (n > (int64_t)E) return set_error(-1, nm + ": " + std::to_string(n) + " edges listed but the graph has " + std::to_string(E) + ": an index is listed twice");
            if (edit_stamp.size() != E || edit_call == 0xFFFFFFFFu) { edit_stamp.assign(E, 0u); edit_call = 0; }
            ++edit_call;
            for (size_t i = 0; i < (size_t)n; ++i) {
                const int64_t e = idx[i];
                if (e < 0 || e >= (int64_t)E) return set_error(-1, nm + ": edge_idx[" + std::to_string(i) + "] = " + std::to_string(e) + " is outside [0, " + std::to_string(E) + ")");
                if (edit_stamp[(size_t)e] == edit_call) return set_error(-1, nm + ": edge " + std::to_string(e) + " is listed twice (edge_idx[" + std::to_string(i) + "])");
                edit_stamp[(size_t)e] = edit_call;
                if (const int m = bad_value(i, (size_t)e); m >= 0) return value_error(i, (size_t)e, m);
                ++s.edges_by_class[type[(size_t)e]];
            }
        } else {
            int64_t cnt[kMaxHostThreads][kEdgeClasses] = {};
            std::atomic<int64_t> first_bad{INT64_MAX};
            parallel_chunks((int)n, [&](int c, int b, int e_end) {
                for (int e = b; e < e_end; ++e) {
                    if (bad_value((size_t)e, (size_t)e) >= 0) { int64_t seen = first_bad.load(); while (e < seen && !first_bad.compare_exchange_weak(seen, e)) {} }
                    ++cnt[c][type[(size_t)e]];
                }
            }, 65536);
            if (first_bad.load() != INT64_MAX) { const size_t e = (size_t)first_bad.load(); return value_error(e, e, bad_value(e, e)); }
            for (int c = 0; c < kMaxHostThreads; ++c) for (int k = 0; k < kEdgeClasses; ++k) s.edges_by_class[k] += cnt[c][k];
        }
        s.edges_listed = n;
        HIP_OK(hipSetDevice(cfg.device));
        const bool had_map = maps.edit_ready;
        if (int rc = edit_prepare(nm)) return rc;
        s.maps_built = had_map ? 0 : 1;
        // ---- values, then the list, into pinned staging; one transfer ----
        const size_t bytes_val = 24 * (size_t)n, bytes = bytes_val + (idx ? 8 * (size_t)n : 0);
        if (int rc = stage_reserve((bytes + sizeof(T) - 1) / sizeof(T))) return rc;
        char* hs = reinterpret_cast<char*>(stage);
        parallel_chunks((int)n, [&](int, int b, int e) {
            std::memcpy(hs + 24 * (size_t)b, inf + 3 * (size_t)b, 24 * (size_t)(e - b));
            if (idx) std::memcpy(hs + bytes_val + 8 * (size_t)b, idx + b, 8 * (size_t)(e - b));
        }, 65536);
        s.ms_host = ms_since();
        HIP_OK(hipMemcpyAsync(maps.edit_buf, hs, bytes, hipMemcpyHostToDevice, stream));
        HIP_OK(hipEventRecord(ev[0], stream));
        launch(k_set_edge_inf<T>, (int)((n + kBlock - 1) / kBlock), (int)n, idx ? (const int64_t*)(maps.edit_buf + bytes_val) : (const int64_t*)nullptr, (const double*)maps.edit_buf,
               (const uint32_t*)maps.edit_map, (const uint8_t*)maps.edit_cls, edit_tables());
        HIP_OK(hipGetLastError());
        HIP_OK(hipEventRecord(ev[1], stream));
        HIP_OK(hipStreamSynchronize(stream));      // the staging buffer is free again; the tables hold the new weights
        { float ms = 0; HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1])); s.ms_device = ms; }
        // ---- host state that mirrors weights; the solver ----
        if (s.edges_by_class[kClassPosePrior] > 0) {
            const std::vector<uint32_t>& loc = edges(nm)->loc;      // built by edit_prepare at the latest
            for (size_t i = 0; i < (size_t)n; ++i) {
                const size_t e = idx ? (size_t)idx[i] : i;
                if (type[e] != kClassPosePrior) continue;
                const size_t k = loc[2 * e];      // which prior record the edited pose prior is
                for (int m = 0; m < 3; ++m) pri_p_w[3 * k + m] = inf[3 * i + m];
            }
        }
        mem.hier_age = -1;      // the weights may move wholesale: the next linearisation builds a fresh hierarchy
        s.ms_total = ms_since();
        if (st_out) *st_out = s;
        return 0;
    }

    int get_edge_information(double* out, int64_t cap_edges) override {
        const std::string nm = "tsgo_get_edge_information";
        if (cfg.world > 1 || collective()) return set_error(-1, nm + ": edge-sharded handles (world > 1) are not supported");
        if (!have_graph_data) return set_error(-3, nm + ": no graph set");
        const size_t E = structure.e_type.size();
        if (cap_edges < (int64_t)E) return set_error(-1, nm + ": cap_edges " + std::to_string(cap_edges) + " is below n_edges = " + std::to_string(E));
        if (E == 0) return 0;
        if (!out) return set_error(-1, nm + ": e_inf_out is NULL");
        HIP_OK(hipSetDevice(cfg.device));
        if (int rc = edit_prepare(nm)) return rc;
        launch(k_get_edge_inf<T>, (int)((E + kBlock - 1) / kBlock), (int)E, (const uint32_t*)maps.edit_map, (const uint8_t*)maps.edit_cls, edit_tables(), reinterpret_cast<double*>(maps.edit_buf));
        HIP_OK(hipGetLastError());
        return copy_sync(out, maps.edit_buf, 24 * E, hipMemcpyDeviceToHost);
    }
