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
// The edge -> slot map (two words per input edge and the edge's class as a byte, tsgo_edit_kernels.h) is built from SellTable::edge and
// Problem::prior_p_edge / prior_l_edge at the first call on a structure and lives where the report maps live: bump-allocated behind what
// the graph owns, kept by a refill, dropped where set_graph releases the slabs (drop_edit_maps beside drop_report_maps).  With it comes
// one device buffer of 32 B per edge that receives a call's list and values in ONE transfer from the pinned staging buffer (the dense
// form fills 24 B per edge of it) and holds the read-out of the get call.  A handle that never edits pays nothing.
    uint32_t* edit_map = nullptr;              // [2 E]
    uint8_t* edit_cls = nullptr;               // [E]
    char* edit_buf = nullptr;                  // [32 E] bytes: (3 n doubles | n int64) of a set call; 3 E doubles of a get call
    std::vector<uint32_t> edit_map_h;          // the map on the host: which prior record an edited pose prior is
    std::vector<uint32_t> edit_stamp;          // [E] the call that last listed the edge (duplicate check in O(n))
    uint32_t edit_call = 0;
    bool edit_ready = false;
    void drop_edit_maps() { edit_map = nullptr; edit_cls = nullptr; edit_buf = nullptr; edit_map_h.clear(); edit_stamp.clear(); edit_call = 0; edit_ready = false; }

    static int edit_axes(uint32_t type) { return type == kClassOdom || type == kClassPosePrior ? 3 : 2; }      // entries of e_inf the class uses
    EditTables<T> edit_tables() { return EditTables<T>{st_p, tp.slots, st_l, tl.slots, st_o, to.slots, pri_p, pri_l}; }

    int edit_prepare(const std::string& nm) {
        if (edit_ready) return 0;
        // what the kernels rely on, checked once per structure: every input edge has exactly the locations its class requires, inside
        // their tables, and no location belongs to two edges (a slot names one edge; an edge takes each of its words once)
        const size_t E = structure.e_type.size();
        const std::vector<uint32_t>& type = structure.e_type;
        std::vector<uint32_t> m(2 * E, kNoEdge), owner(2 * E, kNoEdge);      // owner: the pose a pose-pose slot belongs to
        bool ok = pr.by_pose.slots() < kNoEdge && pr.by_lm.slots() < kNoEdge && pr.odom.slots() < kNoEdge;
        auto take = [&](uint32_t e, int word, size_t at, bool right_class) {
            if (e >= E || !right_class || m[2 * (size_t)e + word] != kNoEdge) { ok = false; return false; }
            m[2 * (size_t)e + word] = (uint32_t)at;
            return true;
        };
        for (size_t k = 0; ok && k < pr.by_pose.edge.size(); ++k) { const uint32_t e = pr.by_pose.edge[k]; if (e != kNoEdge) take(e, 0, k, e < E && type[e] == kClassLm); }
        for (size_t k = 0; ok && k < pr.by_lm.edge.size(); ++k) { const uint32_t e = pr.by_lm.edge[k]; if (e != kNoEdge) take(e, 1, k, e < E && type[e] == kClassLm); }
        const int vps = kWave / std::max(1, pr.odom.G);
        for (int s = 0; ok && s < pr.odom.n_slices; ++s)
            for (size_t row = pr.odom.row_off[(size_t)s]; row < pr.odom.row_off[(size_t)s + 1]; ++row)
                for (int lane = 0; lane < kWave; ++lane) {
                    const size_t k = row * kWave + (size_t)lane;
                    const uint32_t e = pr.odom.edge[k], ix = pr.odom.idx[k];
                    if (e == kNoEdge) continue;
                    const int side = (ix & kDirBit) ? 1 : 0;
                    if (take(e, side, k, e < E && type[e] == ((ix & kVlmBit) ? (uint32_t)kClassVlm : (uint32_t)kClassOdom)))
                        owner[2 * (size_t)e + side] = (uint32_t)(s * vps + lane / pr.odom.G);
                }
        for (size_t k = 0; ok && k < pr.prior_p_edge.size(); ++k) { const uint32_t e = pr.prior_p_edge[k]; take(e, 0, k, e < E && type[e] == kClassPosePrior); }
        for (size_t k = 0; ok && k < pr.prior_l_edge.size(); ++k) { const uint32_t e = pr.prior_l_edge[k]; take(e, 0, k, e < E && type[e] == kClassLmPrior); }
        for (size_t e = 0; ok && e < E; ++e) {
            const uint32_t a = m[2 * e], b = m[2 * e + 1];
            if (type[e] >= (uint32_t)kEdgeClasses || a == kNoEdge) ok = false;
            else if (type[e] >= (uint32_t)kClassPosePrior) ok = b == kNoEdge;
            else if (b == kNoEdge) ok = false;
            // a pose-pose edge: each slot's neighbour is the pose the other slot belongs to (a self-loop: two slots of one pose)
            else if (type[e] != kClassLm) ok = a != b && (pr.odom.idx[a] & kPoseMask) == owner[2 * e + 1] && (pr.odom.idx[b] & kPoseMask) == owner[2 * e];
        }
        if (!ok) return set_error(-30, nm + ": the slot tables do not give every input edge exactly the locations of its type");
        std::vector<uint8_t> cls(E);
        for (size_t e = 0; e < E; ++e) cls[e] = (uint8_t)type[e];
        if (int rc = upload_u32m(&edit_map, m)) return rc;
        if (int rc = dalloc(&edit_cls, E)) return rc;
        if (E) { if (int rc = copy_sync(edit_cls, cls.data(), E, hipMemcpyHostToDevice)) return rc; }
        if (int rc = dalloc(&edit_buf, 32 * std::max<size_t>(E, 1))) return rc;
        edit_map_h.swap(m);
        edit_ready = true;
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
        const bool had_map = edit_ready;
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
        HIP_OK(hipMemcpyAsync(edit_buf, hs, bytes, hipMemcpyHostToDevice, stream));
        HIP_OK(hipEventRecord(ev[0], stream));
        launch(k_set_edge_inf<T>, (int)((n + kBlock - 1) / kBlock), (int)n, idx ? (const int64_t*)(edit_buf + bytes_val) : (const int64_t*)nullptr, (const double*)edit_buf,
               (const uint32_t*)edit_map, (const uint8_t*)edit_cls, edit_tables());
        HIP_OK(hipGetLastError());
        HIP_OK(hipEventRecord(ev[1], stream));
        HIP_OK(hipStreamSynchronize(stream));      // the staging buffer is free again; the tables hold the new weights
        { float ms = 0; HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1])); s.ms_device = ms; }
        // ---- host state that mirrors weights; the solver ----
        if (s.edges_by_class[kClassPosePrior] > 0)
            for (size_t i = 0; i < (size_t)n; ++i) {
                const size_t e = idx ? (size_t)idx[i] : i;
                if (type[e] != kClassPosePrior) continue;
                const size_t k = edit_map_h[2 * e];
                for (int m = 0; m < 3; ++m) pri_p_w[3 * k + m] = inf[3 * i + m];
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
        launch(k_get_edge_inf<T>, (int)((E + kBlock - 1) / kBlock), (int)E, (const uint32_t*)edit_map, (const uint8_t*)edit_cls, edit_tables(), reinterpret_cast<double*>(edit_buf));
        HIP_OK(hipGetLastError());
        return copy_sync(out, edit_buf, 24 * E, hipMemcpyDeviceToHost);
    }
