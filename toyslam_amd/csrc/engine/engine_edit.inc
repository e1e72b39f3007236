// engine/engine_edit.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// tsgo_set_edge_information / tsgo_get_edge_information, and at the end of the file the vertex edits tsgo_set_fixed / tsgo_get_fixed /
// tsgo_set_estimates.  The information diagonal of listed edges is scattered, as (T)value, into every
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

// ---- tsgo_set_fixed / tsgo_get_fixed / tsgo_set_estimates: values of listed VERTICES, in place (DESIGN.md section 22) --------------------
// The fixed list on the device is two plain arrays, gauge_p and gauge_l: 1e6 * the vertex's multiplicity in the list, read at every launch
// by the linearisation, the landmark pass of tsgo_init_estimates and the sampling kernels.  tsgo_set_fixed scatters (T)(1e6 * k) into them
// (k_set_gauge) and nothing else; tsgo_set_estimates scatters pose records, thetas and landmark positions exactly as stage_values writes them
// (k_set_estimates).  The host resolves ids through the structure index (VertexIndex) and sends kind, internal number and value in ONE
// transfer from the pinned staging buffer into a buffer of 48 B per vertex that lives where the edit map lives (StructureMaps).
//
// Host readers of the fixed list see the edit: pr.gauge_p / pr.gauge_l (mb_anchored() in front of the marginals, the gate and the samples;
// tsgo_get_fixed) hold the new terms, and fixed_list() (the breadth-first sources of tsgo_init_estimates) the CANONICAL list: the vertices
// with count > 0 in tsgo_graph vertex order, each repeated count times.  structure.fixed stays what the last tsgo_set_graph carried: same_as
// compares against it, and a refill puts both gauge arrays and the mirrors back (restore_fixed) when an edit is outstanding.
//
// State.  tsgo_set_fixed: the rule of tsgo_set_edge_information (mem.hier_age = -1, everything else stays).  tsgo_set_estimates: the end of
// tsgo_init_estimates (host copy of the estimates current, restart_on_new_estimates, no warm-start history even under warm_requests).
    std::vector<uint32_t> fixed_edit;          // the canonical list while a tsgo_set_fixed is outstanding
    bool fixed_edited = false;
    const std::vector<uint32_t>& fixed_list() const { return fixed_edited ? fixed_edit : structure.fixed; }
    std::vector<uint32_t> vedit_stamp;         // [V] the call that last listed the vertex (duplicate check in O(n))
    uint32_t vedit_call = 0;
    static int32_t gauge_count(double g) { return (int32_t)std::llround(g / kGaugeTerm); }      // 1e6 * k is exact in f64 for every k the call accepts
    int64_t fixed_vertices() const {
        int64_t k = 0;
        for (double g : pr.gauge_p) k += g > 0;
        for (double g : pr.gauge_l) k += g > 0;
        return k;
    }

    int vedit_prepare() {
        if (maps.vedit_ready) return 0;
        if (int rc = dalloc(&maps.vedit_buf, 48 * std::max<size_t>(structure.v_id.size(), 1))) return rc;
        maps.vedit_ready = true;
        return 0;
    }
    // what all three calls check first
    int vedit_enter(const std::string& nm, int64_t n) {
        if (cfg.world > 1 || collective()) return set_error(-1, nm + ": edge-sharded handles (world > 1) are not supported");
        if (!have_graph_data) return set_error(-3, nm + ": no graph set");
        if (n < 0) return set_error(-1, nm + ": n = " + std::to_string(n) + " is negative");
        return 0;
    }
    // ids -> (kind, internal number) per listed vertex; refuses an unknown id and an id listed twice.  Counts poses and landmarks.
    int vedit_resolve(const std::string& nm, int64_t n, const uint32_t* ids, std::vector<MbQuery>& at, tsgo_vertex_edit_stats& s) {
        const size_t V = structure.v_id.size();
        if (n > (int64_t)V) return set_error(-1, nm + ": " + std::to_string(n) + " vertices listed but the graph has " + std::to_string(V) + ": an id is listed twice");
        const VertexIndex& vi = vertices();
        if (vedit_stamp.size() != V || vedit_call == 0xFFFFFFFFu) { vedit_stamp.assign(V, 0u); vedit_call = 0; }
        ++vedit_call;
        at.resize((size_t)n);
        for (size_t i = 0; i < (size_t)n; ++i) {
            const int v = vi.ids.find(ids[i]);
            if (v < 0 || vi.of[(size_t)v].kind < 0) return set_error(-1, nm + ": unknown vertex id " + std::to_string(ids[i]) + " (ids[" + std::to_string(i) + "])");
            if (vedit_stamp[(size_t)v] == vedit_call) return set_error(-1, nm + ": vertex id " + std::to_string(ids[i]) + " is listed twice (ids[" + std::to_string(i) + "])");
            vedit_stamp[(size_t)v] = vedit_call;
            const MbQuery q = vi.of[(size_t)v];
            // what the kernels rely on: the number is inside its array
            if (q.idx < 0 || q.idx >= (q.kind == 0 ? pr.P : pr.L)) return set_error(-30, nm + ": the structure index places vertex id " + std::to_string(ids[i]) + " outside its table");
            at[i] = q;
            ++(q.kind == 0 ? s.poses : s.landmarks);
        }
        s.listed = n;
        return 0;
    }

    int set_fixed(int64_t n, const uint32_t* ids, const int32_t* count, tsgo_vertex_edit_stats* st_out) override {
        const auto wall0 = std::chrono::steady_clock::now();
        auto ms_since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count(); };
        const std::string nm = "tsgo_set_fixed";
        if (int rc = vedit_enter(nm, n)) return rc;
        tsgo_vertex_edit_stats s; std::memset(&s, 0, sizeof(s));
        if (n == 0) { s.fixed_now = fixed_vertices(); s.ms_total = ms_since(); if (st_out) *st_out = s; return 0; }
        if (!ids) return set_error(-1, nm + ": ids is NULL with n = " + std::to_string(n));
        // ---- everything is validated before anything is staged, uploaded or launched ----
        std::vector<MbQuery> at;
        if (int rc = vedit_resolve(nm, n, ids, at, s)) return rc;
        if (count) for (size_t i = 0; i < (size_t)n; ++i)
            if (count[i] < 0 || count[i] > 65535)
                return set_error(-1, nm + ": count[" + std::to_string(i) + "] = " + std::to_string(count[i]) + " (vertex id " + std::to_string(ids[i]) + ") is outside [0, 65535]");
        HIP_OK(hipSetDevice(cfg.device));
        if (int rc = vedit_prepare()) return rc;
        // ---- the terms, then (kind, number), into pinned staging; one transfer ----
        const size_t bytes_val = 8 * (size_t)n, bytes = bytes_val + 8 * (size_t)n;
        if (int rc = stage_reserve((bytes + sizeof(T) - 1) / sizeof(T))) return rc;
        char* hs = reinterpret_cast<char*>(stage);
        double* hv = reinterpret_cast<double*>(hs); uint32_t* hr = reinterpret_cast<uint32_t*>(hs + bytes_val);
        for (size_t i = 0; i < (size_t)n; ++i) {
            hv[i] = kGaugeTerm * (double)(count ? count[i] : 1);
            hr[2 * i] = at[i].kind == 0 ? kEditPose : kEditLm; hr[2 * i + 1] = (uint32_t)at[i].idx;
        }
        s.ms_host = ms_since();
        HIP_OK(hipMemcpyAsync(maps.vedit_buf, hs, bytes, hipMemcpyHostToDevice, stream));
        HIP_OK(hipEventRecord(ev[0], stream));
        launch(k_set_gauge<T>, (int)((n + kBlock - 1) / kBlock), (int)n, (const uint2*)(maps.vedit_buf + bytes_val), (const double*)maps.vedit_buf, gauge_p, pr.P, gauge_l, pr.L);
        HIP_OK(hipGetLastError());
        HIP_OK(hipEventRecord(ev[1], stream));
        HIP_OK(hipStreamSynchronize(stream));      // the staging buffer is free again; the gauge arrays hold the new terms
        { float ms = 0; HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1])); s.ms_device = ms; }
        // ---- the host mirrors, the canonical list; the solver ----
        for (size_t i = 0; i < (size_t)n; ++i) {
            double& g = (at[i].kind == 0 ? pr.gauge_p : pr.gauge_l)[(size_t)at[i].idx];
            s.released += g > 0 && hv[i] == 0;
            g = hv[i];
        }
        const VertexIndex& vi = vertices();
        fixed_edit.clear();
        for (size_t v = 0; v < structure.v_id.size(); ++v) {
            const MbQuery q = vi.of[v];
            if (q.kind < 0) continue;
            const int32_t k = gauge_count((q.kind == 0 ? pr.gauge_p : pr.gauge_l)[(size_t)q.idx]);
            fixed_edit.insert(fixed_edit.end(), (size_t)k, structure.v_id[v]);
            s.fixed_now += k > 0;
        }
        fixed_edited = true;
        mem.hier_age = -1;      // the level-0 diagonal moves by 1e6 per occurrence: the next linearisation builds a fresh hierarchy
        s.ms_total = ms_since();
        if (st_out) *st_out = s;
        return 0;
    }

    int get_fixed(int32_t* out, int64_t cap_vertices) override {
        const std::string nm = "tsgo_get_fixed";
        if (int rc = vedit_enter(nm, 0)) return rc;
        const size_t V = structure.v_id.size();
        if (cap_vertices < (int64_t)V) return set_error(-1, nm + ": cap_vertices " + std::to_string(cap_vertices) + " is below n_vertices = " + std::to_string(V));
        if (V == 0) return 0;
        if (!out) return set_error(-1, nm + ": count_out is NULL");
        const VertexIndex& vi = vertices();
        for (size_t v = 0; v < V; ++v) {
            const MbQuery q = vi.of[v];
            out[v] = q.kind < 0 ? 0 : gauge_count((q.kind == 0 ? pr.gauge_p : pr.gauge_l)[(size_t)q.idx]);
        }
        return 0;
    }

    // A refill while a tsgo_set_fixed is outstanding: the gauge arrays and their mirrors back to the list of the last tsgo_set_graph (which
    // the request repeats: same_as compared it), as build_problem made them.
    int restore_fixed() {
        if (!fixed_edited) return 0;
        const VertexIndex& vi = vertices();
        std::fill(pr.gauge_p.begin(), pr.gauge_p.end(), 0.0); std::fill(pr.gauge_l.begin(), pr.gauge_l.end(), 0.0);
        for (uint32_t id : structure.fixed) {
            const int v = vi.ids.find(id);
            if (v < 0 || vi.of[(size_t)v].kind < 0) continue;
            const MbQuery q = vi.of[(size_t)v];
            (q.kind == 0 ? pr.gauge_p : pr.gauge_l)[(size_t)q.idx] += kGaugeTerm;
        }
        std::vector<T> tmp;
        auto put = [&](T* dst, const std::vector<double>& src) -> int {
            if (src.empty()) return 0;
            tmp.resize(src.size());
            for (size_t k = 0; k < src.size(); ++k) tmp[k] = (T)src[k];
            return copy_sync(dst, tmp.data(), tmp.size() * sizeof(T), hipMemcpyHostToDevice);
        };
        if (int rc = put(gauge_p, pr.gauge_p)) return rc;
        if (int rc = put(gauge_l, pr.gauge_l)) return rc;
        fixed_edited = false; fixed_edit.clear();
        return 0;
    }

    int set_estimates(int64_t n, const uint32_t* ids, const double* v_pos, tsgo_vertex_edit_stats* st_out) override {
        const auto wall0 = std::chrono::steady_clock::now();
        auto ms_since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count(); };
        const std::string nm = "tsgo_set_estimates";
        if (int rc = vedit_enter(nm, n)) return rc;
        tsgo_vertex_edit_stats s; std::memset(&s, 0, sizeof(s));
        const size_t V = structure.v_id.size();
        const size_t P = (size_t)pr.P, L = (size_t)pr.L;
        if (!ids && n != (int64_t)V) return set_error(-1, nm + ": ids is NULL (all vertices in order) but n = " + std::to_string(n) + " and the graph has " + std::to_string(V) + " vertices");
        if (n == 0) { s.fixed_now = fixed_vertices(); s.ms_total = ms_since(); if (st_out) *st_out = s; return 0; }
        if (!v_pos) return set_error(-1, nm + ": v_pos is NULL with n = " + std::to_string(n));
        // ---- everything is validated before anything is staged, uploaded or launched ----
        std::vector<MbQuery> at;
        const VertexIndex& vi = vertices();
        if (ids) { if (int rc = vedit_resolve(nm, n, ids, at, s)) return rc; }
        else {
            if (P + L != V) return set_error(-30, nm + ": the tables hold " + std::to_string(P + L) + " of the graph's " + std::to_string(V) + " vertices");
            s.listed = n; s.poses = (int64_t)P; s.landmarks = (int64_t)L;
        }
        for (size_t i = 0; i < (size_t)n; ++i) {
            const int axes = (ids ? at[i].kind : vi.of[i].kind) == 0 ? 3 : 2;
            for (int m = 0; m < axes; ++m)
                if (!std::isfinite(v_pos[3 * i + m]))
                    return set_error(-2, nm + ": v_pos[" + std::to_string(3 * i + m) + "] = " + std::to_string(v_pos[3 * i + m]) + " (vertex id " +
                                             std::to_string(ids ? ids[i] : structure.v_id[i]) + ") must be finite");
        }
        HIP_OK(hipSetDevice(cfg.device));
        if (int rc = vedit_prepare()) return rc;
        // ---- five numbers per vertex, then (kind, number) of a list, into pinned staging; one transfer.  The dense form goes in the
        // internal numbering, poses first, and needs no list ----
        const size_t bytes_val = 40 * (size_t)n, bytes = bytes_val + (ids ? 8 * (size_t)n : 0);
        if (int rc = stage_reserve((bytes + sizeof(T) - 1) / sizeof(T))) return rc;
        char* hs = reinterpret_cast<char*>(stage);
        double* hv = reinterpret_cast<double*>(hs); uint32_t* hr = reinterpret_cast<uint32_t*>(hs + bytes_val);
        auto five = [](const double* v, bool pose, double* o) {
            o[0] = v[0]; o[1] = v[1]; o[2] = pose ? std::cos(v[2]) : 0.0; o[3] = pose ? std::sin(v[2]) : 0.0; o[4] = pose ? v[2] : 0.0;
        };
        if (ids) {
            for (size_t i = 0; i < (size_t)n; ++i) {
                five(v_pos + 3 * i, at[i].kind == 0, hv + 5 * i);
                hr[2 * i] = at[i].kind == 0 ? kEditPose : kEditLm; hr[2 * i + 1] = (uint32_t)at[i].idx;
            }
        } else {
            parallel_chunks((int)n, [&](int, int b, int e) {
                for (size_t i = (size_t)b; i < (size_t)e; ++i) five(v_pos + 3 * (size_t)(i < P ? pr.pose_vertex[i] : pr.lm_vertex[i - P]), i < P, hv + 5 * i);
            }, 4096);
        }
        s.ms_host = ms_since();
        HIP_OK(hipMemcpyAsync(maps.vedit_buf, hs, bytes, hipMemcpyHostToDevice, stream));
        HIP_OK(hipEventRecord(ev[0], stream));
        launch(k_set_estimates<T>, (int)((n + kBlock - 1) / kBlock), (int)n, ids ? (const uint2*)(maps.vedit_buf + bytes_val) : (const uint2*)nullptr, (const double*)maps.vedit_buf,
               ps, theta, pr.P, lmrec, pr.L);
        HIP_OK(hipGetLastError());
        HIP_OK(hipEventRecord(ev[1], stream));
        // ---- what the host keeps of the estimates: every vertex current.  A list leaves the others where the device has them ----
        std::vector<T> hp, hl;
        if (ids) {
            hp.resize(P * 5); hl.resize(L * kLmRec);
            HIP_OK(hipMemcpyAsync(hp.data(), ps, P * 4 * sizeof(T), hipMemcpyDeviceToHost, stream));
            HIP_OK(hipMemcpyAsync(hp.data() + P * 4, theta, P * sizeof(T), hipMemcpyDeviceToHost, stream));
            if (L) HIP_OK(hipMemcpyAsync(hl.data(), lmrec, hl.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
        }
        HIP_OK(hipStreamSynchronize(stream));      // the staging buffer is free again
        { float ms = 0; HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1])); s.ms_device = ms; }
        if (ids) {
            for (size_t i = 0; i < P; ++i) { pr.pose_xyt[3 * i] = (double)hp[4 * i]; pr.pose_xyt[3 * i + 1] = (double)hp[4 * i + 1]; pr.pose_xyt[3 * i + 2] = (double)hp[4 * P + i]; }
            for (size_t l = 0; l < L; ++l) { pr.lm_xy[2 * l] = (double)hl[l * kLmRec]; pr.lm_xy[2 * l + 1] = (double)hl[l * kLmRec + 1]; }
            for (size_t i = 0; i < (size_t)n; ++i) {      // the listed ones as a tsgo_set_graph would keep them: the caller's f64 values
                const double* v = v_pos + 3 * i; const size_t k = (size_t)at[i].idx;
                if (at[i].kind == 0) { pr.pose_xyt[3 * k] = v[0]; pr.pose_xyt[3 * k + 1] = v[1]; pr.pose_xyt[3 * k + 2] = v[2]; }
                else { pr.lm_xy[2 * k] = v[0]; pr.lm_xy[2 * k + 1] = v[1]; }
            }
        } else {
            for (size_t i = 0; i < P; ++i) { const double* v = v_pos + 3 * (size_t)pr.pose_vertex[i]; pr.pose_xyt[3 * i] = v[0]; pr.pose_xyt[3 * i + 1] = v[1]; pr.pose_xyt[3 * i + 2] = v[2]; }
            for (size_t l = 0; l < L; ++l) { const double* v = v_pos + 3 * (size_t)pr.lm_vertex[l]; pr.lm_xy[2 * l] = v[0]; pr.lm_xy[2 * l + 1] = v[1]; }
        }
        if (int rc = restart_on_new_estimates()) { have_graph_data = false; return rc; }
        mem.carried = false; carry.n = 0;
        HIP_OK(hipStreamSynchronize(stream));
        s.fixed_now = fixed_vertices();
        s.ms_total = ms_since();
        if (st_out) *st_out = s;
        return 0;
    }
