// engine/engine_edge_robust.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// tsgo_set_edge_robust / tsgo_get_edge_robust.  A palette of at most kEdgeRobustMax robust kernels and one byte per input edge: 0 leaves
// the edge to its class (tsgo_set_robust), k >= 1 gives it palette entry k - 1 whatever its class (DESIGN.md section 21).
//
// While any edge has a non-zero entry the handle launches the RK = 2 instantiations of the kernels that robustify (rk(),
// engine_launch.inc); cleared, or with an all-zero mask, it launches exactly what it launched before: RK = 0 or 1.
//
// Device side (RobustArgs, tsgo_kernels.h): the palette as a small table, one byte per SLOT of the three tables and per prior RECORD for
// the kernels that walk tables without slot -> edge maps (k_lin_lm, k_lin_pose, k_chi2, k_chi2_lm_prior), and the caller's byte per EDGE
// for the readers that hold the edge index (report, g'Hg, sampling).  The slot arrays are made here from the slot -> edge lists the
// host layout keeps for every graph (SellTable::edge, Problem::prior_*_edge); padding gets 0.  The buffers are allocated at the first call
// on a structure and live where the report maps live (StructureMaps, tsgo_hip.hip): kept by a refill, dropped where set_graph releases
// the slabs; a call rewrites them.  A handle that never calls pays nothing.
//
// Lifetime of the SETTING: that of an edge-information edit — the next tsgo_set_graph, refill or rebuild, drops it (drop_edge_robust),
// so a reused handle keeps doing what a fresh one does; tsgo_set_robust, tsgo_set_edge_information, tsgo_init_estimates, tsgo_gnc and
// tsgo_optimize keep it.  State: the rule of tsgo_set_robust (a call that changes anything: mem.hier_age = -1, the history stays).
    struct EdgeRobust {
        bool active = false;                       // some edge has a non-zero entry: rk() == 2
        int n_entries = 0;
        tsgo_edge_robust_entry entries[TSGO_EDGE_ROBUST_MAX] = {};
        std::vector<uint8_t> of_edge;              // [E] while active
    } er;
    void drop_edge_robust() { er = EdgeRobust(); }

    int edge_robust_prepare() {
        if (maps.er_ready) return 0;
        if (int rc = dalloc(&maps.er_lm, pr.by_lm.edge.size())) return rc;
        if (int rc = dalloc(&maps.er_pose, pr.by_pose.edge.size())) return rc;
        if (int rc = dalloc(&maps.er_od, pr.odom.edge.size())) return rc;
        if (int rc = dalloc(&maps.er_pp, pr.prior_p_edge.size())) return rc;
        if (int rc = dalloc(&maps.er_pl, pr.prior_l_edge.size())) return rc;
        if (int rc = dalloc(&maps.er_edge, structure.e_type.size())) return rc;
        if (int rc = dalloc(&maps.er_pal, (size_t)kEdgeRobustMax)) return rc;
        maps.er_ready = true;
        return 0;
    }
    static bool same_entry(const tsgo_edge_robust_entry& a, const tsgo_edge_robust_entry& b) {
        return a.kernel == b.kernel && (a.kernel == TSGO_ROBUST_NONE || a.delta == b.delta);      // NONE ignores its width
    }

    int set_edge_robust(int32_t n_entries, const tsgo_edge_robust_entry* entries, const uint8_t* of_edge, int64_t n_mask, tsgo_edge_robust_stats* st_out) override {
        const auto wall0 = std::chrono::steady_clock::now();
        const std::string nm = "tsgo_set_edge_robust";
        // ---- everything is validated before anything changes ----
        if (sizeof(T) != 8) return set_error(-1, nm + ": needs precision = 64");
        if (cfg.world > 1 || collective()) return set_error(-1, nm + ": edge-sharded handles (world > 1) are not supported");
        if (!have_graph_data) return set_error(-3, nm + ": no graph set");
        const size_t E = structure.e_type.size();
        if (n_entries < 0 || n_entries > TSGO_EDGE_ROBUST_MAX)
            return set_error(-1, nm + ": n_entries = " + std::to_string(n_entries) + " is outside [0, " + std::to_string(TSGO_EDGE_ROBUST_MAX) + "]");
        tsgo_edge_robust_stats s; std::memset(&s, 0, sizeof(s));
        const bool clear = n_entries == 0 && !of_edge && n_mask == 0;
        if (!clear) {
            if (n_mask != (int64_t)E) return set_error(-1, nm + ": n_mask = " + std::to_string(n_mask) + " but the graph has n_edges = " + std::to_string(E));
            if (n_entries > 0 && !entries) return set_error(-1, nm + ": entries is NULL with n_entries = " + std::to_string(n_entries));
            if (E > 0 && !of_edge) return set_error(-1, nm + ": entry_of_edge is NULL with n_mask = " + std::to_string(n_mask));
            for (int k = 0; k < n_entries; ++k) {
                if (entries[k].kernel < 0 || entries[k].kernel >= kRobustKinds)
                    return set_error(-1, nm + ": entries[" + std::to_string(k) + "].kernel = " + std::to_string(entries[k].kernel) + " is not a robust kernel id");
                if (entries[k].kernel != TSGO_ROBUST_NONE && !(std::isfinite(entries[k].delta) && entries[k].delta >= 1e-6 && entries[k].delta <= 1e6))
                    return set_error(-1, nm + ": entries[" + std::to_string(k) + "].delta must be finite and within [1e-6, 1e6]");
            }
            for (size_t e = 0; e < E; ++e) {
                if (of_edge[e] > n_entries)
                    return set_error(-1, nm + ": entry_of_edge[" + std::to_string(e) + "] = " + std::to_string((int)of_edge[e]) + " is above n_entries = " + std::to_string(n_entries));
                ++s.edges_by_entry[of_edge[e]];
                if (of_edge[e]) ++s.overridden_by_class[structure.e_type[e]];
            }
        } else s.edges_by_entry[0] = (int64_t)E;
        const bool active = s.edges_by_entry[0] != (int64_t)E;
        // ---- what the call changes ----
        bool changed = active != er.active;
        if (active && er.active) {
            changed = std::memcmp(er.of_edge.data(), of_edge, E) != 0;
            for (size_t e = 0; !changed && e < E; ++e)      // entries count through the edges that use them
                if (of_edge[e] && !same_entry(er.entries[er.of_edge[e] - 1], entries[of_edge[e] - 1])) changed = true;
        }
        if (active) {
            HIP_OK(hipSetDevice(cfg.device));
            if (!edges(nm)) return -30;      // every slot and record names an input edge below E (host/structure_index.h): what slot_bytes indexes by
            if (int rc = edge_robust_prepare()) return rc;
            auto slot_bytes = [&](const std::vector<uint32_t>& edge, uint8_t* dst) -> int {
                if (edge.empty()) return 0;
                std::vector<uint8_t> b(edge.size());
                for (size_t k = 0; k < edge.size(); ++k) b[k] = edge[k] == kNoEdge ? (uint8_t)0 : of_edge[edge[k]];      // padding: 0
                return copy_sync(dst, b.data(), b.size(), hipMemcpyHostToDevice);
            };
            RobustEntry<T> pal[kEdgeRobustMax] = {};
            for (int k = 0; k < n_entries; ++k) { pal[k].kind = entries[k].kernel; pal[k].delta = (T)entries[k].delta; }
            auto upload = [&]() -> int {
                if (int rc = slot_bytes(pr.by_lm.edge, maps.er_lm)) return rc;
                if (int rc = slot_bytes(pr.by_pose.edge, maps.er_pose)) return rc;
                if (int rc = slot_bytes(pr.odom.edge, maps.er_od)) return rc;
                if (int rc = slot_bytes(pr.prior_p_edge, maps.er_pp)) return rc;
                if (int rc = slot_bytes(pr.prior_l_edge, maps.er_pl)) return rc;
                if (int rc = copy_sync(maps.er_edge, of_edge, E, hipMemcpyHostToDevice)) return rc;
                return copy_sync(maps.er_pal, pal, sizeof(pal), hipMemcpyHostToDevice);
            };
            if (int rc = upload()) { drop_edge_robust(); mem.hier_age = -1; return rc; }      // a failed transfer: the arrays are half written, so no setting is in force
            er.active = true; er.n_entries = n_entries;
            for (int k = 0; k < TSGO_EDGE_ROBUST_MAX; ++k) { er.entries[k] = k < n_entries ? entries[k] : tsgo_edge_robust_entry{}; er.entries[k].reserved = 0; }
            er.of_edge.assign(of_edge, of_edge + E);
        } else drop_edge_robust();      // cleared, or an all-zero mask: the same
        if (changed) mem.hier_age = -1;      // the weights may move wholesale: the next linearisation builds a fresh hierarchy
        s.active = active ? 1 : 0;
        s.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
        if (st_out) *st_out = s;
        return 0;
    }

    int get_edge_robust(int32_t* n_out, tsgo_edge_robust_entry* entries_out, uint8_t* of_edge_out, int64_t cap_edges) override {
        const std::string nm = "tsgo_get_edge_robust";
        if (cfg.world > 1 || collective()) return set_error(-1, nm + ": edge-sharded handles (world > 1) are not supported");
        if (!have_graph_data) return set_error(-3, nm + ": no graph set");
        const size_t E = structure.e_type.size();
        if (cap_edges < (int64_t)E) return set_error(-1, nm + ": cap_edges " + std::to_string(cap_edges) + " is below n_edges = " + std::to_string(E));
        if (!n_out) return set_error(-1, nm + ": n_entries_out is NULL");
        if (!entries_out) return set_error(-1, nm + ": entries_out is NULL");
        if (E > 0 && !of_edge_out) return set_error(-1, nm + ": entry_of_edge_out is NULL");
        *n_out = er.n_entries;
        for (int k = 0; k < TSGO_EDGE_ROBUST_MAX; ++k) entries_out[k] = er.entries[k];
        if (er.active) std::memcpy(of_edge_out, er.of_edge.data(), E);
        else if (E) std::memset(of_edge_out, 0, E);
        return 0;
    }
