// engine/engine_init.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// tsgo_init_estimates.  The odometry spanning tree is built on the host from the structure the handle keeps (host/init_tree.h: ids, types,
// the fixed list and the mask; no value enters), handed to the device as two words per pose in the internal numbering — parent, and a slot
// of the pose-pose table that holds the tree edge — and composed there (tsgo_init_kernels.h, DESIGN.md section 16).
//
// The handle keeps no measurement on the host and M^-1 on the device: k_init_rel inverts the slot's planes back, so a handle that never
// calls this pays nothing at tsgo_set_graph (the rule of the report maps, engine_report.inc).  Everything the call needs beyond the
// graph's own buffers — tree words, the two record buffers, the landmark counts — is one allocation that lives for the call.
//
// State: the call CHANGES estimates.  It ends as a values-only tsgo_set_graph does (restart_on_new_estimates: host copy of the estimates,
// lever arms, reset_solver_state), without the warm-start history even under warm_requests: a jump does not continue it.
    int init_estimates(int what, const uint8_t* mask, int64_t n_mask, tsgo_init_stats* st_out) override {
        const auto wall0 = std::chrono::steady_clock::now();
        if (sizeof(T) != 8) return set_error(-1, "tsgo_init_estimates: needs precision = 64");
        if (cfg.world > 1 || collective()) return set_error(-1, "tsgo_init_estimates: edge-sharded handles (world > 1) are not supported");
        if (!have_graph_data) return set_error(-3, "tsgo_init_estimates: no graph set");
        if (what < 0 || what > 3) return set_error(-1, "tsgo_init_estimates: what = " + std::to_string(what) + " is outside 0 .. 3");
        if (what == 0) what = TSGO_INIT_POSES | TSGO_INIT_LANDMARKS;
        const size_t E = structure.e_type.size();
        if (mask && n_mask != (int64_t)E) return set_error(-1, "tsgo_init_estimates: n_mask = " + std::to_string(n_mask) + " but the graph has " + std::to_string(E) + " edges (one byte per edge)");
        if constexpr (sizeof(T) == 8) {
            tsgo_init_stats s; std::memset(&s, 0, sizeof(s));
            const int P = pr.P, L = pr.L;
            const bool poses = (what & TSGO_INIT_POSES) != 0, lms = (what & TSGO_INIT_LANDMARKS) != 0 && L > 0 && tl.n_slices > 0;
            // ---- the tree, then its two words per pose in the internal numbering ----
            InitTree tree;
            const VertexIndex& vi = vertices();
            {
                const std::vector<uint32_t>& fixed = fixed_list();      // the request's list, or the canonical one of a tsgo_set_fixed (engine_edit.inc)
                const tsgo_graph view{(int32_t)structure.v_id.size(), structure.v_id.data(), structure.v_type.data(), nullptr, (int32_t)E, structure.e_type.data(),
                                      structure.e_ids.data(), nullptr, nullptr, (int32_t)fixed.size(), fixed.data()};
                const std::string err = build_init_tree(view, mask, n_mask, tree, &vi.ids);
                if (!err.empty()) return set_error(-2, "tsgo_init_estimates: " + err);
            }
            s.roots_fixed = tree.roots_fixed; s.roots_free = tree.roots_free; s.edges_usable = tree.edges_usable; s.tree_edges = tree.tree_edges;
            s.depth_max = tree.depth_max;
            const int rounds = poses ? tree.rounds() : 0;
            std::vector<int> h_parent; std::vector<uint32_t> h_slot;
            if (poses) {
                const EdgeSlots* es = edges("tsgo_init_estimates");
                if (!es) return -30;
                const size_t So = pr.odom.slots();
                h_parent.assign((size_t)P, -1); h_slot.assign((size_t)P, 0u);
                for (int i = 0; i < P; ++i) {
                    const int v = pr.pose_vertex[(size_t)i], pv = tree.parent[(size_t)v];
                    if (pv < 0) continue;
                    const int e = tree.edge[(size_t)v];
                    // the first slot that holds the tree edge (an ODOM edge: either endpoint's slot keeps the same planes)
                    const uint32_t at = e < 0 || (size_t)e >= E || structure.e_type[(size_t)e] != kClassOdom ? kNoEdge : es->first_odom_slot((size_t)e);
                    // what the kernels rely on: the parent is a pose of this table, the edge sits in a slot of it
                    if (vi.pose_of(pv) < 0 || at == kNoEdge || (size_t)at >= So || So >= (size_t)kInitInverse)
                        return set_error(-30, "tsgo_init_estimates: the pose-pose table does not hold tree edge " + std::to_string(e));
                    h_parent[(size_t)i] = vi.pose_of(pv);
                    h_slot[(size_t)i] = at | (structure.e_ids[2 * (size_t)e] == structure.v_id[(size_t)v] ? kInitInverse : 0u);
                }
            }
            s.ms_tree = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
            // ---- device memory of the call ----
            HIP_OK(hipSetDevice(cfg.device));
            CallScratch scratch; EventPair te;
            int *parent_d = nullptr, *par_d[2] = {nullptr, nullptr}, *counts_d = nullptr; uint32_t* slot_d = nullptr; InitRec* rec_d[2] = {nullptr, nullptr};
            if (poses) {
                scratch.want(&rec_d[0], (size_t)P * sizeof(InitRec)); scratch.want(&rec_d[1], (size_t)P * sizeof(InitRec));
                scratch.want(&par_d[0], (size_t)P * sizeof(int)); scratch.want(&par_d[1], (size_t)P * sizeof(int));
                scratch.want(&parent_d, (size_t)P * sizeof(int)); scratch.want(&slot_d, (size_t)P * sizeof(uint32_t));
            }
            if (lms) scratch.want(&counts_d, (size_t)nbL * 2 * sizeof(int));
            if (int rc = scratch.commit()) return rc;
            if (int rc = te.create()) return rc;
            if (poses) {
                HIP_OK(hipMemcpyAsync(parent_d, h_parent.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice, stream));
                HIP_OK(hipMemcpyAsync(slot_d, h_slot.data(), (size_t)P * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            }
            // ---- the kernels ----
            HIP_OK(hipEventRecord(te[0], stream));
            if (poses) {
                launch(k_init_rel, nbC, P, (const int*)parent_d, (const uint32_t*)slot_d, (const double*)to.st, to.slots, (const double*)ps, rec_d[0], par_d[0]);
                for (int k = 0; k < rounds; ++k)
                    launch(k_init_jump, nbC, P, (const InitRec*)rec_d[k & 1], (const int*)par_d[k & 1], rec_d[(k + 1) & 1], par_d[(k + 1) & 1]);
                launch(k_init_write, nbC, P, (const int*)parent_d, (const InitRec*)rec_d[rounds & 1], (double*)ps, (double*)theta);
            }
            if (lms) pick<1, 2, 4, 8>(pr.by_lm.G, [&](auto g) {
                launch(k_init_landmarks<g>, nbL, tl, (const double*)ps, (const double*)gauge_l, (double*)lmrec, counts_d);
            });
            HIP_OK(hipGetLastError());
            HIP_OK(hipEventRecord(te[1], stream));
            // ---- what the host keeps of the estimates, the counts ----
            std::vector<double> hp, hl; std::vector<int> hc;
            if (poses) { hp.resize((size_t)P * 5); HIP_OK(hipMemcpyAsync(hp.data(), ps, (size_t)P * 4 * sizeof(double), hipMemcpyDeviceToHost, stream)); HIP_OK(hipMemcpyAsync(hp.data() + (size_t)P * 4, theta, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, stream)); }
            if (lms) {
                hl.resize((size_t)L * kLmRec); hc.resize((size_t)nbL * 2);
                HIP_OK(hipMemcpyAsync(hl.data(), lmrec, hl.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
                HIP_OK(hipMemcpyAsync(hc.data(), counts_d, hc.size() * sizeof(int), hipMemcpyDeviceToHost, stream));
            }
            HIP_OK(hipStreamSynchronize(stream));
            { float ms = 0; HIP_OK(hipEventElapsedTime(&ms, te[0], te[1])); s.ms_device = ms; }
            if (poses) for (int i = 0; i < P; ++i) {
                if (h_parent[(size_t)i] < 0) continue;
                pr.pose_xyt[3 * (size_t)i] = hp[4 * (size_t)i]; pr.pose_xyt[3 * (size_t)i + 1] = hp[4 * (size_t)i + 1]; pr.pose_xyt[3 * (size_t)i + 2] = hp[(size_t)P * 4 + (size_t)i];
                ++s.poses_set;
            }
            if (lms) {
                for (int l = 0; l < L; ++l) { pr.lm_xy[2 * (size_t)l] = hl[(size_t)l * kLmRec]; pr.lm_xy[2 * (size_t)l + 1] = hl[(size_t)l * kLmRec + 1]; }
                for (int b = 0; b < nbL; ++b) { s.landmarks_set += hc[2 * (size_t)b]; s.landmarks_unobserved += hc[2 * (size_t)b + 1]; }
            }
            s.rounds = rounds;
            if (int rc = restart_on_new_estimates()) { have_graph_data = false; return rc; }
            mem.carried = false; carry.n = 0;
            HIP_OK(hipStreamSynchronize(stream));
            s.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
            if (st_out) *st_out = s;
            return 0;
        } else return set_error(-1, "tsgo_init_estimates: needs precision = 64");
    }
