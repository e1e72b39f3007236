// engine/engine_report.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// tsgo_edge_report.  One pass of k_edge_report (tsgo_report_kernels.h; the once-per-edge walk of tsgo_edge_walk.h) at the handle's current estimates, on its
// stream: per-edge records (e, s, rho, w) in input edge order and / or the per-class summary (DESIGN.md section 14).
//
// State rule (that of tsgo_marginals): the pass READS estimates, tables and prior records and writes only buffers of its own — the
// slot -> input-edge maps and the workgroup partials, bump-allocated behind everything the graph owns, and a result buffer that lives for
// the call — so the estimates, the solver history and everything the next tsgo_optimize or tsgo_linearize reads stay bit for bit.
//
// The maps (SellTable::edge of by_pose and odom, Problem::prior_p_edge / prior_l_edge) exist on the host for every graph and go to the
// device at the first report on a structure: a handle that never asks pays nothing.  They belong to the STRUCTURE (StructureMaps,
// tsgo_hip.hip): a tsgo_set_graph that reuses it keeps them, one that rebuilds drops them where it releases the slabs.
    bool report_lm_priors() const { return pr.has_priors && tl.n_slices > 0; }
    int report_prepare() {
        if (maps.rep_ready) return 0;
        // what the kernels rely on — every map entry is an input edge, and every input edge sits in exactly one slot the pass evaluates (a
        // record is written once, inside the result buffer) — follows from the structure index's check (host/structure_index.h)
        if (!edges("tsgo_edge_report")) return -30;
        if (int rc = upload_u32m(&maps.rep_lm_edge, pr.by_pose.edge)) return rc;
        if (int rc = upload_u32m(&maps.rep_od_edge, pr.odom.edge)) return rc;
        if (int rc = upload_u32m(&maps.rep_pp_edge, pr.prior_p_edge)) return rc;
        if (int rc = upload_u32m(&maps.rep_pl_edge, pr.prior_l_edge)) return rc;
        if (int rc = dalloc(&maps.rep_part, (size_t)nbP * kEdgeClasses + (size_t)std::max(nbL, 1))) return rc;
        maps.rep_ready = true;
        return 0;
    }
    // the template axes of walk_edges_once (tsgo_edge_walk.h) for this handle: f(g, general, pri) — lanes per pose, general pairs, priors
    template <typename F> void pick_edge_walk(F&& f) {
        pick<1, 2, 4, 8>(pr.by_pose.G, [&](auto g) { pick<0, 1>(oj(), [&](auto general) { pick<0, 1>(pr.has_priors, [&](auto pri) { f(g, general, pri); }); }); });
    }
    // the pass (tsgo_time_kernel 8 too).  rec = nullptr: summary only
    void launch_edge_report(T* rec) {
        if (report_lm_priors()) pick<1, 2, 4, 8>(pr.by_lm.G, [&](auto g) { pick_rk([&](auto rk) {
            launch(k_edge_report_lm_prior<T, g, rk>, nbL, tl, (const T*)lmrec, (const uint32_t*)maps.rep_pl_edge, rec, maps.rep_part + (size_t)nbP * kEdgeClasses, lm_prior_args(), robust_args());
        }); });
        pick_edge_walk([&](auto g, auto general, auto pri) { pick_rk([&](auto rk) {
            launch(k_edge_report<T, g, general, pri, rk>, nbP, tp, to, (const T*)ps, (const T*)lmrec, maps.edge_maps(), rec, maps.rep_part, pri ? pose_prior_args() : no_priors(), robust_args());
        }); });
    }
    // what k_chi2 reads, 4 B of map per evaluated slot, the partials; with records 6 numbers per edge more
    double bytes_report(bool records) {
        const double v = sizeof(T);
        return bytes_chi2() - nbP * v + ((double)pr.n_lm_edges + od_slots_live()) * 4 + (double)(nbP * kEdgeClasses + (report_lm_priors() ? nbL : 0)) * sizeof(ReportPartial<T>) +
               (records ? 6.0 * v * (double)structure.e_type.size() : 0.0);
    }

    int edge_report(double* rec_out, int64_t cap_edges, tsgo_edge_report_stats* st_out) override {
        const auto wall0 = std::chrono::steady_clock::now();
        if (!rec_out && !st_out) return set_error(-1, "tsgo_edge_report: bad argument (rec_out and stats both NULL)");
        if (cfg.world > 1 || collective()) return set_error(-1, "tsgo_edge_report: edge-sharded handles (world > 1) are not supported");
        if (!have_graph_data) return set_error(-3, "tsgo_edge_report: no graph set");
        const size_t E = structure.e_type.size();
        if (rec_out && cap_edges < (int64_t)E) return set_error(-1, "tsgo_edge_report: cap_edges " + std::to_string(cap_edges) + " is below n_edges = " + std::to_string(E));
        HIP_OK(hipSetDevice(cfg.device));
        if (int rc = report_prepare()) return rc;
        CallScratch records; T* rec_dev = nullptr;
        if (rec_out && E > 0) records.want(&rec_dev, 6 * E * sizeof(T));
        if (int rc = records.commit()) return rc;
        launch_edge_report(rec_dev);
        HIP_OK(hipGetLastError());
        const size_t n_main = (size_t)nbP * kEdgeClasses, n_lp = report_lm_priors() ? (size_t)nbL : 0;
        std::vector<ReportPartial<T>> hp(n_main + n_lp);
        HIP_OK(hipMemcpyAsync(hp.data(), maps.rep_part, hp.size() * sizeof(ReportPartial<T>), hipMemcpyDeviceToHost, stream));
        if (rec_dev) {
            if constexpr (sizeof(T) == sizeof(double)) HIP_OK(hipMemcpyAsync(rec_out, rec_dev, 6 * E * sizeof(T), hipMemcpyDeviceToHost, stream));
            else {      // f32 records widened on the host
                std::vector<T> tmp(6 * E);
                HIP_OK(hipMemcpyAsync(tmp.data(), rec_dev, tmp.size() * sizeof(T), hipMemcpyDeviceToHost, stream));
                HIP_OK(hipStreamSynchronize(stream));
                for (size_t k = 0; k < tmp.size(); ++k) rec_out[k] = (double)tmp[k];
            }
        }
        HIP_OK(hipStreamSynchronize(stream));
        if (st_out) {
            tsgo_edge_report_stats s; std::memset(&s, 0, sizeof(s));
            for (int c = 0; c < kEdgeClasses; ++c) {
                tsgo_edge_class_summary& o = s.cls[c];
                uint32_t best = kNoEdge;
                auto fold = [&](const ReportPartial<T>& p) {
                    o.edges += p.edges; o.downweighted += p.down; o.s_sum += (double)p.s_sum; o.rho_sum += (double)p.rho_sum;
                    if (p.edges && ((double)p.s_max > o.s_max || ((double)p.s_max == o.s_max && p.s_max_edge < best))) { o.s_max = (double)p.s_max; best = p.s_max_edge; }
                };
                for (int b = 0; b < nbP; ++b) fold(hp[(size_t)b * kEdgeClasses + c]);
                if (c == kClassLmPrior) for (size_t b = 0; b < n_lp; ++b) fold(hp[n_main + b]);
                o.s_max_edge = best == kNoEdge ? -1 : (int64_t)best;
                s.chi2 += o.rho_sum;
            }
            s.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
            *st_out = s;
        }
        return 0;
    }
