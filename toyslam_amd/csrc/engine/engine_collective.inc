// engine/engine_collective.inc — part of `template <typename T> struct Engine` (tsgo_hip.hip includes it INSIDE the class body):
// all-reduces of an edge-sharded run: RCCL, or the in-process group of TSGO_TESTING builds.
    // The collective path (eager launches, block-Jacobi PCG, all-reduces between kernels) is taken by every shard of a
    // split graph — and by a single shard that was given a communicator (tsgo_comm_init with world = 1), which is how
    // the RCCL plumbing is exercised on a one-GPU box.
    bool collective() const { return pr.world > 1 || comm != nullptr || lgroup != nullptr; }
#ifdef TSGO_TESTING
    template <typename U> int allreduce_local(U* buf, size_t n) {
        tsgo_local_group& G = *lgroup;
        std::vector<unsigned char>& mine = G.stage[cfg.rank];
        mine.resize(n * sizeof(U));
        HIP_OK(hipMemcpyAsync(mine.data(), buf, n * sizeof(U), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        if (!G.barrier()) return set_error(-12, "in-process all-reduce: the other ranks did not arrive (ranks took different decisions?)");   // every rank's contribution is staged
        std::vector<U> sum(n, U(0));
        for (int r = 0; r < G.world; ++r) {
            if (G.stage[r].size() != n * sizeof(U)) return set_error(-12, "in-process all-reduce: ranks disagree on the buffer size");
            const U* src = (const U*)G.stage[r].data();
            for (size_t k = 0; k < n; ++k) sum[k] += src[k];
        }
        if (!G.barrier()) return set_error(-12, "in-process all-reduce: the other ranks did not arrive (ranks took different decisions?)");   // nobody restages while another rank still reads
        HIP_OK(hipMemcpyAsync(buf, sum.data(), n * sizeof(U), hipMemcpyHostToDevice, stream));
        HIP_OK(hipStreamSynchronize(stream));
        return 0;
    }
#else
    template <typename U> int allreduce_local(U*, size_t) { return set_error(-12, "the in-process all-reduce group exists in TSGO_TESTING builds only"); }
#endif
    int allreduce(T* buf, size_t n) {
        if (!collective()) return 0;
        if (lgroup) return allreduce_local(buf, n);
        if (!comm) return set_error(-12, "world > 1 but tsgo_comm_init was not called");
        NCCL_OK(ncclAllReduce(buf, buf, n, sizeof(T) == 8 ? ncclDouble : ncclFloat, ncclSum, comm, stream));
        return 0;
    }
    int allreduce_h(H* buf, size_t n) {       // hierarchy storage type (f32 unless TSGO_HIER_F64)
        if (!collective()) return 0;
        if (lgroup) return allreduce_local(buf, n);
        if (!comm) return set_error(-12, "world > 1 but tsgo_comm_init was not called");
        NCCL_OK(ncclAllReduce(buf, buf, n, sizeof(H) == 8 ? ncclDouble : ncclFloat, ncclSum, comm, stream));
        return 0;
    }
    // One element through the same all-reduce the solver uses, on the engine's stream: every rank contributes rank + 1 and
    // must read world (world + 1) / 2 back.  The first collective of a communicator is where a broken fabric or a missing
    // peer shows (as a hang: bench.py runs this under a watchdog); *ranks_out = what the communicator itself says its size is.
    int comm_selftest(int* ranks_out) override {
        HIP_OK(hipSetDevice(cfg.device));
        int n = 1;
        if (comm) NCCL_OK(ncclCommCount(comm, &n));
#ifdef TSGO_TESTING
        else if (lgroup) n = lgroup->world;
#endif
        if (ranks_out) *ranks_out = n;
        if (!collective()) return 0;
        CallScratch one; T* d = nullptr;
        one.want(&d, sizeof(T));
        if (int rc = one.commit()) return rc;
        T v = (T)(cfg.rank + 1);
        HIP_OK(hipMemcpyAsync(d, &v, sizeof(T), hipMemcpyHostToDevice, stream));
        if (int rc = allreduce(d, 1)) return rc;
        HIP_OK(hipMemcpyAsync(&v, d, sizeof(T), hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        const double want = 0.5 * n * (n + 1.0);
        if (n != std::max(1, cfg.world) || std::fabs((double)v - want) > 1e-6) return set_error(-12, "tsgo_comm_selftest: " + std::to_string(n) + " ranks in the communicator, world " + std::to_string(cfg.world) + ", sum " + std::to_string((double)v) + " instead of " + std::to_string(want));
        return 0;
    }
    // `reps` all-reduces of n numbers back to back on the engine's stream, timed with events (bench.py, N > 1: what one of the solver's
    // collectives costs on this fabric).  A scratch buffer of zeros: the sums stay zeros.
    int comm_time_allreduce(int64_t n, int reps, double* us) override {
        HIP_OK(hipSetDevice(cfg.device));
        *us = 0;
        if (!collective()) return 0;
        CallScratch zeros; T* d = nullptr;
        zeros.want(&d, sizeof(T) * (size_t)n);
        if (int rc = zeros.commit()) return rc;
        HIP_OK(hipMemsetAsync(d, 0, sizeof(T) * (size_t)n, stream));
        for (int k = 0; k < 2; ++k) if (int rc = allreduce(d, (size_t)n)) return rc;       // the first call of a size sets its channels up
        HIP_OK(hipEventRecord(ev[0], stream));
        for (int k = 0; k < reps; ++k) if (int rc = allreduce(d, (size_t)n)) return rc;
        float ms = 0;
        HIP_OK(hipEventRecord(ev[1], stream));
        HIP_OK(hipEventSynchronize(ev[1]));
        HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        *us = 1e3 * ms / reps;
        return 0;
    }
