// engine/sym_testing.inc — TSGO_TESTING builds only, included by tsgo_hip.hip at FILE scope (no engine, no graph):
// tsgo_testing_sym_scan / tsgo_testing_sym_product / tsgo_testing_schur_pattern (include/tsgo_testing.h) run the pattern builders of
// tsgo_sym_kernels.h on caller-given integer arrays, through the launch helpers engine_hierarchy.inc uses and in its order (run_device_schur,
// run_device_products), and hand back everything the kernels wrote.  tests/test_gpu_sym_patterns.py.
namespace {

struct SymScratch {      // call-scoped device memory: freed when the call returns
    std::vector<void*> owned;
    ~SymScratch() { for (void* p : owned) (void)hipFree(p); }
    template <typename U> int get(U** out, size_t n) {
        void* p = nullptr;
        HIP_OK(hipMalloc(&p, std::max<size_t>(1, n) * sizeof(U)));
        owned.push_back(p);
        *out = (U*)p;
        return 0;
    }
    template <typename U> int up(U** out, const U* src, size_t n) {
        if (int rc = get(out, n)) return rc;
        if (n) HIP_OK(hipMemcpy(*out, src, n * sizeof(U), hipMemcpyHostToDevice));
        return 0;
    }
};
template <typename U> int sym_down(U* dst, const U* src, size_t n) {
    if (n) HIP_OK(hipMemcpy(dst, src, n * sizeof(U), hipMemcpyDeviceToHost));
    return 0;
}
// a CSR pointer array: rises from 0
bool sym_ptr_ok(const int32_t* ptr, int n) {
    if (!ptr || ptr[0] != 0) return false;
    for (int i = 0; i < n; ++i) if (ptr[i + 1] < ptr[i]) return false;
    return true;
}
bool sym_in_range(const int32_t* v, int n, int lo, int hi) {
    for (int k = 0; k < n; ++k) if (v[k] < lo || v[k] >= hi) return false;
    return true;
}
bool sym_rises(const uint32_t* v, int b, int e) {
    for (int k = b + 1; k < e; ++k) if (v[k] <= v[k - 1]) return false;
    return true;
}

int sym_scan_run(int n, const int32_t* in, int32_t* out) {
    if (n < 0 || !out || (n > 0 && !in)) return set_error(-1, "tsgo_testing_sym_scan: bad argument");
    int64_t total = 0;
    for (int k = 0; k < n; ++k) { if (in[k] < 0) return set_error(-1, "tsgo_testing_sym_scan: negative entry"); total += in[k]; }
    if (total > INT32_MAX) return set_error(-1, "tsgo_testing_sym_scan: the total exceeds 2^31 - 1 (k_sym_scan returns int)");
    SymScratch S;
    int *d_in, *d_out;
    if (int rc = S.up(&d_in, (const int*)in, (size_t)n)) return rc;
    if (int rc = S.get(&d_out, (size_t)n + 1)) return rc;
    launch_sym_scan(nullptr, n, d_in, d_out);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(nullptr));
    return sym_down((int*)out, (const int*)d_out, (size_t)n + 1);
}

template <int UPPER>
int sym_product_device(int n, const int* xptr, const int* xcol, const int* x_alias, int ny, const int* yptr, const int* ycol, tsgo_testing_sym_out* o) {
    SymScratch S;
    const int nx = xptr[n], nyz = yptr[ny];
    int *d_xptr, *d_xcol, *d_alias = nullptr, *d_yptr, *d_ycol, *d, *m, *zptr, *poff, *flags;
    if (int rc = S.up(&d_xptr, xptr, (size_t)n + 1)) return rc;
    if (int rc = S.up(&d_xcol, xcol, (size_t)nx)) return rc;
    if (x_alias) { if (int rc = S.up(&d_alias, x_alias, (size_t)nx)) return rc; }
    if (int rc = S.up(&d_yptr, yptr, (size_t)ny + 1)) return rc;
    if (int rc = S.up(&d_ycol, ycol, (size_t)nyz)) return rc;
    if (int rc = S.get(&d, (size_t)n)) return rc;
    if (int rc = S.get(&m, (size_t)n)) return rc;
    if (int rc = S.get(&zptr, (size_t)n + 1)) return rc;
    if (int rc = S.get(&poff, (size_t)n + 1)) return rc;
    if (int rc = S.get(&flags, 4)) return rc;
    HIP_OK(hipMemset(flags, 0, 4 * sizeof(int)));
    launch_sym_count<UPPER>(nullptr, n, d_xptr, d_xcol, d_yptr, d_ycol, d, m, flags);
    launch_sym_scan(nullptr, n, d, zptr);
    launch_sym_scan(nullptr, n, m, poff);
    HIP_OK(hipGetLastError());
    int h3[3];
    HIP_OK(hipMemcpy(&h3[0], zptr + n, sizeof(int), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&h3[1], poff + n, sizeof(int), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&h3[2], flags, sizeof(int), hipMemcpyDeviceToHost));
    if (h3[2]) { o->declined = 1; return 0; }      // as the engine: nothing else is launched
    const int nnz = h3[0], pairs = h3[1];
    if (nnz < 0 || pairs < 0 || nnz > o->cap_blocks || pairs > o->cap_pairs) return set_error(-1, "tsgo_testing_sym_product: the output does not fit the capacities given");
    int *zcol, *pl_ptr, *px, *py, *nup = nullptr, *uoff = nullptr, *mirror = nullptr, *upper = nullptr;
    if (int rc = S.get(&zcol, (size_t)nnz)) return rc;
    if (int rc = S.get(&pl_ptr, (size_t)nnz + 1)) return rc;
    if (int rc = S.get(&px, (size_t)pairs)) return rc;
    if (int rc = S.get(&py, (size_t)pairs)) return rc;
    if (UPPER) {
        if (int rc = S.get(&nup, (size_t)n)) return rc;
        if (int rc = S.get(&uoff, (size_t)n + 1)) return rc;
        if (int rc = S.get(&mirror, (size_t)nnz)) return rc;
        if (int rc = S.get(&upper, (size_t)nnz)) return rc;
    }
    launch_sym_fill<UPPER>(nullptr, n, d_xptr, d_xcol, d_alias, d_yptr, d_ycol, zptr, poff, zcol, pl_ptr, px, py, nup);
    HIP_OK(hipMemcpy(pl_ptr + nnz, &pairs, sizeof(int), hipMemcpyHostToDevice));
    if (UPPER) {
        launch_sym_scan(nullptr, n, nup, uoff);
        launch_sym_mirror(nullptr, n, zptr, zcol, uoff, mirror, upper, flags + 2);
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(nullptr));
    o->nnz = nnz; o->pairs = pairs;
    if (int rc = sym_down(o->zptr, (const int*)zptr, (size_t)n + 1)) return rc;
    if (int rc = sym_down(o->zcol, (const int*)zcol, (size_t)nnz)) return rc;
    if (int rc = sym_down(o->pl_ptr, (const int*)pl_ptr, (size_t)nnz + 1)) return rc;
    if (int rc = sym_down(o->px, (const int*)px, (size_t)pairs)) return rc;
    if (int rc = sym_down(o->py, (const int*)py, (size_t)pairs)) return rc;
    if (UPPER) {
        int h2[2];
        HIP_OK(hipMemcpy(&h2[0], uoff + n, sizeof(int), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(&h2[1], flags + 2, sizeof(int), hipMemcpyDeviceToHost));
        if (h2[0] < 0 || h2[0] > nnz) return set_error(-2, "tsgo_testing_sym_product: the scan of n_upper is not a count of blocks");
        o->upper_blocks = h2[0]; o->not_symmetric = h2[1] ? 1 : 0;
        if (int rc = sym_down(o->n_upper, (const int*)nup, (size_t)n)) return rc;
        if (int rc = sym_down(o->mirror, (const int*)mirror, (size_t)nnz)) return rc;
        if (int rc = sym_down(o->upper, (const int*)upper, (size_t)h2[0])) return rc;
    }
    return 0;
}

int sym_product_host(bool upper, int n, const int* xptr, const int* xcol, const int* x_alias, int ny, int nc, const int* yptr, const int* ycol, tsgo_testing_sym_out* o) {
    BlockCsr X, Y, Z;
    X.n_rows = n; X.n_cols = ny; X.ptr.assign(xptr, xptr + n + 1); X.col.assign(xcol, xcol + xptr[n]);
    Y.n_rows = ny; Y.n_cols = nc; Y.ptr.assign(yptr, yptr + ny + 1); Y.col.assign(ycol, ycol + yptr[ny]);
    std::vector<int> alias, mirror;
    if (x_alias) alias.assign(x_alias, x_alias + xptr[n]);
    PairList pl;
    const std::string err = spgemm_sym(X, x_alias ? &alias : nullptr, Y, Z, pl, upper ? &mirror : nullptr);
    if (err.find("not structurally symmetric") != std::string::npos) o->not_symmetric = 1;
    else if (!err.empty()) return set_error(-2, "tsgo_testing_sym_product: " + err);
    const int64_t nnz = Z.nnz(), pairs = (int64_t)pl.x.size();
    if (nnz > o->cap_blocks || pairs > o->cap_pairs) return set_error(-1, "tsgo_testing_sym_product: the output does not fit the capacities given");
    o->nnz = nnz; o->pairs = pairs;
    std::copy(Z.ptr.begin(), Z.ptr.end(), o->zptr); std::copy(Z.col.begin(), Z.col.end(), o->zcol);
    std::copy(pl.ptr.begin(), pl.ptr.end(), o->pl_ptr); std::copy(pl.x.begin(), pl.x.end(), o->px); std::copy(pl.y.begin(), pl.y.end(), o->py);
    if (upper) {
        std::copy(mirror.begin(), mirror.end(), o->mirror);
        int64_t u = 0;
        for (int i = 0; i < n; ++i) {
            int nu = 0;
            for (int z = Z.ptr[i]; z < Z.ptr[i + 1]; ++z) if (Z.col[z] >= i) { o->upper[u++] = z; ++nu; }
            o->n_upper[i] = nu;
        }
        o->upper_blocks = u;
    }
    return 0;
}

int sym_product_run(int builder, int upper, int n, const int32_t* xptr, const int32_t* xcol, const int32_t* x_alias, int ny, int nc, const int32_t* yptr, const int32_t* ycol,
                    tsgo_testing_sym_out* o) {
    const char* bad = "tsgo_testing_sym_product: bad argument";
    if (!o || (builder != 0 && builder != 1) || (upper != 0 && upper != 1) || n < 1 || ny < 0 || nc < 0) return set_error(-1, bad);
    o->nnz = o->pairs = o->upper_blocks = 0; o->declined = o->not_symmetric = 0;
    if (o->cap_blocks < 0 || o->cap_pairs < 0 || !o->zptr || !o->zcol || !o->pl_ptr || !o->px || !o->py) return set_error(-1, bad);
    if (upper && (!o->mirror || !o->upper || !o->n_upper)) return set_error(-1, bad);
    if (upper && nc != n) return set_error(-1, "tsgo_testing_sym_product: an upper product needs a square pattern (nc = n)");
    if (!sym_ptr_ok(xptr, n) || !sym_ptr_ok(yptr, ny)) return set_error(-1, "tsgo_testing_sym_product: a pointer array does not rise from 0");
    if ((xptr[n] > 0 && !xcol) || (yptr[ny] > 0 && !ycol)) return set_error(-1, bad);
    if (!sym_in_range(xcol, xptr[n], 0, ny)) return set_error(-1, "tsgo_testing_sym_product: an X column lies outside [0, ny)");
    if (!sym_in_range(ycol, yptr[ny], 0, nc)) return set_error(-1, "tsgo_testing_sym_product: a Y column lies outside [0, nc)");
    {   // the kernels' precondition: a Y row has every column once
        std::vector<int> seen((size_t)nc, -1);
        for (int k = 0; k < ny; ++k)
            for (int q = yptr[k]; q < yptr[k + 1]; ++q) {
                if (seen[(size_t)ycol[q]] == k) return set_error(-1, "tsgo_testing_sym_product: a Y row holds a column twice");
                seen[(size_t)ycol[q]] = k;
            }
    }
    int64_t pairs = 0;
    for (int a = 0; a < xptr[n]; ++a) pairs += yptr[xcol[a] + 1] - yptr[xcol[a]];
    if (pairs > INT32_MAX) return set_error(-1, "tsgo_testing_sym_product: more than 2^31 - 1 pairs");
    if (builder == 0) return sym_product_host(upper != 0, n, xptr, xcol, x_alias, ny, nc, yptr, ycol, o);
    return upper ? sym_product_device<1>(n, xptr, xcol, x_alias, ny, yptr, ycol, o) : sym_product_device<0>(n, xptr, xcol, x_alias, ny, yptr, ycol, o);
}

int schur_pattern_run(int builder, int P, int L, const int32_t* pp_ptr, const int32_t* pp_lm, const uint32_t* pp_slot, const int32_t* obs_ptr, const int32_t* obs_pose,
                      const uint32_t* obs_slot, const int32_t* od_ptr, const int32_t* od_col, const uint32_t* od_slot, int max_deg, tsgo_testing_schur_out* o) {
    const char* bad = "tsgo_testing_schur_pattern: bad argument";
    if (!o || P < 1 || L < 0 || max_deg < 0) return set_error(-1, bad);
    if (builder != 1) return set_error(-1, "tsgo_testing_schur_pattern: only the device builder (builder = 1) reads these lists");
    o->nnz = o->pairs = o->od = 0; o->declined = 0;
    if (o->cap_blocks < 0 || o->cap_pairs < 0 || o->cap_od < 0 || !o->zptr || !o->zcol || !o->sc_ptr || !o->sc_optr || !o->slot_i || !o->slot_k || !o->os) return set_error(-1, bad);
    if (!sym_ptr_ok(pp_ptr, P) || !sym_ptr_ok(obs_ptr, L) || !sym_ptr_ok(od_ptr, P)) return set_error(-1, "tsgo_testing_schur_pattern: a pointer array does not rise from 0");
    const int n_pp = pp_ptr[P], n_obs = obs_ptr[L], n_od = od_ptr[P];
    if ((n_pp && (!pp_lm || !pp_slot)) || (n_obs && (!obs_pose || !obs_slot)) || (n_od && (!od_col || !od_slot))) return set_error(-1, bad);
    if (!sym_in_range(pp_lm, n_pp, 0, L)) return set_error(-1, "tsgo_testing_schur_pattern: a landmark lies outside [0, L)");
    if (!sym_in_range(obs_pose, n_obs, 0, P) || !sym_in_range(od_col, n_od, 0, P)) return set_error(-1, "tsgo_testing_schur_pattern: a pose lies outside [0, P)");
    for (int i = 0; i < P; ++i) {
        if (!sym_rises(pp_slot, pp_ptr[i], pp_ptr[i + 1]) || !sym_rises(od_slot, od_ptr[i], od_ptr[i + 1]))
            return set_error(-1, "tsgo_testing_schur_pattern: the slots of a pose's edge list or odometry list do not rise");
        for (int e = od_ptr[i]; e < od_ptr[i + 1]; ++e) if (od_col[e] == i) return set_error(-1, "tsgo_testing_schur_pattern: an odometry neighbour is the pose itself");
    }
    {   // the contract of k_s0_fill: the entries of one pose in one observer list come with rising slots
        std::vector<int> last((size_t)P, -1);
        for (int l = 0; l < L; ++l)
            for (int q = obs_ptr[l]; q < obs_ptr[l + 1]; ++q) {
                const int p = obs_pose[q], before = last[(size_t)p];
                if (before >= obs_ptr[l] && obs_slot[q] <= obs_slot[before]) return set_error(-1, "tsgo_testing_schur_pattern: one pose's entries in an observer list do not come with rising slots");
                last[(size_t)p] = q;
            }
    }
    SymScratch S;
    int *d_pp_ptr, *d_pp_lm, *d_obs_ptr, *d_obs_pose, *d_od_ptr, *d_od_col; uint32_t *d_pp_slot, *d_obs_slot, *d_od_slot;
    if (int rc = S.up(&d_pp_ptr, (const int*)pp_ptr, (size_t)P + 1)) return rc;
    if (int rc = S.up(&d_pp_lm, (const int*)pp_lm, (size_t)n_pp)) return rc;
    if (int rc = S.up(&d_pp_slot, pp_slot, (size_t)n_pp)) return rc;
    if (int rc = S.up(&d_obs_ptr, (const int*)obs_ptr, (size_t)L + 1)) return rc;
    if (int rc = S.up(&d_obs_pose, (const int*)obs_pose, (size_t)n_obs)) return rc;
    if (int rc = S.up(&d_obs_slot, obs_slot, (size_t)n_obs)) return rc;
    if (int rc = S.up(&d_od_ptr, (const int*)od_ptr, (size_t)P + 1)) return rc;
    if (int rc = S.up(&d_od_col, (const int*)od_col, (size_t)n_od)) return rc;
    if (int rc = S.up(&d_od_slot, od_slot, (size_t)n_od)) return rc;
    int *d, *m, *mo, *zptr, *poff, *ooff, *flags;
    if (int rc = S.get(&d, (size_t)P)) return rc;
    if (int rc = S.get(&m, (size_t)P)) return rc;
    if (int rc = S.get(&mo, (size_t)P)) return rc;
    if (int rc = S.get(&zptr, (size_t)P + 1)) return rc;
    if (int rc = S.get(&poff, (size_t)P + 1)) return rc;
    if (int rc = S.get(&ooff, (size_t)P + 1)) return rc;
    if (int rc = S.get(&flags, 4)) return rc;
    HIP_OK(hipMemset(flags, 0, 4 * sizeof(int)));
    launch_s0_count(nullptr, P, d_pp_ptr, d_pp_lm, d_obs_ptr, d_obs_pose, d_od_ptr, d_od_col, max_deg, d, m, mo, flags);
    launch_sym_scan(nullptr, P, d, zptr);
    launch_sym_scan(nullptr, P, m, poff);
    launch_sym_scan(nullptr, P, mo, ooff);
    HIP_OK(hipGetLastError());
    int h4[4];
    HIP_OK(hipMemcpy(&h4[0], zptr + P, sizeof(int), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&h4[1], poff + P, sizeof(int), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&h4[2], ooff + P, sizeof(int), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(&h4[3], flags, sizeof(int), hipMemcpyDeviceToHost));
    if (h4[3]) { o->declined = 1; return 0; }      // as the engine: the fill pass is not launched
    const int nnz = h4[0], n_pairs = h4[1], n_os = h4[2];
    if (nnz < 0 || n_pairs < 0 || n_os < 0 || nnz > o->cap_blocks || n_pairs > o->cap_pairs || n_os > o->cap_od)
        return set_error(-1, "tsgo_testing_schur_pattern: the output does not fit the capacities given");
    int *zcol, *sc_ptr, *sc_optr; uint32_t *si, *sk, *os;
    if (int rc = S.get(&zcol, (size_t)nnz)) return rc;
    if (int rc = S.get(&sc_ptr, (size_t)nnz + 1)) return rc;
    if (int rc = S.get(&sc_optr, (size_t)nnz + 1)) return rc;
    if (int rc = S.get(&si, (size_t)n_pairs)) return rc;
    if (int rc = S.get(&sk, (size_t)n_pairs)) return rc;
    if (int rc = S.get(&os, (size_t)n_os)) return rc;
    launch_s0_fill(nullptr, P, d_pp_ptr, d_pp_lm, d_pp_slot, d_obs_ptr, d_obs_pose, d_obs_slot, d_od_ptr, d_od_col, d_od_slot, max_deg, zptr, poff, ooff, zcol, sc_ptr, sc_optr, si, sk, os);
    HIP_OK(hipMemcpy(sc_ptr + nnz, &n_pairs, sizeof(int), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(sc_optr + nnz, &n_os, sizeof(int), hipMemcpyHostToDevice));
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(nullptr));
    o->nnz = nnz; o->pairs = n_pairs; o->od = n_os;
    if (int rc = sym_down(o->zptr, (const int*)zptr, (size_t)P + 1)) return rc;
    if (int rc = sym_down(o->zcol, (const int*)zcol, (size_t)nnz)) return rc;
    if (int rc = sym_down(o->sc_ptr, (const int*)sc_ptr, (size_t)nnz + 1)) return rc;
    if (int rc = sym_down(o->sc_optr, (const int*)sc_optr, (size_t)nnz + 1)) return rc;
    if (int rc = sym_down(o->slot_i, (const uint32_t*)si, (size_t)n_pairs)) return rc;
    if (int rc = sym_down(o->slot_k, (const uint32_t*)sk, (size_t)n_pairs)) return rc;
    return sym_down(o->os, (const uint32_t*)os, (size_t)n_os);
}

}  // namespace
