// tsgo_hip.hip — device side of the C ABI in include/tsgo.h: buffers, launches, the Gauss-Newton
// loop with the reference's stop rules (remote/optimizer/OptimizerCpu.h:80-180), hipGraph replay of
// the PCG iteration, RCCL all-reduces for edge-sharded runs.  Kernels: tsgo_kernels.h, tsgo_amg_kernels.h, tsgo_sym_kernels.h, tsgo_marginal_kernels.h, tsgo_sample_kernels.h, tsgo_leverage_kernels.h, tsgo_init_kernels.h, tsgo_edit_kernels.h, tsgo_gnc_kernels.h, tsgo_mixture_kernels.h, tsgo_dogleg_kernels.h.
//
// One translation unit; the engine class is laid out over this file and engine/*.inc (each included inside the class body):
//   this file                      members (what the solver learns grouped by lifetime: SolverMemory; the structure index and its device maps), configuration / environment (host/knobs.h), device slabs, call-scoped device scratch (CallScratch, EventPair) and upload helpers; the C ABI at the end
//   host/structure_index.h         (host only, no HIP) vertex id -> position -> internal number, input edge -> slots: the one index every reader of the tables uses
//   engine/engine_hierarchy.inc    the multigrid hierarchy on the device: patterns, symbolic products, dense bottom operators
//   engine/engine_graph.inc        tsgo_set_graph: tables, value staging, structure re-use, where SolverMemory starts afresh, solver history across requests
//   engine/engine_launch.inc       every kernel launch of a linearisation / a hierarchy build / a PCG iteration
//   tsgo_block_row.h               (device only) the one walk of a 3x3 block row — lane position, early exit, row dot product — of the multigrid cycle's kernels
//                                  (tsgo_amg_kernels.h), with the 3x3 helpers and the cycle format it reads.  The pair-list products (k_pair_gemm*) and the
//                                  batched cycle of tsgo_marginal_kernels.h (k_mb_bsr: a thread per (row, column)) do NOT use it: they are other shapes
//   engine/engine_collective.inc   the all-reduces of an edge-sharded run
//   engine/engine_solve.inc        the Gauss-Newton and Levenberg-Marquardt loops, the PCG drivers and the retry ladder (do_solve), read-outs
//   engine/engine_probes.inc       timing probes (bench.py)
//   engine/engine_marginals.inc    tsgo_marginals, tsgo_joint_marginals: batched PCG for blocks of H^-1, one column-batch driver for every reader (mb_for_batches)
//   host/batch_plan.h              (host only, no HIP) how the readers cut their columns into batches; the gate's per-batch lists
//   engine/engine_sample.inc       tsgo_sample_marginals: posterior samples by perturb-and-MAP and every vertex's covariance from their second moments
//   engine/engine_leverage.inc     tsgo_edge_leverage: C_e = J_e H^-1 J_e^T and the leverage of every input edge from the same samples (the sampling driver with one more read-out:
//                                  k_lev_acc / k_lev_acc_lm_prior, tsgo_leverage_kernels.h, a fourth visitor of tsgo_edge_walk.h)
//   engine/engine_report.inc       tsgo_edge_report: per-edge residual records and the per-class summary
//   tsgo_edge_walk.h               (device only) the once-per-edge walk of the reader kernels, shared by the report, GNC, max-mixture cost, dogleg g'Hg and leverage passes: every input edge is visited by ONE lane
//                                  (pose-pose edges at their first endpoint, padding never), and a skipped slot is left before anything but its index and map words is
//                                  read — why those passes write per edge with plain stores.  k_chi2 / k_lin_pose (and their landmark twins) intentionally do NOT use it:
//                                  they have no slot -> edge maps, count padding through its zero weight, and must agree with each other on chi^2 bit for bit
//   engine/engine_gate.inc         tsgo_gate_edges: candidate edges against the joint marginal of their vertices (Mahalanobis gate)
//   engine/engine_init.inc         tsgo_init_estimates: estimates from an odometry spanning tree (pointer jumping), landmarks from their observations
//   engine/engine_edit.inc         tsgo_set_edge_information / tsgo_get_edge_information: the information diagonal of listed edges, in place;
//                                  tsgo_set_fixed / tsgo_get_fixed / tsgo_set_estimates: the gauge terms and the estimates of listed vertices, in place
//   engine/engine_edge_robust.inc  tsgo_set_edge_robust / tsgo_get_edge_robust: a palette of robust kernels and one byte per input edge; the per-slot byte arrays of the RK = 2 kernels
//   engine/engine_gnc.inc          tsgo_gnc: graduated non-convexity (truncated least squares), one reweighting pass over the tables per round
//   engine/engine_mixture.inc      tsgo_max_mixture: groups of alternative edges, one switched on; per pass the cost of every member (k_mix_cost, a fifth visitor of
//                                  tsgo_edge_walk.h) and a thread per group that selects and scatters (k_mix_select); kernels: tsgo_mixture_kernels.h (f64 only)
//   engine/engine_dogleg.inc       rules = 3, Powell's dogleg trust-region loop: one linearisation and one solve per ACCEPTED step, trials from the snapshot; tsgo_set_dogleg,
//                                  tsgo_get_dogleg_trace.  Kernels: tsgo_dogleg_kernels.h (f64 only) — the gradient as dense vectors, g'Hg by the once-per-edge walk
//                                  (a third visitor of tsgo_edge_walk.h), the step from the snapshot
//   engine/engine_testing.inc      tsgo_testing_apply, tsgo_testing_warm_start (TSGO_TESTING builds only): the operators PCG applies, read out column by column; the warm start's outputs
//   engine/sym_testing.inc         (file scope, TSGO_TESTING builds only) the pattern builders of tsgo_sym_kernels.h on caller-given arrays
//   engine/lane_testing.inc        (file scope, TSGO_TESTING builds only) the lane sums of tsgo_kernels.h on caller-given values
//
// There is NO CPU fallback in this file: every entry point that computes needs a gfx950 device and
// returns an error otherwise.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/tsgo.h"
#ifdef TSGO_TESTING
#include "../../include/tsgo_testing.h"
#endif
#include "host/amg.h"
#include "host/errors.h"
#include "host/init_tree.h"
#include "host/knobs.h"
#include "host/parallel.h"
#include "host/problem.h"
#include "host/structure_index.h"
#include "tsgo_amg_kernels.h"
#include "tsgo_dogleg_kernels.h"
#include "tsgo_edit_kernels.h"
#include "tsgo_gate_kernels.h"
#include "tsgo_gnc_kernels.h"
#include "tsgo_init_kernels.h"
#include "tsgo_kernels.h"
#include "tsgo_leverage_kernels.h"
#include "tsgo_lm_kernels.h"
#include "tsgo_marginal_kernels.h"
#include "tsgo_mixture_kernels.h"
#include "tsgo_report_kernels.h"
#include "tsgo_sample_kernels.h"
#include "tsgo_sym_kernels.h"

namespace {

using namespace tsgo;

#define HIP_OK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return set_error(-10, std::string(#expr) + ": " + hipGetErrorString(e_));                  \
    } while (0)
#define NCCL_OK(expr)                                                                                  \
    do {                                                                                               \
        ncclResult_t e_ = (expr);                                                                      \
        if (e_ != ncclSuccess)                                                                         \
            return set_error(-11, std::string(#expr) + ": " + ncclGetErrorString(e_));                 \
    } while (0)

// Run-time value -> template argument: f(std::integral_constant<int, Vk>{}) for the listed Vk that equals v, and for the LAST listed value
// when none does (lanes per vertex outside {1, 2, 4} run the 8-lane kernels, lanes per row outside {4, 8, 16, 32} the 64-lane ones).  A flag
// is pick<0, 1>.  Calls nest, one per template axis; the constant a call site receives feeds both its instantiation and its profiler name.
template <int V0, int... Vs, typename F> inline decltype(auto) pick(int v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V0>{});
    else {
        if (v == V0) return f(std::integral_constant<int, V0>{});
        return pick<Vs...>(v, std::forward<F>(f));
    }
}
// A kernel symbol as rocprofv3 prints it, without the namespace: kernel_name("k_schur_lm", "double", 4, 0, 1) = "k_schur_lm<double, 4, 0, 1>".
// Type arguments come as strings, integer arguments as integers or as the constants pick() hands out.
inline void template_arg(std::string& s, const char* type) { s += type; }
inline void template_arg(std::string& s, int value) { s += std::to_string(value); }
template <typename... A> std::string kernel_name(const char* base, const A&... args) {
    std::string s(base);
    if constexpr (sizeof...(A) > 0) {
        const char* sep = "<";
        ((s += sep, template_arg(s, args), sep = ", "), ...);
        s += ">";
    }
    return s;
}

}  // namespace

#ifdef TSGO_TESTING
// An all-reduce among engine handles of ONE process (typically sharing one device): every rank stages its buffer in host
// memory, all ranks meet, every rank sums the staged buffers in rank order (same bits everywhere, as with RCCL) and copies
// the sum back.  Slow by design; it exists so that the edge-sharded device path (shard tables, ownership rules, per-rank
// level-0 lists, where the all-reduces sit) can be run with 2, 3, ... ranks on a box with a single GPU, where RCCL refuses
// two ranks on one device.  tests/test_gpu_sharded_inprocess.py.
struct tsgo_local_group {
    int world = 1;
    std::mutex m; std::condition_variable cv;
    int arrived = 0; long generation = 0;
    std::vector<std::vector<unsigned char>> stage;
    bool broken = false;                     // a rank gave up waiting: every later barrier fails at once
    // false: the other ranks did not arrive within kLocalBarrierSeconds (they took a different decision, or one of them
    // returned with an error) — the caller reports that instead of waiting forever
    bool barrier() {
        std::unique_lock<std::mutex> l(m);
        if (broken) return false;
        const long gen = generation;
        if (++arrived == world) { arrived = 0; ++generation; cv.notify_all(); return true; }
        if (!cv.wait_for(l, std::chrono::seconds(kLocalBarrierSeconds), [&] { return generation != gen || broken; }) || broken) {
            broken = true; cv.notify_all();
            return false;
        }
        return true;
    }
    static constexpr int kLocalBarrierSeconds = 120;
};
#else
struct tsgo_local_group;      // in-process all-reduce group: TSGO_TESTING builds only (include/tsgo_testing.h)
#endif

namespace {

// The multigrid pattern builder runs on a thread of its own and does its device work (symbolic products) on a stream of its own:
// the helpers below use the calling thread's stream, which is this one on the builder thread and the engine's elsewhere.
thread_local hipStream_t t_builder_stream = nullptr;

struct IEngine {
    virtual ~IEngine() {}
    virtual int set_graph(const tsgo_graph& g) = 0;
    virtual int optimize(int iterations, tsgo_stats* st) = 0;
    virtual int get_vertices(double* out) = 0;
    virtual int linearize(double* diag, double* grad, double* chi2) = 0;
    virtual int solve_step(double* delta, double* chi2, int* iters) = 0;
    virtual int time_kernel(int which, int reps, double* us, double* bytes) = 0;
    virtual int cycle_probe(int reps, tsgo_cycle_level* out, int cap) = 0;
    virtual int profile_iteration(int reps, tsgo_prof_entry* out, int cap) = 0;
    virtual int comm_selftest(int* ranks_out) = 0;
    virtual int comm_time_allreduce(int64_t n, int reps, double* us) = 0;
    virtual void reset_history() = 0;
    virtual int set_robust(const tsgo_robust& r) = 0;
    virtual void get_robust(tsgo_robust* out) const = 0;
    virtual int set_dogleg(const tsgo_dogleg_params& p) = 0;
    virtual void get_dogleg(tsgo_dogleg_params* out) const = 0;
    virtual void get_dogleg_trace(tsgo_dogleg_trace* out) const = 0;
    virtual int marginals(const uint32_t* ids, int n_ids, double rel_tol, double* cov, tsgo_marginal_stats* st) = 0;
    virtual int joint_marginals(const uint32_t* ids, int n_ids, double rel_tol, double* cov, int64_t cov_cap, int* dim_out, tsgo_marginal_stats* st) = 0;
    virtual int sample_marginals(int n_samples, uint64_t seed, double rel_tol, double* cov, int64_t cap_vertices, double* samples, int64_t samples_cap,
                                 tsgo_sample_stats* st) = 0;
    virtual int edge_leverage(int n_samples, uint64_t seed, double rel_tol, double* rec_out, int64_t cap_edges, tsgo_leverage_stats* st) = 0;
    virtual int edge_report(double* rec_out, int64_t cap_edges, tsgo_edge_report_stats* st) = 0;
    virtual int gate_edges(int n, const uint32_t* e_type, const uint32_t* e_ids, const double* e_meas, const double* e_inf, double rel_tol, double* rec_out,
                           double* innov_out, tsgo_gate_stats* st) = 0;
    virtual int init_estimates(int what, const uint8_t* mask, int64_t n_mask, tsgo_init_stats* st) = 0;
    virtual int set_edge_information(int64_t n, const int64_t* edge_idx, const double* e_inf, tsgo_edge_info_stats* st) = 0;
    virtual int get_edge_information(double* e_inf_out, int64_t cap_edges) = 0;
    virtual int set_fixed(int64_t n, const uint32_t* ids, const int32_t* count, tsgo_vertex_edit_stats* st) = 0;
    virtual int get_fixed(int32_t* count_out, int64_t cap_vertices) = 0;
    virtual int set_estimates(int64_t n, const uint32_t* ids, const double* v_pos, tsgo_vertex_edit_stats* st) = 0;
    virtual int set_edge_robust(int32_t n_entries, const tsgo_edge_robust_entry* entries, const uint8_t* of_edge, int64_t n_mask, tsgo_edge_robust_stats* st) = 0;
    virtual int get_edge_robust(int32_t* n_out, tsgo_edge_robust_entry* entries_out, uint8_t* of_edge_out, int64_t cap_edges) = 0;
    virtual int gnc(const tsgo_gnc_params& p, const uint8_t* subject, int64_t n_mask, double* w_out, int64_t cap_edges, tsgo_gnc_stats* st) = 0;
    virtual int max_mixture(const tsgo_mixture_params& p, int64_t n_groups, const int64_t* group_off, const int64_t* member_edge, const double* log_weight,
                            int32_t* selected_out, int64_t cap_groups, double* cost_out, int64_t cap_members, tsgo_mixture_stats* st) = 0;
#ifdef TSGO_TESTING
    virtual int testing_apply(int which, const double* in, double* out, int n_cols) = 0;
    virtual int testing_warm_start(int n_plant, const double* plant, int fused, tsgo_testing_warm_out* out) = 0;
#endif
    ncclComm_t comm = nullptr;
    tsgo_local_group* lgroup = nullptr;      // in-process stand-in for the communicator (tests on a one-GPU box; always null outside TSGO_TESTING builds)
};

constexpr int kRhoSteps = 16, kRhoBlocks = 64, kRhoEvery = 8;   // smoother-damping estimate: power steps, partial sums, refresh period
constexpr int kAmgStallIter = 400;      // a multigrid-preconditioned solve that has not even halved r^T M^-1 r by this iteration is treated as a
constexpr double kAmgStallRatio = 0.5;  // failed preconditioner (stagnation) and repeated with block-Jacobi; one that is converging, however slowly
                                        // (odometry-only graphs under the analytic Jacobians are beam-like: 600 iterations at 12k poses, where
                                        // block-Jacobi needs > 10^5), runs on to pcg_max_iters
constexpr double kMediumPairList = 6;   // Galerkin products whose average pair list is longer than this share an output block among 8 lanes,
constexpr double kLongPairList = 16;    // ... longer than this among 16 lanes ...
constexpr double kVeryLongPairList = 200; // ... or a whole wavefront
constexpr int kHierMaxAge = 4;          // a multigrid hierarchy serves at most this many consecutive linearisations (2: 4.32, 3: 4.25, 4: 4.16, 6: 4.16 ms per step at 100k poses, profiles/r03h_*) ...
constexpr int kYoungLins = 6, kYoungMaxAge = 2;   // ... a graph's first linearisations: two per hierarchy at most (do_linearize)
constexpr double kHostSlowFraction = 0.6;   // use_graphs = 2: eager launches need the host to be done enqueueing a burst well before the device is done running it.  At 100k
                                            // poses the host needs 0.4 of the solve's time (90 of 217 us per iteration) and eager wins by 2 %; at 10k poses 0.9 (90 of 99 us):
                                            // eager is then as fast on a good run (2.25 ms per step against 2.32) and 20-30 % slower on a bad one — replay
constexpr int kPaceLead = 1;             // do_solve_paced: iterations the host enqueues ahead of the one whose gate has run
constexpr int kHierSlack = 2;           // ... and is rebuilt as soon as a solve needs more than this many iterations over its first
constexpr int kPackedCycleMaxIters = 64; // a multigrid solve that needs more iterations than this is on an ill-conditioned graph: its cycle leaves the packed halves for f32
constexpr int kHierFreshAbove = 64;     // ... and at every linearisation while solves take more iterations than this (a build costs about four)
constexpr double kProfBlockUsPerLaunch = 10.0;   // tsgo_profile_iteration: host time allowed per enqueued launch + event behind the blocking kernel
constexpr int kChunk = 16;   // PCG iterations per captured hipGraph (even: the state ring has 2 slots)
constexpr int kChunkAmg = 2; // with the multigrid V-cycle an iteration is ~30 launches and a solve ~50 iterations

// Holds its stream for `ms` milliseconds (constant-rate 100 MHz counter), bounded: at most a few hundred ms whatever is asked.
__global__ void k_wait_ms(int ms) {
    const long long ticks = (long long)(ms < 0 ? 0 : (ms > 400 ? 400 : ms)) * 100000ll;
    const long long t0 = (long long)wall_clock64();
    while ((long long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}

template <typename T> struct DevLevel {      // device copy of one AmgLevel (host/amg.h) + its numeric arrays
    int n = 0, n_agg = 0, nnzA = 0, nnzP = 0, nnzT = 0, nnzNext = 0;
    double pairs_T = 0, pairs_A = 0;      // average pair-list lengths of the two Galerkin products
    int *A_ptr = nullptr, *A_col = nullptr, *A_row = nullptr, *diag = nullptr;
    int *P_ptr = nullptr, *P_col = nullptr, *P_row = nullptr, *p_self = nullptr, *ps_ptr = nullptr, *ps_x = nullptr, *ps_y = nullptr;
    int *R_ptr = nullptr, *R_col = nullptr, *r_to_p = nullptr, *p_to_r = nullptr;
    int *ts_ptr = nullptr, *ts_x = nullptr, *ts_y = nullptr, *as_ptr = nullptr, *as_x = nullptr, *as_y = nullptr, *as_mirror = nullptr, *as_upper = nullptr;
    int n_upper = 0;
    int *T_ptr = nullptr, *T_col = nullptr;      // pattern of T = A P (the factored dense level reads it: E = P - W T)
    bool patterns_up = false;      // A / P / R patterns are on the device already (the device built this level's pair-list products)
    bool products_dev = false;     // ts_* / as_* were built on the device (tsgo_sym_kernels.h): nothing of them exists on the host
    using H = HT<T>;                              // hierarchy storage type (tsgo_amg_kernels.h)
    T* rel = nullptr;
    H *A = nullptr, *Dinv = nullptr, *P = nullptr, *Tv = nullptr, *Rv = nullptr;
    uint32_t *Apm = nullptr, *Ppm = nullptr, *Rpm = nullptr;       // cycle format: the same blocks, plane-major within each row, f32 or packed half (tsgo_amg_kernels.h)
    void *r = nullptr, *z = nullptr, *res = nullptr, *z2 = nullptr;      // cycle vectors: CV<T>, or T under Engine::cyc64 (launch_vcycle_v)
};

template <typename T> struct Engine : IEngine {
    tsgo_config cfg;
    Problem pr;
    hipStream_t stream = nullptr, stream2 = nullptr;     // stream2: the pattern builder thread's
    hipStream_t cs() const { return t_builder_stream ? t_builder_stream : stream; }
    std::mutex slab_mu;                                    // the slab allocator is shared by the two threads of tsgo_set_graph
    // Device memory of a graph is bump-allocated from a few large slabs that the handle keeps: tsgo_set_graph with a new
    // structure frees nothing and allocates nothing as long as the new graph fits in what an earlier one needed (hipFree is
    // synchronous and a request makes ~230 allocations).  Slabs grow geometrically (64 MB ... 1 GB each) and are returned
    // to the driver when the handle is destroyed.
    struct Slab { char* base; size_t cap, used; };
    std::vector<Slab> slabs; size_t slab_total = 0;
    static constexpr size_t kSlabMin = size_t(64) << 20, kSlabMax = size_t(1) << 30;
    bool have_graph_data = false;
    double ms_setup = 0;
    // Structure of the graph the device tables were built for (a SLAM front-end resends the same
    // graph with new estimates).  A request with the same vertex ids / types, edge list and fixed list only refills
    // state and measurement planes: no layout build, no multigrid patterns, no table or hierarchy upload, no capture.
    struct Structure {
        std::vector<uint32_t> v_id, v_type, e_type, e_ids, fixed;
        bool same_as(const tsgo_graph& g) const {
            auto eq = [](const std::vector<uint32_t>& a, const uint32_t* b, size_t n) { return a.size() == n && (n == 0 || std::memcmp(a.data(), b, n * sizeof(uint32_t)) == 0); };
            return g.n_vertices >= 0 && g.n_edges >= 0 && g.n_fixed >= 0 && eq(v_id, g.v_id, (size_t)g.n_vertices) && eq(v_type, g.v_type, (size_t)g.n_vertices) &&
                   eq(e_type, g.e_type, (size_t)g.n_edges) && eq(e_ids, g.e_ids, 2 * (size_t)g.n_edges) && eq(fixed, g.fixed, (size_t)g.n_fixed);
        }
        void take(const tsgo_graph& g) {
            v_id.assign(g.v_id, g.v_id + g.n_vertices); v_type.assign(g.v_type, g.v_type + g.n_vertices);
            e_type.assign(g.e_type, g.e_type + g.n_edges); e_ids.assign(g.e_ids, g.e_ids + 2 * (size_t)g.n_edges);
            fixed.assign(g.fixed, g.fixed + g.n_fixed);
        }
    } structure;
    bool last_set_reused = false;
    std::vector<double> lm_values;                 // per LM edge: (zx, zy, w0, w1), scratch of stage_values
    T* stage = nullptr; size_t stage_cap = 0;      // pinned staging for everything that goes to the device in type T
    T *st_p = nullptr, *st_l = nullptr, *st_o = nullptr;   // the static planes of the three tables (Table<T>::st, writable)

    // device
    T *ps = nullptr, *theta = nullptr, *lmrec = nullptr, *gauge_p = nullptr, *gauge_l = nullptr;
    Table<T> tp{}, tl{}, to{};
    // unary priors (Problem::prior_*; null when the graph has none): CSR offsets, records in T, the landmark priors' chi^2 partials (nbL)
    uint32_t *pri_p_off = nullptr, *pri_l_off = nullptr;
    T *pri_p = nullptr, *pri_l = nullptr, *pri_lchi = nullptr;
    T *part = nullptr, *dp = nullptr, *minv = nullptr, *r = nullptr, *p = nullptr, *q = nullptr, *x = nullptr, *zc = nullptr;
    float *zc32 = nullptr, *tvec32 = nullptr;      // f32 copies of the gathered records, read by the two products inside the multigrid cycle
    T *sbuf = nullptr, *tvec = nullptr, *ninv = nullptr, *dl = nullptr, *gpart[2] = {nullptr, nullptr}, *npart = nullptr;
    CgState<T>* st[2] = {nullptr, nullptr};
    CgState<T>* h_state = nullptr;     // pinned
    int* h_flag = nullptr;             // pinned, coherent: what the gate of the last launched iteration saw (k_iter_gate, do_solve_paced)
    T* h_scratch = nullptr;            // pinned, partials_max() of them: where fetch_partials copies to when there are no step reports
    // Step reports (one-shard handles; k_report, engine_solve.inc: wait_report): the device stores chi^2 / ||delta|| partials into h_rep
    // and then a sequence number into its first word; the host thread polls that word instead of draining the stream.  Pinned, coherent;
    // one cache line for the word, the partials behind it.  Sized by the largest graph the handle has seen, freed with the handle.
    uint64_t* h_rep = nullptr; size_t rep_cap = 0;
    static constexpr size_t kRepHead = 64 / sizeof(T);      // the word's cache line, in elements of T
    T* rep_data() const { return reinterpret_cast<T*>(h_rep) + kRepHead; }
    // rules = 2 and 3 only (null otherwise): the estimates before a trial's step (k_lm_state), and the partials one trial brings back in one fetch:
    // lm_red = [ |d_p|^2 (nbC) | |d_l|^2 (nbL) | pred, poses (nbC) | pred, landmarks (nbL) | chi^2 at the trial point (nbP) ] (rules = 3: the last alone, in front)
    T *snap_ps = nullptr, *snap_theta = nullptr, *snap_lm = nullptr, *lm_red = nullptr;
    int nbP = 0, nbL = 0, nbC = 0;
    bool fuse_post_smooth = true;      // the level-0 post-smoothing in the epilogue of the cycle's second product (research: TSGO_FUSE_POST=0 = k_smooth0)
    double hier_shift_cfg = 0;         // the hier_shift a graph starts with (0; research: TSGO_HIER_SHIFT)
    bool fold_gate = true;             // the stopping rule in workgroup 0 of the iteration's first product (research: TSGO_FOLD_GATE=0 = its own kernel)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // step reports: a second set, so that a step's device times are read while the next step runs (end_step_timing); evc = the set being recorded
    hipEvent_t ev_b[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t* evc = ev; hipEvent_t* ev_pending = nullptr;
    bool pending_solved = true;        // ... and whether the pending set's step linearised and solved (a dogleg trial that reused a solve did not)
    static constexpr int kDecideSolves = 3;
    bool replayed = false;             // the last tsgo_optimize replayed captured iterations (tsgo_stats.graph_replay)
    // ---- What the solver learns while it runs has one of three lifetimes; a new member goes into one of the three groups.
    // 1. Forgotten at EVERY tsgo_set_graph, refill or new structure (a refilled handle does, bit for bit, what a fresh one does): reset_solver_state()
    //    assigns fresh_memory(); refill_values() and carry_in() then put the warm-start history back under warm_requests.
    //    (Not solver memory, but of this lifetime too: the per-edge robust setting `er`, engine_edge_robust.inc — dropped by refill() and set_graph
    //    themselves, not by reset_solver_state(), which tsgo_init_estimates also runs and which must keep it.)
    static constexpr int kAgeSlots = 16;
    struct SolverMemory {
        bool have_prev = false;            // warm start: hist[0] holds the pose delta of the previous solve
        int n_prev = 0;                    // ... how many consecutive deltas are held
        int n_tested = 0;                  // ... orders 1..n_tested of the extrapolation have an error in warm_err (k_save_x)
        bool carried = false;              // ... the history came from the previous request: the first warm start made from it is checked (do_solve)
        int predicted_cg = 0;              // burst prediction (do_solve_once): PCG iterations of the last solve,
        int iters_by_age[kAgeSlots] = {};  // ... of the last solve that ran on a hierarchy of that age,
        int iters_fresh = 0, iters_last = 0;   // ... of the last solve on a fresh hierarchy and of the last multigrid solve (do_linearize's refresh rule too)
        int hier_age = -1;                 // hierarchy age: linearisations the hierarchy has served; -1: no valid hierarchy
        int lin_count = 0;                 // ... hierarchy builds so far (the damping estimate is refreshed at every kRhoEvery-th)
        int n_lins = 0;                    // ... linearisations of this graph so far
        int n_decided = 0, n_slow_seen = 0, n_host_slow = 0, n_paced_slow = 0;   // eager / replay / paced: what do_solve_once and do_solve_paced have counted
        double ref_us_per_iter = 0;        // ... the device's time per iteration as the burst path measured it (the graph's first solves)
        bool cy16 = true;                  // a hard graph (do_solve): the cycle's copies of A_l, P_l, R_l are packed half floats (20 B per block; f32: 36 B), tsgo_config.cycle_storage until a solve shows it too ill-conditioned for 11-bit blocks
        double hier_shift = 0;             // ... relative raise of the diagonal of the hierarchy's level-0 matrix: hier_shift_cfg until a breakdown
    } mem;
    SolverMemory fresh_memory() const { SolverMemory m; m.cy16 = cfg.cycle_storage != 32; m.hier_shift = hier_shift_cfg; return m; }
    // 2. Belongs to the TABLES: reset where set_graph builds a new structure, kept by a refill.
    int optimize_calls_on_tables = 0;  // tsgo_optimize calls since the tables were built (lazy hipGraph capture, see set_graph)
    hipGraphExec_t cg_graph = nullptr; // (also dropped when the cycle leaves or re-enters the packed format: it holds those kernels)
    double od_live = -1;               // live ODOM slots of this shard (the byte models'), counted once per structure (od_slots_live)
    bool schur_dev = false;            // level 0's pattern and contribution lists were built on the device (run_device_schur)
    // Where the request's vertices and edges sit in the tables (host/structure_index.h), and the device maps the readers make of that.  Each
    // part is built by the first call that needs it — a handle that never asks pays nothing at tsgo_set_graph — and bump-allocated behind
    // what the graph owns; all of it goes in ONE place, drop_structure_maps(), where set_graph releases the slabs.  world == 1 handles only:
    // every reader refuses an edge-sharded handle before it would build anything.
    StructureIndex sindex;
    struct StructureMaps {
        // tsgo_edge_report (engine_report.inc): slot -> input edge of by_pose and odom, record -> input edge of the two prior lists
        uint32_t *rep_lm_edge = nullptr, *rep_od_edge = nullptr, *rep_pp_edge = nullptr, *rep_pl_edge = nullptr;
        ReportPartial<T>* rep_part = nullptr;      // [nbP][kEdgeClasses] of k_edge_report, then [nbL] of k_edge_report_lm_prior
        bool rep_ready = false;
        EdgeMaps edge_maps() const { return EdgeMaps{rep_lm_edge, rep_od_edge, rep_pp_edge}; }      // what walk_edges_once takes (tsgo_edge_walk.h)
        // tsgo_set / get_edge_information (engine_edit.inc): EdgeSlots::loc and cls on the device
        uint32_t* edit_map = nullptr;              // [2 E]
        uint8_t* edit_cls = nullptr;               // [E]
        char* edit_buf = nullptr;                  // [32 E] bytes: (3 n doubles | n int64) of a set call; 3 E doubles of a get call
        bool edit_ready = false;
        // tsgo_set_fixed / tsgo_set_estimates (engine_edit.inc): what a call sends, (values | kind and internal number) of its listed vertices
        char* vedit_buf = nullptr;                 // [48 V] bytes
        bool vedit_ready = false;
        // tsgo_sample_marginals (engine_sample.inc): slot -> input edge of by_lm (the other tables' are the report's), internal pose /
        // landmark -> position in the request's vertex arrays
        uint32_t* smp_lm_edge = nullptr;
        int *smp_pose_vertex = nullptr, *smp_lm_vertex = nullptr;
        bool smp_ready = false;
        // tsgo_set_edge_robust (engine_edge_robust.inc): a byte per slot of by_lm, by_pose and odom, per record of the two prior lists and per
        // input edge, and the palette (RobustArgs, tsgo_kernels.h)
        uint8_t *er_lm = nullptr, *er_pose = nullptr, *er_od = nullptr, *er_pp = nullptr, *er_pl = nullptr, *er_edge = nullptr;
        RobustEntry<T>* er_pal = nullptr;
        bool er_ready = false;
    } maps;
    void drop_structure_maps() { sindex.clear(); maps = StructureMaps(); }
    const VertexIndex& vertices() { return sindex.vertices(structure.v_id, pr); }
    // null after set_error(-30, nm: ...) when the tables fail the check of build_edge_slots
    const EdgeSlots* edges(const std::string& nm) {
        std::string err;
        const EdgeSlots* es = sindex.edges(pr, structure.e_type, err);
        if (!es) set_error(-30, nm + ": " + err);
        return es;
    }
    // 3. Belongs to the HANDLE: never reset.  (With tsgo_robust robust, engine_launch.inc.)
    int n_fallbacks = 0, n_hier_retries = 0, n_hier_shifts = 0, n_cycle_f32_switches = 0, n_carried = 0, n_carry_dropped = 0, structure_reuses = 0;
    uint64_t rep_seq = 0;              // step reports sent so far (64 bits, per handle: no wrap-around path)
    uint32_t paced_base = 0;           // sequence numbers grow ACROSS solves: a gate of an earlier solve that is still queued when a retry
                                       // starts the next one (pace_lead > 1, hierarchy / block-Jacobi repeats) reports a number <= base and is ignored
    // (these two survive tsgo_set_graph while the counters that derive them — n_decided, n_slow_seen, n_host_slow, n_paced_slow — do not)
    double dev_us_per_iter = 0;        // wall time of the last multigrid solve over its iterations
    bool host_slow = false;            // use_graphs = 2: the host thread has been seen to enqueue too slowly for eager launches (do_solve_once)
    // multigrid preconditioner.  Edge-sharded runs use it too: every rank holds the whole hierarchy (patterns from the whole graph,
    // level-0 blocks all-reduced, everything below computed redundantly); only the level-0 contribution lists are per shard
    bool amg_on = false;
    AmgSym amg;
    std::vector<DevLevel<T>> lv;
    int *sc_ptr = nullptr, *sc_optr = nullptr; uint32_t *sc_si = nullptr, *sc_sk = nullptr, *sc_os = nullptr;
    int *last_ptr = nullptr, *last_col = nullptr; int nb_last = 0, nnz_last = 0;
    using H = HT<T>;
    H* A_last = nullptr;
    T *inv_last = nullptr, *rzpart = nullptr, *fold_part = nullptr;
    void *r_last = nullptr, *z_last = nullptr;      // cycle vectors (as DevLevel::r)
    double ms_amg_symbolic = 0;
    T *omega_dev = nullptr, *one_dev = nullptr, *gscale_dev = nullptr, *pw_a = nullptr, *pw_b = nullptr, *rho_part = nullptr;
    T* h_rho = nullptr;                 // pinned
    std::vector<double> omega_host;    // smoother damping per level (diagnostics)
    int hier_max_age = kHierMaxAge, hier_slack = kHierSlack;
    T* hist[kMaxWarm] = {};            // pose deltas of the last solves, newest first (warm start)
    T* warm_err = nullptr;             // [kMaxWarm][nbC]
    int* warm_order_dev = nullptr;     // the order the last warm start took (diagnostics)
    // Coefficients of every extrapolation order (k_pack_x): row m-1 = (-1)^j C(m, j+1) a^(j+1), a = 1 - step.
    void warm_coefficients(WarmTerms<T>& w) const {
        const double a = 1.0 - step_scale();
        for (int m = 1; m <= kMaxWarm; ++m) {
            double binom = 1, apow = 1;
            for (int j = 1; j <= kMaxWarm; ++j) {
                if (j <= m) { binom = binom * (m - j + 1) / j; apow *= a; w.c[m - 1][j - 1] = (T)((j & 1 ? 1.0 : -1.0) * binom * apow); }
                else w.c[m - 1][j - 1] = T(0);
            }
        }
    }
    int coarse_sweeps = kCoarseSweeps;
    std::vector<int> sweeps_list;      // research: sweeps per side on levels 1, 2, ... (TSGO_SWEEPS_LIST="2,2,1"; the last entry repeats)
    int nu_at(size_t l) const {
        if (!sweeps_list.empty()) return sweeps_list[std::min(l - 1, sweeps_list.size() - 1)];
        return coarse_sweeps != kCoarseSweeps ? (lv[l].n <= kSmallLevelRows ? kSmallLevelSweeps : coarse_sweeps) : sweeps_per_side(l, lv[l].n);
    }
    bool low_cycle = true;     // f32 slot planes for the Schur products inside the multigrid cycle
    size_t cyw() const { return mem.cy16 ? (size_t)kCyWordsF16 : (size_t)kCyWordsF32; }
    // the cycle's vectors below level 0 (DevLevel::r / z / res / z2, r_last / z_last, tail_t) hold CV<T>; cyc64 = T instead (testing builds:
    // TSGO_CYCLE_VEC64, host/knobs.h).  Fixed for the handle's life: the buffers are sized by it.
    bool cyc64 = false;
    size_t cv_bytes() const { return cyc64 ? sizeof(T) : sizeof(CV<T>); }
    int valloc(void** out, size_t n) { char* d = nullptr; if (int rc = dalloc(&d, n * cv_bytes())) return rc; *out = d; return 0; }

    // Environment, read ONCE per handle (tsgo_create).  Operational: verbosity / timing traces.  Research and test hooks
    // (TSGO_RESEARCH_ENV: only builds with -DTSGO_TESTING see them, host/knobs.h).
    bool say_env = false, solve_timing = false, stage_timing = false;
    bool hook_inject_amg_failure = false;      // TSGO_INJECT_AMG_FAILURE: the first multigrid solve of every tsgo_optimize is declared broken down
    bool hook_force_host_slow = false;         // TSGO_FORCE_HOST_SLOW: the handle believes its host thread is too slow for eager launches
    bool hook_force_paced = false;             // TSGO_FORCE_PACED: paced eager launches from the first solve on (no timing heuristics)
    int pace_lead = kPaceLead;                 // TSGO_PACE_LEAD: iterations enqueued ahead of the gate that has reported
    bool step_drains = false;                  // TSGO_STEP_DRAINS=1 (every build, host/knobs.h; same results): copy + synchronise instead of device reports
    explicit Engine(const tsgo_config& c) : cfg(c) {
        say_env = c.verbose || getenv("TSGO_VERBOSE") != nullptr;
        solve_timing = getenv("TSGO_SOLVE_TIMING") != nullptr;
        stage_timing = getenv("TSGO_STAGE_TIMING") != nullptr;
        if (const char* e = TSGO_RESEARCH_ENV("TSGO_SWEEPS_LIST")) for (const char* q = e; *q;) { sweeps_list.push_back(std::max(1, std::min(4, atoi(q)))); while (*q && *q != ',') ++q; if (*q == ',') ++q; }
        explicit0 = c.cycle_level0 != 0;
        cyc64 = TSGO_CYCLE_VEC64();
        if (const char* e = TSGO_RESEARCH_ENV("TSGO_HOST_PRODUCTS")) device_products = atoi(e) == 0;
        if (const char* e = TSGO_RESEARCH_ENV("TSGO_SYM_DECLINE")) sym_decline = atoi(e);
        if (const char* e = TSGO_RESEARCH_ENV("TSGO_HIER_MAX_AGE")) hier_max_age = std::max(1, atoi(e));
        if (const char* e = TSGO_RESEARCH_ENV("TSGO_HIER_SLACK")) hier_slack = std::max(0, atoi(e));
        if (const char* e = TSGO_RESEARCH_ENV("TSGO_PACE_LEAD")) pace_lead = std::max(1, atoi(e));
        if (const char* e = TSGO_RESEARCH_ENV("TSGO_LPR_XCD")) lpr_xcd = atoi(e) != 0;
        if (const char* e = TSGO_RESEARCH_ENV("TSGO_FOLD_GATE")) fold_gate = atoi(e) != 0;
        if (const char* e = TSGO_RESEARCH_ENV("TSGO_HIER_SHIFT")) hier_shift_cfg = atof(e);
        if (const char* e = TSGO_RESEARCH_ENV("TSGO_FUSE_POST")) fuse_post_smooth = atoi(e) != 0;
        hook_inject_amg_failure = TSGO_RESEARCH_ENV("TSGO_INJECT_AMG_FAILURE") != nullptr;
        hook_force_host_slow = TSGO_RESEARCH_ENV("TSGO_FORCE_HOST_SLOW") != nullptr;
        hook_force_paced = TSGO_RESEARCH_ENV("TSGO_FORCE_PACED") != nullptr;
        step_drains = tsgo_step_drains();
        mem = fresh_memory();
    }

    ~Engine() override { release(); for (Slab& sl : slabs) (void)hipFree(sl.base); if (carry_dev) (void)hipFree(carry_dev); if (stage) (void)hipHostFree(stage); if (h_rep) (void)hipHostFree(h_rep); if (stream) (void)hipStreamDestroy(stream); if (stream2) (void)hipStreamDestroy(stream2); for (auto& e : ev) if (e) (void)hipEventDestroy(e); for (auto& e : ev_b) if (e) (void)hipEventDestroy(e); for (auto& m : prof) (void)hipEventDestroy(m.e); }

    void release() {
        if (amg_builder.joinable()) amg_builder.join();
        if (cg_graph) { (void)hipGraphExecDestroy(cg_graph); cg_graph = nullptr; }
        for (Slab& sl : slabs) sl.used = 0;
        if (h_state) { (void)hipHostFree(h_state); h_state = nullptr; }
        if (h_flag) { (void)hipHostFree(h_flag); h_flag = nullptr; }
        if (h_scratch) { (void)hipHostFree(h_scratch); h_scratch = nullptr; }
        if (h_rho) { (void)hipHostFree(h_rho); h_rho = nullptr; }
        have_graph_data = false;
    }
    // The staging buffer survives release(): it is sized by the largest table seen and reused across requests.
    int stage_reserve(size_t n) {
        if (n <= stage_cap) return 0;
        if (stage) { (void)hipHostFree(stage); stage = nullptr; stage_cap = 0; }
        n += n / 4;                               // headroom for a growing graph: pinning memory is the expensive part
        HIP_OK(hipHostMalloc((void**)&stage, n * sizeof(T)));
        stage_cap = n;
        return 0;
    }

    // The report buffer survives release() like the staging buffer: n elements of T behind the word's cache line.  A larger graph gets a
    // larger buffer; nothing is in flight into the old one (every report is waited for), the synchronisation is for error paths.
    int rep_reserve(size_t n) {
        if (h_rep && n <= rep_cap) return 0;
        if (h_rep) { HIP_OK(hipStreamSynchronize(stream)); (void)hipHostFree(h_rep); h_rep = nullptr; rep_cap = 0; }
        n += n / 4;
        HIP_OK(hipHostMalloc((void**)&h_rep, (kRepHead + n) * sizeof(T), hipHostMallocCoherent));
        std::memset(h_rep, 0, kRepHead * sizeof(T));      // (rep_seq keeps counting: the next report's number is above anything the word has held)
        rep_cap = n;
        return 0;
    }

    int init() {
        HIP_OK(hipSetDevice(cfg.device));
        HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        HIP_OK(hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking));
        for (auto& e : ev) HIP_OK(hipEventCreate(&e));
        for (auto& e : ev_b) HIP_OK(hipEventCreate(&e));
        return 0;
    }

    double ms_in_malloc = 0; int n_malloc = 0;
    // Every copy and fill goes through THIS engine's stream (never the legacy default stream): several engines serve
    // requests from different threads of one process, and a legacy-stream call in one thread is refused by the runtime
    // while another thread captures a graph.
    int copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        HIP_OK(hipMemcpyAsync(dst, src, bytes, kind, cs()));
        HIP_OK(hipStreamSynchronize(cs()));
        return 0;
    }
    int fill_zero(void* dst, size_t bytes) { HIP_OK(hipMemsetAsync(dst, 0, bytes, cs())); return 0; }
    template <typename U> int dalloc(U** out, size_t n) {
        std::lock_guard<std::mutex> guard(slab_mu);
        const size_t bytes = (std::max<size_t>(n, 1) * sizeof(U) + 255) & ~size_t(255);
        for (Slab& sl : slabs)
            if (sl.used + bytes <= sl.cap) { *out = (U*)(sl.base + sl.used); sl.used += bytes; return 0; }
        const size_t cap = std::max(bytes, std::min(kSlabMax, std::max(kSlabMin, slab_total)));
        void* ptr = nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        HIP_OK(hipMalloc(&ptr, cap));
        ms_in_malloc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); ++n_malloc;
        slabs.push_back({(char*)ptr, cap, bytes}); slab_total += cap;
        *out = (U*)ptr;
        return 0;
    }
    // Device memory that lives for ONE call (what dalloc is for a graph): want() lists the buffers, commit() makes one hipMalloc of their sizes,
    // each rounded up to 256 B, and hands the pointers out in the order asked (no allocation when the sum is 0); freed with the object.
    struct CallScratch {
        char* base = nullptr; size_t total = 0; std::vector<std::pair<void**, size_t>> wants;
        CallScratch() = default; CallScratch(const CallScratch&) = delete; void operator=(const CallScratch&) = delete;
        ~CallScratch() { if (base) (void)hipFree(base); }
        template <typename U> void want(U** out, size_t bytes) { wants.push_back({(void**)out, (bytes + 255) & ~size_t(255)}); total += wants.back().second; }
        int commit() {
            if (total) HIP_OK(hipMalloc((void**)&base, total));
            size_t off = 0;
            for (auto& w : wants) { *w.first = base + off; off += w.second; }
            return 0;
        }
    };
    // ... and a pair of events that lives for one call
    struct EventPair {
        hipEvent_t e[2] = {nullptr, nullptr}; EventPair() = default; EventPair(const EventPair&) = delete; void operator=(const EventPair&) = delete;
        ~EventPair() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
        int create() { HIP_OK(hipEventCreate(&e[0])); HIP_OK(hipEventCreate(&e[1])); return 0; }
        hipEvent_t operator[](int k) const { return e[k]; }
    };
    int upload_T(T** out, const double* src, size_t n) {
        if (int rc = dalloc(out, n)) return rc;
        if (n == 0) return 0;
        std::vector<T> tmp(n);
        for (size_t k = 0; k < n; ++k) tmp[k] = (T)src[k];
        { if (int rc_ = copy_sync(*out, tmp.data(), n * sizeof(T), hipMemcpyHostToDevice)) return rc_; }
        return 0;
    }
    int upload_u32(const uint32_t** out, const std::vector<uint32_t>& v) {
        uint32_t* d = nullptr;
        if (int rc = dalloc(&d, v.size())) return rc;
        if (!v.empty()) { if (int rc_ = copy_sync(d, v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) return rc_; }
        *out = d;
        return 0;
    }
    int upload_u32m(uint32_t** out, const std::vector<uint32_t>& v) {
        if (int rc = dalloc(out, v.size())) return rc;
        if (!v.empty()) { if (int rc_ = copy_sync(*out, v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) return rc_; }
        return 0;
    }
#include "engine/engine_hierarchy.inc"
#include "engine/engine_graph.inc"
#include "engine/engine_launch.inc"
#include "engine/engine_collective.inc"
#include "engine/engine_solve.inc"
#include "engine/engine_probes.inc"
#include "engine/engine_marginals.inc"
#include "engine/engine_gate.inc"
#include "engine/engine_report.inc"
#include "engine/engine_sample.inc"
#include "engine/engine_leverage.inc"
#include "engine/engine_init.inc"
#include "engine/engine_edit.inc"
#include "engine/engine_edge_robust.inc"
#include "engine/engine_gnc.inc"
#include "engine/engine_mixture.inc"
#include "engine/engine_dogleg.inc"
#ifdef TSGO_TESTING
#include "engine/engine_testing.inc"
#endif
};

}  // namespace

#ifdef TSGO_TESTING
#include "engine/sym_testing.inc"
#include "engine/lane_testing.inc"
#endif

struct tsgo_optimizer {
    tsgo_config cfg;
    IEngine* eng = nullptr;
};

extern "C" {

int tsgo_create(const tsgo_config* cfg, tsgo_optimizer** out) {
    if (!out) return tsgo::set_error(-1, "tsgo_create: null argument");
    tsgo_config c;
    if (cfg) c = *cfg; else tsgo_default_config(&c);
    if (c.precision != 32 && c.precision != 64) return tsgo::set_error(-1, "tsgo_create: precision must be 32 or 64");
    if (c.world < 1) c.world = 1;
    if (c.pcg_rel_tol <= 0) c.pcg_rel_tol = 1e-10;
    if (c.pcg_max_iters <= 0) c.pcg_max_iters = 20000;
    if (c.rules == 2) {
        if (c.precision != 64) return tsgo::set_error(-1, "tsgo_create: rules = 2 (Levenberg-Marquardt) needs precision = 64: the gain ratio near the optimum is below f32 resolution");
        if (c.world > 1) return tsgo::set_error(-1, "tsgo_create: rules = 2 (Levenberg-Marquardt) does not support edge-sharded handles (world > 1)");
        if (!(c.lm_lambda0 > 0)) c.lm_lambda0 = 1e-3;
        if (!(c.lm_chi2_rel_tol >= 0)) c.lm_chi2_rel_tol = 1e-6;
    }
    if (c.rules == 3) {
        if (c.precision != 64) return tsgo::set_error(-1, "tsgo_create: rules = 3 (dogleg) needs precision = 64: the gain ratio near the optimum is below f32 resolution");
        if (c.world > 1) return tsgo::set_error(-1, "tsgo_create: rules = 3 (dogleg) does not support edge-sharded handles (world > 1)");
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return tsgo::set_error(-10, "tsgo_create: no HIP device is visible; this library has no CPU fallback");
    if (c.device < 0 || c.device >= n_dev) return tsgo::set_error(-10, "tsgo_create: device ordinal out of range");
    auto* o = new tsgo_optimizer();
    o->cfg = c;
    int rc;
    if (c.precision == 64) { auto* e = new Engine<double>(c); rc = e->init(); o->eng = e; }
    else { auto* e = new Engine<float>(c); rc = e->init(); o->eng = e; }
    if (rc) { delete o->eng; delete o; return rc; }
    *out = o;
    return 0;
}

void tsgo_destroy(tsgo_optimizer* o) {
    if (!o) return;
    if (o->eng && o->eng->comm) (void)ncclCommDestroy(o->eng->comm);
    delete o->eng;
    delete o;
}

int tsgo_set_graph(tsgo_optimizer* o, const tsgo_graph* g) {
    if (!o || !g) return tsgo::set_error(-1, "tsgo_set_graph: null argument");
    return o->eng->set_graph(*g);
}
int tsgo_optimize(tsgo_optimizer* o, int32_t iterations, tsgo_stats* st) {
    if (!o) return tsgo::set_error(-1, "tsgo_optimize: null argument");
    return o->eng->optimize(iterations, st);
}
int tsgo_get_vertices(tsgo_optimizer* o, double* out) {
    if (!o || !out) return tsgo::set_error(-1, "tsgo_get_vertices: null argument");
    return o->eng->get_vertices(out);
}
int tsgo_linearize(tsgo_optimizer* o, double* diag, double* grad, double* chi2) {
    if (!o || !diag || !grad || !chi2) return tsgo::set_error(-1, "tsgo_linearize: null argument");
    return o->eng->linearize(diag, grad, chi2);
}
int tsgo_solve_step(tsgo_optimizer* o, double* delta, double* chi2, int32_t* iters) {
    if (!o || !delta || !chi2) return tsgo::set_error(-1, "tsgo_solve_step: null argument");
    return o->eng->solve_step(delta, chi2, iters);
}
int tsgo_time_kernel(tsgo_optimizer* o, int32_t which, int32_t reps, double* us, double* bytes) {
    if (!o || !us || !bytes || reps <= 0) return tsgo::set_error(-1, "tsgo_time_kernel: bad argument");
    return o->eng->time_kernel(which, reps, us, bytes);
}
int tsgo_cycle_probe(tsgo_optimizer* o, int32_t reps, tsgo_cycle_level* out, int32_t cap) {
    if (!o || !out || reps <= 0 || cap <= 0) return tsgo::set_error(-1, "tsgo_cycle_probe: bad argument");
    return o->eng->cycle_probe(reps, out, cap);
}
int tsgo_profile_iteration(tsgo_optimizer* o, int32_t reps, tsgo_prof_entry* out, int32_t cap) {
    if (!o || !out || reps <= 0 || cap <= 0) return tsgo::set_error(-1, "tsgo_profile_iteration: bad argument");
    return o->eng->profile_iteration(reps, out, cap);
}
#ifdef TSGO_TESTING
int tsgo_local_group_create(int32_t world, tsgo_local_group** out) {
    if (!out || world < 1) return tsgo::set_error(-1, "tsgo_local_group_create: bad argument");
    auto* g = new tsgo_local_group(); g->world = world; g->stage.resize(world);
    *out = g;
    return 0;
}
void tsgo_local_group_destroy(tsgo_local_group* g) { delete g; }
int tsgo_comm_init_local(tsgo_optimizer* o, tsgo_local_group* g) {
    if (!o || !g) return tsgo::set_error(-1, "tsgo_comm_init_local: null argument");
    if (o->cfg.world != g->world || o->cfg.rank < 0 || o->cfg.rank >= g->world) return tsgo::set_error(-1, "tsgo_comm_init_local: the handle's rank / world do not fit the group");
    o->eng->lgroup = g;
    return 0;
}
int tsgo_testing_apply(tsgo_optimizer* o, int32_t which, const double* in, double* out, int32_t n_cols) {
    if (!o) return tsgo::set_error(-1, "tsgo_testing_apply: null handle");
    return o->eng->testing_apply(which, in, out, n_cols);
}
int tsgo_testing_warm_start(tsgo_optimizer* o, int32_t n_plant, const double* plant, int32_t fused, tsgo_testing_warm_out* out) {
    if (!o) return tsgo::set_error(-1, "tsgo_testing_warm_start: null handle");
    return o->eng->testing_warm_start(n_plant, plant, fused, out);
}
int tsgo_testing_sym_scan(int32_t n, const int32_t* in, int32_t* out) { return sym_scan_run(n, in, out); }
int tsgo_testing_lane_sums(const float* in32, const double* in64, float* out32, double* out64) {
    if (!in32 || !in64 || !out32 || !out64) return tsgo::set_error(-1, "tsgo_testing_lane_sums: null argument");
    if (int rc = lane_sums_run<float>(in32, out32)) return rc;
    return lane_sums_run<double>(in64, out64);
}
int tsgo_testing_sym_product(int32_t builder, int32_t upper, int32_t n, const int32_t* xptr, const int32_t* xcol, const int32_t* x_alias, int32_t ny, int32_t nc,
                             const int32_t* yptr, const int32_t* ycol, tsgo_testing_sym_out* out) {
    return sym_product_run(builder, upper, n, xptr, xcol, x_alias, ny, nc, yptr, ycol, out);
}
int tsgo_testing_schur_pattern(int32_t builder, int32_t P, int32_t L, const int32_t* pp_ptr, const int32_t* pp_lm, const uint32_t* pp_slot, const int32_t* obs_ptr,
                               const int32_t* obs_pose, const uint32_t* obs_slot, const int32_t* od_ptr, const int32_t* od_col, const uint32_t* od_slot,
                               int32_t max_pair_degree, tsgo_testing_schur_out* out) {
    return schur_pattern_run(builder, P, L, pp_ptr, pp_lm, pp_slot, obs_ptr, obs_pose, obs_slot, od_ptr, od_col, od_slot, max_pair_degree, out);
}
#endif
int tsgo_marginals(tsgo_optimizer* o, const uint32_t* ids, int32_t n_ids, double rel_tol, double* cov_out, tsgo_marginal_stats* stats) {
    if (!o) return tsgo::set_error(-1, "tsgo_marginals: null handle");
    return o->eng->marginals(ids, n_ids, rel_tol, cov_out, stats);
}
int tsgo_joint_marginals(tsgo_optimizer* o, const uint32_t* ids, int32_t n_ids, double rel_tol, double* cov_out, int64_t cov_cap, int32_t* dim_out,
                         tsgo_marginal_stats* stats) {
    if (!o) return tsgo::set_error(-1, "tsgo_joint_marginals: null handle");
    return o->eng->joint_marginals(ids, n_ids, rel_tol, cov_out, cov_cap, dim_out, stats);
}
int tsgo_sample_marginals(tsgo_optimizer* o, int32_t n_samples, uint64_t seed, double rel_tol, double* cov_out, int64_t cap_vertices, double* samples_out,
                          int64_t samples_cap, tsgo_sample_stats* stats) {
    if (!o) return tsgo::set_error(-1, "tsgo_sample_marginals: null handle");
    return o->eng->sample_marginals(n_samples, seed, rel_tol, cov_out, cap_vertices, samples_out, samples_cap, stats);
}
int tsgo_edge_leverage(tsgo_optimizer* o, int32_t n_samples, uint64_t seed, double rel_tol, double* rec_out, int64_t cap_edges, tsgo_leverage_stats* stats) {
    if (!o) return tsgo::set_error(-1, "tsgo_edge_leverage: null handle");
    return o->eng->edge_leverage(n_samples, seed, rel_tol, rec_out, cap_edges, stats);
}
int tsgo_edge_report(tsgo_optimizer* o, double* rec_out, int64_t cap_edges, tsgo_edge_report_stats* stats) {
    if (!o) return tsgo::set_error(-1, "tsgo_edge_report: null handle");
    return o->eng->edge_report(rec_out, cap_edges, stats);
}
int tsgo_gate_edges(tsgo_optimizer* o, int32_t n, const uint32_t* e_type, const uint32_t* e_ids, const double* e_meas, const double* e_inf, double rel_tol,
                    double* rec_out, double* innov_out, tsgo_gate_stats* stats) {
    if (!o) return tsgo::set_error(-1, "tsgo_gate_edges: null handle");
    return o->eng->gate_edges(n, e_type, e_ids, e_meas, e_inf, rel_tol, rec_out, innov_out, stats);
}
int tsgo_init_estimates(tsgo_optimizer* o, int32_t what, const uint8_t* odom_mask, int64_t n_mask, tsgo_init_stats* stats) {
    if (!o) return tsgo::set_error(-1, "tsgo_init_estimates: null handle");
    return o->eng->init_estimates(what, odom_mask, n_mask, stats);
}
int tsgo_set_edge_information(tsgo_optimizer* o, int64_t n, const int64_t* edge_idx, const double* e_inf, tsgo_edge_info_stats* stats) {
    if (!o) return tsgo::set_error(-1, "tsgo_set_edge_information: null handle");
    return o->eng->set_edge_information(n, edge_idx, e_inf, stats);
}
int tsgo_get_edge_information(tsgo_optimizer* o, double* e_inf_out, int64_t cap_edges) {
    if (!o) return tsgo::set_error(-1, "tsgo_get_edge_information: null handle");
    return o->eng->get_edge_information(e_inf_out, cap_edges);
}
int tsgo_set_fixed(tsgo_optimizer* o, int64_t n, const uint32_t* ids, const int32_t* count, tsgo_vertex_edit_stats* stats) {
    if (!o) return tsgo::set_error(-1, "tsgo_set_fixed: null handle");
    return o->eng->set_fixed(n, ids, count, stats);
}
int tsgo_get_fixed(tsgo_optimizer* o, int32_t* count_out, int64_t cap_vertices) {
    if (!o) return tsgo::set_error(-1, "tsgo_get_fixed: null handle");
    return o->eng->get_fixed(count_out, cap_vertices);
}
int tsgo_set_estimates(tsgo_optimizer* o, int64_t n, const uint32_t* ids, const double* v_pos, tsgo_vertex_edit_stats* stats) {
    if (!o) return tsgo::set_error(-1, "tsgo_set_estimates: null handle");
    return o->eng->set_estimates(n, ids, v_pos, stats);
}
int tsgo_gnc(tsgo_optimizer* o, const tsgo_gnc_params* params, const uint8_t* subject, int64_t n_mask, double* w_out, int64_t cap_edges, tsgo_gnc_stats* stats) {
    if (!o || !params) return tsgo::set_error(-1, "tsgo_gnc: null handle or params");
    return o->eng->gnc(*params, subject, n_mask, w_out, cap_edges, stats);
}
int tsgo_max_mixture(tsgo_optimizer* o, const tsgo_mixture_params* params, int64_t n_groups, const int64_t* group_off, const int64_t* member_edge, const double* log_weight,
                     int32_t* selected_out, int64_t cap_groups, double* cost_out, int64_t cap_members, tsgo_mixture_stats* stats) {
    if (!o || !params) return tsgo::set_error(-1, "tsgo_max_mixture: null handle or params");
    return o->eng->max_mixture(*params, n_groups, group_off, member_edge, log_weight, selected_out, cap_groups, cost_out, cap_members, stats);
}
void tsgo_reset_history(tsgo_optimizer* o) {
    if (o && o->eng) o->eng->reset_history();
}
int tsgo_set_robust(tsgo_optimizer* o, const tsgo_robust* r) {
    if (!o || !r) return tsgo::set_error(-1, "tsgo_set_robust: null argument");
    static const char* const cls[kEdgeClasses] = {"ODOM", "LM", "virtual landmark", "pose prior", "landmark prior"};
    for (int k = 0; k < kEdgeClasses; ++k) {
        if (r->kernel[k] < 0 || r->kernel[k] >= kRobustKinds)
            return tsgo::set_error(-1, std::string("tsgo_set_robust: unknown robust kernel ") + std::to_string(r->kernel[k]) + " for class " + cls[k]);
        if (r->kernel[k] != TSGO_ROBUST_NONE && !(std::isfinite(r->delta[k]) && r->delta[k] >= 1e-6 && r->delta[k] <= 1e6))
            return tsgo::set_error(-1, std::string("tsgo_set_robust: delta of class ") + cls[k] + " must be finite and within [1e-6, 1e6]");
    }
    return o->eng->set_robust(*r);
}
int tsgo_get_robust(tsgo_optimizer* o, tsgo_robust* out) {
    if (!o || !out) return tsgo::set_error(-1, "tsgo_get_robust: null argument");
    o->eng->get_robust(out);
    return 0;
}
int tsgo_set_edge_robust(tsgo_optimizer* o, int32_t n_entries, const tsgo_edge_robust_entry* entries, const uint8_t* entry_of_edge, int64_t n_mask,
                         tsgo_edge_robust_stats* stats) {
    if (!o) return tsgo::set_error(-1, "tsgo_set_edge_robust: null handle");
    return o->eng->set_edge_robust(n_entries, entries, entry_of_edge, n_mask, stats);
}
int tsgo_get_edge_robust(tsgo_optimizer* o, int32_t* n_entries_out, tsgo_edge_robust_entry* entries_out, uint8_t* entry_of_edge_out, int64_t cap_edges) {
    if (!o) return tsgo::set_error(-1, "tsgo_get_edge_robust: null handle");
    return o->eng->get_edge_robust(n_entries_out, entries_out, entry_of_edge_out, cap_edges);
}
int tsgo_set_dogleg(tsgo_optimizer* o, const tsgo_dogleg_params* p) {
    if (!o || !p) return tsgo::set_error(-1, "tsgo_set_dogleg: null argument");
    if (!(std::isfinite(p->radius0) && std::isfinite(p->radius_min) && std::isfinite(p->radius_max) && std::isfinite(p->chi2_rel_tol)))
        return tsgo::set_error(-1, "tsgo_set_dogleg: every parameter must be finite");
    if (!(0 < p->radius_min && p->radius_min <= p->radius0 && p->radius0 <= p->radius_max))
        return tsgo::set_error(-1, "tsgo_set_dogleg: the radii must satisfy 0 < radius_min <= radius0 <= radius_max");
    if (p->chi2_rel_tol < 0) return tsgo::set_error(-1, "tsgo_set_dogleg: chi2_rel_tol must not be negative");
    return o->eng->set_dogleg(*p);
}
int tsgo_get_dogleg(tsgo_optimizer* o, tsgo_dogleg_params* out) {
    if (!o || !out) return tsgo::set_error(-1, "tsgo_get_dogleg: null argument");
    o->eng->get_dogleg(out);
    return 0;
}
int tsgo_get_dogleg_trace(tsgo_optimizer* o, tsgo_dogleg_trace* out) {
    if (!o || !out) return tsgo::set_error(-1, "tsgo_get_dogleg_trace: null argument");
    o->eng->get_dogleg_trace(out);
    return 0;
}
int tsgo_comm_selftest(tsgo_optimizer* o, int32_t* ranks_out) {
    if (!o) return tsgo::set_error(-1, "tsgo_comm_selftest: null argument");
    int n = 0;
    const int rc = o->eng->comm_selftest(&n);
    if (ranks_out) *ranks_out = n;
    return rc;
}
int tsgo_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}
int tsgo_comm_time_allreduce(tsgo_optimizer* o, int64_t n_elements, int32_t reps, double* us_per_call) {
    if (!o || !us_per_call || n_elements <= 0 || reps <= 0) return tsgo::set_error(-1, "tsgo_comm_time_allreduce: bad argument");
    return o->eng->comm_time_allreduce(n_elements, reps, us_per_call);
}
int tsgo_comm_unique_id(uint8_t id_out[128]) {
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId id;
    NCCL_OK(ncclGetUniqueId(&id));
    std::memcpy(id_out, &id, 128);
    return 0;
}
int tsgo_comm_init(tsgo_optimizer* o, const uint8_t id_in[128]) {
    if (!o || !id_in) return tsgo::set_error(-1, "tsgo_comm_init: null argument");
    HIP_OK(hipSetDevice(o->cfg.device));
    ncclUniqueId id;
    std::memcpy(&id, id_in, 128);
    NCCL_OK(ncclCommInitRank(&o->eng->comm, o->cfg.world, id, o->cfg.rank));
    return 0;
}

}  // extern "C"
