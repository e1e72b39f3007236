/* tsgo_testing.h — entry points that exist ONLY in libtsgo_hip_testing.so (built with -DTSGO_TESTING, toyslam_amd/build.py).
 *
 * The shipped libtsgo_hip.so and graph_optimizer contain neither these symbols nor the test hooks / research variables of
 * toyslam_amd/csrc/host/knobs.h (TSGO_INJECT_AMG_FAILURE, TSGO_FORCE_HOST_SLOW, TSGO_FORCE_PACED, TSGO_SYM_DECLINE, TSGO_HIER_*,
 * TSGO_AGG*, TSGO_HOST_PRODUCTS, ...).  Everything else — kernels, host code, the C ABI of tsgo.h — is the same source. */
#ifndef TSGO_TESTING_H
#define TSGO_TESTING_H

#include "tsgo.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The same sharded path among handles of ONE process (one thread per handle; they may share a device): the all-reduces
 * go through host memory instead of RCCL.  For tests on a box with a single GPU, where RCCL refuses two ranks on one
 * device — it is what lets `world` = 2, 3 run the device kernels' ownership rules there.  The group outlives its handles. */
typedef struct tsgo_local_group tsgo_local_group;
int tsgo_local_group_create(int32_t world, tsgo_local_group** out);
void tsgo_local_group_destroy(tsgo_local_group* group);
int tsgo_comm_init_local(tsgo_optimizer* opt, tsgo_local_group* group);

/* The operators the PCG of `opt` applies, column by column, with the launches the solver itself makes (tests/test_gpu_precond_operator.py).
 * in / out: n_cols columns of 3 * P doubles each (column c at offset c * 3 * P), in the order of the graph's POSE vertices (not the
 * device's pose numbering).  The call linearises at the current estimates and builds a hierarchy for that linearisation; like
 * tsgo_marginals it restores every device byte of the handle afterwards, so the next tsgo_optimize / tsgo_solve_step computes what it
 * would have without the call.  Sharded handles (world > 1) are refused.
 *   which 0: y = S x by PCG's own product, in the handle's precision.
 *         1: y = S x by the product INSIDE the multigrid cycle (tsgo_config.cycle_level0 = 0: the f32-copy passes; 1: the explicit
 *            level-0 matrix in the cycle's storage format).  An error on a block-Jacobi handle.
 *         2: z = M^-1 r as one PCG iteration applies it: the level-0 pre-smoothing as the vector step leaves it, then the V-cycle
 *            (block-Jacobi handle: the inverse diagonal blocks).
 *         3: the batched cycle of tsgo_marginals on all n_cols columns at once (n_cols <= the batch width, 16 by default; precision 64);
 *            no column is stopped.  which <= 2 loop over the columns. */
int tsgo_testing_apply(tsgo_optimizer* opt, int32_t which, const double* in, double* out, int32_t n_cols);

/* The PCG warm start of `opt` (engine/engine_solve.inc: launch_warm; kernels k_pack_x, k_warm_residual, k_warm_scale, and k_save_x /
 * k_save_update, which leave the history and the prediction errors): what it decides and writes, read out of the handle
 * (tests/test_gpu_warm_start.py).  All vectors are 3 * P doubles in the order of the graph's POSE vertices, as in tsgo_testing_apply,
 * widened from the handle's precision.  The call linearises at the current estimates (without damping) with a hierarchy built for that
 * linearisation, runs launch_warm as do_solve does when `warmed`, and reads; like tsgo_testing_apply it restores every device byte of the
 * handle afterwards, and the solver's host-side memory (the counters below, the rotation of the history buffers) as well: the next
 * tsgo_optimize computes, bit for bit, what it would have without the call.
 *   n_plant = 0: the history the handle holds.
 *   n_plant = 1 .. 12: the history is forgotten first, then `plant` (n_plant deltas of 3 * P doubles, OLDEST first, each rounded to the
 *     handle's precision) is recorded delta by delta through the code the Gauss-Newton loops record a solved delta with (record_delta):
 *     fused = 0 by k_save_x, fused = 1 by k_save_update with step 0, which leaves the estimates alone.  Only the last 6 are kept.
 * Refused: a handle without a graph, a sharded handle (world > 1), n_plant outside [0, 12], n_plant > 0 without `plant`, fused not 0 or 1. */
typedef struct tsgo_testing_warm_out {
    int32_t warmed;                 /* do_solve's own test: cfg.warm_start && have_prev && step_scale() < 1 */
    int32_t n_prev, n_tested, n_max;/* as launch_warm computes them */
    int32_t order;                  /* *warm_order_dev */
    int32_t done;                   /* st[0]->done after k_warm_scale (multigrid); 0 for block-Jacobi */
    int32_t carried;                /* mem.carried */
    double err[6];                  /* row m of warm_err summed over the workgroups, m < n_tested; 0 beyond */
    double scale, bdb, rdr;         /* *gscale_dev and the sums of the two partial arrays k_warm_scale read */
    double *hist;                   /* n_prev x 3P, newest first; may be NULL */
    double *b, *x0, *r0;            /* 3P each: r before launch_warm, x and r after it; each may be NULL */
} tsgo_testing_warm_out;
/* warmed = 0: the counters and b are returned, everything else is 0 / untouched. */
int tsgo_testing_warm_start(tsgo_optimizer* opt, int32_t n_plant, const double* plant, int32_t fused, tsgo_testing_warm_out* out);

/* ---- the device pattern builders (toyslam_amd/csrc/tsgo_sym_kernels.h) on caller-given integer arrays: tests/test_gpu_sym_patterns.py.
 * No handle, no graph, no linearisation: each call allocates its own device scratch, launches the kernels through the launch helpers the
 * engine itself uses (the same geometry) on the null stream, copies everything they wrote back and frees the scratch before it returns.
 * A refused input or a capacity that is too small is an error return (tsgo_last_error), never a write past the end of an array. */

/* k_sym_scan: out[0 .. n] = exclusive scan of in[0 .. n), out[n] = the total.  n >= 0; entries >= 0.  The kernel returns int: a total of
 * 2^31 or more is refused here — in the engine the host builder refuses such a hierarchy ("exceed 2^31 pairs") where the device's
 * count would wrap. */
int tsgo_testing_sym_scan(int32_t n, const int32_t* in, int32_t* out);

typedef struct tsgo_testing_sym_out {
    int64_t cap_blocks, cap_pairs; /* in: entries the caller's arrays hold (zcol, mirror, upper: cap_blocks; pl_ptr: cap_blocks + 1; px, py: cap_pairs) */
    int32_t* zptr;                 /* n + 1 */
    int32_t* zcol;                 /* the distinct columns of every row, ascending */
    int32_t* pl_ptr;               /* nnz + 1: the list offsets per block */
    int32_t* px;                   /* the lists: x block (or its alias) ... */
    int32_t* py;                   /* ... and y block of every pair, in walking order within a block */
    int32_t* mirror;               /* upper: per block below the diagonal the block it mirrors, -1 elsewhere (may be null when upper = 0) */
    int32_t* upper;                /* upper: the blocks on or above the diagonal, in block order (may be null when upper = 0) */
    int32_t* n_upper;              /* upper: n entries, blocks on or above the diagonal per row (may be null when upper = 0) */
    int64_t nnz, pairs, upper_blocks;   /* out: entries written */
    int32_t declined;              /* out: the count pass raised its overflow word; nothing else was launched, nothing else is returned */
    int32_t not_symmetric;         /* out: k_sym_mirror's `bad` / the host builder's error text; every array is returned all the same */
} tsgo_testing_sym_out;

/* Z = X * Y on patterns with the pair lists of every Z block.  X: n rows (xptr, xcol; x_alias optional, one entry per X block),
 * Y: ny rows and nc columns (yptr, ycol).  builder = 1: the device sequence of the engine (count, two scans, fill; upper: the scan of
 * n_upper and k_sym_mirror).  builder = 0: the host builder (host/amg.cpp: spgemm_sym) on the same arrays; it never declines, and its
 * `upper` / `n_upper` are read off Z (column >= row).  upper = 1 is the symmetric product: only blocks on or above the diagonal get lists.
 * Refused: n < 1, upper with nc != n, pointers that do not rise from 0, an X column outside [0, ny), a Y column outside [0, nc), a Y row
 * that holds a column twice (the kernels' precondition: "a Y row has every column once"), more than 2^31 - 1 pairs. */
int tsgo_testing_sym_product(int32_t builder, int32_t upper, int32_t n, const int32_t* xptr, const int32_t* xcol, const int32_t* x_alias, int32_t ny, int32_t nc,
                             const int32_t* yptr, const int32_t* ycol, tsgo_testing_sym_out* out);

typedef struct tsgo_testing_schur_out {
    int64_t cap_blocks, cap_pairs, cap_od;   /* in: zcol: cap_blocks; sc_ptr, sc_optr: cap_blocks + 1; slot_i, slot_k: cap_pairs; os: cap_od */
    int32_t* zptr;                 /* P + 1 */
    int32_t* zcol;
    int32_t* sc_ptr;               /* nnz + 1: offsets of a block's pairs */
    int32_t* sc_optr;              /* nnz + 1: offsets of a block's odometry slots */
    uint32_t* slot_i;
    uint32_t* slot_k;
    uint32_t* os;
    int64_t nnz, pairs, od;        /* out */
    int32_t declined;              /* out: k_s0_count's overflow word; k_s0_fill was not launched */
    int32_t reserved;
} tsgo_testing_schur_out;

/* Level 0: the pattern of the explicit Schur complement with its slot-pair and odometry lists (k_s0_count, three scans, k_s0_fill) from the
 * nine arrays of host/amg.h: SchurCsr.  builder must be 1: the host's level-0 builder reads the slot tables of a whole graph, not these lists
 * (tests/test_gpu_parity.py compares the two through the engine).  Refused: pointers that do not rise from 0, a landmark outside [0, L), a
 * pose outside [0, P), an odometry neighbour that is the pose itself, slots of one pose's edge or odometry list that do not rise, and two
 * entries of ONE pose in ONE observer list whose slots do not rise (the contract the kernel's comment states). */
int tsgo_testing_schur_pattern(int32_t builder, int32_t P, int32_t L, const int32_t* pp_ptr, const int32_t* pp_lm, const uint32_t* pp_slot, const int32_t* obs_ptr,
                               const int32_t* obs_pose, const uint32_t* obs_slot, const int32_t* od_ptr, const int32_t* od_col, const uint32_t* od_slot,
                               int32_t max_pair_degree, tsgo_testing_schur_out* out);

/* The lane sums of the kernels (toyslam_amd/csrc/tsgo_kernels.h: lane_xor, group_sum, wave_sum, block_sum2) on caller-given values, in ONE
 * workgroup of 256 threads: tests/test_gpu_lane_sums.py.  No handle, no graph.  in32 / in64: 256 values, thread t holds in[t].
 * out32 / out64: 10 rows of 256, row-major, entry t of a row = what thread t got:
 *   rows 0 .. 6   group_sum<T, G>(in[t]) for G = 1, 2, 4, 8, 16, 32, 64 (masks ascending)
 *   row 7         wave_sum<T>(in[t]) (masks descending)
 *   rows 8, 9     block_sum2 of a = in[t] and b = in[255 - t]: the workgroup's sums of a and of b. */
int tsgo_testing_lane_sums(const float* in32, const double* in64, float* out32, double* out64);

#ifdef __cplusplus
}
#endif
#endif /* TSGO_TESTING_H */
