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

#ifdef __cplusplus
}
#endif
#endif /* TSGO_TESTING_H */
