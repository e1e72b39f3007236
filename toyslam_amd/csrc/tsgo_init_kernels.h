// tsgo_init_kernels.h — tsgo_init_estimates on the device (engine/engine_init.inc): pose estimates composed along
// an odometry spanning tree by pointer jumping, landmark estimates as the mean of their observations.  f64 only.
//
// One 32-byte record per pose, 32-byte aligned: a rigid transform (x, y, cos, sin).  After k_init_rel a root holds its absolute pose and
// every other pose the transform relative to its tree parent; a pass of k_init_jump composes every record with its parent's and moves its
// parent pointer to the grandparent, so after ceil(log2(depth_max + 1)) passes every record is absolute and every pointer -1.  A pass
// reads one buffer and writes the other: no atomics, no ordering between workgroups, O(P log depth) work whatever the shape of the tree.
// The only irregular access of a pass is the parent's record: one aligned 32-byte gather (two 16-byte loads from one sector) and the
// 4-byte pointer beside it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tsgo_kernels.h"

namespace tsgo {

struct __attribute__((aligned(32))) InitRec { double x, y, c, s; };
constexpr uint32_t kInitInverse = 0x80000000u;      // tree slot word: the pose is the edge's id1, its transform the inverse of the measurement's

__device__ __forceinline__ InitRec init_load(const InitRec* p) {
    const double2 a = *reinterpret_cast<const double2*>(&p->x), b = *reinterpret_cast<const double2*>(&p->c);
    return InitRec{a.x, a.y, b.x, b.y};
}
__device__ __forceinline__ void init_store(InitRec* p, const InitRec& r) {
    *reinterpret_cast<double2*>(&p->x) = make_double2(r.x, r.y);
    *reinterpret_cast<double2*>(&p->c) = make_double2(r.c, r.s);
}
// a o b: b's frame expressed in the frame a is expressed in
__device__ __forceinline__ InitRec init_compose(const InitRec& a, const InitRec& b) {
    return InitRec{a.x + a.c * b.x - a.s * b.y, a.y + a.s * b.x + a.c * b.y, a.c * b.c - a.s * b.s, a.s * b.c + a.c * b.s};
}

// Per pose (internal numbering).  tree_parent: the parent's internal number, -1 for a root.  tree_slot: a slot of the pose-pose table that
// holds the pose's tree edge (either endpoint's: both keep the same planes), with kInitInverse when the pose is the edge's id1.  The slot
// keeps rows 0-1 of M^-1 (OD_MI0 ..): M is recovered in f64 with the last row taken as (0, 0, 1), then theta = atan2(M10, M00), t = (M02, M12).
__global__ __launch_bounds__(kBlock) void k_init_rel(int P, const int* __restrict__ tree_parent, const uint32_t* __restrict__ tree_slot,
                                                     const double* __restrict__ od_st, size_t od_slots, const double* __restrict__ ps,
                                                     InitRec* __restrict__ rec, int* __restrict__ par) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P) return;
    const int p = tree_parent[i];
    InitRec r;
    if (p < 0) {
        const double2 q01 = ld2<double>(ps + (size_t)i * 4), q23 = ld2<double>(ps + (size_t)i * 4 + 2);
        r = InitRec{q01.x, q01.y, q23.x, q23.y};
    } else {
        const uint32_t w = tree_slot[i];
        const size_t k = (size_t)(w & ~kInitInverse);
        double mi[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) mi[m] = od_st[(size_t)(OD_MI0 + m) * od_slots + k];
        const double det = mi[0] * mi[4] - mi[1] * mi[3];
        const double m00 = mi[4] / det, m10 = -mi[3] / det;
        const double tx = (mi[1] * mi[5] - mi[4] * mi[2]) / det, ty = (mi[3] * mi[2] - mi[0] * mi[5]) / det;
        const double th = atan2(m10, m00), c = cos(th), s = sin(th);
        if (w & kInitInverse) r = InitRec{-(c * tx + s * ty), s * tx - c * ty, c, -s};
        else r = InitRec{tx, ty, c, s};
    }
    init_store(rec + i, r);
    par[i] = p;
}

__global__ __launch_bounds__(kBlock) void k_init_jump(int P, const InitRec* __restrict__ rec_in, const int* __restrict__ par_in,
                                                      InitRec* __restrict__ rec_out, int* __restrict__ par_out) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P) return;
    const int p = par_in[i];
    InitRec r = init_load(rec_in + i);
    int pp = -1;
    if (p >= 0) {
        pp = par_in[p];
        r = init_compose(init_load(rec_in + p), r);
    }
    init_store(rec_out + i, r);
    par_out[i] = pp;
}

// Every pose that is not a root takes its composed record, written as k_pose_update writes a pose.
__global__ __launch_bounds__(kBlock) void k_init_write(int P, const int* __restrict__ tree_parent, const InitRec* __restrict__ rec,
                                                       double* __restrict__ ps, double* __restrict__ theta) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P || tree_parent[i] < 0) return;
    const InitRec r = init_load(rec + i);
    const double th = atan2(r.s, r.c);
    double* q = ps + (size_t)i * 4;
    q[0] = r.x; q[1] = r.y; q[2] = cos(th); q[3] = sin(th);
    theta[i] = th;
}

// Per landmark, over the landmark-major LM table (G lanes a landmark): the plain mean of t_pose + R_pose z over the slots whose two weights
// are both > 0 (padding slots have zero weights and drop out by the same test).  A fixed landmark (gauge > 0) and one without such a slot
// keep their record.  counts[2 * workgroup] = landmarks written, [+ 1] = non-fixed landmarks left as they were.
template <int G>
__global__ __launch_bounds__(kBlock) void k_init_landmarks(Table<double> tb, const double* __restrict__ ps, const double* __restrict__ gauge_l,
                                                           double* __restrict__ lmrec, int* __restrict__ counts) {
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    const bool valid = wk.live && wk.vertex < tb.n_vertices;
    double sx = 0, sy = 0, n = 0;
    const uint32_t r0 = wk.live ? tb.row_off[wk.slice] : 0u, r1 = wk.live ? tb.row_off[wk.slice + 1] : 0u;
    for (uint32_t row = r0; row < r1; ++row) {
        const size_t k = (size_t)row * 64 + wk.lane;
        const uint32_t i = tb.idx[k];
        const LmMeas<double> z = lm_meas<double>(tb, k);
        const double2 q01 = ld2<double>(ps + (size_t)i * 4), q23 = ld2<double>(ps + (size_t)i * 4 + 2);
        if (z.w0 > 0.0 && z.w1 > 0.0) {
            sx += q01.x + q23.x * z.zx - q23.y * z.zy;
            sy += q01.y + q23.y * z.zx + q23.x * z.zy;
            n += 1.0;
        }
    }
    sx = group_sum<double, G>(sx); sy = group_sum<double, G>(sy); n = group_sum<double, G>(n);
    int wrote = 0, left = 0;
    if (valid && wk.head && !(gauge_l[wk.vertex] > 0.0)) {
        if (n > 0.0) { st2<double>(lmrec + (size_t)wk.vertex * kLmRec, sx / n, sy / n); wrote = 1; }
        else left = 1;
    }
    const int n_wrote = __syncthreads_count(wrote), n_left = __syncthreads_count(left);      // (every wave arrives: none left early)
    if (threadIdx.x == 0) { counts[2 * blockIdx.x] = n_wrote; counts[2 * blockIdx.x + 1] = n_left; }
}

}  // namespace tsgo
