// tsgo_leverage_kernels.h — the leverage of every edge from posterior samples (tsgo_edge_leverage, include/tsgo.h;
// engine/engine_leverage.inc).  With delta_k ~ N(0, H^-1) of tsgo_sample_marginals, y = J_e delta_k has the
// covariance C_e = J_e H^-1 J_e^T of the predicted measurement of edge e, and h_e = tr(Omega_a C_e) is the edge's leverage.  After the
// solve of a batch of NV samples, behind k_mb_schur_lm (t = Y^T X) and beside k_smp_acc_pose / k_smp_acc_lm:
//
//   k_lev_acc            classes 0 .. 3 on walk_edges_once (tsgo_edge_walk.h): one lane meets each edge once
//   k_lev_acc_lm_prior   class 4 on walk_lm_priors_once
//
// What the visiting lane does: A, B and a = w_robust * inf from the static planes and the estimates with the edge functions every
// linearisation runs (lm_linearize, odom_linearize + odom_jacobians, vlm_linearize, the prior functions; the robust kernel of the EDGE,
// robust_at on ra.edge, as the sampling kernels select it) — nothing is restated — then for every live column c < nc, ascending, the
// gathered delta of its own pose x[(i NV + c) 3], of the neighbour pose (its index from qj) or of the landmark, u - t at [(l NV + c) 2]
// read from the two buffers the solve leaves (staging delta_l would cost a pass that writes L NV 2 numbers to save one load per LM edge
// and column of a line that the pose-major walk finds in L2 anyway), y = A delta_first + B delta_second, the six products y y^T and
// sum_j a_j y_j^2 in registers, and ONE read-modify-write of acc[e] = (c00 c01 c02 c11 c12 c22 h dof_a) per batch: four pair loads and
// four pair stores of a 64-byte record.  One visit per edge, so one writer: plain stores, no atomics.  dof_a, the number of the class's
// axes with a_j > 0, is stored, not added.  The dof-2 classes add nothing to c02, c12, c22: they stay the 0 the buffer starts with.
//
// Loads.  u and t are pairs at 16-byte multiples.  A pose's delta is three numbers at (i NV + c) 24 bytes: under an even NV 16-byte
// aligned in an even column and 8 bytes past that in an odd one, so the columns are walked two at a time with one pair and one single
// load each (lev_columns, pose_delta<PAR>); NV = 1 takes three singles.  Only T = double is instantiated; RK = 1 (the class kernels,
// the default setting included) or 2, as in tsgo_sample_kernels.h.
#pragma once
#include <type_traits>

#include "tsgo_edge_walk.h"
#include "tsgo_kernels.h"

namespace tsgo {

// One batch: columns 0 .. nc - 1 of NV hold samples; x [P][NV][3], u and t [L][NV][2], acc [E][8]
template <typename T> struct LevBatch { int NV, nc; const T *x, *u, *t; T* acc; };

template <typename T> struct LevDelta { T v0, v1, v2; };
// PAR: the column's parity under an even NV, 2 under NV = 1
template <typename T, int PAR> __device__ __forceinline__ LevDelta<T> pose_delta(const T* __restrict__ x, size_t i, int NV, int c) {
    const T* p = x + (i * (size_t)NV + (size_t)c) * 3;
    if constexpr (PAR == 0) { const auto a = ld2<T>(p); return {a.x, a.y, p[2]}; }
    else if constexpr (PAR == 1) { const auto a = ld2<T>(p + 1); return {p[0], a.x, a.y}; }
    else return {p[0], p[1], p[2]};
}
// f(c, parity constant) for c = 0 .. nc - 1, ascending
template <typename F> __device__ __forceinline__ void lev_columns(int NV, int nc, F&& f) {
    if ((NV & 1) == 0) {
        for (int c = 0; c < nc; c += 2) {
            f(c, std::integral_constant<int, 0>{});
            if (c + 1 < nc) f(c + 1, std::integral_constant<int, 1>{});
        }
    } else {
        for (int c = 0; c < nc; ++c) f(c, std::integral_constant<int, 2>{});
    }
}

template <typename T> struct LevSum {
    T c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0, h = 0;
    __device__ __forceinline__ void add2(T y0, T y1, T a0, T a1) {
        c00 += y0 * y0; c01 += y0 * y1; c11 += y1 * y1;
        h += a0 * y0 * y0 + a1 * y1 * y1;
    }
    __device__ __forceinline__ void add3(T y0, T y1, T y2, T a0, T a1, T a2) {
        c00 += y0 * y0; c01 += y0 * y1; c02 += y0 * y2; c11 += y1 * y1; c12 += y1 * y2; c22 += y2 * y2;
        h += a0 * y0 * y0 + a1 * y1 * y1 + a2 * y2 * y2;
    }
};
template <typename T> __device__ __forceinline__ T lev_dof(T a0, T a1, T a2 = T(0)) { return T((a0 > T(0)) + (a1 > T(0)) + (a2 > T(0))); }
// the batch's sums into the edge's record
template <typename T> __device__ __forceinline__ void lev_store(T* __restrict__ acc, uint32_t e, const LevSum<T>& s, T dof) {
    T* q = acc + (size_t)e * 8;
    const auto q01 = ld2<T>(q), q23 = ld2<T>(q + 2), q45 = ld2<T>(q + 4), q67 = ld2<T>(q + 6);
    st2<T>(q, q01.x + s.c00, q01.y + s.c01); st2<T>(q + 2, q23.x + s.c02, q23.y + s.c11);
    st2<T>(q + 4, q45.x + s.c12, q45.y + s.c22); st2<T>(q + 6, q67.x + s.h, dof);
}

// classes 0 .. 3 (walk_edges_once); i: the visiting lane's own pose
template <typename T, int RK> struct LevVisitor {
    const Table<T>& tb;
    const Table<T>& od;
    const RobustArgs<T>& ra;
    const T* __restrict__ ps;
    const size_t i;
    const int odom_analytic;
    const LevBatch<T>& b;
    const Robust<T> rk_lm = robust_class<RK>(ra, kClassLm), rk_odom = robust_class<RK>(ra, kClassOdom);
    // A = [-R^T | (ppy, -ppx)], B = R^T
    __device__ __forceinline__ void lm(uint32_t e, size_t k, const PoseAt<T>& p, T lx, T ly) {
        const LmMeas<T> z = lm_meas<T>(tb, k);
        const size_t l = tb.idx[k];
        const LmLin<T> o = lm_linearize<T>(p.x, p.y, p.c, p.s, lx, ly, z.zx, z.zy, z.w0, z.w1, robust_at<RK>(ra, rk_lm, ra.edge, e));
        LevSum<T> s;
        lev_columns(b.NV, b.nc, [&](int c, auto par) {
            const LevDelta<T> d = pose_delta<T, decltype(par)::value>(b.x, i, b.NV, c);
            const size_t kk = (l * (size_t)b.NV + (size_t)c) * 2;
            const auto uu = ld2<T>(b.u + kk), tt = ld2<T>(b.t + kk);
            const T gx = (uu.x - tt.x) - d.v0, gy = (uu.y - tt.y) - d.v1;
            s.add2(p.c * gx + p.s * gy + o.ppy * d.v2, p.c * gy - p.s * gx - o.ppx * d.v2, o.a0, o.a1);
        });
        lev_store<T>(b.acc, e, s, lev_dof<T>(o.a0, o.a1));
    }
    // A = [[-M, q], [0 0 -kappa]], B = [[M, 0], [0 0 kappa]] (odom_jacobians); the reference's constants are M = I, q = 0, kappa = 1
    __device__ __forceinline__ void odom(uint32_t e, size_t k, const PoseAt<T>& p, const T* qj) {
        const OdomMeas<T> z = odom_meas<T>(od, k);
        const PoseAt<T> pj = pose_at<T>(qj);
        const size_t j = (size_t)(qj - ps) / 4;
        const OdomLin<T> o = odom_linearize<T>(p.x, p.y, p.c, p.s, pj.x, pj.y, pj.c, pj.s, z.mi, z.w, robust_at<RK>(ra, rk_odom, ra.edge, e));
        OdomJac<T> jac{T(1), T(0), T(0), T(1), T(0), T(0), T(1)};
        if (odom_analytic) jac = odom_jacobians<T>(p.x, p.y, p.c, p.s, pj.x, pj.y, pj.c, pj.s, z.mi);
        LevSum<T> s;
        lev_columns(b.NV, b.nc, [&](int c, auto par) {
            const LevDelta<T> d1 = pose_delta<T, decltype(par)::value>(b.x, i, b.NV, c), d2 = pose_delta<T, decltype(par)::value>(b.x, j, b.NV, c);
            const T gx = d2.v0 - d1.v0, gy = d2.v1 - d1.v1;
            s.add3(jac.m00 * gx + jac.m01 * gy + jac.q0 * d1.v2, jac.m10 * gx + jac.m11 * gy + jac.q1 * d1.v2, jac.kappa * (d2.v2 - d1.v2), o.a[0], o.a[1], o.a[2]);
        });
        lev_store<T>(b.acc, e, s, lev_dof<T>(o.a[0], o.a[1], o.a[2]));
    }
    // A = [I | u], B = -[I | v] (vlm_linearize, seen from the edge's first pose)
    __device__ __forceinline__ void vlm(uint32_t e, size_t k, const PoseAt<T>& p, const T* qj) {
        const OdomMeas<T> z = odom_meas<T>(od, k);
        const PoseAt<T> pj = pose_at<T>(qj);
        const size_t j = (size_t)(qj - ps) / 4;
        const VlmLin<T> v = vlm_linearize<T>(p.x, p.y, p.c, p.s, pj.x, pj.y, pj.c, pj.s, z.mi[0], z.mi[1], z.mi[2], z.mi[3], z.w[0], z.w[1],
                                             robust_at<RK>(ra, robust_class<RK>(ra, kClassVlm), ra.edge, e));
        LevSum<T> s;
        lev_columns(b.NV, b.nc, [&](int c, auto par) {
            const LevDelta<T> d1 = pose_delta<T, decltype(par)::value>(b.x, i, b.NV, c), d2 = pose_delta<T, decltype(par)::value>(b.x, j, b.NV, c);
            s.add2((d1.v0 + v.u0 * d1.v2) - (d2.v0 + v.v0 * d2.v2), (d1.v1 + v.u1 * d1.v2) - (d2.v1 + v.v1 * d2.v2), v.om0, v.om1);
        });
        lev_store<T>(b.acc, e, s, lev_dof<T>(v.om0, v.om1));
    }
    // A = blockdiag(R_m^T, 1)
    __device__ __forceinline__ void pose_prior(uint32_t e, const T* q, const PoseAt<T>& p) {
        const auto m01 = ld2<T>(q), cs = ld2<T>(q + PRI_C), w01 = ld2<T>(q + PRI_W0);
        const PosePriorLin<T> o = pose_prior_linearize<T>(m01.x, m01.y, cs.x, cs.y, w01.x, w01.y, q[PRI_W2], p.x, p.y, p.c, p.s,
                                                          robust_at<RK>(ra, robust_class<RK>(ra, kClassPosePrior), ra.edge, e));
        LevSum<T> s;
        lev_columns(b.NV, b.nc, [&](int c, auto par) {
            const LevDelta<T> d = pose_delta<T, decltype(par)::value>(b.x, i, b.NV, c);
            s.add3(cs.x * d.v0 + cs.y * d.v1, cs.x * d.v1 - cs.y * d.v0, d.v2, o.a0, o.a1, o.a2);
        });
        lev_store<T>(b.acc, e, s, lev_dof<T>(o.a0, o.a1, o.a2));
    }
};

// class 4 (walk_lm_priors_once): A = I; l: the visiting lane's landmark
template <typename T, int RK> struct LevLmPriorVisitor {
    const RobustArgs<T>& ra;
    const size_t l;
    const LevBatch<T>& b;
    __device__ __forceinline__ void lm_prior(uint32_t e, const T* q, T lx, T ly) {
        const auto m = ld2<T>(q + PRL_MX), w = ld2<T>(q + PRL_W0);
        const LmPriorLin<T> o = lm_prior_linearize<T>(m.x, m.y, w.x, w.y, lx, ly, robust_at<RK>(ra, robust_class<RK>(ra, kClassLmPrior), ra.edge, e));
        LevSum<T> s;
        for (int c = 0; c < b.nc; ++c) {
            const size_t kk = (l * (size_t)b.NV + (size_t)c) * 2;
            const auto uu = ld2<T>(b.u + kk), tt = ld2<T>(b.t + kk);
            s.add2(uu.x - tt.x, uu.y - tt.y, o.a0, o.a1);
        }
        lev_store<T>(b.acc, e, s, lev_dof<T>(o.a0, o.a1));
    }
};

// G, OJ, PRI: the walk's axes (under OJ a kVlmMask slot is a virtual landmark measurement); odom_analytic: the handle's odom_jacobian
template <typename T, int G, int OJ, int PRI, int RK>
__global__ __launch_bounds__(kBlock) void k_lev_acc(Table<T> tb, Table<T> od, const T* __restrict__ ps, const T* __restrict__ lmrec, const EdgeMaps maps,
                                                    const PriorArgs<T> pa, const RobustArgs<T> ra, int odom_analytic, const LevBatch<T> b) {
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    LevVisitor<T, RK> v{tb, od, ra, ps, (size_t)wk.vertex, odom_analytic, b};
    walk_edges_once<T, OJ, PRI>(wk, tb, od, ps, lmrec, maps, pa, v);
}

template <typename T, int G, int RK>
__global__ __launch_bounds__(kBlock) void k_lev_acc_lm_prior(Table<T> tb, const T* __restrict__ lmrec, const uint32_t* __restrict__ pri_edge, const PriorArgs<T> pa,
                                                             const RobustArgs<T> ra, const LevBatch<T> b) {
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    LevLmPriorVisitor<T, RK> v{ra, (size_t)wk.vertex, b};
    walk_lm_priors_once<T>(wk, tb, lmrec, pri_edge, pa, v);
}

}  // namespace tsgo
