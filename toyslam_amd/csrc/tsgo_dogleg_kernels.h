// tsgo_dogleg_kernels.h — device passes of Powell's dogleg trust-region loop (tsgo_config.rules = 3, engine/engine_dogleg.inc: dogleg_loop).
//
// One linearisation and one solve serve every trial until a step is accepted: a trial step is d = c1 g + c2 d_gn with g = b the gradient
// the linearisation left, d_gn the solved Gauss-Newton step and two scalars the host derives from four numbers, g'g, g'd_gn, |d_gn|^2 and
// g'Hg.  Three passes, f64 only:
//   k_dl_gradient      once per solve: g as dense vectors gp[P][3] / gl[L][2] (a landmark's from D_l u, one 2x2 inverse per landmark here
//                      instead of one per slot in the edge pass) and the partials of g'g, g'd_gn, |d_gn|^2
//   k_dl_ghg           once per solve: g'Hg = sum over edges of w (J g)' Omega (J g), by the once-per-edge walk (tsgo_edge_walk.h) with the
//   (+ _lm_prior)      Jacobians and robust weights of the linearisation; H itself is never formed
//   k_dl_step          once per trial: estimates = snapshot (+) (c1 g + c2 d_gn)
// The snapshot (k_lm_state), the chi^2-only pass (k_chi2) and the report path are those of rules = 2 (tsgo_lm_kernels.h).  No atomics:
// per-workgroup partials, summed in a fixed order on the host in f64 like every other partial of the engine.
#pragma once
#include "tsgo_edge_walk.h"
#include "tsgo_kernels.h"

namespace tsgo {

// thread = pose and thread = landmark over one grid.  A pose's gradient is part[i][6..8] (zero at a fixed pose: zero_fixed), a landmark's
// D_l u with D_l = (D_l^-1)^-1 from lmrec[l][2..4] and u = lmrec[l][5..6] — the arithmetic of Engine::linearize's read-out; a landmark
// without edges has D_l^-1 = 0 and g = 0.  x / dl: the solved step (poses; landmarks after the back-substitution).
// red = [ g'g | g'd | d'd ], gridDim.x partials each.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_dl_gradient(int P, int L, const T* __restrict__ part, const T* __restrict__ lmrec, const T* __restrict__ x,
                                                        const T* __restrict__ dl, T* __restrict__ gp, T* __restrict__ gl, T* __restrict__ red) {
    __shared__ T sh[kWavesPerBlock];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    T gg = 0, gd = 0, dd = 0;
    if (i < P) {
        const T* b = part + (size_t)i * 18 + 6;
        const T g0 = b[0], g1 = b[1], g2 = b[2];
        const T d0 = x[(size_t)i * 3], d1 = x[(size_t)i * 3 + 1], d2 = x[(size_t)i * 3 + 2];
        gp[(size_t)i * 3] = g0; gp[(size_t)i * 3 + 1] = g1; gp[(size_t)i * 3 + 2] = g2;
        gg += g0 * g0 + g1 * g1 + g2 * g2; gd += g0 * d0 + g1 * d1 + g2 * d2; dd += d0 * d0 + d1 * d1 + d2 * d2;
    }
    if (i < L) {
        const T* lr = lmrec + (size_t)i * kLmRec;
        const auto n01 = ld2<T>(lr + 2), n2u = ld2<T>(lr + 4);
        const T u0 = n2u.y, u1 = lr[6];
        T dxx, dxy, dyy;
        inv_sym2<T>(n01.x, n01.y, n2u.x, dxx, dxy, dyy);
        const T g0 = dxx * u0 + dxy * u1, g1 = dxy * u0 + dyy * u1;
        const auto d = ld2<T>(dl + (size_t)i * 2);
        st2<T>(gl + (size_t)i * 2, g0, g1);
        gg += g0 * g0 + g1 * g1; gd += g0 * d.x + g1 * d.y; dd += d.x * d.x + d.y * d.y;
    }
    const T tgg = block_sum<T>(gg, sh);
    if (threadIdx.x == 0) red[blockIdx.x] = tgg;
    const T tgd = block_sum<T>(gd, sh);
    if (threadIdx.x == 0) red[(size_t)gridDim.x + blockIdx.x] = tgd;
    const T tdd = block_sum<T>(dd, sh);
    if (threadIdx.x == 0) red[(size_t)2 * gridDim.x + blockIdx.x] = tdd;
}

// What the lane that visits an edge adds to g'Hg: v = A g_1 + B g_2 with the Jacobians the linearisation uses for the edge's class, then
// sum_k a_k v_k^2 with a = robust weight * information, from the same edge function call (and robust_class<RK> selection) the report and
// the linearisation make (RK = 2: the byte of the visited edge, robust_at on ra.edge).  g1: the gradient of the walking lane's own pose, loaded once; a neighbour's (gp[j], gl[l]) is gathered BEHIND
// the slot's coalesced plane loads (the walk's VGPR note).  The walk hands over neither the landmark's nor the neighbour's number: the
// first is the slot's index word again (the walk has it in a register already: the same address, no store in between), the second
// follows from the record pointer.  The visitor writes nothing, so "skipped before loaded" asks nothing of it.
// classes 0 .. 3 (walk_edges_once)
template <typename T, int OJ, int RK> struct GhgVisitor {
    using Kernel = decltype(robust_class<RK>(RobustArgs<T>{}, 0));
    const Table<T>& tb;
    const Table<T>& od;
    const RobustArgs<T>& ra;
    const T* __restrict__ ps;
    const T* __restrict__ gp;
    const T* __restrict__ gl;
    const int analytic;            // OJ only: ODOM edges under the analytic Jacobians (odom_jacobians), else the constants -I / +I
    const T g1x, g1y, g1t;
    const Kernel rk_lm = robust_class<RK>(ra, kClassLm), rk_odom = robust_class<RK>(ra, kClassOdom);
    T acc = 0;
    // A = [-R^T | (ppy, -ppx)], B = R^T
    __device__ __forceinline__ void lm(uint32_t e, size_t k, const PoseAt<T>& p, T lx, T ly) {
        const LmMeas<T> z = lm_meas<T>(tb, k);
        const uint32_t l = tb.idx[k];
        const LmLin<T> o = lm_linearize<T>(p.x, p.y, p.c, p.s, lx, ly, z.zx, z.zy, z.w0, z.w1, robust_at<RK>(ra, rk_lm, ra.edge, e));
        const auto g2 = ld2<T>(gl + (size_t)l * 2);
        const T d0 = g2.x - g1x, d1 = g2.y - g1y;
        const T v0 = p.c * d0 + p.s * d1 + o.ppy * g1t, v1 = p.c * d1 - p.s * d0 - o.ppx * g1t;
        acc += o.a0 * v0 * v0 + o.a1 * v1 * v1;
    }
    // constants: A = -I, B = +I; analytic (tsgo_math.h): A = [[-M, q], [0 0 -kappa]], B = [[M, 0], [0 0 kappa]]
    __device__ __forceinline__ void odom(uint32_t e, size_t k, const PoseAt<T>& p, const T* qj) {
        const OdomMeas<T> z = odom_meas<T>(od, k);
        const PoseAt<T> pj = pose_at<T>(qj);
        const T* g2 = gp + (size_t)((qj - ps) >> 2) * 3;
        const T t0 = g2[0] - g1x, t1 = g2[1] - g1y, tt = g2[2] - g1t;
        const OdomLin<T> o = odom_linearize<T>(p.x, p.y, p.c, p.s, pj.x, pj.y, pj.c, pj.s, z.mi, z.w, robust_at<RK>(ra, rk_odom, ra.edge, e));
        T v0 = t0, v1 = t1, vt = tt;
        if (OJ && analytic) {
            const OdomJac<T> j = odom_jacobians<T>(p.x, p.y, p.c, p.s, pj.x, pj.y, pj.c, pj.s, z.mi);
            v0 = j.m00 * t0 + j.m01 * t1 + j.q0 * g1t; v1 = j.m10 * t0 + j.m11 * t1 + j.q1 * g1t; vt = j.kappa * tt;
        }
        acc += o.a[0] * v0 * v0 + o.a[1] * v1 * v1 + o.a[2] * vt * vt;
    }
    // e = T1 p1 - T2 p2: A = [I | u], B = -[I | v] (vlm_linearize: u, v)
    __device__ __forceinline__ void vlm(uint32_t e, size_t k, const PoseAt<T>& p, const T* qj) {
        const OdomMeas<T> z = odom_meas<T>(od, k);
        const PoseAt<T> pj = pose_at<T>(qj);
        const T* g2 = gp + (size_t)((qj - ps) >> 2) * 3;
        const T g2x = g2[0], g2y = g2[1], g2t = g2[2];
        const VlmLin<T> o = vlm_linearize<T>(p.x, p.y, p.c, p.s, pj.x, pj.y, pj.c, pj.s, z.mi[0], z.mi[1], z.mi[2], z.mi[3], z.w[0], z.w[1],
                                                   robust_at<RK>(ra, robust_class<RK>(ra, kClassVlm), ra.edge, e));
        const T v0 = (g1x + o.u0 * g1t) - (g2x + o.v0 * g2t), v1 = (g1y + o.u1 * g1t) - (g2y + o.v1 * g2t);
        acc += o.om0 * v0 * v0 + o.om1 * v1 * v1;
    }
    // J = blockdiag(R_m^T, 1)
    __device__ __forceinline__ void pose_prior(uint32_t e, const T* q, const PoseAt<T>& p) {
        const auto m01 = ld2<T>(q), cs = ld2<T>(q + PRI_C), w01 = ld2<T>(q + PRI_W0);
        const PosePriorLin<T> o = pose_prior_linearize<T>(m01.x, m01.y, cs.x, cs.y, w01.x, w01.y, q[PRI_W2], p.x, p.y, p.c, p.s,
                                                                    robust_at<RK>(ra, robust_class<RK>(ra, kClassPosePrior), ra.edge, e));
        const T v0 = cs.x * g1x + cs.y * g1y, v1 = cs.x * g1y - cs.y * g1x;
        acc += o.a0 * v0 * v0 + o.a1 * v1 * v1 + o.a2 * g1t * g1t;
    }
};

// class 4 (walk_lm_priors_once): J = I
template <typename T, int RK> struct GhgLmPriorVisitor {
    const RobustArgs<T>& ra;
    const T gx, gy;
    T acc = 0;
    __device__ __forceinline__ void lm_prior(uint32_t e, const T* q, T lx, T ly) {
        const auto m = ld2<T>(q + PRL_MX), w = ld2<T>(q + PRL_W0);
        const LmPriorLin<T> o = lm_prior_linearize<T>(m.x, m.y, w.x, w.y, lx, ly, robust_at<RK>(ra, robust_class<RK>(ra, kClassLmPrior), ra.edge, e));
        acc += o.a0 * gx * gx + o.a1 * gy * gy;
    }
};

// Landmark priors' share of g'Hg, one partial per workgroup into out[blockIdx.x].  Graphs with priors only.
template <typename T, int G, int RK = 0>
__global__ __launch_bounds__(kBlock) void k_dl_ghg_lm_prior(Table<T> tb, const T* __restrict__ lmrec, const uint32_t* __restrict__ pri_edge,
                                                            const T* __restrict__ gl, T* __restrict__ out, const PriorArgs<T> pa, const RobustArgs<T> ra) {
    __shared__ T sh[kWavesPerBlock];
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    const int lc = (wk.live && wk.vertex < tb.n_vertices) ? wk.vertex : 0;      // (tb.n_vertices >= 1 here: the kernel is launched for tables with slices)
    const auto g = ld2<T>(gl + (size_t)lc * 2);
    GhgLmPriorVisitor<T, RK> v{ra, g.x, g.y};
    walk_lm_priors_once<T>(wk, tb, lmrec, pri_edge, pa, v);
    const T total = block_sum<T>(v.acc, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = total;
}

// Classes 0 .. 3; G, OJ, PRI: the walk's axes, RK the robust axis, as in k_edge_report.  One partial per workgroup into out[blockIdx.x].
// The gauge term of H adds gamma_v |g_v|^2 = 0 (g is zero at fixed vertices) and has no pass.
template <typename T, int G, int OJ = 0, int PRI = 0, int RK = 0>
__global__ __launch_bounds__(kBlock) void k_dl_ghg(Table<T> tb, Table<T> od, const T* __restrict__ ps, const T* __restrict__ lmrec, const EdgeMaps maps,
                                                   const T* __restrict__ gp, const T* __restrict__ gl, T* __restrict__ out, int odom_analytic,
                                                   const PriorArgs<T> pa, const RobustArgs<T> ra) {
    __shared__ T sh[kWavesPerBlock];
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    const int ic = (wk.live && wk.vertex < tb.n_vertices) ? wk.vertex : tb.n_vertices - 1;      // a lane past the last vertex visits nothing
    const T* g1 = gp + (size_t)ic * 3;
    GhgVisitor<T, OJ, RK> v{tb, od, ra, ps, gp, gl, odom_analytic, g1[0], g1[1], g1[2]};
    walk_edges_once<T, OJ, PRI>(wk, tb, od, ps, lmrec, maps, pa, v);
    const T total = block_sum<T>(v.acc, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = total;
}

// The trial step, FROM THE SNAPSHOT (k_lm_state<T, 0>): a re-tried step does not depend on what the rejected one wrote.  Poses as
// k_pose_update_lm writes them (theta = atan2(sin, cos) + d_theta, translation added in the world frame), landmarks by plain addition.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_dl_step(int P, int L, T c1, T c2, const T* __restrict__ gp, const T* __restrict__ x, const T* __restrict__ gl,
                                                    const T* __restrict__ dl, const T* __restrict__ snap_ps, const T* __restrict__ snap_lm,
                                                    T* __restrict__ ps, T* __restrict__ theta, T* __restrict__ lmrec) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < P) {
        const T d0 = c1 * gp[(size_t)i * 3] + c2 * x[(size_t)i * 3], d1 = c1 * gp[(size_t)i * 3 + 1] + c2 * x[(size_t)i * 3 + 1];
        const T d2 = c1 * gp[(size_t)i * 3 + 2] + c2 * x[(size_t)i * 3 + 2];
        const auto s01 = ld2<T>(snap_ps + (size_t)i * 4), s23 = ld2<T>(snap_ps + (size_t)i * 4 + 2);
        const T th = atan2(s23.y, s23.x) + d2;
        st2<T>(ps + (size_t)i * 4, s01.x + d0, s01.y + d1);
        st2<T>(ps + (size_t)i * 4 + 2, cos(th), sin(th));
        theta[i] = th;
    }
    if (i < L) {
        const auto s = ld2<T>(snap_lm + (size_t)i * 2), g = ld2<T>(gl + (size_t)i * 2), d = ld2<T>(dl + (size_t)i * 2);
        st2<T>(lmrec + (size_t)i * kLmRec, s.x + (c1 * g.x + c2 * d.x), s.y + (c1 * g.y + c2 * d.y));
    }
}

}  // namespace tsgo
