// tsgo_sample_kernels.h — posterior samples by perturb-and-MAP (tsgo_sample_marginals, include/tsgo.h; engine/engine_sample.inc;
// DESIGN.md section 19).  Sample k solves H delta = b_k with b_k = sum_e J_e^T Omega_w,e^(1/2) xi_e + sqrt(gamma_v) xi_v, xi iid N(0, I):
// Cov(b) = H, so delta ~ N(0, H^-1).  The solve is the batched PCG of tsgo_marginal_kernels.h; this file holds what is new around it:
//
//   k_smp_rhs_lm     per landmark:  b_l of the batch's columns, stored as u_l = Dl^-1 b_l             ([L][NV][2])
//   k_smp_rhs_pose   per pose:      b_p - W u into the batch's right-hand side r                      ([P][NV][3])
//   k_smp_acc_pose / k_smp_acc_lm   after the solve: delta_p = X, delta_l = u_l - Y_l^T X (t = Y^T X from k_mb_schur_lm), second moments
//                                   added to the call's accumulators over the batch's live columns in ascending order, samples staged
//
// The two right-hand-side kernels keep the SELL shape of k_mb_schur_lm / k_mb_schur_pose (one wavefront per slice, G lanes per vertex) and
// read the slot -> input-edge maps the once-per-edge readers read (EdgeMaps, tsgo_edge_walk.h) but walk differently, at BOTH endpoints of
// an edge, so they do not use that header's walk: a slot regenerates the noise of ITS edge from
// noise(seed, 0, edge, sample) (tsgo_math.h), so an edge's noise is computed once per endpoint and never stored.  A, B and the weights
// a = w_robust * inf come from the edge functions every linearisation runs (lm_linearize, odom_linearize + odom_jacobians, vlm_linearize,
// the prior functions) with the handle's robust setting read at run time (Robust<T>; the default setting is Huber 1.5, the arithmetic of
// the compile-time kernel bit for bit).  Everything is recomputed from the static planes, so the layout of the dynamic ones (three planes
// or the general eight) does not enter and neither kernel has an OJ / PRI axis.  RK = 1 (the default: the class kernels) or 2
// (tsgo_set_edge_robust: the byte of the slot's input edge, robust_at on ra.edge — the edge index is in a register for the noise anyway).
//
// Single writer, no atomics: a vertex's sums stay in its G lanes (group_sum, a fixed xor order), its head lane adds the priors and the
// gauge term in input order and writes the vertex's entries of every column.  Columns are walked CH at a time with the accumulators in
// fully unrolled register arrays; a wider batch re-walks the (cache-resident) slots per chunk.  Padding columns of a part-filled batch
// (c >= nc) get a zero right-hand side, which k_mb_start finishes at once.  Only T = double is instantiated.
#pragma once
#include "tsgo_marginal_kernels.h"

namespace tsgo {

// One batch: samples k0 .. k0 + nc - 1 in columns 0 .. nc - 1 of NV
struct SampleBatch { SampleSeed seed; int k0, nc, NV; };

constexpr uint32_t kNoiseEdge = 0u, kNoiseGauge = 1u;      // noise() tags

template <typename T, int G, int CH, int RK = 1>
__global__ __launch_bounds__(kBlock) void k_smp_rhs_lm(Table<T> tb, const T* __restrict__ ps, const T* __restrict__ lmrec, const uint32_t* __restrict__ lm_edge,
                                                       const uint32_t* __restrict__ pl_edge, const int* __restrict__ lm_vertex, const T* __restrict__ gauge_l,
                                                       const PriorArgs<T> pa, const RobustArgs<T> ra, const SampleBatch sb, T* __restrict__ u) {
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    if (!wk.live) return;
    const int slice = wk.slice, lane = wk.lane, l = wk.vertex;
    const bool valid = l < tb.n_vertices;
    const int lc = valid ? l : tb.n_vertices - 1;
    const T* lr = lmrec + (size_t)lc * kLmRec;
    const T lx = lr[0], ly = lr[1];
    const Robust<T> rk_lm{ra.kind[kClassLm], ra.delta[kClassLm]}, rk_lp{ra.kind[kClassLmPrior], ra.delta[kClassLmPrior]};
    const uint32_t r0 = tb.row_off[slice], r1 = tb.row_off[slice + 1];
    for (int c0 = 0; c0 < sb.NV; c0 += CH) {
        T acc[CH][2];
#pragma unroll
        for (int j = 0; j < CH; ++j) { acc[j][0] = 0; acc[j][1] = 0; }
        if (c0 < sb.nc) {      // wave-uniform
            for (uint32_t row = r0; row < r1; ++row) {
                const size_t k = (size_t)row * 64 + lane;
                const uint32_t e = lm_edge[k];
                if (e == kNoEdge) continue;      // padding
                const uint32_t i = tb.idx[k];
                const LmMeas<T> z = lm_meas<T>(tb, k);
                const auto q01 = ld2<T>(ps + (size_t)i * 4), q23 = ld2<T>(ps + (size_t)i * 4 + 2);
                const T c = q23.x, s = q23.y;
                const LmLin<T> o = lm_linearize<T>(q01.x, q01.y, c, s, lx, ly, z.zx, z.zy, z.w0, z.w1, robust_at<RK>(ra, rk_lm, ra.edge, e));
                const T sa0 = sqrt(o.a0), sa1 = sqrt(o.a1);
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    if (c0 + j < sb.nc) {
                        double n0, n1;
                        sample_noise2(sb.seed, kNoiseEdge, e, (uint32_t)(sb.k0 + c0 + j), n0, n1);
                        const T h0 = sa0 * (T)n0, h1 = sa1 * (T)n1;      // B^T eta = R eta
                        acc[j][0] += c * h0 - s * h1; acc[j][1] += s * h0 + c * h1;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) { acc[j][0] = group_sum<T, G>(acc[j][0]); acc[j][1] = group_sum<T, G>(acc[j][1]); }
        if (valid && wk.head) {
            const T ixx = lr[2], ixy = lr[3], iyy = lr[4];
            const T ga = gauge_l[l];
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                if (c0 + j >= sb.NV) continue;
                T b0 = acc[j][0], b1 = acc[j][1];
                if (c0 + j < sb.nc) {
                    const uint32_t ks = (uint32_t)(sb.k0 + c0 + j);
                    if (pa.off) {
                        for (uint32_t k = pa.off[l]; k < pa.off[l + 1]; ++k) {      // landmark priors: A = I
                            const T* q = pa.rec + (size_t)k * PRI_LM_REC;
                            const auto m = ld2<T>(q + PRL_MX), w = ld2<T>(q + PRL_W0);
                            const LmPriorLin<T> o = lm_prior_linearize<T>(m.x, m.y, w.x, w.y, lx, ly, robust_at<RK>(ra, rk_lp, ra.edge, pl_edge[k]));
                            double n0, n1;
                            sample_noise2(sb.seed, kNoiseEdge, pl_edge[k], ks, n0, n1);
                            b0 += sqrt(o.a0) * (T)n0; b1 += sqrt(o.a1) * (T)n1;
                        }
                    }
                    if (ga > T(0)) {
                        double n0, n1;
                        sample_noise2(sb.seed, kNoiseGauge, (uint32_t)lm_vertex[l], ks, n0, n1);
                        const T sg = sqrt(ga);
                        b0 += sg * (T)n0; b1 += sg * (T)n1;
                    }
                }
                st2<T>(u + ((size_t)l * sb.NV + c0 + j) * 2, ixx * b0 + ixy * b1, ixy * b0 + iyy * b1);
            }
        }
    }
}

template <typename T, int G, int CH, int RK = 1>
__global__ __launch_bounds__(kBlock) void k_smp_rhs_pose(Table<T> tb, Table<T> od, const T* __restrict__ ps, const T* __restrict__ lmrec,
                                                         const uint32_t* __restrict__ lm_edge, const uint32_t* __restrict__ od_edge,
                                                         const uint32_t* __restrict__ pp_edge, const int* __restrict__ pose_vertex,
                                                         const T* __restrict__ gauge_p, const T* __restrict__ u, const PriorArgs<T> pa, const RobustArgs<T> ra,
                                                         int odom_analytic, const SampleBatch sb, T* __restrict__ r) {
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    if (!wk.live) return;
    const int slice = wk.slice, lane = wk.lane, i = wk.vertex;
    const bool valid = i < tb.n_vertices;
    const int ic = valid ? i : tb.n_vertices - 1;
    const auto p01 = ld2<T>(ps + (size_t)ic * 4), p23 = ld2<T>(ps + (size_t)ic * 4 + 2);
    const T x0 = p01.x, y0 = p01.y, c = p23.x, s = p23.y;
    const Robust<T> rk_lm{ra.kind[kClassLm], ra.delta[kClassLm]}, rk_odom{ra.kind[kClassOdom], ra.delta[kClassOdom]};
    const Robust<T> rk_vlm{ra.kind[kClassVlm], ra.delta[kClassVlm]}, rk_pp{ra.kind[kClassPosePrior], ra.delta[kClassPosePrior]};
    const uint32_t lr0 = tb.row_off[slice], lr1 = tb.row_off[slice + 1], or0 = od.row_off[slice], or1 = od.row_off[slice + 1];
    for (int c0 = 0; c0 < sb.NV; c0 += CH) {
        T acc[CH][3];
#pragma unroll
        for (int j = 0; j < CH; ++j) { acc[j][0] = 0; acc[j][1] = 0; acc[j][2] = 0; }
        if (c0 < sb.nc) {      // wave-uniform
            for (uint32_t row = lr0; row < lr1; ++row) {
                const size_t k = (size_t)row * 64 + lane;
                const uint32_t e = lm_edge[k];
                if (e == kNoEdge) continue;
                const uint32_t l = tb.idx[k];
                const LmMeas<T> z = lm_meas<T>(tb, k);
                const auto l01 = ld2<T>(lmrec + (size_t)l * kLmRec);
                const LmLin<T> o = lm_linearize<T>(x0, y0, c, s, l01.x, l01.y, z.zx, z.zy, z.w0, z.w1, robust_at<RK>(ra, rk_lm, ra.edge, e));
                const T sa0 = sqrt(o.a0), sa1 = sqrt(o.a1);
                const T* ul = u + ((size_t)l * sb.NV + c0) * 2;
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    if (c0 + j < sb.nc) {
                        double n0, n1;
                        sample_noise2(sb.seed, kNoiseEdge, e, (uint32_t)(sb.k0 + c0 + j), n0, n1);
                        const auto uu = ld2<T>(ul + 2 * j);
                        // A^T eta - W_il u_l with A = [-R^T | (ppy, -ppx)], W_il = A^T diag(a) R^T: A^T (eta - diag(a) R^T u)
                        const T m0 = sa0 * (T)n0 - o.a0 * (c * uu.x + s * uu.y), m1 = sa1 * (T)n1 - o.a1 * (c * uu.y - s * uu.x);
                        acc[j][0] -= c * m0 - s * m1; acc[j][1] -= s * m0 + c * m1; acc[j][2] += o.ppy * m0 - o.ppx * m1;
                    }
                }
            }
            for (uint32_t row = or0; row < or1; ++row) {
                const size_t k = (size_t)row * 64 + lane;
                const uint32_t e = od_edge[k];
                if (e == kNoEdge) continue;
                const uint32_t raw = od.idx[k];
                const bool second = (raw & kDirMask) != 0;
                const uint32_t jn = raw & kPoseIdxMask;
                const OdomMeas<T> z = odom_meas<T>(od, k);
                const auto j01 = ld2<T>(ps + (size_t)jn * 4), j23 = ld2<T>(ps + (size_t)jn * 4 + 2);
                const T xj = j01.x, yj = j01.y, cj = j23.x, sj = j23.y;
                if (raw & kVlmMask) {      // e = T1 p1 - T2 p2: [I | u] at the first endpoint, -[I | u] at the second, u of the slot's own pose
                    const VlmLin<T> v = vlm_linearize<T>(x0, y0, c, s, xj, yj, cj, sj, z.mi[0], z.mi[1], z.mi[2], z.mi[3], z.w[0], z.w[1], robust_at<RK>(ra, rk_vlm, ra.edge, e));
                    const T sg = second ? T(-1) : T(1), s0 = sg * sqrt(v.om0), s1 = sg * sqrt(v.om1);
#pragma unroll
                    for (int j = 0; j < CH; ++j) {
                        if (c0 + j < sb.nc) {
                            double n0, n1;
                            sample_noise2(sb.seed, kNoiseEdge, e, (uint32_t)(sb.k0 + c0 + j), n0, n1);
                            const T h0 = s0 * (T)n0, h1 = s1 * (T)n1;
                            acc[j][0] += h0; acc[j][1] += h1; acc[j][2] += v.u0 * h0 + v.u1 * h1;
                        }
                    }
                    continue;
                }
                const Robust<T> rk_slot = robust_at<RK>(ra, rk_odom, ra.edge, e);
                const OdomLin<T> o = second ? odom_linearize<T>(xj, yj, cj, sj, x0, y0, c, s, z.mi, z.w, rk_slot)
                                            : odom_linearize<T>(x0, y0, c, s, xj, yj, cj, sj, z.mi, z.w, rk_slot);
                const T sa0 = sqrt(o.a[0]), sa1 = sqrt(o.a[1]), sa2 = sqrt(o.a[2]);
                // A = [[-M, q], [0 0 -kappa]], B = [[M, 0], [0 0 kappa]] (odom_jacobians); the reference's constants are M = I, q = 0, kappa = 1
                OdomJac<T> jac{T(1), T(0), T(0), T(1), T(0), T(0), T(1)};
                if (odom_analytic) jac = second ? odom_jacobians<T>(xj, yj, cj, sj, x0, y0, c, s, z.mi) : odom_jacobians<T>(x0, y0, c, s, xj, yj, cj, sj, z.mi);
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    if (c0 + j < sb.nc) {
                        double n0, n1, n2;
                        sample_noise3(sb.seed, kNoiseEdge, e, (uint32_t)(sb.k0 + c0 + j), n0, n1, n2);
                        const T h0 = sa0 * (T)n0, h1 = sa1 * (T)n1, h2 = sa2 * (T)n2;
                        const T t0 = jac.m00 * h0 + jac.m10 * h1, t1 = jac.m01 * h0 + jac.m11 * h1;      // M^T eta_t
                        if (second) { acc[j][0] += t0; acc[j][1] += t1; acc[j][2] += jac.kappa * h2; }
                        else { acc[j][0] -= t0; acc[j][1] -= t1; acc[j][2] += jac.q0 * h0 + jac.q1 * h1 - jac.kappa * h2; }
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) { acc[j][0] = group_sum<T, G>(acc[j][0]); acc[j][1] = group_sum<T, G>(acc[j][1]); acc[j][2] = group_sum<T, G>(acc[j][2]); }
        if (valid && wk.head) {
            const T ga = gauge_p[i];
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                if (c0 + j >= sb.NV) continue;
                T b0 = acc[j][0], b1 = acc[j][1], b2 = acc[j][2];
                if (c0 + j < sb.nc) {
                    const uint32_t ks = (uint32_t)(sb.k0 + c0 + j);
                    if (pa.off) {
                        for (uint32_t k = pa.off[i]; k < pa.off[i + 1]; ++k) {      // pose priors: A = blockdiag(R_m^T, 1)
                            const T* q = pa.rec + (size_t)k * PRI_POSE_REC;
                            const auto m01 = ld2<T>(q), cs = ld2<T>(q + PRI_C), w01 = ld2<T>(q + PRI_W0);
                            const PosePriorLin<T> o = pose_prior_linearize<T>(m01.x, m01.y, cs.x, cs.y, w01.x, w01.y, q[PRI_W2], x0, y0, c, s, robust_at<RK>(ra, rk_pp, ra.edge, pp_edge[k]));
                            double n0, n1, n2;
                            sample_noise3(sb.seed, kNoiseEdge, pp_edge[k], ks, n0, n1, n2);
                            const T h0 = sqrt(o.a0) * (T)n0, h1 = sqrt(o.a1) * (T)n1;
                            b0 += cs.x * h0 - cs.y * h1; b1 += cs.y * h0 + cs.x * h1; b2 += sqrt(o.a2) * (T)n2;
                        }
                    }
                    if (ga > T(0)) {
                        double n0, n1, n2;
                        sample_noise3(sb.seed, kNoiseGauge, (uint32_t)pose_vertex[i], ks, n0, n1, n2);
                        const T sg = sqrt(ga);
                        b0 += sg * (T)n0; b1 += sg * (T)n1; b2 += sg * (T)n2;
                    }
                }
                T* ri = r + ((size_t)i * sb.NV + c0 + j) * 3;
                ri[0] = b0; ri[1] = b1; ri[2] = b2;
            }
        }
    }
}

// ---- read-out: one thread per vertex, the batch's live columns in ascending order -----------------------------------------------------
// acc_p[i] = (00 01 02 11 12 22) of sum delta delta^T, acc_l[l] = (00 01 11); stage (may be null): [nc][V][3] at the vertex's position in
// the request's vertex arrays, a landmark's third entry 0.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_smp_acc_pose(int P, int NV, int nc, const T* __restrict__ x, const int* __restrict__ pose_vertex,
                                                         int64_t V, T* __restrict__ acc_p, double* __restrict__ stage) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= P) return;
    T* a = acc_p + (size_t)i * 6;
    T a00 = a[0], a01 = a[1], a02 = a[2], a11 = a[3], a12 = a[4], a22 = a[5];
    const size_t v = (size_t)pose_vertex[i];
    for (int c = 0; c < nc; ++c) {
        const T* xi = x + ((size_t)i * NV + c) * 3;
        const T d0 = xi[0], d1 = xi[1], d2 = xi[2];
        a00 += d0 * d0; a01 += d0 * d1; a02 += d0 * d2; a11 += d1 * d1; a12 += d1 * d2; a22 += d2 * d2;
        if (stage) { double* o = stage + ((size_t)c * (size_t)V + v) * 3; o[0] = (double)d0; o[1] = (double)d1; o[2] = (double)d2; }
    }
    a[0] = a00; a[1] = a01; a[2] = a02; a[3] = a11; a[4] = a12; a[5] = a22;
}

// delta_l = u_l - t_l, t = Dl^-1 W_l^T X = Y_l^T X (k_mb_schur_lm over the landmark's own slots)
template <typename T>
__global__ __launch_bounds__(kBlock) void k_smp_acc_lm(int L, int NV, int nc, const T* __restrict__ u, const T* __restrict__ t, const int* __restrict__ lm_vertex,
                                                       int64_t V, T* __restrict__ acc_l, double* __restrict__ stage) {
    const int l = blockIdx.x * kBlock + threadIdx.x;
    if (l >= L) return;
    T* a = acc_l + (size_t)l * 3;
    T a00 = a[0], a01 = a[1], a11 = a[2];
    const size_t v = (size_t)lm_vertex[l];
    for (int c = 0; c < nc; ++c) {
        const size_t k = ((size_t)l * NV + c) * 2;
        const T d0 = u[k] - t[k], d1 = u[k + 1] - t[k + 1];
        a00 += d0 * d0; a01 += d0 * d1; a11 += d1 * d1;
        if (stage) { double* o = stage + ((size_t)c * (size_t)V + v) * 3; o[0] = (double)d0; o[1] = (double)d1; o[2] = 0.0; }
    }
    a[0] = a00; a[1] = a01; a[2] = a11;
}

}  // namespace tsgo
