// tsgo_lm_kernels.h — device passes of the Levenberg-Marquardt loop (tsgo_config.rules = 2, engine/engine_solve.inc: lm_loop).
//
// A trial needs three things the Gauss-Newton loops do not: the robustified chi^2 at the trial point WITHOUT a linearisation (k_chi2), the
// decrease the quadratic model predicts for the solved step (k_pose_update_lm for the poses; the landmarks' share rides in the
// back-substitution, k_schur_lm<.., 2>), and a way back when the step is refused (k_lm_state).  No atomics: per-workgroup partials, summed in
// a fixed order on the host in f64 like every other partial of the engine.
#pragma once
#include "tsgo_kernels.h"

namespace tsgo {

// chi^2 of the landmark priors (edge type 4), one partial per workgroup into pa.lm_chi: the landmark -> lane -> workgroup map and the order
// of the sums are k_lin_lm<.., 1>'s, so that k_chi2 below folds the same partials the linearisation would.  Graphs with priors only.
template <typename T, int G, int RK = 0>
__global__ __launch_bounds__(kBlock) void k_chi2_lm_prior(Table<T> tb, const T* __restrict__ lmrec, const PriorArgs<T> pa, const RobustArgs<T> ra) {
    __shared__ T red[kWavesPerBlock];
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    const int l = wk.vertex;
    T chi = 0;
    if (wk.live && l < tb.n_vertices && wk.head) {
        const T lx = lmrec[(size_t)l * kLmRec], ly = lmrec[(size_t)l * kLmRec + 1];
        for (uint32_t k = pa.off[l]; k < pa.off[l + 1]; ++k) {
            const T* q = pa.rec + (size_t)k * PRI_LM_REC;
            const auto m = ld2<T>(q + PRL_MX), w = ld2<T>(q + PRL_W0);
            chi += lm_prior_linearize<T>(m.x, m.y, w.x, w.y, lx, ly, robust_at<RK>(ra, robust_class<RK>(ra, kClassLmPrior), ra.lm_prior, k)).rho;
        }
    }
    const T total = block_sum<T>(chi, red);
    if (threadIdx.x == 0) pa.lm_chi[blockIdx.x] = total;
}

// Robustified chi^2 at the current estimates, without a linearisation: estimates, measurements and weights are read (16 B of a landmark
// record instead of 56), no Jacobian product is formed and one number per workgroup is written.  The chi^2 of an accepted trial point has
// to BE the chi^2 the next linearisation (k_lin_lm, k_lin_pose) reports.  By construction: the walk position (walk_of), the slot loads
// (lm_meas, odom_meas) and the per-edge arithmetic (lm_linearize, odom_linearize, vlm_linearize, pose_prior_linearize,
// lm_prior_linearize) are the ones k_lin_pose calls.  Still a convention kept by hand in both kernels: rows in table order, a pose-pose
// slot (listed at both endpoints) counted at the edge's first, a vertex's priors folded by its head lane after its rows, the landmark
// priors' partials added by workgroup 0.  OJ = 1: virtual landmark slots (kVlmMask); the ODOM residual is the same under either Jacobians.
// RK (RobustArgs, tsgo_kernels.h): the same class -> kernel selection as k_lin_lm / k_lin_pose, through the same edge functions, so the rule
// above holds under every robust kernel the handle is given; RK = 2 reads the same per-slot and per-record bytes as k_lin_pose (robust_at).
template <typename T, int G, int OJ = 0, int PRI = 0, int RK = 0>
__global__ __launch_bounds__(kBlock) void k_chi2(Table<T> tb, Table<T> od, const T* __restrict__ ps, const T* __restrict__ lmrec,
                                                 T* __restrict__ chi_part, const PriorArgs<T> pa, const RobustArgs<T> ra) {
    __shared__ T red[kWavesPerBlock];
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    const int slice = wk.slice, lane = wk.lane, i = wk.vertex;
    const bool valid = wk.live && i < tb.n_vertices;
    const auto rk_lm = robust_class<RK>(ra, kClassLm), rk_odom = robust_class<RK>(ra, kClassOdom);
    T chi = 0;
    if (wk.live) {
        const int ic = valid ? i : tb.n_vertices - 1;
        const auto q01 = ld2<T>(ps + (size_t)ic * 4), q23 = ld2<T>(ps + (size_t)ic * 4 + 2);
        const T x0 = q01.x, y0 = q01.y, c = q23.x, s = q23.y;
#pragma unroll 2
        for (uint32_t row = tb.row_off[slice], r1 = tb.row_off[slice + 1]; row < r1; ++row) {
            const size_t k = (size_t)row * 64 + lane;
            const uint32_t l = tb.idx[k];
            const LmMeas<T> z = lm_meas<T>(tb, k);
            const auto l01 = ld2<T>(lmrec + (size_t)l * kLmRec);
            chi += lm_linearize<T>(x0, y0, c, s, l01.x, l01.y, z.zx, z.zy, z.w0, z.w1, robust_at<RK>(ra, rk_lm, ra.by_pose, k)).rho;
        }
        for (uint32_t row = od.row_off[slice], r1 = od.row_off[slice + 1]; row < r1; ++row) {
            const size_t k = (size_t)row * 64 + lane;
            const uint32_t raw = od.idx[k];
            if (raw & kDirMask) continue;      // the edge's second endpoint: counted at the first
            const uint32_t j = raw & kPoseIdxMask;
            const OdomMeas<T> z = odom_meas<T>(od, k);
            const auto j01 = ld2<T>(ps + (size_t)j * 4), j23 = ld2<T>(ps + (size_t)j * 4 + 2);
            if (OJ && (raw & kVlmMask)) chi += vlm_linearize<T>(x0, y0, c, s, j01.x, j01.y, j23.x, j23.y, z.mi[0], z.mi[1], z.mi[2], z.mi[3], z.w[0], z.w[1], robust_at<RK>(ra, robust_class<RK>(ra, kClassVlm), ra.odom, k)).rho;
            else chi += odom_linearize<T>(x0, y0, c, s, j01.x, j01.y, j23.x, j23.y, z.mi, z.w, robust_at<RK>(ra, rk_odom, ra.odom, k)).rho;      // a padding slot has w = 0: rho = 0
        }
        if constexpr (PRI != 0) {
            if (valid && wk.head)
                for (uint32_t k = pa.off[i]; k < pa.off[i + 1]; ++k) {
                    const T* q = pa.rec + (size_t)k * PRI_POSE_REC;
                    const auto m01 = ld2<T>(q), cs = ld2<T>(q + PRI_C), w01 = ld2<T>(q + PRI_W0);
                    chi += pose_prior_linearize<T>(m01.x, m01.y, cs.x, cs.y, w01.x, w01.y, q[PRI_W2], x0, y0, c, s, robust_at<RK>(ra, robust_class<RK>(ra, kClassPosePrior), ra.pose_prior, k)).rho;
                }
        }
    }
    if constexpr (PRI != 0) {
        if (blockIdx.x == 0) for (int k = threadIdx.x; k < pa.n_lm_chi; k += kBlock) chi += pa.lm_chi[k];
    }
    const T total = block_sum<T>(chi, red);
    if (threadIdx.x == 0) chi_part[blockIdx.x] = total;
}

// The estimates a trial may have to return to: pose records (x, y, cos, sin), theta and the landmark positions (the first two numbers of a
// landmark record; the rest of it belongs to the linearisation, which is redone after a rejection anyway).  RESTORE = 0: estimates -> snapshot,
// 1: snapshot -> estimates; plain copies, so the restored estimates are bit for bit what they were.
template <typename T, int RESTORE>
__global__ __launch_bounds__(kBlock) void k_lm_state(int P, int L, T* __restrict__ ps, T* __restrict__ theta, T* __restrict__ lmrec,
                                                     T* __restrict__ snap_ps, T* __restrict__ snap_theta, T* __restrict__ snap_lm) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < P) {
        T* a = ps + (size_t)i * 4; T* b = snap_ps + (size_t)i * 4;
        if (RESTORE) { const auto v0 = ld2<T>(b), v1 = ld2<T>(b + 2); st2<T>(a, v0.x, v0.y); st2<T>(a + 2, v1.x, v1.y); theta[i] = snap_theta[i]; }
        else { const auto v0 = ld2<T>(a), v1 = ld2<T>(a + 2); st2<T>(b, v0.x, v0.y); st2<T>(b + 2, v1.x, v1.y); snap_theta[i] = theta[i]; }
    }
    if (i < L) {
        T* a = lmrec + (size_t)i * kLmRec; T* b = snap_lm + (size_t)i * 2;
        if (RESTORE) { const auto v = ld2<T>(b); st2<T>(a, v.x, v.y); }
        else { const auto v = ld2<T>(a); st2<T>(b, v.x, v.y); }
    }
}

// k_pose_update with the full step of a trial (pose += delta, VertexSe2::Update as there), and in the same pass the poses' share of the
// predicted decrease: b_p^T d + lambda |d|^2 with b_p as the linearisation left it in part[i][6..8] (zero at a fixed pose).
template <typename T>
__global__ __launch_bounds__(kBlock) void k_pose_update_lm(int P, const T* __restrict__ x, T* __restrict__ ps, T* __restrict__ theta,
                                                           const T* __restrict__ part, T lambda, T* __restrict__ norm_part, T* __restrict__ pred_part) {
    __shared__ T red[kWavesPerBlock];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    T nrm = 0, prd = 0;
    if (i < P) {
        const T d0 = x[(size_t)i * 3], d1 = x[(size_t)i * 3 + 1], d2 = x[(size_t)i * 3 + 2];
        const T* b = part + (size_t)i * 18 + 6;
        nrm = d0 * d0 + d1 * d1 + d2 * d2;
        prd = b[0] * d0 + b[1] * d1 + b[2] * d2 + lambda * nrm;
        T* q = ps + (size_t)i * 4;
        const T th = atan2(q[3], q[2]) + d2;
        q[0] += d0; q[1] += d1; q[2] = cos(th); q[3] = sin(th);
        theta[i] = th;
    }
    const T total = block_sum<T>(nrm, red);
    if (threadIdx.x == 0) norm_part[blockIdx.x] = total;
    const T tp = block_sum<T>(prd, red);
    if (threadIdx.x == 0) pred_part[blockIdx.x] = tp;
}

}  // namespace tsgo
