// tsgo_gate_kernels.h — tsgo_gate_edges (include/tsgo.h; engine/engine_gate.inc): candidate edges tested against
// the joint marginal of their vertices, d2 = e^T S^-1 e with S = J Sigma J^T + Omega^-1.
//
// The columns of Sigma come from the batched solve of tsgo_marginal_kernels.h, and the rows against a batch's columns from the unchanged
// k_mb_joint on a per-batch item list.  The two kernels here do the rest:
//   k_gate_scatter   after every batch: moves (row, column) entries of k_mb_joint's [rows][NV] slice into sig[K][6][6], the pair block of
//                    every candidate that has a vertex among the batch's columns.  Slot 0 of a candidate (its first vertex) owns rows and
//                    columns 0 .. 2, slot 1 rows and columns 3 .. 5; a landmark uses two of its three, a unary candidate slot 0 only.
//   k_gate_eval      once, at the end: one thread per candidate, everything in registers.
// Every entry of sig is written by exactly one thread of one batch (a column of Sigma is solved once), with plain stores: no atomics, a
// repeated call gives the same bits.  f64 throughout (tsgo_gate_edges refuses f32 handles; the f32 instantiation exists to compile).
#pragma once
#include "tsgo_marginal_kernels.h"

namespace tsgo {

// One candidate, prepared on the host with the functions build_problem uses for graph edges: m = the top two rows of meas^-1 (ODOM), (zx, zy)
// (LM), (p1x, p1y, p2x, p2y) (virtual landmark), (mx, my, cos, sin) (pose prior), (mx, my) (landmark prior); w = the raw information diagonal.
// i0, i1: internal pose / landmark numbers (i1 = i0 for a unary type).
template <typename T> struct GateCand { int type, i0, i1, pad; T m[6]; T w[3]; T pad2; };
// (GateJob, one candidate's visit in one batch: host/batch_plan.h)

constexpr int kGateSig = 36;      // doubles per candidate: the 6 x 6 pair block
constexpr int kGateRec = 8;       // (e0, e1, e2, s, d2, dof, logdet, status)

// kind (0 pose, 1 landmark, -1 none) of a candidate's slot
__host__ __device__ __forceinline__ int gate_slot_kind(int type, int slot) {
    if (slot == 0) return type == kClassLmPrior ? 1 : 0;
    return type == kClassLm ? 1 : (type == kClassOdom || type == kClassVlm ? 0 : -1);
}

// One thread per (job, batch column).  cols: the batch's columns (kind -1 = padding of a part-filled batch); slice: k_mb_joint's output.
template <typename T, int NV>
__global__ __launch_bounds__(kBlock) void k_gate_scatter(int n_jobs, const GateJob* __restrict__ jobs, const GateCand<T>* __restrict__ cands,
                                                         const MbColumn* __restrict__ cols, const double* __restrict__ slice, double* __restrict__ sig) {
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_jobs * NV) return;
    const int c = t % NV;
    const MbColumn col = cols[c];
    if (col.kind < 0) return;
    const GateJob job = jobs[t / NV];
    const GateCand<T>& cd = cands[job.cand];
    const int type = cd.type;
    double* s = sig + (size_t)job.cand * kGateSig;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
        if (col.kind != gate_slot_kind(type, sb) || col.idx != (sb ? cd.i1 : cd.i0)) continue;
        const int cpos = 3 * sb + col.comp;
#pragma unroll
        for (int sa = 0; sa < 2; ++sa) {
            const int ka = gate_slot_kind(type, sa);
            if (ka < 0) continue;
            const int r0 = sa ? job.r1 : job.r0, na = ka == 0 ? 3 : 2;
            for (int a = 0; a < na; ++a) s[(3 * sa + a) * 6 + cpos] = slice[(size_t)(r0 + a) * NV + c];
        }
    }
}

// Residual and Jacobians J = [A | B] (3 x 6: A in columns 0 .. 2, B in 3 .. 5; rows beyond dof and columns a vertex does not have are 0)
// of one candidate at the current estimates, by the edge functions of tsgo_math.h; the record's (e, s) by edge_record, as tsgo_edge_report
// writes them.  The candidate itself is not robustified.  Every type writes all three rows whole, so that the entries stay scalars
// (registers) through the branches.
template <typename T>
__device__ __forceinline__ void gate_linearize(const GateCand<T>& cd, const T* __restrict__ ps, const T* __restrict__ lmrec, EdgeRecord<T>& r, T J[3][6], int& dof) {
    const Robust<T> rk{kRobustNone, T(1)};
    const T z = T(0), one = T(1);
    auto row = [&](int a, T j0, T j1, T j2, T j3, T j4, T j5) { J[a][0] = j0; J[a][1] = j1; J[a][2] = j2; J[a][3] = j3; J[a][4] = j4; J[a][5] = j5; };
    const T* m = cd.m;
    if (cd.type == kClassLmPrior) {
        const auto l01 = ld2<T>(lmrec + (size_t)cd.i0 * kLmRec);
        r = edge_record<T>(lm_prior_linearize<T>(m[0], m[1], cd.w[0], cd.w[1], l01.x, l01.y, rk), cd.w[0], cd.w[1], rk);
        row(0, one, z, z, z, z, z);
        row(1, z, one, z, z, z, z);
        row(2, z, z, z, z, z, z);
        dof = 2;
        return;
    }
    const auto p01 = ld2<T>(ps + (size_t)cd.i0 * 4), p23 = ld2<T>(ps + (size_t)cd.i0 * 4 + 2);
    const T x = p01.x, y = p01.y, c = p23.x, s = p23.y;
    if (cd.type == kClassPosePrior) {
        r = edge_record<T>(pose_prior_linearize<T>(m[0], m[1], m[2], m[3], cd.w[0], cd.w[1], cd.w[2], x, y, c, s, rk), cd.w[0], cd.w[1], cd.w[2], rk);
        row(0, m[2], m[3], z, z, z, z);       // blockdiag(R_m^T, 1)
        row(1, -m[3], m[2], z, z, z, z);
        row(2, z, z, one, z, z, z);
        dof = 3;
        return;
    }
    if (cd.type == kClassLm) {
        const auto l01 = ld2<T>(lmrec + (size_t)cd.i1 * kLmRec);
        const LmLin<T> o = lm_linearize<T>(x, y, c, s, l01.x, l01.y, m[0], m[1], cd.w[0], cd.w[1], rk);
        r = edge_record<T>(o, cd.w[0], cd.w[1], rk);
        row(0, -c, -s, o.ppy, c, s, z);       // A = [-R^T | (ppy, -ppx)], B = R^T
        row(1, s, -c, -o.ppx, -s, c, z);
        row(2, z, z, z, z, z, z);
        dof = 2;
        return;
    }
    const auto n01 = ld2<T>(ps + (size_t)cd.i1 * 4), n23 = ld2<T>(ps + (size_t)cd.i1 * 4 + 2);
    if (cd.type == kClassVlm) {
        const VlmLin<T> o = vlm_linearize<T>(x, y, c, s, n01.x, n01.y, n23.x, n23.y, m[0], m[1], m[2], m[3], cd.w[0], cd.w[1], rk);
        r = edge_record<T>(o, cd.w[0], cd.w[1], rk);
        row(0, one, z, o.u0, -one, z, -o.v0);      // A = [I | dR1/dth p1], B = -[I | dR2/dth p2]
        row(1, z, one, o.u1, z, -one, -o.v1);
        row(2, z, z, z, z, z, z);
        dof = 2;
        return;
    }
    r = edge_record<T>(odom_linearize<T>(x, y, c, s, n01.x, n01.y, n23.x, n23.y, m, cd.w, rk), cd.w, rk);
    const OdomJac<T> j = odom_jacobians<T>(x, y, c, s, n01.x, n01.y, n23.x, n23.y, m);
    row(0, -j.m00, -j.m01, j.q0, j.m00, j.m01, z);      // A = [[-M, q], [0 0 -kappa]], B = [[M, 0], [0 0 kappa]]
    row(1, -j.m10, -j.m11, j.q1, j.m10, j.m11, z);
    row(2, z, z, -j.kappa, z, z, j.kappa);
    dof = 3;
}

// One thread per candidate: Sigma = (sig + sig^T) / 2, S = J Sigma J^T + Omega^-1 (upper triangle computed, mirrored: exactly symmetric),
// its Cholesky factor, d2 = |L^-1 e|^2, logdet = 2 sum ln L_kk.  rec[k] = (e0, e1, e2, s, d2, dof, logdet, status); status 1 (d2 = logdet
// = NaN) when a pivot is not positive.  innov (may be nullptr): S row-major in the leading dof x dof of 9 doubles, the rest 0.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_gate_eval(int n, const GateCand<T>* __restrict__ cands, const T* __restrict__ ps, const T* __restrict__ lmrec,
                                                      const double* __restrict__ sig, double* __restrict__ rec, double* __restrict__ innov) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const GateCand<T>& cd = cands[k];
    EdgeRecord<T> r; T Jt[3][6]; int dof;
    gate_linearize<T>(cd, ps, lmrec, r, Jt, dof);
    const double* sg = sig + (size_t)k * kGateSig;
    double P[3][6];      // J Sigma
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            double acc = 0;
#pragma unroll
            for (int j = 0; j < 6; ++j) acc += (double)Jt[a][j] * (0.5 * (sg[j * 6 + b] + sg[b * 6 + j]));
            P[a][b] = acc;
        }
    double S[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            double acc = 0;
#pragma unroll
            for (int j = 0; j < 6; ++j) acc += P[a][j] * (double)Jt[b][j];
            if (a == b) acc += a < dof ? 1.0 / (double)cd.w[a] : 1.0;      // the unused third axis of a 2-dof class: a unit pivot, taken out below
            S[a][b] = acc; S[b][a] = acc;
        }
    const double e[3] = {(double)r.e0, (double)r.e1, dof == 3 ? (double)r.e2 : 0.0};
    // Cholesky, written out (row by row: the pivots v00, v11, v22 must be positive)
    const double l00 = sqrt(S[0][0]), l10 = S[1][0] / l00, l20 = S[2][0] / l00;
    const double v11 = S[1][1] - l10 * l10, l11 = sqrt(v11), l21 = (S[2][1] - l20 * l10) / l11;
    const double v22 = S[2][2] - l20 * l20 - l21 * l21, l22 = sqrt(v22);
    const bool ok = S[0][0] > 0.0 && v11 > 0.0 && v22 > 0.0;
    const double y0 = e[0] / l00, y1 = (e[1] - l10 * y0) / l11, y2 = (e[2] - l20 * y0 - l21 * y1) / l22;
    const double d2 = y0 * y0 + y1 * y1 + (dof == 3 ? y2 * y2 : 0.0);
    const double logdet = 2.0 * (log(l00) + log(l11) + (dof == 3 ? log(l22) : 0.0));
    const double nan = __builtin_nan("");
    double* o = rec + (size_t)k * kGateRec;
    o[0] = e[0]; o[1] = e[1]; o[2] = e[2]; o[3] = (double)r.s;
    o[4] = ok ? d2 : nan; o[5] = (double)dof; o[6] = ok ? logdet : nan; o[7] = ok ? 0.0 : 1.0;
    if (innov) {
        double* q = innov + (size_t)k * 9;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) q[3 * a + b] = (a < dof && b < dof) ? S[a][b] : 0.0;
    }
}

}  // namespace tsgo
