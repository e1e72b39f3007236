// tsgo_report_kernels.h — the per-edge residual report (tsgo_edge_report, include/tsgo.h; engine/engine_report.inc).
//
// One pass over the graph at the current estimates that keeps what every linearisation computes per edge and folds away: the residual e,
// s = e^T Omega e with the RAW information, rho(s) and the robust scale w = rho'(s) of the edge's class.  k_edge_report makes k_chi2's walk
// (tsgo_lm_kernels.h): walk_of, the LM rows of the by_pose table through lm_meas, the pose-pose rows of the odom table through odom_meas
// with an edge evaluated at its FIRST endpoint only (kDirMask slots skipped, kVlmMask slots to vlm_linearize), a vertex's pose priors by
// its head lane; k_edge_report_lm_prior is to it what k_chi2_lm_prior is to k_chi2.  The residual arithmetic is not restated: the same edge
// functions with the same robust_class<RK> selection, and edge_record (tsgo_math.h) for the record.
//
// Output.  A live slot k writes its six numbers to rec[6 * edge_of_slot[k]] (three pair stores: 48 B in f64, 16-byte aligned): the
// slot -> input-edge maps are the host layout's (SellTable::edge, Problem::prior_*_edge), every input edge sits in exactly one evaluated
// slot, so every record is written once, by one lane, with plain stores.  Padding slots (kNoEdge) write nothing and count nothing.
// rec == nullptr: summary only.  In the same pass every workgroup writes one ReportPartial per edge class — count, down-weighted count,
// sum of s, sum of rho, the largest s and its edge — which the host folds in workgroup order in f64.  The arg-max rule (the largest s; among
// equal ones the LOWEST input index) is the same total order in a lane, across a wave, across the waves of a workgroup and on the host,
// so the edge reported does not depend on the layout.  No atomics.
#pragma once
#include "tsgo_kernels.h"

namespace tsgo {

// one edge class of one workgroup; an empty class is (0, 0, 0, 0, 0, kNoEdge)
template <typename T> struct ReportPartial { T s_sum, rho_sum, s_max; uint32_t edges, down, s_max_edge; };

template <typename T> __device__ __forceinline__ bool report_beats(T s, uint32_t e, T s_best, uint32_t e_best) {
    return s > s_best || (s == s_best && e < e_best);
}

template <typename T> struct ReportAcc {
    ReportPartial<T> p{T(0), T(0), T(0), 0u, 0u, kNoEdge};
    __device__ __forceinline__ void add(const EdgeRecord<T>& r, uint32_t e) {
        p.s_sum += r.s; p.rho_sum += r.rho; p.edges += 1u; p.down += r.w < T(1) ? 1u : 0u;
        if (report_beats(r.s, e, p.s_max, p.s_max_edge)) { p.s_max = r.s; p.s_max_edge = e; }
    }
    __device__ __forceinline__ void merge(const ReportPartial<T>& o) {
        p.s_sum += o.s_sum; p.rho_sum += o.rho_sum; p.edges += o.edges; p.down += o.down;
        if (report_beats(o.s_max, o.s_max_edge, p.s_max, p.s_max_edge)) { p.s_max = o.s_max; p.s_max_edge = o.s_max_edge; }
    }
    // xor butterfly: every lane ends with the wave's partial
    __device__ __forceinline__ void wave_fold() {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            ReportPartial<T> o;
            o.s_sum = __shfl_xor(p.s_sum, m); o.rho_sum = __shfl_xor(p.rho_sum, m); o.s_max = __shfl_xor(p.s_max, m);
            o.edges = __shfl_xor(p.edges, m); o.down = __shfl_xor(p.down, m); o.s_max_edge = __shfl_xor(p.s_max_edge, m);
            merge(o);
        }
    }
};

template <typename T> __device__ __forceinline__ void record_store(T* __restrict__ rec, uint32_t e, const EdgeRecord<T>& r) {
    T* q = rec + (size_t)e * 6;
    st2<T>(q, r.e0, r.e1); st2<T>(q + 2, r.e2, r.s); st2<T>(q + 4, r.rho, r.w);
}

// Landmark priors (edge type 4): k_chi2_lm_prior's walk; one ReportPartial (class 4) per workgroup into out[blockIdx.x].  Graphs with priors only.
template <typename T, int G, int RK = 0>
__global__ __launch_bounds__(kBlock) void k_edge_report_lm_prior(Table<T> tb, const T* __restrict__ lmrec, const uint32_t* __restrict__ pri_edge,
                                                                 T* __restrict__ rec, ReportPartial<T>* __restrict__ out, const PriorArgs<T> pa, const RobustArgs<T> ra) {
    __shared__ ReportPartial<T> red[kWavesPerBlock];
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    const int l = wk.vertex;
    ReportAcc<T> acc;
    if (wk.live && l < tb.n_vertices && wk.head) {
        const T lx = lmrec[(size_t)l * kLmRec], ly = lmrec[(size_t)l * kLmRec + 1];
        const auto rk = robust_class<RK>(ra, kClassLmPrior);
        for (uint32_t k = pa.off[l]; k < pa.off[l + 1]; ++k) {
            const T* q = pa.rec + (size_t)k * PRI_LM_REC;
            const auto m = ld2<T>(q + PRL_MX), w = ld2<T>(q + PRL_W0);
            const EdgeRecord<T> r = edge_record<T>(lm_prior_linearize<T>(m.x, m.y, w.x, w.y, lx, ly, rk), w.x, w.y, rk);
            const uint32_t e = pri_edge[k];
            acc.add(r, e);
            if (rec) record_store<T>(rec, e, r);
        }
    }
    acc.wave_fold();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc.p;
    __syncthreads();
    if (threadIdx.x == 0) {
        ReportAcc<T> t; t.p = red[0];
#pragma unroll
        for (int k = 1; k < kWavesPerBlock; ++k) t.merge(red[k]);
        out[blockIdx.x] = t.p;
    }
}

// Classes 0 .. 3 (ODOM, LM, virtual landmark, pose prior): k_chi2's walk and template axes.  lm_edge / od_edge: input edge of every slot of
// tb / od (kNoEdge = padding), pp_edge: of every pose prior record.  out[blockIdx.x * kEdgeClasses + class]; the fifth entry stays empty
// here (the landmark priors' partials come from k_edge_report_lm_prior, the host folds both).
template <typename T, int G, int OJ = 0, int PRI = 0, int RK = 0>
__global__ __launch_bounds__(kBlock) void k_edge_report(Table<T> tb, Table<T> od, const T* __restrict__ ps, const T* __restrict__ lmrec,
                                                        const uint32_t* __restrict__ lm_edge, const uint32_t* __restrict__ od_edge,
                                                        const uint32_t* __restrict__ pp_edge, T* __restrict__ rec, ReportPartial<T>* __restrict__ out,
                                                        const PriorArgs<T> pa, const RobustArgs<T> ra) {
    __shared__ ReportPartial<T> red[kWavesPerBlock][kEdgeClasses];
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    const int slice = wk.slice, lane = wk.lane, i = wk.vertex;
    const bool valid = wk.live && i < tb.n_vertices;
    const auto rk_lm = robust_class<RK>(ra, kClassLm), rk_odom = robust_class<RK>(ra, kClassOdom);
    ReportAcc<T> a_odom, a_lm, a_vlm, a_pp;
    if (wk.live) {
        const int ic = valid ? i : tb.n_vertices - 1;
        const auto q01 = ld2<T>(ps + (size_t)ic * 4), q23 = ld2<T>(ps + (size_t)ic * 4 + 2);
        const T x0 = q01.x, y0 = q01.y, c = q23.x, s = q23.y;
#pragma unroll 2
        for (uint32_t row = tb.row_off[slice], r1 = tb.row_off[slice + 1]; row < r1; ++row) {
            const size_t k = (size_t)row * 64 + lane;
            const uint32_t e = lm_edge[k];
            const uint32_t l = tb.idx[k];
            const LmMeas<T> z = lm_meas<T>(tb, k);
            const auto l01 = ld2<T>(lmrec + (size_t)l * kLmRec);
            const EdgeRecord<T> r = edge_record<T>(lm_linearize<T>(x0, y0, c, s, l01.x, l01.y, z.zx, z.zy, z.w0, z.w1, rk_lm), z.w0, z.w1, rk_lm);
            if (e != kNoEdge) { a_lm.add(r, e); if (rec) record_store<T>(rec, e, r); }
        }
        for (uint32_t row = od.row_off[slice], r1 = od.row_off[slice + 1]; row < r1; ++row) {
            const size_t k = (size_t)row * 64 + lane;
            const uint32_t raw = od.idx[k];
            if (raw & kDirMask) continue;      // the edge's second endpoint: reported at the first
            const uint32_t e = od_edge[k];
            if (e == kNoEdge) continue;        // padding
            const uint32_t j = raw & kPoseIdxMask;
            const OdomMeas<T> z = odom_meas<T>(od, k);
            const auto j01 = ld2<T>(ps + (size_t)j * 4), j23 = ld2<T>(ps + (size_t)j * 4 + 2);
            if (OJ && (raw & kVlmMask)) {
                const auto rk_vlm = robust_class<RK>(ra, kClassVlm);
                const EdgeRecord<T> r = edge_record<T>(vlm_linearize<T>(x0, y0, c, s, j01.x, j01.y, j23.x, j23.y, z.mi[0], z.mi[1], z.mi[2], z.mi[3], z.w[0], z.w[1], rk_vlm), z.w[0], z.w[1], rk_vlm);
                a_vlm.add(r, e); if (rec) record_store<T>(rec, e, r);
            } else {
                const EdgeRecord<T> r = edge_record<T>(odom_linearize<T>(x0, y0, c, s, j01.x, j01.y, j23.x, j23.y, z.mi, z.w, rk_odom), z.w, rk_odom);
                a_odom.add(r, e); if (rec) record_store<T>(rec, e, r);
            }
        }
        if constexpr (PRI != 0) {
            if (valid && wk.head) {
                const auto rk_pp = robust_class<RK>(ra, kClassPosePrior);
                for (uint32_t k = pa.off[i]; k < pa.off[i + 1]; ++k) {
                    const T* q = pa.rec + (size_t)k * PRI_POSE_REC;
                    const auto m01 = ld2<T>(q), cs = ld2<T>(q + PRI_C), w01 = ld2<T>(q + PRI_W0);
                    const T w2 = q[PRI_W2];
                    const EdgeRecord<T> r = edge_record<T>(pose_prior_linearize<T>(m01.x, m01.y, cs.x, cs.y, w01.x, w01.y, w2, x0, y0, c, s, rk_pp), w01.x, w01.y, w2, rk_pp);
                    const uint32_t e = pp_edge[k];
                    a_pp.add(r, e); if (rec) record_store<T>(rec, e, r);
                }
            }
        }
    }
    a_odom.wave_fold(); a_lm.wave_fold();
    if constexpr (OJ != 0) a_vlm.wave_fold();
    if constexpr (PRI != 0) a_pp.wave_fold();
    if ((threadIdx.x & 63) == 0) {
        ReportPartial<T>* w = red[threadIdx.x >> 6];
        w[kClassOdom] = a_odom.p; w[kClassLm] = a_lm.p; w[kClassVlm] = a_vlm.p; w[kClassPosePrior] = a_pp.p; w[kClassLmPrior] = ReportAcc<T>{}.p;
    }
    __syncthreads();
    if (threadIdx.x < kEdgeClasses) {
        ReportAcc<T> t; t.p = red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < kWavesPerBlock; ++k) t.merge(red[k][threadIdx.x]);
        out[(size_t)blockIdx.x * kEdgeClasses + threadIdx.x] = t.p;
    }
}

}  // namespace tsgo
