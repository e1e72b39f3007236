// tsgo_report_kernels.h — the per-edge residual report (tsgo_edge_report, include/tsgo.h; engine/engine_report.inc).
//
// One pass over the graph at the current estimates that keeps what every linearisation computes per edge and folds away: the residual e,
// s = e^T Omega e with the RAW information, rho(s) and the robust scale w = rho'(s) of the edge's class.  Which lane meets which edge is
// tsgo_edge_walk.h's (every input edge once, by one lane); what happens there is ReportVisitor's: the slot's measurement and weights
// through lm_meas / odom_meas, the prior record's own, the edge functions of the linearisation with the same robust_class<RK> selection
// (RK = 2, tsgo_set_edge_robust: the byte of the visited edge, robust_at on ra.edge; the class summaries stay indexed by the edge's type),
// and edge_record (tsgo_math.h) for the record.  The residual arithmetic is not restated.
//
// Output.  The lane that visits edge e writes its six numbers to rec[6 * e] (three pair stores: 48 B in f64, 16-byte aligned): one
// visit per edge, so every record is written once, with plain stores.  Padding is never visited: it writes nothing and counts nothing.
// rec == nullptr: summary only.  In the same pass every workgroup writes one ReportPartial per edge class — count, down-weighted count,
// sum of s, sum of rho, the largest s and its edge — which the host folds in workgroup order in f64.  The arg-max rule (the largest s; among
// equal ones the LOWEST input index) is the same total order in a lane, across a wave, across the waves of a workgroup and on the host,
// so the edge reported does not depend on the layout.  No atomics.
#pragma once
#include "tsgo_edge_walk.h"
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

// What the lane that visits an edge does with it: the edge function of the edge's class on the slot's (the record's) own measurement and
// weights, the record into the class's accumulator and, with rec, into rec[6 e].
// classes 0 .. 3 (walk_edges_once)
template <typename T, int RK> struct ReportVisitor {
    using Kernel = decltype(robust_class<RK>(RobustArgs<T>{}, 0));
    const Table<T>& tb;
    const Table<T>& od;
    const RobustArgs<T>& ra;
    T* __restrict__ rec;
    const Kernel rk_lm = robust_class<RK>(ra, kClassLm), rk_odom = robust_class<RK>(ra, kClassOdom);
    ReportAcc<T> acc[kEdgeClasses];      // the fifth stays empty
    __device__ __forceinline__ void put(int cls, uint32_t e, const EdgeRecord<T>& r) { acc[cls].add(r, e); if (rec) record_store<T>(rec, e, r); }
    __device__ __forceinline__ void lm(uint32_t e, size_t k, const PoseAt<T>& p, T lx, T ly) {
        const LmMeas<T> z = lm_meas<T>(tb, k);
        const auto rk = robust_at<RK>(ra, rk_lm, ra.edge, e);
        put(kClassLm, e, edge_record<T>(lm_linearize<T>(p.x, p.y, p.c, p.s, lx, ly, z.zx, z.zy, z.w0, z.w1, rk), z.w0, z.w1, rk));
    }
    __device__ __forceinline__ void odom(uint32_t e, size_t k, const PoseAt<T>& p, const T* qj) {
        const OdomMeas<T> z = odom_meas<T>(od, k);
        const PoseAt<T> pj = pose_at<T>(qj);
        const auto rk = robust_at<RK>(ra, rk_odom, ra.edge, e);
        put(kClassOdom, e, edge_record<T>(odom_linearize<T>(p.x, p.y, p.c, p.s, pj.x, pj.y, pj.c, pj.s, z.mi, z.w, rk), z.w, rk));
    }
    __device__ __forceinline__ void vlm(uint32_t e, size_t k, const PoseAt<T>& p, const T* qj) {
        const OdomMeas<T> z = odom_meas<T>(od, k);
        const PoseAt<T> pj = pose_at<T>(qj);
        const auto rk = robust_at<RK>(ra, robust_class<RK>(ra, kClassVlm), ra.edge, e);
        put(kClassVlm, e, edge_record<T>(vlm_linearize<T>(p.x, p.y, p.c, p.s, pj.x, pj.y, pj.c, pj.s, z.mi[0], z.mi[1], z.mi[2], z.mi[3], z.w[0], z.w[1], rk), z.w[0], z.w[1], rk));
    }
    __device__ __forceinline__ void pose_prior(uint32_t e, const T* q, const PoseAt<T>& p) {
        const auto m01 = ld2<T>(q), cs = ld2<T>(q + PRI_C), w01 = ld2<T>(q + PRI_W0);
        const T w2 = q[PRI_W2];
        const auto rk = robust_at<RK>(ra, robust_class<RK>(ra, kClassPosePrior), ra.edge, e);
        put(kClassPosePrior, e, edge_record<T>(pose_prior_linearize<T>(m01.x, m01.y, cs.x, cs.y, w01.x, w01.y, w2, p.x, p.y, p.c, p.s, rk), w01.x, w01.y, w2, rk));
    }
};

// class 4 (walk_lm_priors_once)
template <typename T, int RK> struct ReportLmPriorVisitor {
    const RobustArgs<T>& ra;
    T* __restrict__ rec;
    ReportAcc<T> acc;
    __device__ __forceinline__ void lm_prior(uint32_t e, const T* q, T lx, T ly) {
        const auto m = ld2<T>(q + PRL_MX), w = ld2<T>(q + PRL_W0);
        const auto rk = robust_at<RK>(ra, robust_class<RK>(ra, kClassLmPrior), ra.edge, e);
        const EdgeRecord<T> r = edge_record<T>(lm_prior_linearize<T>(m.x, m.y, w.x, w.y, lx, ly, rk), w.x, w.y, rk);
        acc.add(r, e);
        if (rec) record_store<T>(rec, e, r);
    }
};

// Landmark priors (class 4): one ReportPartial per workgroup into out[blockIdx.x].  Graphs with priors only.
template <typename T, int G, int RK = 0>
__global__ __launch_bounds__(kBlock) void k_edge_report_lm_prior(Table<T> tb, const T* __restrict__ lmrec, const uint32_t* __restrict__ pri_edge,
                                                                 T* __restrict__ rec, ReportPartial<T>* __restrict__ out, const PriorArgs<T> pa, const RobustArgs<T> ra) {
    __shared__ ReportPartial<T> red[kWavesPerBlock];
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    ReportLmPriorVisitor<T, RK> v{ra, rec};
    walk_lm_priors_once<T>(wk, tb, lmrec, pri_edge, pa, v);
    ReportAcc<T>& acc = v.acc;
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

// Classes 0 .. 3 (ODOM, LM, virtual landmark, pose prior); G, OJ, PRI: the walk's axes.  out[blockIdx.x * kEdgeClasses + class]; the fifth
// entry stays empty here (the landmark priors' partials come from k_edge_report_lm_prior, the host folds both).
template <typename T, int G, int OJ = 0, int PRI = 0, int RK = 0>
__global__ __launch_bounds__(kBlock) void k_edge_report(Table<T> tb, Table<T> od, const T* __restrict__ ps, const T* __restrict__ lmrec, const EdgeMaps maps,
                                                        T* __restrict__ rec, ReportPartial<T>* __restrict__ out, const PriorArgs<T> pa, const RobustArgs<T> ra) {
    __shared__ ReportPartial<T> red[kWavesPerBlock][kEdgeClasses];
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    ReportVisitor<T, RK> v{tb, od, ra, rec};
    walk_edges_once<T, OJ, PRI>(wk, tb, od, ps, lmrec, maps, pa, v);
    v.acc[kClassOdom].wave_fold(); v.acc[kClassLm].wave_fold();
    if constexpr (OJ != 0) v.acc[kClassVlm].wave_fold();
    if constexpr (PRI != 0) v.acc[kClassPosePrior].wave_fold();
    if ((threadIdx.x & 63) == 0) {
        ReportPartial<T>* w = red[threadIdx.x >> 6];
#pragma unroll
        for (int c = 0; c < kEdgeClasses; ++c) w[c] = v.acc[c].p;
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
