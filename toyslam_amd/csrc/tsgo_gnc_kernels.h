// tsgo_gnc_kernels.h — one round of graduated non-convexity (tsgo_gnc, include/tsgo.h; engine/engine_gnc.inc):
// evaluate every edge at the current estimates, turn its squared residual into the truncated-least-squares weight of this round's mu
// (gnc_tls_weight, tsgo_math.h) and scatter w * base into every place the handle keeps the edge's information.  f64 handles only.
//
// Which lane meets which edge is tsgo_edge_walk.h's: every input edge once, by one lane, and a skipped slot is left before anything of it
// but its index and map words is read.  What happens there is GncVisitor's: the residual from the edge functions under the "none"
// selection, handed the BASE information of the edge (base[3 e ..], what the handle held when the call started), so
// s = sum_k base_k e_k^2 is written term for term as edge_record writes it and does not depend on the weight the tables hold at that
// moment.  The static planes are read for the measurement only: this pass never loads a weight plane.
//
// Single writer.  One lane visits edge e.  No lane of this pass reads a weight plane, and the walk leaves the slot at the edge's second
// endpoint before its measurement is loaded, so nothing reads what that lane is about to write.  That lane is the only writer of both
// locations of the edge (the two words of its EdgeSlots entry, tsgo_edit_kernels.h) and of w_buf[e].  Hence plain stores, no atomics, no
// read-modify-write, and a repeated launch at the same estimates and mu writes the same bits.
//
// Subject edges: barc2[class] > 0 and (subject == nullptr or subject[e] != 0).  An exempt edge gets w_buf[e] = 1 and none of its
// information is written; a dormant subject edge (base 0) has s = 0, w = 1 and is rewritten as 0.
//
// PROBE = 1 writes nothing and only reduces (the first pass of a call: q_max).  Per workgroup ONE GncPartial — max q, sum of w s, the
// counts of weights that are 0, 1 and in between — folded across lanes and waves as ReportAcc is and on the host in workgroup order in
// f64.  The counts are integers and the max is a max: neither depends on the lanes per vertex or on the fold order.
#pragma once
#include "tsgo_edge_walk.h"
#include "tsgo_edit_kernels.h"
#include "tsgo_kernels.h"

namespace tsgo {

struct GncPartial { double q_max, cost; uint32_t n_zero, n_one, n_between, pad; };

struct GncArgs {
    double barc2[kEdgeClasses];      // inlier threshold on s per class; <= 0: the class is exempt
    double mu;
    const double* base;              // [3 E] the information the handle held when the call started
    const uint8_t* subject;          // [E] or null (every edge of a subject class)
    const uint8_t* cls;              // [E] EdgeSlots::cls
    const uint32_t* map;             // [2 E] EdgeSlots::loc
    double* w_buf;                   // [E] this round's weights
};

struct GncAcc {
    GncPartial p{0.0, 0.0, 0u, 0u, 0u, 0u};
    __device__ __forceinline__ void merge(const GncPartial& o) {
        p.q_max = o.q_max > p.q_max ? o.q_max : p.q_max; p.cost += o.cost; p.n_zero += o.n_zero; p.n_one += o.n_one; p.n_between += o.n_between;
    }
    __device__ __forceinline__ void wave_fold() {      // xor butterfly: every lane ends with the wave's partial
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            GncPartial o;
            o.q_max = __shfl_xor(p.q_max, m); o.cost = __shfl_xor(p.cost, m);
            o.n_zero = __shfl_xor(p.n_zero, m); o.n_one = __shfl_xor(p.n_one, m); o.n_between = __shfl_xor(p.n_between, m); o.pad = 0u;
            merge(o);
        }
    }
    // wave partials through LDS, workgroup partial to out[blockIdx.x]
    __device__ __forceinline__ void block_store(GncPartial* red, GncPartial* __restrict__ out) {
        wave_fold();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = p;
        __syncthreads();
        if (threadIdx.x == 0) {
            GncAcc t; t.p = red[0];
#pragma unroll
            for (int k = 1; k < kWavesPerBlock; ++k) t.merge(red[k]);
            out[blockIdx.x] = t.p;
        }
    }
};

// What the lane that evaluated edge e does with its residual: s from the base information, the weight, both stores, the partial.
template <typename T, int PROBE> __device__ __forceinline__ void gnc_edge(const GncArgs& ga, const EditTables<T>& et, uint32_t e, const EdgeRecord<T>& r, GncAcc& acc) {
    const uint8_t cls = ga.cls[e];
    const double barc2 = ga.barc2[cls];
    const bool is_subject = barc2 > 0.0 && (ga.subject == nullptr || ga.subject[e] != 0);
    if (!is_subject) { if (!PROBE) ga.w_buf[e] = 1.0; return; }
    const double s = (double)r.s, q = s / barc2;
    acc.p.q_max = q > acc.p.q_max ? q : acc.p.q_max;
    if (PROBE) return;
    const double w = gnc_tls_weight(q, ga.mu);
    acc.p.cost += w * s;
    acc.p.n_zero += w == 0.0 ? 1u : 0u; acc.p.n_one += w == 1.0 ? 1u : 0u; acc.p.n_between += (w != 0.0 && w != 1.0) ? 1u : 0u;
    const double* b = ga.base + 3 * (size_t)e;
    const uint2 at = *reinterpret_cast<const uint2*>(ga.map + 2 * (size_t)e);
    edge_inf_store<T>(et, cls, at, (T)(w * b[0]), (T)(w * b[1]), (T)(w * b[2]));
    ga.w_buf[e] = w;
}

// The visit: the slot's measurement planes (the record's measurement), the base information of e, the edge function, gnc_edge.
template <typename T> __device__ __forceinline__ T gnc_base(const GncArgs& ga, uint32_t e, int m) { return (T)ga.base[3 * (size_t)e + m]; }

// classes 0 .. 3 (walk_edges_once)
template <typename T, int PROBE> struct GncVisitor {
    const Table<T>& tb;
    const Table<T>& od;
    const GncArgs& ga;
    const EditTables<T>& et;
    const Robust<T> none{kRobustNone, T(0)};
    GncAcc acc;
    __device__ __forceinline__ T base(uint32_t e, int m) const { return gnc_base<T>(ga, e, m); }
    __device__ __forceinline__ void put(uint32_t e, const EdgeRecord<T>& r) { gnc_edge<T, PROBE>(ga, et, e, r, acc); }
    __device__ __forceinline__ void lm(uint32_t e, size_t k, const PoseAt<T>& p, T lx, T ly) {
        const auto zz = ld2<T>(tb.st + 2 * k);      // the measurement pair alone: the weight pair behind it is this lane's to write
        const T w0 = base(e, 0), w1 = base(e, 1);
        put(e, edge_record<T>(lm_linearize<T>(p.x, p.y, p.c, p.s, lx, ly, zz.x, zz.y, w0, w1, none), w0, w1, none));
    }
    __device__ __forceinline__ void odom_planes(size_t k, T (&mi)[6]) const {
#pragma unroll
        for (int m = 0; m < 6; ++m) mi[m] = od.st[(size_t)(OD_MI0 + m) * od.slots + k];
    }
    __device__ __forceinline__ void odom(uint32_t e, size_t k, const PoseAt<T>& p, const T* qj) {
        T mi[6]; odom_planes(k, mi);
        const PoseAt<T> pj = pose_at<T>(qj);
        const T w[3] = {base(e, 0), base(e, 1), base(e, 2)};
        put(e, edge_record<T>(odom_linearize<T>(p.x, p.y, p.c, p.s, pj.x, pj.y, pj.c, pj.s, mi, w, none), w, none));
    }
    __device__ __forceinline__ void vlm(uint32_t e, size_t k, const PoseAt<T>& p, const T* qj) {
        T mi[6]; odom_planes(k, mi);
        const PoseAt<T> pj = pose_at<T>(qj);
        const T w0 = base(e, 0), w1 = base(e, 1);
        put(e, edge_record<T>(vlm_linearize<T>(p.x, p.y, p.c, p.s, pj.x, pj.y, pj.c, pj.s, mi[0], mi[1], mi[2], mi[3], w0, w1, none), w0, w1, none));
    }
    __device__ __forceinline__ void pose_prior(uint32_t e, const T* q, const PoseAt<T>& p) {
        const auto m01 = ld2<T>(q), cs = ld2<T>(q + PRI_C);
        const T w0 = base(e, 0), w1 = base(e, 1), w2 = base(e, 2);
        put(e, edge_record<T>(pose_prior_linearize<T>(m01.x, m01.y, cs.x, cs.y, w0, w1, w2, p.x, p.y, p.c, p.s, none), w0, w1, w2, none));
    }
};

// class 4 (walk_lm_priors_once)
template <typename T, int PROBE> struct GncLmPriorVisitor {
    const GncArgs& ga;
    const EditTables<T>& et;
    GncAcc acc;
    __device__ __forceinline__ void lm_prior(uint32_t e, const T* q, T lx, T ly) {
        const auto m = ld2<T>(q + PRL_MX);
        const Robust<T> none{kRobustNone, T(0)};
        const T w0 = gnc_base<T>(ga, e, 0), w1 = gnc_base<T>(ga, e, 1);
        gnc_edge<T, PROBE>(ga, et, e, edge_record<T>(lm_prior_linearize<T>(m.x, m.y, w0, w1, lx, ly, none), w0, w1, none), acc);
    }
};

// Landmark priors (class 4): one GncPartial per workgroup into out[blockIdx.x].  Graphs with priors only.
template <typename T, int G, int PROBE>
__global__ __launch_bounds__(kBlock) void k_gnc_reweight_lm_prior(Table<T> tb, const T* __restrict__ lmrec, const uint32_t* __restrict__ pri_edge,
                                                                  GncPartial* __restrict__ out, const PriorArgs<T> pa, const GncArgs ga, EditTables<T> et) {
    __shared__ GncPartial red[kWavesPerBlock];
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    GncLmPriorVisitor<T, PROBE> v{ga, et};
    walk_lm_priors_once<T>(wk, tb, lmrec, pri_edge, pa, v);
    v.acc.block_store(red, out);
}

// Classes 0 .. 3 (ODOM, LM, virtual landmark, pose prior); G, OJ, PRI: the walk's axes.
template <typename T, int G, int OJ, int PRI, int PROBE>
__global__ __launch_bounds__(kBlock) void k_gnc_reweight(Table<T> tb, Table<T> od, const T* __restrict__ ps, const T* __restrict__ lmrec, const EdgeMaps maps,
                                                         GncPartial* __restrict__ out, const PriorArgs<T> pa, const GncArgs ga, EditTables<T> et) {
    __shared__ GncPartial red[kWavesPerBlock];
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    GncVisitor<T, PROBE> v{tb, od, ga, et};
    walk_edges_once<T, OJ, PRI>(wk, tb, od, ps, lmrec, maps, pa, v);
    v.acc.block_store(red, out);
}

}  // namespace tsgo
