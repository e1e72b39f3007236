// tsgo_mixture_kernels.h — one selection pass of max-mixture edges (tsgo_max_mixture, include/tsgo.h; engine/engine_mixture.inc; DESIGN.md
// section 24): evaluate the cost of every member edge at the current estimates, pick the cheapest member of every group, switch it on and
// its siblings off in every place the handle keeps an edge's information.  f64 handles only.  Two launches, ordered by the stream:
//
// 1. k_mix_cost / k_mix_cost_lm_prior.  Which lane meets which edge is tsgo_edge_walk.h's: every input edge once, by one lane.  What happens
//    there is MixVisitor's: member_of[e] first (one 32-bit word per input edge, kNoMember for an edge in no group) — a non-member is left
//    before its measurement planes or its base are loaded.  A member's residual comes from the edge functions under the "none" selection,
//    handed the BASE information of the edge (base[3 e ..], what the handle held when the call started), so s = sum_k base_k e_k^2 is
//    written term for term as edge_record writes it and does not depend on what the tables hold at that moment (a switched-off member has
//    0 there).  The static planes are read for the measurement only: this pass never loads a weight plane.  cost[m] = s + k[m], one plain
//    store by the one lane that visits the edge: the cost does not depend on the lanes per vertex.  This pass writes nothing else.
//
// 2. k_mix_select.  One thread per group (groups are short: TSGO_MIX_MAX_MEMBERS).  The thread walks its members in order, a cost that is
//    not finite counting as +inf, and keeps the first smallest (strict comparison: a tie goes to the lowest position, a group of +inf
//    costs to position 0).  sel[g] holds the previous selection on entry (kMixNone before the first pass) and this pass's on exit.  A group
//    whose selection moved stores base to both locations of the winner and 0 to both locations of every other member (edge_inf_store and
//    the edge -> slot map, tsgo_edit_kernels.h); a group whose selection stayed would store the bits that are there and stores nothing.
//    Single writer: an edge is in at most one group (the host's check), a group has one thread, and pass 1 has finished (stream order) and
//    read no weight plane: plain stores, no atomics, no read-modify-write.  Per workgroup ONE MixPartial {groups whose selection moved,
//    sum of the winners' costs}, summed by block_sum2 (lanes, then waves 0 .. 3) and folded on the host in workgroup order.
//
// Around them, one thread per member each: k_mix_members at the start of a call (member_of and the members' base rows for the host, which
// makes k of them) and k_mix_restore at its end under keep_selection = 0 (the base information back: the same single writer).
#pragma once
#include "tsgo_edge_walk.h"
#include "tsgo_edit_kernels.h"
#include "tsgo_kernels.h"

namespace tsgo {

constexpr uint32_t kNoMember = 0xFFFFFFFFu;      // member_of[e]: the edge is in no group
constexpr int32_t kMixNone = -1;                 // sel[g]: nothing selected yet

struct MixPartial { double changed, cost_sum; };      // (a count of at most kBlock per workgroup: exact as a double, and block_sum2 takes both)

struct MixArgs {
    const uint32_t* member_of;       // [E] position of the edge in the member arrays, kNoMember
    const double* base;              // [3 E] the information the handle held when the call started
    const double* k;                 // [M] -(sum of ln base over the used axes) - 2 log_weight, from the host
    double* cost;                    // [M] s + k
};

// classes 0 .. 3 (walk_edges_once).  The edge functions and the base hand-over are GncVisitor's (tsgo_gnc_kernels.h); the membership test
// in front and the store behind are this pass's.
template <typename T> struct MixVisitor {
    const Table<T>& tb;
    const Table<T>& od;
    const MixArgs& ma;
    const Robust<T> none{kRobustNone, T(0)};
    __device__ __forceinline__ T base(uint32_t e, int m) const { return (T)ma.base[3 * (size_t)e + m]; }
    __device__ __forceinline__ void put(uint32_t m, const EdgeRecord<T>& r) { ma.cost[m] = (double)r.s + ma.k[m]; }
    __device__ __forceinline__ void lm(uint32_t e, size_t k, const PoseAt<T>& p, T lx, T ly) {
        const uint32_t m = ma.member_of[e];
        if (m == kNoMember) return;
        const auto zz = ld2<T>(tb.st + 2 * k);      // the measurement pair alone
        const T w0 = base(e, 0), w1 = base(e, 1);
        put(m, edge_record<T>(lm_linearize<T>(p.x, p.y, p.c, p.s, lx, ly, zz.x, zz.y, w0, w1, none), w0, w1, none));
    }
    __device__ __forceinline__ void odom_planes(size_t k, T (&mi)[6]) const {
#pragma unroll
        for (int m = 0; m < 6; ++m) mi[m] = od.st[(size_t)(OD_MI0 + m) * od.slots + k];
    }
    __device__ __forceinline__ void odom(uint32_t e, size_t k, const PoseAt<T>& p, const T* qj) {
        const uint32_t m = ma.member_of[e];
        if (m == kNoMember) return;
        T mi[6]; odom_planes(k, mi);
        const PoseAt<T> pj = pose_at<T>(qj);
        const T w[3] = {base(e, 0), base(e, 1), base(e, 2)};
        put(m, edge_record<T>(odom_linearize<T>(p.x, p.y, p.c, p.s, pj.x, pj.y, pj.c, pj.s, mi, w, none), w, none));
    }
    __device__ __forceinline__ void vlm(uint32_t e, size_t k, const PoseAt<T>& p, const T* qj) {
        const uint32_t m = ma.member_of[e];
        if (m == kNoMember) return;
        T mi[6]; odom_planes(k, mi);
        const PoseAt<T> pj = pose_at<T>(qj);
        const T w0 = base(e, 0), w1 = base(e, 1);
        put(m, edge_record<T>(vlm_linearize<T>(p.x, p.y, p.c, p.s, pj.x, pj.y, pj.c, pj.s, mi[0], mi[1], mi[2], mi[3], w0, w1, none), w0, w1, none));
    }
    __device__ __forceinline__ void pose_prior(uint32_t e, const T* q, const PoseAt<T>& p) {
        const uint32_t m = ma.member_of[e];
        if (m == kNoMember) return;
        const auto m01 = ld2<T>(q), cs = ld2<T>(q + PRI_C);
        const T w0 = base(e, 0), w1 = base(e, 1), w2 = base(e, 2);
        put(m, edge_record<T>(pose_prior_linearize<T>(m01.x, m01.y, cs.x, cs.y, w0, w1, w2, p.x, p.y, p.c, p.s, none), w0, w1, w2, none));
    }
};

// class 4 (walk_lm_priors_once)
template <typename T> struct MixLmPriorVisitor {
    const MixArgs& ma;
    __device__ __forceinline__ void lm_prior(uint32_t e, const T* q, T lx, T ly) {
        const uint32_t m = ma.member_of[e];
        if (m == kNoMember) return;
        const auto z = ld2<T>(q + PRL_MX);
        const Robust<T> none{kRobustNone, T(0)};
        const T w0 = (T)ma.base[3 * (size_t)e], w1 = (T)ma.base[3 * (size_t)e + 1];
        ma.cost[m] = (double)edge_record<T>(lm_prior_linearize<T>(z.x, z.y, w0, w1, lx, ly, none), w0, w1, none).s + ma.k[m];
    }
};

// Landmark priors (class 4).  Graphs with priors only.
template <typename T, int G>
__global__ __launch_bounds__(kBlock) void k_mix_cost_lm_prior(Table<T> tb, const T* __restrict__ lmrec, const uint32_t* __restrict__ pri_edge, const PriorArgs<T> pa,
                                                              const MixArgs ma) {
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    MixLmPriorVisitor<T> v{ma};
    walk_lm_priors_once<T>(wk, tb, lmrec, pri_edge, pa, v);
}

// Classes 0 .. 3 (ODOM, LM, virtual landmark, pose prior); G, OJ, PRI: the walk's axes.
template <typename T, int G, int OJ, int PRI>
__global__ __launch_bounds__(kBlock) void k_mix_cost(Table<T> tb, Table<T> od, const T* __restrict__ ps, const T* __restrict__ lmrec, const EdgeMaps maps,
                                                     const PriorArgs<T> pa, const MixArgs ma) {
    const Walk wk = walk_of<G>(tb.n_slices, table_xcd8(tb));
    MixVisitor<T> v{tb, od, ma};
    walk_edges_once<T, OJ, PRI>(wk, tb, od, ps, lmrec, maps, pa, v);
}

struct MixGroups {
    int n_groups;
    const uint32_t* off;             // [n_groups + 1] into the member arrays
    const uint32_t* edge;            // [M] input edge of each member
    const double* cost;              // [M] of pass 1
    const double* base;              // [3 E]
    const uint8_t* cls;              // [E] EdgeSlots::cls
    const uint32_t* map;             // [2 E] EdgeSlots::loc
    int32_t* sel;                    // [n_groups] in: the previous selection; out: this pass's
};

// base (on = true) or 0 into every location of edge e
template <typename T> __device__ __forceinline__ void mix_store(const MixGroups& mg, const EditTables<T>& et, uint32_t e, bool on) {
    const double* b = mg.base + 3 * (size_t)e;
    const uint2 at = *reinterpret_cast<const uint2*>(mg.map + 2 * (size_t)e);
    edge_inf_store<T>(et, mg.cls[e], at, on ? (T)b[0] : T(0), on ? (T)b[1] : T(0), on ? (T)b[2] : T(0));
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_mix_select(const MixGroups mg, EditTables<T> et, MixPartial* __restrict__ out) {
    __shared__ double red[2 * kWavesPerBlock];
    const int g = blockIdx.x * kBlock + threadIdx.x;
    double changed = 0.0, cost = 0.0;
    if (g < mg.n_groups) {
        const uint32_t m0 = mg.off[g], m1 = mg.off[g + 1];
        const double inf = __builtin_huge_val();
        int32_t best = 0;
        double c_best = inf;
        for (uint32_t m = m0; m < m1; ++m) {
            const double c = mg.cost[m];
            if (c - c == 0.0 && c < c_best) { c_best = c; best = (int32_t)(m - m0); }      // c - c == 0: c is finite
        }
        cost = c_best;
        if (mg.sel[g] != best) {
            changed = 1.0;
            for (uint32_t m = m0; m < m1; ++m) mix_store<T>(mg, et, mg.edge[m], (int32_t)(m - m0) == best);
            mg.sel[g] = best;
        }
    }
    block_sum2<double>(changed, cost, red);
    if (threadIdx.x == 0) out[blockIdx.x] = MixPartial{changed, cost};
}

// One thread per member, at the start of a call: member_of[e] = m (the array was filled with kNoMember) and the member's base information
// gathered into member_base[3 m ..], which the host checks and turns into k.  Writes buffers of the call only.
__global__ __launch_bounds__(kBlock) void k_mix_members(int n_members, const uint32_t* __restrict__ edge, const double* __restrict__ base, uint32_t* __restrict__ member_of,
                                                        double* __restrict__ member_base) {
    const int m = blockIdx.x * kBlock + threadIdx.x;
    if (m >= n_members) return;
    const size_t e = edge[m];
    member_of[e] = (uint32_t)m;
#pragma unroll
    for (int a = 0; a < 3; ++a) member_base[3 * (size_t)m + a] = base[3 * e + a];
}

// One thread per member: the base information back into every location of its edge.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_mix_restore(int n_members, const MixGroups mg, EditTables<T> et) {
    const int m = blockIdx.x * kBlock + threadIdx.x;
    if (m < n_members) mix_store<T>(mg, et, mg.edge[m], true);
}

}  // namespace tsgo
