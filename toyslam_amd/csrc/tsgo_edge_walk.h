// tsgo_edge_walk.h — which lane evaluates which input edge: the ONE walk of the reader kernels that visit every input edge exactly once
// (the edge report, tsgo_report_kernels.h; the GNC reweighting pass, tsgo_gnc_kernels.h; the max-mixture cost pass, tsgo_mixture_kernels.h; the dogleg loop's g'Hg pass, tsgo_dogleg_kernels.h; the leverage read-out, tsgo_leverage_kernels.h).  Device only.  Who does NOT use it and why:
// the file table of tsgo_hip.hip.
//
// walk_edges_once, classes 0 .. 3, one lane of a by_pose slice (walk_of), in this order:
//   - the LM rows of the by_pose table; a slot whose map entry is kNoEdge is padding and is skipped;
//   - the pose-pose rows of the odom table.  An edge is listed at both endpoints and evaluated at its FIRST only: a kDirMask slot is
//     skipped, then kNoEdge padding; under OJ a kVlmMask slot is a virtual landmark measurement (T1 p1 - T2 p2, seen from the first pose);
//   - under PRI, the pose priors of a valid vertex, by its head lane, in record order.
// walk_lm_priors_once, class 4, one lane of a by_lm slice: the landmark priors of a valid landmark, by its head lane, in record order.
// The visitor is called once per edge with the input index e from the maps (EdgeMaps: the host layout's SellTable::edge of by_pose and
// odom, Problem::prior_p_edge; prior_l_edge for class 4), the slot k or the prior record q, and the estimates.  Measurements, weights,
// the robust kernel and the edge function are the visitor's: that is where the readers differ.  The walk does not know who calls it.
//
// Once per edge.  Every input edge sits in exactly one evaluated slot or prior record — the structure index's check on the host
// (host/structure_index.h, build_edge_slots), made before the maps reach the device — so ONE lane visits it, and a visitor may write
// what belongs to edge e (a record, a weight, the edge's information at BOTH endpoints) with plain stores and no atomics.
//
// Skipped before loaded.  Of a slot that is skipped, the walk reads the index word and the map word, nothing else: no measurement, no
// weight, no gathered record.  A visitor that writes the static planes of the slot at an edge's second endpoint (GNC) relies on it:
// nothing reads what the visiting lane is about to write.  On the LM rows both words are loaded AND WAITED FOR before the test, padding
// included (the index table is never written, so that is safe): left alone, the compiler sinks the index load behind the test, and a
// slot then costs three dependent memory round trips (map, index, gather) instead of two.
#pragma once
#include "tsgo_kernels.h"

namespace tsgo {

// slot -> input edge of by_pose and odom (kNoEdge = padding), record -> input edge of the pose priors
struct EdgeMaps { const uint32_t *lm, *od, *pp; };

// pose record i of ps: (x, y, cos, sin)
template <typename T> struct PoseAt { T x, y, c, s; };
template <typename T> __device__ __forceinline__ PoseAt<T> pose_at(const T* __restrict__ ps, size_t i = 0) {
    const auto q01 = ld2<T>(ps + i * 4), q23 = ld2<T>(ps + i * 4 + 2);
    return {q01.x, q01.y, q23.x, q23.y};
}

// visitor: lm(e, k, pose, lx, ly), odom(e, k, pose, qj), vlm(e, k, pose, qj), pose_prior(e, q, pose).  qj: the neighbour's pose record,
// pose_at<T>(qj) — a pointer, so that the visitor gathers it BEHIND its coalesced plane loads as the kernels always did (gathered
// first, the f32 report needs 82 VGPRs instead of 80 and loses a wave per SIMD)
template <typename T, int OJ, int PRI, typename V>
__device__ __forceinline__ void walk_edges_once(const Walk& wk, const Table<T>& tb, const Table<T>& od, const T* __restrict__ ps, const T* __restrict__ lmrec,
                                                const EdgeMaps& maps, const PriorArgs<T>& pa, V& visitor) {
    if (!wk.live) return;
    const int slice = wk.slice, lane = wk.lane, i = wk.vertex;
    const bool valid = i < tb.n_vertices;
    const PoseAt<T> p = pose_at<T>(ps, (size_t)(valid ? i : tb.n_vertices - 1));      // a lane past the last vertex walks padding only
    for (uint32_t row = tb.row_off[slice], r1 = tb.row_off[slice + 1]; row < r1; ++row) {
        const size_t k = (size_t)row * 64 + lane;
        const uint32_t e = maps.lm[k];
        uint32_t l = tb.idx[k];
        issue_before_exit(l);              // l is loaded and waited for here, beside the map word ("Skipped before loaded")
        if (e == kNoEdge) continue;        // padding
        const auto l01 = ld2<T>(lmrec + (size_t)l * kLmRec);
        visitor.lm(e, k, p, l01.x, l01.y);
    }
    for (uint32_t row = od.row_off[slice], r1 = od.row_off[slice + 1]; row < r1; ++row) {
        const size_t k = (size_t)row * 64 + lane;
        const uint32_t raw = od.idx[k];
        if (raw & kDirMask) continue;      // the edge's second endpoint: visited at the first
        const uint32_t e = maps.od[k];
        if (e == kNoEdge) continue;        // padding
        const T* qj = ps + (size_t)(raw & kPoseIdxMask) * 4;
        if (OJ && (raw & kVlmMask)) visitor.vlm(e, k, p, qj);
        else visitor.odom(e, k, p, qj);
    }
    if constexpr (PRI != 0) {
        if (valid && wk.head)
            for (uint32_t k = pa.off[i]; k < pa.off[i + 1]; ++k) visitor.pose_prior(maps.pp[k], pa.rec + (size_t)k * PRI_POSE_REC, p);
    }
}

// visitor: lm_prior(e, q, lx, ly); pri_edge: record -> input edge of the landmark priors
template <typename T, typename V>
__device__ __forceinline__ void walk_lm_priors_once(const Walk& wk, const Table<T>& tb, const T* __restrict__ lmrec, const uint32_t* __restrict__ pri_edge,
                                                    const PriorArgs<T>& pa, V& visitor) {
    const int l = wk.vertex;
    if (!(wk.live && l < tb.n_vertices && wk.head)) return;
    const T lx = lmrec[(size_t)l * kLmRec], ly = lmrec[(size_t)l * kLmRec + 1];
    for (uint32_t k = pa.off[l]; k < pa.off[l + 1]; ++k) visitor.lm_prior(pri_edge[k], pa.rec + (size_t)k * PRI_LM_REC, lx, ly);
}

}  // namespace tsgo
