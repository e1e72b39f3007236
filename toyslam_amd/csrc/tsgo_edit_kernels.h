// tsgo_edit_kernels.h — tsgo_set_edge_information / tsgo_get_edge_information on the device (engine/engine_edit.inc):
// the information diagonal of listed edges written into, or read back from, every place the handle keeps it.  At the end of the file the
// two scatters over listed VERTICES, tsgo_set_fixed and tsgo_set_estimates.
//
// A weight on the device is a plain copy of tsgo_graph.e_inf in the handle's scalar type (engine_graph.inc: stage_values, stage_priors),
// so an edit is a scatter of (T)value and nothing else.  Where an input edge lives is the edge -> slot map: two 32-bit words per edge,
//   LM                        its slot in by_pose, its slot in by_lm          (the (w0, w1) pair of the pair-plane-major static planes)
//   ODOM, virtual landmark    its slot at id1, its slot at id2 (kDirBit)      (planes OD_W0 .. of the pose-pose table; two distinct slots of one pose for a self-loop)
//   pose / landmark prior     its record, kNoEdge                             (PRI_W0 .. / PRL_W0 .. of the record)
// and the edge's class as one byte per edge (tsgo_graph.e_type).  The host builds and checks the map once per structure: every edge has
// exactly these locations, every location is inside its table, and no location belongs to two edges.  With the host's duplicate check
// on the list every address below has ONE writer: plain stores, no atomics, no read-modify-write.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tsgo_kernels.h"

namespace tsgo {

template <typename T> struct EditTables {      // the writable static planes of the three tables and the prior records (null without priors)
    T* st_p; size_t slots_p;
    T* st_l; size_t slots_l;
    T* st_o; size_t slots_o;
    T* pri_p; T* pri_l;
};

// (T)(w0, w1, w2) into every location of ONE edge: its class byte and the two words of its map entry say where (the table above).  The one
// statement of "where a weight lives" for writers: k_set_edge_inf below and the reweighting pass of tsgo_gnc (tsgo_gnc_kernels.h).
template <typename T> __device__ __forceinline__ void edge_inf_store(const EditTables<T>& t, uint8_t cls, uint2 at, T w0, T w1, T w2) {
    switch (cls) {
    case kClassLm:
        st2<T>(t.st_p + 2 * (t.slots_p + at.x), w0, w1);
        st2<T>(t.st_l + 2 * (t.slots_l + at.y), w0, w1);
        break;
    case kClassOdom:
        t.st_o[(size_t)OD_W0 * t.slots_o + at.x] = w0; t.st_o[(size_t)(OD_W0 + 1) * t.slots_o + at.x] = w1; t.st_o[(size_t)(OD_W0 + 2) * t.slots_o + at.x] = w2;
        t.st_o[(size_t)OD_W0 * t.slots_o + at.y] = w0; t.st_o[(size_t)(OD_W0 + 1) * t.slots_o + at.y] = w1; t.st_o[(size_t)(OD_W0 + 2) * t.slots_o + at.y] = w2;
        break;
    case kClassVlm:
        t.st_o[(size_t)OD_W0 * t.slots_o + at.x] = w0; t.st_o[(size_t)(OD_W0 + 1) * t.slots_o + at.x] = w1;
        t.st_o[(size_t)OD_W0 * t.slots_o + at.y] = w0; t.st_o[(size_t)(OD_W0 + 1) * t.slots_o + at.y] = w1;
        break;
    case kClassPosePrior: {
        T* q = t.pri_p + (size_t)at.x * PRI_POSE_REC;
        q[PRI_W0] = w0; q[PRI_W1] = w1; q[PRI_W2] = w2;
        break;
    }
    case kClassLmPrior: {
        T* q = t.pri_l + (size_t)at.x * PRI_LM_REC;
        q[PRL_W0] = w0; q[PRL_W1] = w1;
        break;
    }
    default: break;
    }
}

// One thread per LISTED edge: edge list[i] (i when list is null) takes inf[3 i ..].
template <typename T>
__global__ __launch_bounds__(kBlock) void k_set_edge_inf(int n, const int64_t* __restrict__ list, const double* __restrict__ inf, const uint32_t* __restrict__ map,
                                                         const uint8_t* __restrict__ cls, EditTables<T> t) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const size_t e = list ? (size_t)list[i] : (size_t)i;
    const uint2 at = *reinterpret_cast<const uint2*>(map + 2 * e);
    edge_inf_store<T>(t, cls[e], at, (T)inf[3 * (size_t)i], (T)inf[3 * (size_t)i + 1], (T)inf[3 * (size_t)i + 2]);
}

// One thread per edge of the graph: what its FIRST location holds, widened; entries the class does not use are 0.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_get_edge_inf(int n_edges, const uint32_t* __restrict__ map, const uint8_t* __restrict__ cls, EditTables<T> t,
                                                         double* __restrict__ out) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_edges) return;
    const size_t at = map[2 * (size_t)e];
    double w0 = 0, w1 = 0, w2 = 0;
    switch (cls[e]) {
    case kClassLm: { const auto w = ld2<T>(t.st_p + 2 * (t.slots_p + at)); w0 = (double)w.x; w1 = (double)w.y; break; }
    case kClassOdom: w2 = (double)t.st_o[(size_t)(OD_W0 + 2) * t.slots_o + at]; [[fallthrough]];
    case kClassVlm: w0 = (double)t.st_o[(size_t)OD_W0 * t.slots_o + at]; w1 = (double)t.st_o[(size_t)(OD_W0 + 1) * t.slots_o + at]; break;
    case kClassPosePrior: { const T* q = t.pri_p + at * PRI_POSE_REC; w0 = (double)q[PRI_W0]; w1 = (double)q[PRI_W1]; w2 = (double)q[PRI_W2]; break; }
    case kClassLmPrior: { const T* q = t.pri_l + at * PRI_LM_REC; w0 = (double)q[PRL_W0]; w1 = (double)q[PRL_W1]; break; }
    default: break;
    }
    out[3 * (size_t)e] = w0; out[3 * (size_t)e + 1] = w1; out[3 * (size_t)e + 2] = w2;
}

// ---- tsgo_set_fixed / tsgo_set_estimates (engine/engine_edit.inc): values of listed VERTICES ------------------------
// A listed vertex arrives as two 32-bit words the host resolved through the structure index (VertexIndex): its kind (0 pose, 1 landmark)
// and its number in the internal numbering, checked there against P and L.  The host's duplicate check gives every address ONE writer.
constexpr uint32_t kEditPose = 0, kEditLm = 1;

// One thread per listed vertex: (T)val[i], the gauge term 1e6 * multiplicity, into gauge_p / gauge_l.  Nothing else is written.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_set_gauge(int n, const uint2* __restrict__ ref, const double* __restrict__ val, T* __restrict__ gauge_p, int n_pose,
                                                      T* __restrict__ gauge_l, int n_lm) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint2 at = ref[i];
    const T g = (T)val[i];
    if (at.x == kEditPose) { if (at.y < (uint32_t)n_pose) gauge_p[at.y] = g; }
    else if (at.y < (uint32_t)n_lm) gauge_l[at.y] = g;
}

// One thread per listed vertex: val[5 i ..] = (x, y, cos theta, sin theta, theta), taken on the host in f64, written as stage_values writes
// them (engine_graph.inc) — a pose's record and its theta, or the first two entries of a landmark's record (the others are what a
// linearisation derives).  ref null: the dense form, every vertex in the internal numbering: thread i < n_pose is pose i, the others
// landmark i - n_pose.
template <typename T>
__global__ __launch_bounds__(kBlock) void k_set_estimates(int n, const uint2* __restrict__ ref, const double* __restrict__ val, T* __restrict__ ps, T* __restrict__ theta,
                                                          int n_pose, T* __restrict__ lmrec, int n_lm) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint2 at = ref ? ref[i] : (i < n_pose ? make_uint2(kEditPose, (uint32_t)i) : make_uint2(kEditLm, (uint32_t)(i - n_pose)));
    const double* v = val + 5 * (size_t)i;
    if (at.x == kEditPose) {
        if (at.y >= (uint32_t)n_pose) return;
        T* q = ps + 4 * (size_t)at.y;
        q[0] = (T)v[0]; q[1] = (T)v[1]; q[2] = (T)v[2]; q[3] = (T)v[3];
        theta[at.y] = (T)v[4];
    } else if (at.y < (uint32_t)n_lm) {
        T* q = lmrec + (size_t)kLmRec * at.y;
        q[0] = (T)v[0]; q[1] = (T)v[1];
    }
}

}  // namespace tsgo
