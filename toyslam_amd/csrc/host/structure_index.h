// host/structure_index.h — where the vertices and edges of a request sit in the tables build_problem made of it (host/problem.h).  Three
// lookups every reader of a handle's tables needs, stated once.  Plain host index logic, no HIP: tests/cpp/structure_index_dump.cpp compiles
// it with g++ and tests/test_structure_index_cpu.py compares it with brute-force restatements.
//   IdMap        vertex id -> position in the request's vertex arrays
//   VertexIndex  ... and position -> (pose | landmark, internal number)
//   EdgeSlots    input edge -> the table slots / prior record that hold it, with the check that every edge has exactly those
//   StructureIndex  a VertexIndex and an EdgeSlots of one structure, each built by the first call that asks for it
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "batch_plan.h"        // MbQuery
#include "problem.h"

namespace tsgo {

// A flat table when the ids are (nearly) dense, as the reference's client sends them (python/slam_main.py:161-185 numbers vertices
// 0..V-1): max_id < slack * n + 1024; a hash map for anything else.
class IdMap {
    bool flat_ = false;
    uint32_t max_id_ = 0;
    std::vector<int> table_;
    std::unordered_map<uint32_t, int> hash_;
public:
    // false: an id occurs twice; *dup (when given) = the first id, in input order, that repeats an earlier one.  The map is complete
    // either way, and a repeated id keeps its first position.
    bool build(const uint32_t* ids, int n, int slack, uint32_t* dup = nullptr) {
        max_id_ = 0;
        for (int i = 0; i < n; ++i) max_id_ = std::max(max_id_, ids[i]);
        flat_ = n > 0 && (uint64_t)max_id_ < (uint64_t)slack * (uint64_t)n + 1024;
        table_.assign(flat_ ? (size_t)max_id_ + 1 : 0, -1);
        hash_.clear();
        if (!flat_) hash_.reserve((size_t)n * 2);
        bool unique = true;
        for (int i = 0; i < n; ++i) {
            bool fresh;
            if (flat_) { fresh = table_[ids[i]] < 0; if (fresh) table_[ids[i]] = i; }
            else fresh = hash_.emplace(ids[i], i).second;
            if (!fresh && unique) { unique = false; if (dup) *dup = ids[i]; }
        }
        return unique;
    }
    int find(uint32_t id) const {      // the position, -1 for an id that is not there
        if (flat_) return id <= max_id_ ? table_[id] : -1;
        const auto it = hash_.find(id);
        return it == hash_.end() ? -1 : it->second;
    }
    bool flat() const { return flat_; }
};

constexpr int kVertexIdSlack = 4;      // IdMap slack for a request's vertex ids

// of[v]: what the vertex at position v is in the internal numbering (Problem::pose_vertex / lm_vertex inverted); kind = -1 for a vertex
// that is neither a pose nor a landmark this shard owns.
struct VertexIndex {
    IdMap ids;
    std::vector<MbQuery> of;
    void build(const uint32_t* v_id, int n_vertices, const Problem& pr) {
        ids.build(v_id, n_vertices, kVertexIdSlack);      // build_problem has refused duplicate ids
        of.assign((size_t)n_vertices, MbQuery{-1, 0});
        for (int i = 0; i < pr.P; ++i) of[(size_t)pr.pose_vertex[(size_t)i]] = MbQuery{0, i};
        for (int l = 0; l < pr.L; ++l) of[(size_t)pr.lm_vertex[(size_t)l]] = MbQuery{1, l};
    }
    int pose_of(int v) const { return of[(size_t)v].kind == 0 ? of[(size_t)v].idx : -1; }
};

// loc: two words per input edge, cls: its class as a byte (what tsgo_edit_kernels.h reads).
//   LM edge         word 0 its by_pose slot, word 1 its by_lm slot
//   pose-pose edge  word `side` its odom slot at that endpoint (side 1: kDirBit; ODOM and virtual-landmark edges)
//   prior           word 0 its record number (Problem::prior_p_edge / prior_l_edge), word 1 kNoEdge
struct EdgeSlots {
    std::vector<uint32_t> loc;
    std::vector<uint8_t> cls;
    uint32_t first_odom_slot(size_t e) const { return std::min(loc[2 * e], loc[2 * e + 1]); }      // the lower of a pose-pose edge's two slots
};

// What the kernels that go from an edge to its slots, or from a slot to its edge, rely on: every input edge has exactly the locations its
// class requires, inside their tables, and no location belongs to two edges (a slot names one edge; an edge takes each of its words once);
// the two slots of a pose-pose edge name each other's pose.  Returns the empty string or the error text.
//
// This implies what the edge report's pass needs of its slot -> edge maps — every entry is an input edge, and every input edge sits in
// exactly one slot the pass evaluates (by_pose slots, odom slots without kDirBit, prior records): an entry that is taken is below E and of
// the class of its table, so the three evaluated sets are disjoint; within one, word 0 is taken at most once per edge; and every edge has
// its word 0.
inline std::string build_edge_slots(const Problem& pr, const std::vector<uint32_t>& type, EdgeSlots& out) {
    enum : uint32_t { kOdom = 0, kLm = 1, kVlm = 2, kPosePrior = 3, kLmPrior = 4, kClasses = 5 };      // tsgo_graph.e_type (kClass* of tsgo_math.h, which a plain host file cannot include)
    const size_t E = type.size();
    std::vector<uint32_t> m(2 * E, kNoEdge), owner(2 * E, kNoEdge);      // owner: the pose a pose-pose slot belongs to
    bool ok = pr.by_pose.slots() < kNoEdge && pr.by_lm.slots() < kNoEdge && pr.odom.slots() < kNoEdge;
    auto take = [&](uint32_t e, int word, size_t at, bool right_class) {
        if (e >= E || !right_class || m[2 * (size_t)e + word] != kNoEdge) { ok = false; return false; }
        m[2 * (size_t)e + word] = (uint32_t)at;
        return true;
    };
    for (size_t k = 0; ok && k < pr.by_pose.edge.size(); ++k) { const uint32_t e = pr.by_pose.edge[k]; if (e != kNoEdge) take(e, 0, k, e < E && type[e] == kLm); }
    for (size_t k = 0; ok && k < pr.by_lm.edge.size(); ++k) { const uint32_t e = pr.by_lm.edge[k]; if (e != kNoEdge) take(e, 1, k, e < E && type[e] == kLm); }
    const int vps = kWave / std::max(1, pr.odom.G);
    for (int s = 0; ok && s < pr.odom.n_slices; ++s)
        for (size_t row = pr.odom.row_off[(size_t)s]; row < pr.odom.row_off[(size_t)s + 1]; ++row)
            for (int lane = 0; lane < kWave; ++lane) {
                const size_t k = row * kWave + (size_t)lane;
                const uint32_t e = pr.odom.edge[k], ix = pr.odom.idx[k];
                if (e == kNoEdge) continue;
                const int side = (ix & kDirBit) ? 1 : 0;
                if (take(e, side, k, e < E && type[e] == ((ix & kVlmBit) ? kVlm : kOdom)))
                    owner[2 * (size_t)e + side] = (uint32_t)(s * vps + lane / pr.odom.G);
            }
    for (size_t k = 0; ok && k < pr.prior_p_edge.size(); ++k) { const uint32_t e = pr.prior_p_edge[k]; take(e, 0, k, e < E && type[e] == kPosePrior); }
    for (size_t k = 0; ok && k < pr.prior_l_edge.size(); ++k) { const uint32_t e = pr.prior_l_edge[k]; take(e, 0, k, e < E && type[e] == kLmPrior); }
    for (size_t e = 0; ok && e < E; ++e) {
        const uint32_t a = m[2 * e], b = m[2 * e + 1];
        if (type[e] >= kClasses || a == kNoEdge) ok = false;
        else if (type[e] >= kPosePrior) ok = b == kNoEdge;
        else if (b == kNoEdge) ok = false;
        // a pose-pose edge: each slot's neighbour is the pose the other slot belongs to (a self-loop: two slots of one pose)
        else if (type[e] != kLm) ok = a != b && (pr.odom.idx[a] & kPoseMask) == owner[2 * e + 1] && (pr.odom.idx[b] & kPoseMask) == owner[2 * e];
    }
    if (!ok) return "the slot tables do not give every input edge exactly the locations of its type";
    out.loc.swap(m);
    out.cls.resize(E);
    for (size_t e = 0; e < E; ++e) out.cls[e] = (uint8_t)type[e];
    return std::string();
}

// The index of ONE structure (a handle's tables): each half is built by the first call that needs it, so a handle that never asks pays
// nothing; clear() where the tables go.
class StructureIndex {
    VertexIndex vert_; EdgeSlots edge_;
    bool have_vert_ = false, have_edge_ = false;
public:
    const VertexIndex& vertices(const std::vector<uint32_t>& v_id, const Problem& pr) {
        if (!have_vert_) { vert_.build(v_id.data(), (int)v_id.size(), pr); have_vert_ = true; }
        return vert_;
    }
    // null with the text of build_edge_slots in err when the tables fail its check (nothing is kept then)
    const EdgeSlots* edges(const Problem& pr, const std::vector<uint32_t>& e_type, std::string& err) {
        if (!have_edge_) { err = build_edge_slots(pr, e_type, edge_); if (!err.empty()) return nullptr; have_edge_ = true; }
        return &edge_;
    }
    void clear() { *this = StructureIndex(); }
};

}  // namespace tsgo
