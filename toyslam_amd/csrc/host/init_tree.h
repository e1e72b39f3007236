// init_tree.h — the odometry spanning tree behind tsgo_init_estimates / tsgo_init_tree (include/tsgo.h).
//
// Host only, sequential, header only (host_api.cpp and the engine both include it).  The tree depends on the STRUCTURE of the graph and on
// the mask alone — vertex ids and types, edge types and ids, the fixed list — never on estimates, measurements or information values:
//   usable edge : e_type == 0, id1 != id2, and (mask == NULL or mask[e] != 0); edge types 1-4 never enter the tree
//   sources     : the fixed pose vertices in order of first occurrence in the fixed list, depth 0, all in the FIFO queue at the start
//   scan        : a popped vertex walks its usable incident edges in increasing input edge index; an unvisited other endpoint becomes
//                 its child through that edge (of duplicate edges the lowest index wins)
//   free roots  : when the queue runs empty and poses remain, the unvisited pose with the lowest input vertex index becomes a root
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/tsgo.h"
#include "structure_index.h"

namespace tsgo {

struct InitTree {
    std::vector<int32_t> parent, edge, depth;   // per vertex in tsgo_graph order: parent's position / input edge (-1 for roots and landmarks), depth (-1 for landmarks)
    int64_t roots_fixed = 0, roots_free = 0, edges_usable = 0, tree_edges = 0;
    int32_t depth_max = 0;
    int32_t rounds() const { int32_t r = 0; while (((int64_t)1 << r) < (int64_t)depth_max + 1) ++r; return r; }      // ceil(log2(depth_max + 1))
};

// Returns the empty string on success, otherwise the error text.  Reads v_id, v_type, e_type, e_ids and fixed of g; nothing else.
// ids: the map of g.v_id when the caller holds one (the engine: the ids are then known to be distinct), else one is built here.
inline std::string build_init_tree(const tsgo_graph& g, const uint8_t* mask, int64_t n_mask, InitTree& t, const IdMap* ids = nullptr) {
    if (g.n_vertices < 0 || g.n_edges < 0 || g.n_fixed < 0) return "negative count";
    if (mask && n_mask != (int64_t)g.n_edges) return "n_mask = " + std::to_string(n_mask) + " but the graph has " + std::to_string(g.n_edges) + " edges (one byte per edge)";
    const int nV = g.n_vertices, nE = g.n_edges;
    int typed = 0;      // vertices before the first of unknown type: vertex by vertex the type is checked before the id (as build_problem does)
    while (typed < nV && g.v_type[typed] <= 1) ++typed;
    IdMap own;
    if (!ids) {
        uint32_t dup = 0;
        if (!own.build(g.v_id, typed, kVertexIdSlack, &dup)) return "duplicate vertex id " + std::to_string(dup);
        ids = &own;
    }
    if (typed < nV) return "unknown vertex type " + std::to_string(g.v_type[typed]);
    t = InitTree();
    t.parent.assign((size_t)nV, -1); t.edge.assign((size_t)nV, -1); t.depth.assign((size_t)nV, -1);
    // usable edges by endpoint (CSR over vertex positions; filled in edge order, so every list is in increasing edge index)
    std::vector<int> ea((size_t)nE, -1), eb((size_t)nE, -1);
    std::vector<int64_t> off((size_t)nV + 1, 0);
    for (int e = 0; e < nE; ++e) {
        if (g.e_type[e] != 0) continue;
        const uint32_t id1 = g.e_ids[2 * (size_t)e], id2 = g.e_ids[2 * (size_t)e + 1];
        const int a = ids->find(id1), b = ids->find(id2);
        if (a < 0 || b < 0) return "edge " + std::to_string(e) + " refers to an unknown vertex id";
        if (g.v_type[a] != 0 || g.v_type[b] != 0) return "ODOM edge " + std::to_string(e) + " must join two Se2 vertices";
        if (id1 == id2 || (mask && mask[e] == 0)) continue;
        ea[(size_t)e] = a; eb[(size_t)e] = b;
        ++off[(size_t)a + 1]; ++off[(size_t)b + 1];
        ++t.edges_usable;
    }
    for (int v = 0; v < nV; ++v) off[(size_t)v + 1] += off[(size_t)v];
    std::vector<int> adj((size_t)off[(size_t)nV]);
    {
        std::vector<int64_t> fill(off.begin(), off.end() - 1);
        for (int e = 0; e < nE; ++e) if (ea[(size_t)e] >= 0) { adj[(size_t)fill[(size_t)ea[(size_t)e]]++] = e; adj[(size_t)fill[(size_t)eb[(size_t)e]]++] = e; }
    }
    std::vector<int> queue; queue.reserve((size_t)nV);
    size_t head = 0;
    for (int i = 0; i < g.n_fixed; ++i) {
        const int v = ids->find(g.fixed[i]);
        if (v < 0) return "fixed vertex id " + std::to_string(g.fixed[i]) + " is unknown";
        if (g.v_type[v] != 0 || t.depth[(size_t)v] >= 0) continue;      // a landmark, or a pose listed before
        t.depth[(size_t)v] = 0; queue.push_back(v); ++t.roots_fixed;
    }
    int next_free = 0;
    for (;;) {
        while (head < queue.size()) {
            const int v = queue[head++];
            for (int64_t k = off[(size_t)v]; k < off[(size_t)v + 1]; ++k) {
                const int e = adj[(size_t)k];
                const int u = ea[(size_t)e] == v ? eb[(size_t)e] : ea[(size_t)e];
                if (t.depth[(size_t)u] >= 0) continue;
                t.depth[(size_t)u] = t.depth[(size_t)v] + 1; t.parent[(size_t)u] = v; t.edge[(size_t)u] = e;
                if (t.depth[(size_t)u] > t.depth_max) t.depth_max = t.depth[(size_t)u];
                ++t.tree_edges;
                queue.push_back(u);
            }
        }
        while (next_free < nV && (g.v_type[next_free] != 0 || t.depth[(size_t)next_free] >= 0)) ++next_free;
        if (next_free >= nV) break;
        t.depth[(size_t)next_free] = 0; queue.push_back(next_free); ++t.roots_free;
    }
    return std::string();
}

}  // namespace tsgo
