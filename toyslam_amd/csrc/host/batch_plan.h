// host/batch_plan.h — how the readers of H^-1 (engine/engine_marginals.inc, engine/engine_gate.inc) cut their query columns into batches of
// NV columns for the batched solve (tsgo_marginal_kernels.h), and the lists their read-out kernels take.  Plain host index logic, no HIP:
// tests/cpp/batch_plan_dump.cpp compiles it alone.  A pose has three columns, a landmark two.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

namespace tsgo {
// One query column: a unit column of pose `idx` (comp = 0, 1, 2), or column `comp` of Y_l = W_{:,l} Dl^-1 for landmark `idx`.  As an ITEM of
// a read-out kernel (k_mb_extract, k_mb_joint): a vertex, comp = its first column / row there.
struct MbColumn { int kind, idx, comp, pad; };      // kind 0 pose, 1 landmark, -1 none
struct MbQuery { int kind, idx; };                  // a queried vertex: kind as above, internal pose / landmark number
// One candidate's visit in one batch: the first rows of its two vertices in that batch's k_mb_joint slice (r1 unused for a unary type)
struct GateJob { int cand, r0, r1, pad; };
inline int mb_columns_of(int kind) { return kind == 0 ? 3 : 2; }
using BatchRanges = std::vector<std::pair<int, int>>;      // per batch: (first column, columns) in a column list

// tsgo_marginals: queries packed whole, in order, into batches of at most NV columns.  all = every query's columns; items[q].comp = the
// first column of query q WITHIN its batch; batch b reads out queries q_off[b] .. q_off[b + 1].  narrow: a query has more columns than a
// batch is wide (NV = 1) — nothing is packed, the caller solves column by column.
struct QueryBatches { std::vector<MbColumn> all, items; BatchRanges ranges; std::vector<int> q_off{0}; bool narrow = false; };
inline QueryBatches whole_query_batches(const std::vector<MbQuery>& qs, int NV) {
    QueryBatches pl;
    for (const MbQuery& q : qs) pl.narrow |= mb_columns_of(q.kind) > NV;
    if (pl.narrow) return pl;
    for (size_t q0 = 0, q1 = 0; q0 < qs.size(); q0 = q1) {
        const int j0 = (int)pl.all.size();
        int nc = 0;
        for (; q1 < qs.size(); ++q1) {
            const int need = mb_columns_of(qs[q1].kind);
            if (nc + need > NV && nc > 0) break;
            pl.items.push_back(MbColumn{qs[q1].kind, qs[q1].idx, nc, 0});
            for (int k = 0; k < need; ++k) pl.all.push_back(MbColumn{qs[q1].kind, qs[q1].idx, k, 0});
            nc += need;
        }
        pl.ranges.push_back({j0, nc});
        pl.q_off.push_back((int)q1);
    }
    return pl;
}
// tsgo_joint_marginals, tsgo_gate_edges: D columns in order, NV per batch — every batch but the last is full, and a vertex's columns
// may straddle two batches
inline BatchRanges full_batches(int D, int NV) {
    BatchRanges r;
    for (int j0 = 0; j0 < D; j0 += NV) r.push_back({j0, std::min(NV, D - j0)});
    return r;
}
// tsgo_gate_edges: the items (k_mb_joint) and jobs (k_gate_scatter) of every batch of full_batches, one batch after the other.  verts: the
// distinct vertices, col0[v] the first of v's columns (ascending); cand_v: 2 per candidate, its vertices' numbers in verts (equal for a
// unary candidate).  After a batch only the candidates that have a vertex among its columns get a job; the batch's items are those
// candidates' vertices (each once), comp = the vertex's first row in the batch's slice.  max_rows: the tallest slice (at least 1).
struct GateLists { std::vector<MbColumn> items; std::vector<GateJob> jobs; std::vector<int> item_off, job_off; int max_rows = 1; };      // offsets: per batch + 1
inline GateLists gate_batch_lists(const std::vector<MbQuery>& verts, const std::vector<int>& col0, const std::vector<int>& cand_v, int NV) {
    const int K = (int)(cand_v.size() / 2), V = (int)verts.size();
    const int D = V ? col0[(size_t)V - 1] + mb_columns_of(verts[(size_t)V - 1].kind) : 0;
    const int nb = (D + NV - 1) / NV;
    std::vector<int> v_off((size_t)V + 1, 0), v_cand;      // candidates of every distinct vertex (a unary candidate once)
    auto second = [&](int k) { return cand_v[2 * (size_t)k + 1] != cand_v[2 * (size_t)k]; };
    for (int k = 0; k < K; ++k) { ++v_off[(size_t)cand_v[2 * (size_t)k] + 1]; if (second(k)) ++v_off[(size_t)cand_v[2 * (size_t)k + 1] + 1]; }
    for (int v = 0; v < V; ++v) v_off[(size_t)v + 1] += v_off[(size_t)v];
    v_cand.resize((size_t)v_off[(size_t)V]);
    std::vector<int> fill(v_off.begin(), v_off.end() - 1);
    for (int k = 0; k < K; ++k) { v_cand[(size_t)fill[(size_t)cand_v[2 * (size_t)k]]++] = k; if (second(k)) v_cand[(size_t)fill[(size_t)cand_v[2 * (size_t)k + 1]]++] = k; }
    GateLists gl;
    gl.item_off.assign((size_t)nb + 1, 0); gl.job_off.assign((size_t)nb + 1, 0);
    std::vector<int> cand_stamp((size_t)K, -1), vert_stamp((size_t)V, -1), vert_row((size_t)V, 0);
    for (int b = 0, v_lo = 0; b < nb; ++b) {
        const int j0 = b * NV, j1 = std::min(D, j0 + NV);
        while (col0[(size_t)v_lo] + mb_columns_of(verts[(size_t)v_lo].kind) <= j0) ++v_lo;      // first vertex with a column >= j0
        int rows = 0;
        auto row_of = [&](int v) {
            if (vert_stamp[(size_t)v] != b) {
                vert_stamp[(size_t)v] = b; vert_row[(size_t)v] = rows;
                gl.items.push_back(MbColumn{verts[(size_t)v].kind, verts[(size_t)v].idx, rows, 0});
                rows += mb_columns_of(verts[(size_t)v].kind);
            }
            return vert_row[(size_t)v];
        };
        for (int v = v_lo; v < V && col0[(size_t)v] < j1; ++v)
            for (int q = v_off[(size_t)v]; q < v_off[(size_t)v + 1]; ++q) {
                const int k = v_cand[(size_t)q];
                if (cand_stamp[(size_t)k] == b) continue;
                cand_stamp[(size_t)k] = b;
                const int r0 = row_of(cand_v[2 * (size_t)k]), r1 = row_of(cand_v[2 * (size_t)k + 1]);
                gl.jobs.push_back(GateJob{k, r0, r1, 0});
            }
        gl.item_off[(size_t)b + 1] = (int)gl.items.size(); gl.job_off[(size_t)b + 1] = (int)gl.jobs.size();
        gl.max_rows = std::max(gl.max_rows, rows);
    }
    return gl;
}
}  // namespace tsgo
