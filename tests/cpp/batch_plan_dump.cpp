// batch_plan_dump.cpp — the batch planning of the H^-1 readers (toyslam_amd/csrc/host/batch_plan.h) run on the host.  One case per line of
// stdin, one line of integers per case on stdout (tests/test_batch_plan_cpu.py compares them with a brute-force restatement):
//   W NV n kind*n                        whole_query_batches (query q has idx = q): narrow nb (j0 nc)*nb q_off*(nb+1) n_items (kind idx comp)*
//                                        n_all (kind idx comp)*
//   F D NV                               full_batches: nb (j0 nc)*nb
//   G NV V (kind idx col0)*V K (a b)*K   gate_batch_lists: nb max_rows item_off*(nb+1) job_off*(nb+1) n_items (kind idx comp)* n_jobs (cand r0 r1)*
#include <cstdio>
#include <vector>

#include "host/batch_plan.h"

using namespace tsgo;

static bool get(int& v) { return std::scanf("%d", &v) == 1; }
static void put_columns(const std::vector<MbColumn>& c) {
    std::printf(" %zu", c.size());
    for (const MbColumn& m : c) std::printf(" %d %d %d", m.kind, m.idx, m.comp);
}

int main() {
    char what;
    while (std::scanf(" %c", &what) == 1) {
        if (what == 'W') {
            int NV, n;
            if (!get(NV) || !get(n) || n < 0) return 1;
            std::vector<MbQuery> qs((size_t)n);
            for (int q = 0; q < n; ++q) { qs[(size_t)q].idx = q; if (!get(qs[(size_t)q].kind)) return 1; }
            const QueryBatches pl = whole_query_batches(qs, NV);
            std::printf("%d %zu", pl.narrow ? 1 : 0, pl.ranges.size());
            for (const auto& r : pl.ranges) std::printf(" %d %d", r.first, r.second);
            for (int q : pl.q_off) std::printf(" %d", q);
            put_columns(pl.items); put_columns(pl.all);
        } else if (what == 'F') {
            int D, NV;
            if (!get(D) || !get(NV)) return 1;
            const BatchRanges r = full_batches(D, NV);
            std::printf("%zu", r.size());
            for (const auto& p : r) std::printf(" %d %d", p.first, p.second);
        } else if (what == 'G') {
            int NV, V, K;
            if (!get(NV) || !get(V) || V < 0) return 1;
            std::vector<MbQuery> verts((size_t)V); std::vector<int> col0((size_t)V);
            for (int v = 0; v < V; ++v) if (!get(verts[(size_t)v].kind) || !get(verts[(size_t)v].idx) || !get(col0[(size_t)v])) return 1;
            if (!get(K) || K < 0) return 1;
            std::vector<int> cand_v(2 * (size_t)K);
            for (int& c : cand_v) if (!get(c) || c < 0 || c >= V) return 1;
            const GateLists gl = gate_batch_lists(verts, col0, cand_v, NV);
            std::printf("%zu %d", gl.item_off.size() - 1, gl.max_rows);
            for (int o : gl.item_off) std::printf(" %d", o);
            for (int o : gl.job_off) std::printf(" %d", o);
            put_columns(gl.items);
            std::printf(" %zu", gl.jobs.size());
            for (const GateJob& j : gl.jobs) std::printf(" %d %d %d", j.cand, j.r0, j.r1);
        } else return 1;
        std::printf("\n");
    }
    return 0;
}
