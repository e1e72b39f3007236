// structure_index_dump.cpp — the structure index (toyslam_amd/csrc/host/structure_index.h) run on the host, on tables build_problem
// (host/problem.cpp) makes.  One case per line of stdin, one line of integers per case on stdout (tests/test_structure_index_cpu.py
// compares them with brute-force restatements):
//   I slack n id*n q id*q      IdMap: unique flat dup find*q                  (dup: the reported id, -1 when unique)
//   V GRAPH                    VertexIndex: P L pose_vertex*P lm_vertex*L (kind idx)*nV find(v_id)*nV
//   E GRAPH                    EdgeSlots: failed E loc*2E cls*E TABLE(by_pose) TABLE(by_lm) TABLE(odom) LIST(prior_p_edge) LIST(prior_l_edge)
//   N what GRAPH               build_edge_slots on a damaged copy of the tables: failed_before failed_after
//                              what = 0 an entry of by_lm.edge cleared, 1 an entry of by_pose.edge written over another, 2 the neighbour
//                              in an odom.idx entry changed, 3 the first pose prior record pointing at an LM edge
//   GRAPH = world rank lanes_per_pose lanes_per_lm nV (id type)*nV nE (type id1 id2)*nE nF id*nF
//   TABLE = G slots (edge idx)*slots          LIST = n value*n          (unsigned values print as they are, kNoEdge = 4294967295)
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "host/problem.h"
#include "host/structure_index.h"

using namespace tsgo;

static bool get(long long& v) { return std::scanf("%lld", &v) == 1; }

struct Graph {
    std::vector<uint32_t> v_id, v_type, e_type, e_ids, fixed;
    std::vector<double> v_pos, e_meas, e_inf;
    BuildOptions opt;
    bool read() {
        long long a, b, c, d, n;
        if (!get(a) || !get(b) || !get(c) || !get(d)) return false;
        opt.world = (int)a; opt.rank = (int)b; opt.lanes_per_pose = (int)c; opt.lanes_per_lm = (int)d; opt.fill_planes = false;
        if (!get(n) || n < 0) return false;
        for (long long i = 0; i < n; ++i) { if (!get(a) || !get(b)) return false; v_id.push_back((uint32_t)a); v_type.push_back((uint32_t)b); }
        v_pos.assign(3 * v_id.size(), 0.0);
        if (!get(n) || n < 0) return false;
        for (long long i = 0; i < n; ++i) { if (!get(a) || !get(b) || !get(c)) return false; e_type.push_back((uint32_t)a); e_ids.push_back((uint32_t)b); e_ids.push_back((uint32_t)c); }
        for (size_t e = 0; e < e_type.size(); ++e) { const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; e_meas.insert(e_meas.end(), eye, eye + 9); e_inf.insert(e_inf.end(), 3, 1.0); }
        if (!get(n) || n < 0) return false;
        for (long long i = 0; i < n; ++i) { if (!get(a)) return false; fixed.push_back((uint32_t)a); }
        return true;
    }
    bool build(Problem& pr) const {
        const tsgo_graph g{(int32_t)v_id.size(), v_id.data(), v_type.data(), v_pos.data(), (int32_t)e_type.size(), e_type.data(), e_ids.data(), e_meas.data(), e_inf.data(),
                           (int32_t)fixed.size(), fixed.data()};
        const std::string err = build_problem(g, opt, pr);
        if (!err.empty()) std::fprintf(stderr, "build_problem: %s\n", err.c_str());
        return err.empty();
    }
};

static void put_list(const std::vector<uint32_t>& v) { std::printf(" %zu", v.size()); for (uint32_t x : v) std::printf(" %u", x); }
static void put_table(const SellTable& t) {
    std::printf(" %d %zu", t.G, t.slots());
    for (size_t k = 0; k < t.slots(); ++k) std::printf(" %u %u", t.edge[k], t.idx[k]);
}

int main() {
    char what;
    while (std::scanf(" %c", &what) == 1) {
        if (what == 'I') {
            long long slack, n, q, v;
            if (!get(slack) || !get(n) || n < 0) return 1;
            std::vector<uint32_t> ids((size_t)n);
            for (uint32_t& id : ids) { if (!get(v)) return 1; id = (uint32_t)v; }
            IdMap m;
            uint32_t dup = 0;
            const bool unique = m.build(ids.data(), (int)n, (int)slack, &dup);
            std::printf("%d %d %lld", unique ? 1 : 0, m.flat() ? 1 : 0, unique ? -1ll : (long long)dup);
            if (!get(q) || q < 0) return 1;
            for (long long k = 0; k < q; ++k) { if (!get(v)) return 1; std::printf(" %d", m.find((uint32_t)v)); }
        } else if (what == 'V') {
            Graph g; Problem pr;
            if (!g.read() || !g.build(pr)) return 1;
            VertexIndex vi;
            vi.build(g.v_id.data(), (int)g.v_id.size(), pr);
            std::printf("%d %d", pr.P, pr.L);
            for (int v : pr.pose_vertex) std::printf(" %d", v);
            for (int v : pr.lm_vertex) std::printf(" %d", v);
            if (vi.of.size() != g.v_id.size()) return 1;
            for (const MbQuery& q : vi.of) std::printf(" %d %d", q.kind, q.idx);
            for (uint32_t id : g.v_id) std::printf(" %d", vi.ids.find(id));
        } else if (what == 'E') {
            Graph g; Problem pr;
            if (!g.read() || !g.build(pr)) return 1;
            EdgeSlots es;
            const bool failed = !build_edge_slots(pr, g.e_type, es).empty();
            std::printf("%d %zu", failed ? 1 : 0, g.e_type.size());
            if (!failed) { for (uint32_t x : es.loc) std::printf(" %u", x); for (uint8_t c : es.cls) std::printf(" %d", (int)c); }
            put_table(pr.by_pose); put_table(pr.by_lm); put_table(pr.odom);
            put_list(pr.prior_p_edge); put_list(pr.prior_l_edge);
        } else if (what == 'N') {
            long long kind;
            Graph g; Problem pr;
            if (!get(kind) || !g.read() || !g.build(pr)) return 1;
            EdgeSlots es;
            const bool before = !build_edge_slots(pr, g.e_type, es).empty();
            auto live = [](const std::vector<uint32_t>& edge, size_t from) { size_t k = from; while (k < edge.size() && edge[k] == kNoEdge) ++k; return k; };
            if (kind == 0) { const size_t k = live(pr.by_lm.edge, 0); if (k >= pr.by_lm.edge.size()) return 1; pr.by_lm.edge[k] = kNoEdge; }
            else if (kind == 1) {
                const size_t a = live(pr.by_pose.edge, 0), b = live(pr.by_pose.edge, a + 1);
                if (b >= pr.by_pose.edge.size()) return 1;
                pr.by_pose.edge[b] = pr.by_pose.edge[a];
            } else if (kind == 2) {
                const size_t k = live(pr.odom.edge, 0);
                if (k >= pr.odom.edge.size() || pr.P < 2) return 1;
                const uint32_t ix = pr.odom.idx[k];
                pr.odom.idx[k] = (ix & ~kPoseMask) | (((ix & kPoseMask) + 1) % (uint32_t)pr.P);      // no longer the pose the edge's other slot belongs to
            } else if (kind == 3) {
                size_t lm = 0;
                while (lm < g.e_type.size() && g.e_type[lm] != 1u) ++lm;
                if (lm >= g.e_type.size() || pr.prior_p_edge.empty()) return 1;
                pr.prior_p_edge[0] = (uint32_t)lm;
            } else return 1;
            std::printf("%d %d", before ? 1 : 0, build_edge_slots(pr, g.e_type, es).empty() ? 0 : 1);
        } else return 1;
        std::printf("\n");
    }
    return 0;
}
