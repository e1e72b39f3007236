// Builds a small graph with every edge type of include/tsgo.hpp's Graph, prior edges included, and prints the tsgo_graph arrays it
// hands to the C ABI (tests/test_priors_cpu.py compares them with toyslam_amd.graph.GraphArrays.from_optgraph).  Header only: no
// library is linked.
#include <cstdio>

#include "tsgo.hpp"

int main() {
    tsgo::Graph g;
    g.AddVertex(0, tsgo::VertexType::Se2, 1.0, 2.0, 0.3);
    g.AddVertex(1, tsgo::VertexType::Se2, 2.0, 2.5, 0.4);
    g.AddVertex(2, tsgo::VertexType::Point2, 3.0, 1.0);
    g.AddEdgeSe2(0, 1, 1.0, 0.5, 0.1, 4.0, 4.0, 65.0);
    g.AddEdgeSe2Point2(0, 2, 2.2, 0.4, 44.0, 44.0);
    g.AddEdgePosePrior(1, 1.9, 2.4, 0.35, 10.0, 20.0, 30.0);
    g.AddEdgeLandmarkPrior(2, 3.1, 0.9, 5.0, 6.0);
    g.FixVertex(0);
    const tsgo_graph v = g.View();
    for (int i = 0; i < v.n_vertices; ++i)
        std::printf("v %u %u %.17g %.17g %.17g\n", v.v_id[i], v.v_type[i], v.v_pos[3 * i], v.v_pos[3 * i + 1], v.v_pos[3 * i + 2]);
    for (int e = 0; e < v.n_edges; ++e) {
        std::printf("e %u %u %u", v.e_type[e], v.e_ids[2 * e], v.e_ids[2 * e + 1]);
        for (int k = 0; k < 9; ++k) std::printf(" %.17g", v.e_meas[9 * e + k]);
        for (int k = 0; k < 3; ++k) std::printf(" %.17g", v.e_inf[3 * e + k]);
        std::printf("\n");
    }
    for (int i = 0; i < v.n_fixed; ++i) std::printf("f %u\n", v.fixed[i]);
    return 0;
}
