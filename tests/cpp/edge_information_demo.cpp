// Calls OptimizerHip::SetEdgeInformation / EdgeInformation the way a front-end would after a robust run (compiled by
// tests/test_edge_info_cpu.py with -Wall -Wextra -Werror; not run there): an odometry chain with one true and one false closure; the
// report's down-weighted closures are switched off and the graph is finished under the plain cost.
#include <cmath>
#include <cstdio>
#include <vector>

#include "tsgo.hpp"

int main() {
    tsgo::Graph graph;
    const int n = 12;
    const double c = std::cos(0.1), s = std::sin(0.1);
    const double step[9] = {c, -s, 1.0, s, c, 0.0, 0.0, 0.0, 1.0}, w3[3] = {100.0, 100.0, 400.0};
    double x = 0, y = 0, th = 0;
    for (int k = 0; k < n; ++k) {
        graph.AddVertex((unsigned)k, tsgo::VertexType::Se2, x, y, th);
        x += std::cos(th); y += std::sin(th); th += 0.1;
    }
    for (int k = 0; k + 1 < n; ++k) graph.AddEdge(tsgo::EdgeType::Se2, (unsigned)k, (unsigned)k + 1, step, w3);
    const double wrong[9] = {1.0, 0.0, 5.0, 0.0, 1.0, -3.0, 0.0, 0.0, 1.0};
    graph.AddEdge(tsgo::EdgeType::Se2, 2u, 9u, wrong, w3);      // a false closure
    graph.FixVertex(0u);

    tsgo_config cfg = tsgo::OptimizerHip::LevenbergMarquardtConfig();
    tsgo::OptimizerHip optimizer(30, &cfg);
    optimizer.SetRobust(tsgo::EdgeType::Se2, TSGO_ROBUST_CAUCHY, 1.0);
    optimizer.Optimize(&graph);
    const std::vector<double> rec = optimizer.EdgeReport();
    std::vector<int64_t> off;
    for (size_t e = 0; e < graph.EdgeCount(); ++e) if (rec[6 * e + 5] < 0.01) off.push_back((int64_t)e);
    tsgo_edge_info_stats st{};
    if (!off.empty()) optimizer.SetEdgeInformation(off, std::vector<double>(off.size() * 3, 0.0), &st);
    const std::vector<double> inf = optimizer.EdgeInformation();
    std::printf("switched off %lld of %zu edges (map built: %d); last edge now (%g, %g, %g)\n", (long long)st.edges_listed, graph.EdgeCount(), st.maps_built,
                inf[inf.size() - 3], inf[inf.size() - 2], inf[inf.size() - 1]);
    optimizer.SetRobust(tsgo::EdgeType::Se2, TSGO_ROBUST_HUBER, 1.5);
    optimizer.SetEdgeInformation(std::vector<int64_t>(), inf);      // the dense form: every edge in order (here: what the handle holds)
    return 0;
}
