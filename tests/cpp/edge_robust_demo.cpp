// Calls OptimizerHip::SetEdgeRobust / EdgeRobust the way a pose-graph front-end would (compiled by tests/test_edge_robust_cpu.py with
// -Wall -Wextra -Werror; not run there): an odometry chain with one true and one false closure, all of edge type 0.  The chain stays
// quadratic (an exempt entry), the closures take Cauchy 1.0: what tsgo_set_robust alone cannot say.
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
    optimizer.SetGraph(graph);
    const std::vector<tsgo_edge_robust_entry> palette = {{TSGO_ROBUST_NONE, 0, 0.0}, {TSGO_ROBUST_CAUCHY, 0, 1.0}};
    std::vector<uint8_t> entry;                                 // the chain: exempt; the closure (the last edge): Cauchy
    for (size_t e = 0; e < graph.EdgeCount(); ++e) entry.push_back(e + 1 < graph.EdgeCount() ? 1 : 2);
    tsgo_edge_robust_stats st{};
    optimizer.SetEdgeRobust(palette, entry, &st);
    optimizer.OptimizeHeld(&graph);
    const std::vector<double> rec = optimizer.EdgeReport();
    std::vector<uint8_t> back;
    const std::vector<tsgo_edge_robust_entry> held = optimizer.EdgeRobust(graph.EdgeCount(), &back);
    std::printf("%lld edges exempt, %lld under Cauchy (active: %d); %zu entries held; the closure's weight is %g, the chain's %g\n", (long long)st.edges_by_entry[1],
                (long long)st.edges_by_entry[2], st.active, held.size(), rec[6 * (graph.EdgeCount() - 1) + 5], rec[5]);
    optimizer.SetEdgeRobust({}, {});                            // cleared: the class kernels alone again
    return back.back() == 2 ? 0 : 1;
}
