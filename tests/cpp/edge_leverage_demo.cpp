// Calls OptimizerHip::EdgeLeverage the way a front-end that prunes its graph would (compiled by tests/test_edge_leverage_demo.py with
// -Wall -Wextra -Werror and run there: without a device the constructor's error is printed and the exit code is 1): an odometry chain
// with one closure, a landmark seen twice and a landmark seen once.  After the optimisation the leverage of every edge says which
// observations the map merely repeats (low h: candidates for disable_edges) and which nothing checks (h = dof: the chain's bridges, the
// only observation of a landmark).
#include <cmath>
#include <cstdio>
#include <exception>
#include <vector>

#include "tsgo.hpp"

int main() {
    tsgo::Graph graph;
    const int n = 12;
    const double c = std::cos(0.1), s = std::sin(0.1);
    const double step[9] = {c, -s, 1.0, s, c, 0.0, 0.0, 0.0, 1.0}, w3[3] = {100.0, 100.0, 400.0};
    double x = 0, y = 0, th = 0;
    for (int k = 0; k < n; ++k) {
        graph.AddVertex((unsigned)k, tsgo::VertexType::Se2, x + 0.01 * k, y, th);
        x += std::cos(th); y += std::sin(th); th += 0.1;
    }
    for (int k = 0; k + 1 < n; ++k) graph.AddEdge(tsgo::EdgeType::Se2, (unsigned)k, (unsigned)k + 1, step, w3);
    graph.AddEdgeSe2(2u, 9u, 5.7, 3.6, 0.7, 100.0, 100.0, 400.0);      // a closure
    graph.AddVertex(100u, tsgo::VertexType::Point2, 3.0, 2.0);
    graph.AddVertex(101u, tsgo::VertexType::Point2, 9.0, 4.0);
    graph.AddEdgeSe2Point2(3u, 100u, 2.0, 0.4, 50.0, 50.0);
    graph.AddEdgeSe2Point2(5u, 100u, 2.5, 1.9, 50.0, 50.0);
    graph.AddEdgeSe2Point2(10u, 101u, 2.2, -0.3, 50.0, 50.0);      // the only observation of landmark 101: the last edge
    graph.FixVertex(0u);

    try {
        tsgo_config cfg = tsgo::OptimizerHip::LevenbergMarquardtConfig();
        tsgo::OptimizerHip optimizer(10, &cfg);
        optimizer.Optimize(&graph);
        tsgo_leverage_stats st{};
        const size_t E = graph.EdgeCount();
        const std::vector<double> rec = optimizer.EdgeLeverage(E, 256, 7, &st);
        size_t lowest = 0;
        for (size_t e = 1; e < E; ++e)
            if (rec[8 * e + 7] - rec[8 * e + 6] > rec[8 * lowest + 7] - rec[8 * lowest + 6]) lowest = e;
        std::printf("%zu edges (%lld odometry, %lld landmark), %lld unknowns, %d samples; the last edge weights %g axes\n", E, (long long)st.edges[0],
                    (long long)st.edges[1], (long long)st.unknowns, st.samples, rec[8 * (E - 1) + 7]);
        std::printf("trace %.3f; leverage of the only observation of a landmark %.3f of 2; the most redundant edge is %zu (h = %.3f of %g)\n", st.trace,
                    rec[8 * (E - 1) + 6], lowest, rec[8 * lowest + 6], rec[8 * lowest + 7]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
