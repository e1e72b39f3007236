// Calls OptimizerHip::SetFixed / Release / FixedCounts / SetEstimates the way a front-end would (compiled by tests/test_vertex_edit_cpu.py
// with -Wall -Wextra -Werror and run there: without a device the constructor's error is printed and the exit code is 1): an odometry chain
// anchored at pose 0 is optimised, the anchor is moved to the last pose so that the marginals are relative to the robot, and one pose is
// relocalised by hand before the graph is optimised again with everything the handle holds.
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
    graph.FixVertex(0u);

    try {
        tsgo_config cfg = tsgo::OptimizerHip::LevenbergMarquardtConfig();
        tsgo::OptimizerHip optimizer(10, &cfg);
        optimizer.Optimize(&graph);
        const unsigned last = (unsigned)n - 1;
        tsgo_vertex_edit_stats st{};
        optimizer.SetFixed({0u, last}, {0, 1}, &st);      // the anchor moves from pose 0 to the robot
        const std::vector<int32_t> counts = optimizer.FixedCounts(graph.VertexCount());
        const std::vector<double> cov = optimizer.Marginals({0u, last});
        std::printf("listed %lld, released %lld, fixed now %lld; count of pose 0: %d, of pose %u: %d; var x of pose 0: %g, of pose %u: %g\n", (long long)st.listed,
                    (long long)st.released, (long long)st.fixed_now, counts[0], last, counts[last], cov[0], last, cov[9]);
        const tsgo::Graph::Position p = graph.GetVertex(5u);
        optimizer.SetEstimates({5u}, {p.x + 0.3, p.y - 0.2, p.theta + 0.05}, &st);      // a relocalisation hypothesis for one pose
        optimizer.OptimizeHeld(&graph);
        optimizer.Release({last});
        optimizer.SetFixed({0u});
        std::vector<double> all;
        for (unsigned k = 0; k < (unsigned)n; ++k) { const tsgo::Graph::Position q = graph.GetVertex(k); all.insert(all.end(), {q.x, q.y, q.theta}); }
        optimizer.SetEstimates(std::vector<uint32_t>(), all);      // the dense form: every vertex in order
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
