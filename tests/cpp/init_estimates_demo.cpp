// Calls OptimizerHip::InitEstimates the way a front-end would before its first Optimize (compiled by tests/test_init_guess_cpu.py with
// -Wall -Wextra -Werror; not run there): a short odometry chain with one landmark, every estimate but the fixed pose at zero.
#include <cmath>
#include <cstdio>
#include <vector>

#include "tsgo.hpp"

int main() {
    tsgo::Graph graph;
    const int n = 8;
    for (int k = 0; k < n; ++k) graph.AddVertex((unsigned)k, tsgo::VertexType::Se2, 0.0, 0.0, 0.0);
    graph.AddVertex(100u, tsgo::VertexType::Point2, 0.0, 0.0, 0.0);
    const double c = std::cos(0.1), s = std::sin(0.1);
    const double step[9] = {c, -s, 1.0, s, c, 0.0, 0.0, 0.0, 1.0}, w3[3] = {100.0, 100.0, 400.0};
    for (int k = 0; k + 1 < n; ++k) graph.AddEdge(tsgo::EdgeType::Se2, (unsigned)k, (unsigned)k + 1, step, w3);
    const double seen[9] = {2.0, 0.5, 0, 0, 0, 0, 0, 0, 0}, w2[3] = {50.0, 50.0, 0.0};
    graph.AddEdge(tsgo::EdgeType::Se2Point2, 3u, 100u, seen, w2);
    graph.FixVertex(0u);

    const tsgo_config cfg = tsgo::OptimizerHip::LevenbergMarquardtConfig();
    tsgo::OptimizerHip optimizer(30, &cfg);
    optimizer.SetGraph(graph);
    std::vector<uint8_t> mask(graph.EdgeCount(), 1);
    const tsgo_init_stats all = optimizer.InitEstimates(&graph);
    const tsgo_init_stats poses = optimizer.InitEstimates(nullptr, TSGO_INIT_POSES, mask);
    std::printf("poses set %lld (%lld), landmarks set %lld, depth %d, rounds %d\n", (long long)all.poses_set, (long long)poses.poses_set,
                (long long)all.landmarks_set, all.depth_max, all.rounds);
    optimizer.Optimize(&graph);
    const tsgo::Graph::Position last = graph.GetVertex((unsigned)n - 1);
    std::printf("last pose %.6f %.6f %.6f\n", last.x, last.y, last.theta);
    return 0;
}
