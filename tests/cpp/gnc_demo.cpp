// Calls OptimizerHip::Gnc the way a back-end would when it cannot trust its closures (compiled by tests/test_gnc_cpu.py with -Wall
// -Wextra -Werror; not run there): an odometry chain with one false closure.  The chain is exempt (known inliers), the closure is
// subject; the plain cost is selected first (textbook GNC), and the weights come back with the estimates.
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
    optimizer.SetRobust(tsgo::EdgeType::Se2, TSGO_ROBUST_NONE, 0.0);
    optimizer.SetGraph(graph);
    std::vector<uint8_t> subject(graph.EdgeCount(), 0);
    if (!subject.empty()) subject.back() = 1;                                   // the chain is trusted, the closure is not
    tsgo_gnc_params params = tsgo::OptimizerHip::DefaultGnc();
    params.inner_iterations = 5;
    tsgo_gnc_stats st{};
    const std::vector<double> w = optimizer.Gnc(params, subject, &graph, &st);
    std::printf("%d rounds, stop %d, q_max %g; the closure's weight is %g; %lld subject ODOM edges\n", st.rounds, st.stop_reason, st.q_max, w.back(),
                (long long)st.subject_by_class[0]);
    return 0;
}
