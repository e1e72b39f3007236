// edge_report_dump.cpp — the device's per-edge report arithmetic (toyslam_amd/csrc/tsgo_math.h: the edge functions and edge_record, what
// k_edge_report runs per slot) on the host.  Reads the file named on the command line, one edge per line:
//     class kind delta v0 ... v16
// class = tsgo_graph.e_type; kind = TSGO_ROBUST_* (or -1: the compile-time Huber 1.5 the default setting runs); v = the edge's inputs in the
// form the device tables hold them (unused entries 0):
//     0 ODOM            x1 y1 c1 s1  x2 y2 c2 s2  mi[0..5]  w0 w1 w2            (mi: rows 0-1 of the inverse measurement)
//     1 LM              x y c s  lx ly  zx zy  w0 w1
//     2 virtual lm      x y c s  xn yn cn sn  pox poy pnx pny  w0 w1            (seen from the edge's first pose)
//     3 pose prior      mx my cm sm  w0 w1 w2  x y c s
//     4 landmark prior  mx my  w0 w1  lx ly
// Prints per line, with every digit, (e0 e1 e2 s rho w) in double and then the same evaluated in float.
// tests/test_edge_report_cpu.py compares the output with the numpy restatement (tests/edge_report.py).
#include <cstdio>

#include "tsgo_math.h"

namespace {

template <typename T, typename K> tsgo::EdgeRecord<T> eval(int cls, const double* d, const K& rk) {
    T v[17];
    for (int k = 0; k < 17; ++k) v[k] = (T)d[k];
    switch (cls) {
        case tsgo::kClassOdom: return tsgo::edge_record<T>(tsgo::odom_linearize<T>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v + 8, v + 14, rk), v + 14, rk);
        case tsgo::kClassLm: return tsgo::edge_record<T>(tsgo::lm_linearize<T>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], rk), v[8], v[9], rk);
        case tsgo::kClassVlm:
            return tsgo::edge_record<T>(tsgo::vlm_linearize<T>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13], rk), v[12], v[13], rk);
        case tsgo::kClassPosePrior:
            return tsgo::edge_record<T>(tsgo::pose_prior_linearize<T>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], rk), v[4], v[5], v[6], rk);
        default: return tsgo::edge_record<T>(tsgo::lm_prior_linearize<T>(v[0], v[1], v[2], v[3], v[4], v[5], rk), v[2], v[3], rk);
    }
}

template <typename T> tsgo::EdgeRecord<T> eval_kind(int cls, int kind, double delta, const double* d) {
    if (kind < 0) return eval<T>(cls, d, tsgo::HuberDefault{});
    return eval<T>(cls, d, tsgo::Robust<T>{kind, (T)delta});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: edge_report_dump FILE\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::perror(argv[1]); return 2; }
    int cls, kind;
    double delta, d[17];
    for (;;) {
        if (std::fscanf(f, "%d %d %lf", &cls, &kind, &delta) != 3) break;
        bool ok = cls >= 0 && cls < tsgo::kEdgeClasses;
        for (int k = 0; k < 17 && ok; ++k) ok = std::fscanf(f, "%lf", &d[k]) == 1;
        if (!ok) { std::fprintf(stderr, "edge_report_dump: malformed line\n"); std::fclose(f); return 1; }
        const tsgo::EdgeRecord<double> a = eval_kind<double>(cls, kind, delta, d);
        const tsgo::EdgeRecord<float> b = eval_kind<float>(cls, kind, delta, d);
        std::printf("%a %a %a %a %a %a %a %a %a %a %a %a\n", a.e0, a.e1, a.e2, a.s, a.rho, a.w, (double)b.e0, (double)b.e1, (double)b.e2, (double)b.s, (double)b.rho, (double)b.w);
    }
    std::fclose(f);
    return 0;
}
