// gnc_weight_dump.cpp — the device's GNC weight function (toyslam_amd/csrc/tsgo_math.h: gnc_tls_weight) run on the host: reads "q mu"
// lines (hexadecimal floats) from stdin and prints the weight of each with every digit.  tests/test_gnc_cpu.py compares the output with
// the numpy restatement (tests/gnc.py: tls_weight).
#include <cstdio>

#include "tsgo_math.h"

int main() {
    double q, mu;
    while (std::scanf("%la %la", &q, &mu) == 2) std::printf("%a\n", tsgo::gnc_tls_weight(q, mu));
    return 0;
}
