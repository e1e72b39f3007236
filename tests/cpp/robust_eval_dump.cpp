// robust_eval_dump.cpp — the device's robust-kernel arithmetic (toyslam_amd/csrc/tsgo_math.h: robust_eval, huber) run on the host:
// reads "kind delta s" lines from stdin and prints, per line and with every digit, rho and w in double and in float
// (for kind = 1 and delta = 1.5 also what the fixed-width huber() gives).  tests/test_robust_cpu.py compares the output with numpy.
#include <cstdio>

#include "tsgo_math.h"

int main() {
    int kind;
    double delta, s;
    while (std::scanf("%d %lf %lf", &kind, &delta, &s) == 3) {
        double rho = 0, w = 0, hrho = 0, hw = 0;
        float rho32 = 0, w32 = 0, hrho32 = 0, hw32 = 0;
        tsgo::robust_eval<double>(kind, delta, s, rho, w);
        tsgo::robust_eval<float>(kind, (float)delta, (float)s, rho32, w32);
        tsgo::huber<double>(s, hrho, hw);
        tsgo::huber<float>((float)s, hrho32, hw32);
        std::printf("%a %a %a %a %a %a %a %a\n", rho, w, (double)rho32, (double)w32, hrho, hw, (double)hrho32, (double)hw32);
    }
    return 0;
}
