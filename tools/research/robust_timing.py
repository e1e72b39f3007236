"""What a non-default robust kernel (tsgo_set_robust) costs on the device at config 3 (c3_100k): the linearisation kernels (tsgo_time_kernel 3
k_lin_lm, 4 k_lin_pose), the chi^2-only pass of a rules = 2 trial (7) and the linearisation ms per Gauss-Newton step of a 10-iteration run, under
  default       Huber 1.5 everywhere: the RK = 0 instantiations, the code a handle ran before the setting existed
  cauchy_all    Cauchy 1.0 on every class: RK = 1
  cauchy_odom   Cauchy 1.0 on ODOM only: RK = 1, Huber through the run-time selection on the other classes
Every figure is the median of `--repeats` measurements (each the average of 50 back-to-back launches, after a warm-up set that is thrown
away), with the smallest and largest beside it: the spread is what a difference between two cases has to exceed.  One JSON line per case.

    python tools/research/robust_timing.py [workload] [--repeats N] [--cases default,cauchy_all,cauchy_odom] [--out FILE]
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from toyslam_amd import synth  # noqa: E402
from toyslam_amd.optimizer import HipOptimizer  # noqa: E402

CASES = {"default": None, "cauchy_all": dict(all=("cauchy", 1.0)), "cauchy_odom": dict(odom=("cauchy", 1.0))}


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def measure(g, setting, repeats):
    rec = {}
    o = HipOptimizer(rules="lm", odom_jacobian="analytic")          # (tsgo_time_kernel 7 needs a rules = 2 handle)
    try:
        if setting:
            o.set_robust(**setting)
        o.set_graph(g)
        for which, name in ((3, "k_lin_lm_us"), (4, "k_lin_pose_us"), (7, "k_chi2_us")):
            o.time_kernel(which, reps=50)                            # warm-up: code objects, clocks
            rec[name] = spread([o.time_kernel(which, reps=50)[0] for _ in range(repeats)])
    finally:
        o.close()
    o = HipOptimizer()                                               # the benchmarked loop: rules = 0
    try:
        if setting:
            o.set_robust(**setting)
        ms = []
        for k in range(repeats + 1):
            o.set_graph(g); r = o.optimize(10)
            if k:                                                    # the first run loads code objects and grows the pools
                ms.append(r["ms_linearize"] / r["iters"])
        rec["linearize_ms_per_step"] = spread(ms)
        rec["chi2_last"] = float(r["chi2_last"])
    finally:
        o.close()
    return rec


def main():
    argv = sys.argv[1:]
    opt = {"--repeats": "7", "--cases": ",".join(CASES), "--out": ""}
    for k in list(opt):
        if k in argv:
            i = argv.index(k)
            opt[k] = argv[i + 1]
            del argv[i:i + 2]
    name = argv[0] if argv else "c3_100k"
    g = synth.make_config(name)
    lines = []
    for case in opt["--cases"].split(","):
        rec = dict(workload=name, case=case, repeats=int(opt["--repeats"]))
        rec.update(measure(g, CASES[case], int(opt["--repeats"])))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if opt["--out"]:
        with open(opt["--out"], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
