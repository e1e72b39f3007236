"""What the per-edge residual report (tsgo_edge_report) costs on the device at config 3 (c3_100k), from ONE rules = 2 handle:
  k_chi2_us            tsgo_time_kernel 7: the chi^2-only pass, which reads the same tables
  summary_pass_us      tsgo_time_kernel 8: the report's pass without its record stores (device time of the launches)
  summary_call_ms      edge_report(records=False): the whole call, host clock (launch, partials back, host fold)
  full_call_ms         edge_report(): the whole call, host clock (result buffer allocated, pass with stores, 48 B per edge copied back into
                       pageable memory, buffer freed), and the device's own ms_total of it
Every figure is the median of `--repeats` measurements with the smallest and largest beside it (the kernel figures each the average of 50
back-to-back launches after a warm-up set that is thrown away).  Under the default setting (RK = 0) and under Cauchy 1.0 everywhere (RK = 1).
One JSON line per case.

    python tools/research/edge_report_timing.py [workload] [--repeats N] [--out FILE]
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from toyslam_amd import synth  # noqa: E402
from toyslam_amd.optimizer import HipOptimizer  # noqa: E402

CASES = {"default": None, "cauchy_all": dict(all=("cauchy", 1.0))}


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def measure(g, setting, repeats):
    rec = {}
    o = HipOptimizer(rules="lm", odom_jacobian="analytic")          # (tsgo_time_kernel 7 needs a rules = 2 handle)
    try:
        if setting:
            o.set_robust(**setting)
        o.set_graph(g)
        rec["edges"] = int(o.n_edges)
        for which, name in ((7, "k_chi2"), (8, "summary_pass")):
            o.time_kernel(which, reps=50)                            # warm-up: code objects, clocks, the maps' upload
            runs = [o.time_kernel(which, reps=50) for _ in range(repeats)]
            rec[name + "_us"] = spread([r[0] for r in runs]); rec[name + "_bytes"] = runs[0][1]
        for records, name in ((False, "summary_call_ms"), (True, "full_call_ms")):
            o.edge_report(records=records)
            ms = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                _rec, summ = o.edge_report(records=records)
                ms.append(1e3 * (time.perf_counter() - t0))
            rec[name] = spread(ms)
        rec["chi2"] = summ["chi2"]
        rec["downweighted"] = {c: summ[c]["downweighted"] for c in summ if c != "chi2"}
    finally:
        o.close()
    return rec


def main():
    argv = sys.argv[1:]
    opt = {"--repeats": "7", "--out": ""}
    for k in list(opt):
        if k in argv:
            i = argv.index(k)
            opt[k] = argv[i + 1]
            del argv[i:i + 2]
    name = argv[0] if argv else "c3_100k"
    g = synth.make_config(name)
    lines = []
    for case, setting in CASES.items():
        rec = dict(workload=name, case=case, repeats=int(opt["--repeats"]))
        rec.update(measure(g, setting, int(opt["--repeats"])))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if opt["--out"]:
        with open(opt["--out"], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
