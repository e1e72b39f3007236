"""What the Levenberg-Marquardt loop (tsgo_config.rules = 2) costs and buys on the device at config 3 (c3_100k) under the analytic ODOM
Jacobians: trials, rejections and wall time until its own stop, against the fixed-step rules (rules = 0) run from the same start to their own
stop, both final chi^2 values, and — from the same handle — the device time of the chi^2-only pass of a trial (tsgo_time_kernel 7) next to the
linearisation it stands in for (3 + 4).  Each run is made twice on its handle and the second is reported (the first loads code objects and
grows the pools).  Prints one JSON line per record.

    python tools/research/lm_timing.py [workload] [--out FILE]
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from toyslam_amd import synth  # noqa: E402
from toyslam_amd.optimizer import HipOptimizer  # noqa: E402


def main():
    argv = sys.argv[1:]
    out = None
    if "--out" in argv:
        k = argv.index("--out")
        out = argv[k + 1]
        del argv[k:k + 2]
    name = argv[0] if argv else "c3_100k"
    g = synth.make_config(name)
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for rules, cap in (("lm", 50), ("cpp", 256)):
        o = HipOptimizer(rules=rules, odom_jacobian="analytic")
        try:
            o.set_graph(g); o.optimize(cap)
            o.set_graph(g); r = o.optimize(cap)
            rec = dict(workload=name, rules=rules, odom_jacobian="analytic", cap=cap, linearisations=r["iters"], stop=r["stop"], rejected=r["rejected"],
                       ms_total=r["ms_total"], ms_linearize=r["ms_linearize"], ms_solve=r["ms_solve"], ms_update=r["ms_update"],
                       pcg_iters_total=int(r["cg_total"]), chi2_first=float(r["chi2"][0]))
            if rules == "lm":
                acc = (r["lm_gain"] > 0) & (r["lm_pred"] > 0)
                rec.update(chi2_final=float(r["lm_chi2_trial"][acc][-1]) if acc.any() else float(r["chi2"][0]), lambda_last=r["lambda_last"],
                           gain=[round(float(x), 4) for x in r["lm_gain"]])
                emit(rec)
                chi2_pass = o.time_kernel(7, reps=50)
                lin_lm = o.time_kernel(3, reps=50)
                lin_pose = o.time_kernel(4, reps=50)
                emit(dict(workload=name, rules=rules, chi2_pass_us=chi2_pass[0], chi2_pass_bytes=chi2_pass[1], lin_lm_us=lin_lm[0], lin_pose_us=lin_pose[0],
                          linearisation_us=lin_lm[0] + lin_pose[0], chi2_pass_cheaper=bool(chi2_pass[0] < lin_lm[0] + lin_pose[0])))
            else:
                # chi2_last is the chi^2 at the last linearisation: the step after it is not evaluated by these rules
                rec.update(chi2_final=float(r["chi2_last"]))
                emit(rec)
        finally:
            o.close()
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
