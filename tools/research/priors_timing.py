"""What unary priors (edge types 3 and 4) cost on the device at config 3 (c3_100k): the two linearisation kernels (tsgo_time_kernel 3
and 4) and whole Gauss-Newton steps (ms per step over a 10-step run after 2 warm-up steps) for the graph as it is, with priors on 1 % of
its poses and landmarks, and with a prior on every pose and every landmark.  The fixed vertex stays, so the solves are alike.  Prints one
JSON line per case.

    python tools/research/priors_timing.py [workload] [--out FILE]
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from tests import priors  # noqa: E402
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
    cases = [("none", g), ("1% of poses and landmarks", priors.with_priors(g, 0.01, 0.01, seed=1, n_far=0, n_dup=0, noise=0.01)),
             ("every pose and landmark", priors.with_priors(g, 1.0, 1.0, seed=1, n_far=0, n_dup=0, noise=0.01))]
    lines = []
    for label, gg in cases:
        o = HipOptimizer()
        try:
            o.set_graph(gg)
            lin_lm = o.time_kernel(3, reps=50)
            lin_pose = o.time_kernel(4, reps=50)
            o.optimize(2)
            o.set_graph(gg)
            r = o.optimize(10)
        finally:
            o.close()
        rec = dict(workload=name, priors=label, n_prior_edges=int((gg.e_type >= 3).sum()), lin_lm_us=lin_lm[0], lin_pose_us=lin_pose[0],
                   iters=r["iters"], ms_per_step=r["ms_total"] / max(1, r["iters"]), ms_linearize_per_step=r["ms_linearize"] / max(1, r["iters"]),
                   chi2_last=r["chi2_last"], pcg_iters_total=int(r["cg_total"]))
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
