"""Timing of tsgo_joint_marginals at config 3 (c3_100k), multigrid preconditioner, default batch width: 16, 64 and 256 vertices near
the end of the trajectory (three poses to one landmark), and tsgo_marginals of the same ids for comparison (the same PCG columns, packed whole
per query there, fully here).  Prints one JSON line per case.  A call on two of the ids goes first (it loads the kernels).

    python tools/research/joint_marginals_timing.py [workload] [--out FILE]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np  # noqa: E402

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
    poses = g.v_id[g.v_type == 0]; lms = g.v_id[g.v_type == 1]
    tail = lambda n_p, n_l: np.concatenate([poses[-n_p:], lms[-n_l:]])
    cases = [("16 vertices (12 poses, 4 landmarks)", tail(12, 4)), ("64 vertices (48 poses, 16 landmarks)", tail(48, 16)),
             ("256 vertices (192 poses, 64 landmarks)", tail(192, 64))]
    lines = []
    o = HipOptimizer()
    try:
        o.set_graph(g)
        o.optimize(3)
        for label, ids in cases:
            for call in ("joint", "diagonal"):
                run = (lambda q: o.joint_marginals(q)[2]) if call == "joint" else (lambda q: o.marginals(q)[1])
                run(ids[:2])
                t0 = time.perf_counter()
                st = run(ids)
                wall = time.perf_counter() - t0
                rec = dict(workload=name, call="tsgo_joint_marginals" if call == "joint" else "tsgo_marginals", case=label, ids=len(ids),
                           width=st["batch_width"], columns=st["columns"], batches=st["batches"], pcg_iters_max=st["pcg_iters_max"],
                           pcg_iters_per_column=round(st["pcg_iters_total"] / max(1, st["columns"]), 2), fallbacks=st["fallbacks"],
                           ms_total=round(st["ms_total"], 3), ms_solve=round(st["ms_solve"], 3), wall_s=round(wall, 4),
                           columns_per_s=round(st["columns"] / (st["ms_solve"] / 1e3), 1),
                           ms_outside_batches=round(st["ms_total"] - st["ms_solve"], 3))
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    finally:
        o.close()
    if out:
        with open(out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
