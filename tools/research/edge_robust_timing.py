"""What a per-edge robust setting (tsgo_set_edge_robust) costs on the device at config 3 (c3_100k): the linearisation kernels
(tsgo_time_kernel 3 k_lin_lm, 4 k_lin_pose) and the chi^2-only pass of a rules = 2 trial (7) on ONE handle in three states, alternating
  cleared       no per-edge setting: the RK = 0 instantiations (the default class setting)
  chain_exempt  the odometry chain (ODOM edges between consecutive vertex ids) exempt, every other edge left to its class: RK = 2, one entry
  all           every edge given an entry of a three-kernel palette (none, Cauchy, Geman-McClure) by index mod 3: RK = 2, rows that mix kernels
Every figure is the median of `--repeats` measurements (each the average of 50 back-to-back launches; a first round over the three states is
thrown away), with the smallest and largest beside it: the spread is what a difference between two states has to exceed.  The states
alternate inside every repeat, so drift of the clocks hits all three alike.  One JSON line per state.

    python tools/research/edge_robust_timing.py [workload] [--repeats N] [--out FILE]
"""
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from toyslam_amd import synth  # noqa: E402
from toyslam_amd.optimizer import HipOptimizer  # noqa: E402

KERNELS = ((3, "k_lin_lm_us"), (4, "k_lin_pose_us"), (7, "k_chi2_us"))


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main():
    argv = sys.argv[1:]
    opt = {"--repeats": "7", "--out": ""}
    for k in list(opt):
        if k in argv:
            i = argv.index(k)
            opt[k] = argv[i + 1]
            del argv[i:i + 2]
    name = argv[0] if argv else "c3_100k"
    repeats = int(opt["--repeats"])
    g = synth.make_config(name)
    E = len(g.e_type)
    a, b = g.e_ids[:, 0].astype(np.int64), g.e_ids[:, 1].astype(np.int64)
    chain = ((g.e_type == 0) & (np.abs(a - b) == 1)).astype(np.uint8)
    states = {"cleared": lambda o: o.clear_edge_robust(), "chain_exempt": lambda o: o.set_edge_robust(["none"], chain),
              "all": lambda o: o.set_edge_robust(["none", ("cauchy", 1.0), ("geman_mcclure", 2.0)], 1 + np.arange(E) % 3)}
    got = {s: {n: [] for _w, n in KERNELS} for s in states}
    o = HipOptimizer(rules="lm", odom_jacobian="analytic")          # (tsgo_time_kernel 7 needs a rules = 2 handle)
    try:
        o.set_graph(g)
        for rep in range(repeats + 1):
            for s, put in states.items():
                put(o)
                for which, n in KERNELS:
                    us = o.time_kernel(which, reps=50)[0]
                    if rep:                                          # the first round loads code objects
                        got[s][n].append(us)
    finally:
        o.close()
    lines = []
    for s in states:
        rec = dict(workload=name, state=s, repeats=repeats, edges=int(E), chain_edges=int(chain.sum()))
        rec.update({n: spread(v) for n, v in got[s].items()})
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if opt["--out"]:
        with open(opt["--out"], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
