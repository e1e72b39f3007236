"""What one selection pass of tsgo_max_mixture costs at config 3 (c3_100k), beside its nearest relative, on ONE handle in ONE job:
  mixture   tsgo_max_mixture with inner_iterations = 0, rounds_max = 1, keep_selection = 0: two passes (the round's and the one that finds
            the selection stable), each k_mix_cost over the tables plus k_mix_select over the groups.  ms_select is the hipEvent time of
            the kernels: one pass is ms_select / passes.  The whole call (base read-out, constants, uploads, passes, restore) is given too.
  gnc       tsgo_gnc with inner_iterations = 0 on the same member edges: ms_reweight / rounds as the stats give it (the probe pass
            included in the numerator), and one round by difference, (ms_reweight at R rounds - at 1 round) / (R - 1).
The groups: 10 000 random ODOM edges, each with a null twin (graph.with_null_twins) — c3_100k has no loop closures, so these stand in for
closure twins, as in gnc_timing.py.  Every figure is the median of `--repeats` measurements after one warm-up, with the smallest and
largest beside it.  One JSON line per case.

    python tools/research/mixture_timing.py [workload] [--repeats N] [--groups N] [--rounds R] [--out FILE]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from toyslam_amd import graph, synth  # noqa: E402
from toyslam_amd.optimizer import HipOptimizer  # noqa: E402


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main():
    argv = sys.argv[1:]
    opt = {"--repeats": "9", "--groups": "10000", "--rounds": "9", "--out": ""}
    for k in list(opt):
        if k in argv:
            i = argv.index(k)
            opt[k] = argv[i + 1]
            del argv[i:i + 2]
    name = argv[0] if argv else "c3_100k"
    repeats, n_groups, rounds = int(opt["--repeats"]), int(opt["--groups"]), int(opt["--rounds"])
    plain = synth.make_config(name)
    rng = np.random.default_rng(0)
    g, groups = graph.with_null_twins(plain, rng.choice(np.where(plain.e_type == 0)[0], n_groups, replace=False), 1e-6)
    E = g.n_edges
    mask = np.zeros(E, np.uint8); mask[np.concatenate(groups)] = 1
    lines = []

    def emit(case, rec):
        lines.append(json.dumps(dict(workload=name, edges=E, groups=n_groups, members=int(mask.sum()), case=case, repeats=repeats, **rec)))
        print(lines[-1], flush=True)

    o = HipOptimizer()
    try:
        o.set_robust(all="none"); o.set_graph(g); o.optimize(2)

        def mixture():
            t0 = time.perf_counter()
            st = o.max_mixture(groups, inner_iterations=0, rounds_max=1, keep_selection=False)
            assert st["passes"] == 2 and st["stop"] == "stable", (st["passes"], st["stop"])
            return 1e3 * (time.perf_counter() - t0), st

        mixture()      # warm-up: the maps of the structure are built by the first call
        runs = [mixture() for _ in range(repeats)]
        emit("mixture_select_only", dict(passes=2, ms_select_per_pass=spread([st["ms_select"] / st["passes"] for _ms, st in runs]),
                                         call_ms=spread([ms for ms, _st in runs]), call_ms_in_library=spread([st["ms_total"] for _ms, st in runs]),
                                         on_null=int(sum(runs[0][1]["selected"] == 1))))
        s_max = float(o.edge_report()[0]["s"][mask != 0].max())
        barc2 = [min(11.345, s_max / 4.0), 9.210, 9.210, 11.345, 9.210]      # rounds run whatever the estimates: the largest q is at least 4

        def gnc(r):
            st = o.gnc(barc2=barc2, subject=mask, inner_iterations=0, rounds_max=r, mu_step=1.05, keep_weights=False, weights=False)
            assert st["rounds"] == r, (st["rounds"], st["stop"])
            return st

        gnc(1); gnc(rounds)
        one = [gnc(1) for _ in range(repeats)]
        many = [gnc(rounds) for _ in range(repeats)]
        emit("gnc_reweight_only", dict(rounds=rounds, ms_reweight_over_rounds=spread([st["ms_reweight"] / st["rounds"] for st in many]),
                                       ms_reweight_per_round_by_difference=spread([(m["ms_reweight"] - a["ms_reweight"]) / (rounds - 1) for a, m in zip(one, many)]),
                                       call_ms_in_library_one_round=spread([st["ms_total"] for st in one])))
    finally:
        o.close()
    if opt["--out"]:
        with open(opt["--out"], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
