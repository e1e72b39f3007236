"""What changing edge weights costs at config 3 (c3_100k), on ONE handle, three ways:
  refill               the same-structure tsgo_set_graph (all a caller had before tsgo_set_edge_information): host clock of the call and
                       the handle's own ms_setup (read from the tsgo_optimize(1) that follows)
  dense                tsgo_set_edge_information with edge_idx = NULL: every edge, 24 B per edge over the host link
  sparse_13, sparse_10000   a list of 13 / of 10 000 distinct random edges
For the edit calls: host clock of the whole Python call, and the call's own ms_total, ms_host (validation, staging) and ms_device (hipEvent
time of k_set_edge_inf).  Also the get call (edge_information) and the first edit on the structure, which builds and uploads the edge -> slot
map.  Every figure is the median of `--repeats` measurements with the smallest and largest beside it.  One JSON line per case.

    python tools/research/edge_information_timing.py [workload] [--repeats N] [--out FILE]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from toyslam_amd import synth  # noqa: E402
from toyslam_amd.optimizer import HipOptimizer  # noqa: E402


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return 1e3 * (time.perf_counter() - t0), out


def edit_case(o, e_inf, edges, repeats):
    o.set_edge_information(e_inf, edges)
    runs = [timed(lambda: o.set_edge_information(e_inf, edges)) for _ in range(repeats)]
    rec = dict(n=len(e_inf), call_ms=spread([ms for ms, _st in runs]))
    for k in ("ms_total", "ms_host", "ms_device"):
        rec[k] = spread([st[k] for _ms, st in runs])
    return rec


def main():
    argv = sys.argv[1:]
    opt = {"--repeats": "9", "--out": ""}
    for k in list(opt):
        if k in argv:
            i = argv.index(k)
            opt[k] = argv[i + 1]
            del argv[i:i + 2]
    name = argv[0] if argv else "c3_100k"
    repeats = int(opt["--repeats"])
    g = synth.make_config(name)
    E = g.n_edges
    rng = np.random.default_rng(0)
    lines = []

    def emit(case, rec):
        lines.append(json.dumps(dict(workload=name, edges=E, case=case, repeats=repeats, **rec)))
        print(lines[-1], flush=True)

    o = HipOptimizer()
    try:
        o.set_graph(g); o.optimize(2)
        setup, wall = [], []
        for _ in range(repeats):
            ms, _none = timed(lambda: o.set_graph(g))
            r = o.optimize(1)
            assert r["structure_reused"]
            wall.append(ms); setup.append(r["ms_setup"])
        emit("refill", dict(n=E, call_ms=spread(wall), ms_setup=spread(setup)))
        ms, st = timed(lambda: o.set_edge_information(g.e_inf[:1], [0]))
        assert st["maps_built"] == 1
        emit("first_call_builds_the_map", dict(n=1, call_ms=ms, ms_total=st["ms_total"], ms_host=st["ms_host"], ms_device=st["ms_device"]))
        emit("dense", edit_case(o, g.e_inf, None, repeats))
        for n in (13, 10000):
            edges = rng.choice(E, n, replace=False)
            emit("sparse_%d" % n, edit_case(o, g.e_inf[edges], edges, repeats))
        emit("get", dict(n=E, call_ms=spread([timed(o.edge_information)[0] for _ in range(repeats)])))
        r = o.optimize(2)
        emit("optimize_after", dict(n=0, chi2=float(r["chi2"][-1]), cg_iters=[int(k) for k in r["cg_iters"]]))
    finally:
        o.close()
    if opt["--out"]:
        with open(opt["--out"], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
