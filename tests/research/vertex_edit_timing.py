"""What editing vertices costs at config 3 (c3_100k), on ONE handle, beside what a caller paid for the same change before the edits existed:
  rebuild              tsgo_set_graph with another fixed list (the anchor moved from the first to the last pose and back): same_as fails on
                       the list, so the layout, the slot tables and the multigrid patterns are built again
  refill               the same-structure tsgo_set_graph with other v_pos
  set_fixed_N          tsgo_set_fixed with 1, 1 000 and all vertices listed (the counts the handle holds: no value changes)
  set_estimates_N      tsgo_set_estimates with 1 and 1 000 vertices listed, with all of them listed, and in the dense form (ids = NULL), at
                       the estimates the handle holds
For the set_graph calls: host clock of the Python call and the handle's own ms_setup (read from the tsgo_optimize(1) that follows).  For the
edits: host clock of the whole Python call and the call's own ms_total, ms_host (validation, staging) and ms_device (hipEvent time of the
kernel); tsgo_set_estimates ends with the solver's restart (lever arms of the multigrid hierarchy from the new estimates), which ms_total
includes.  Every figure is the median of `--repeats` measurements with the smallest and largest beside it.  One JSON line per case.

    python tests/research/vertex_edit_timing.py [workload] [--repeats N] [--out FILE]
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


def edit_case(call, n, repeats):
    call()
    runs = [timed(call) for _ in range(repeats)]
    rec = dict(n=n, call_ms=spread([ms for ms, _st in runs]))
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
    V = len(g.v_id)
    rng = np.random.default_rng(0)
    lines = []

    def emit(case, rec):
        lines.append(json.dumps(dict(workload=name, vertices=V, case=case, repeats=repeats, **rec)))
        print(lines[-1], flush=True)

    def set_graph_case(o, graphs, reused):
        wall, setup = [], []
        for k in range(repeats):
            ms, _none = timed(lambda: o.set_graph(graphs[k % 2]))
            r = o.optimize(1)
            assert bool(r["structure_reused"]) == reused
            wall.append(ms); setup.append(r["ms_setup"])
        return dict(n=V, call_ms=spread(wall), ms_setup=spread(setup))

    o = HipOptimizer()
    try:
        o.set_graph(g); o.optimize(2)
        other = g.copy(); other.fixed = np.array([g.v_id[g.v_type == 0][-1]], np.uint32)
        emit("rebuild", set_graph_case(o, (other, g), False))
        shifted = g.copy(); shifted.v_pos[:, :2] += 1e-3
        o.set_graph(g); o.optimize(1)
        emit("refill", set_graph_case(o, (shifted, g), True))
        o.set_graph(g); o.optimize(2)
        ms, st = timed(lambda: o.set_fixed(g.fixed[:1], 1))
        emit("first_call_allocates_the_buffer", dict(n=1, call_ms=ms, ms_total=st["ms_total"], ms_host=st["ms_host"], ms_device=st["ms_device"]))
        held = o.fixed_counts()
        for n in (1, 1000, V):
            rows = np.arange(V) if n == V else np.sort(rng.choice(V, n, replace=False))
            emit("set_fixed_%d" % n, edit_case(lambda: o.set_fixed(g.v_id[rows], held[rows]), n, repeats))
        emit("get_fixed", dict(n=V, call_ms=spread([timed(o.fixed_counts)[0] for _ in range(repeats)])))
        v = o.vertices()
        for n in (1, 1000, V):
            rows = np.arange(V) if n == V else np.sort(rng.choice(V, n, replace=False))
            emit("set_estimates_%d" % n, edit_case(lambda: o.set_vertices(v[rows], g.v_id[rows]), n, repeats))
        emit("set_estimates_dense", edit_case(lambda: o.set_vertices(v), V, repeats))
        r = o.optimize(2)
        emit("optimize_after", dict(n=0, chi2=float(r["chi2"][-1]), cg_iters=[int(k) for k in r["cg_iters"]]))
    finally:
        o.close()
    if opt["--out"]:
        with open(opt["--out"], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
