"""Timing of tsgo_marginals at config 3 (c3_100k): 8 / 64 / 512 poses and 64 landmarks, at the default batch width and at widths 1
and 16 (TSGO_MARGINAL_WIDTH, read by the testing build only).  Prints one JSON line per case: columns per second, PCG iterations per
batch and ms per batch iteration (the device time of the batches over their summed maximum iteration counts).

    python tools/research/marginals_timing.py [workload] [--out FILE]
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
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    name = args[0] if args else "c3_100k"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    g = synth.make_config(name)
    poses = g.v_id[g.v_type == 0]; lms = g.v_id[g.v_type == 1]
    pick = lambda a, n: a[np.linspace(0, len(a) - 1, n).astype(int)]
    cases = [("8 poses", pick(poses, 8)), ("64 poses", pick(poses, 64)), ("512 poses", pick(poses, 512)), ("64 landmarks", pick(lms, 64))]
    lines = []
    for pc in ("amg", "jacobi"):
        o = HipOptimizer(preconditioner=pc, testing=True)
        try:
            o.set_graph(g)
            o.optimize(3)
            for width in ("16", "8", "1"):
                os.environ["TSGO_MARGINAL_WIDTH"] = width
                for label, ids in cases:
                    if width == "1" and len(ids) > 64:
                        continue          # the width-1 baseline: one column per launch chain
                    if pc == "jacobi" and (len(ids) > 64 or width != "8"):
                        continue
                    o.marginals(ids[:2])                       # warm-up of this width's kernels
                    t0 = time.perf_counter()
                    _cov, st = o.marginals(ids)
                    wall = time.perf_counter() - t0
                    it_batches = st["pcg_iters_max"]
                    rec = dict(workload=name, preconditioner=pc, width=st["batch_width"], case=label, columns=st["columns"], batches=st["batches"],
                               pcg_iters_max=st["pcg_iters_max"], pcg_iters_per_batch=st["pcg_iters_total"] / max(1, st["columns"]) ,
                               ms_total=round(st["ms_total"], 3), ms_solve=round(st["ms_solve"], 3), wall_s=round(wall, 4),
                               columns_per_s=round(st["columns"] / (st["ms_solve"] / 1e3), 1),
                               fallbacks=st["fallbacks"])
                    rec["ms_per_batch_iteration"] = round(st["ms_solve"] / max(1, st["batches"] * max(1, it_batches)), 4)
                    print(json.dumps(rec), flush=True)
                    lines.append(rec)
        finally:
            os.environ.pop("TSGO_MARGINAL_WIDTH", None)
            o.close()
    if out:
        with open(out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
