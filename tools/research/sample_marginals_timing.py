"""Timing of tsgo_sample_marginals at config 3 (c3_100k), multigrid preconditioner, default batch width: K = 16, 64 and 256 samples,
cov_out only (no samples copied back).  Records ms_total, ms_noise (the right-hand-side kernels), ms_readout and samples/s of the
batched solve, beside the columns/s of tsgo_marginals on 16 poses in the same run (DESIGN.md section 11's figure): a sample is one
column of the same solve with a dense right-hand side.  Prints one JSON line per case.  A K = 1 call goes first (it loads the kernels
and uploads the maps).

    python tools/research/sample_marginals_timing.py [workload] [--out FILE]
"""
import json
import os
import sys
import time

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
    o = HipOptimizer()
    try:
        o.set_graph(g)
        o.optimize(3)
        o.sample_marginals(1)
        poses = g.v_id[g.v_type == 0][-16:]
        o.marginals(poses[:1])
        st = o.marginals(poses)[1]
        rec = dict(workload=name, call="tsgo_marginals", columns=st["columns"], width=st["batch_width"], batches=st["batches"],
                   pcg_iters_max=st["pcg_iters_max"], ms_total=round(st["ms_total"], 3), ms_solve=round(st["ms_solve"], 3),
                   columns_per_s=round(st["columns"] / (st["ms_solve"] / 1e3), 1))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        for K in (16, 64, 256):
            t0 = time.perf_counter()
            st = o.sample_marginals(K, seed=1)["stats"]
            wall = time.perf_counter() - t0
            sv = st["solve"]
            rec = dict(workload=name, call="tsgo_sample_marginals", samples=K, vertices=len(g.v_id), width=sv["batch_width"], batches=sv["batches"],
                       pcg_iters_max=sv["pcg_iters_max"], pcg_iters_per_sample=round(sv["pcg_iters_total"] / K, 2), fallbacks=sv["fallbacks"],
                       ms_total=round(st["ms_total"], 3), ms_solve=round(sv["ms_solve"], 3), ms_noise=round(st["ms_noise"], 3),
                       ms_readout=round(st["ms_readout"], 3), wall_s=round(wall, 4), samples_per_s=round(K / (sv["ms_solve"] / 1e3), 1),
                       rel_std_error=round((2.0 / K) ** 0.5, 4))
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
