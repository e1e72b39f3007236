"""Timing of tsgo_edge_leverage at config 3 (c3_100k), multigrid preconditioner, default batch width: K = 16 and 64 samples, beside
tsgo_sample_marginals (cov_out only) of the same K in the same run.  Records ms_total, ms_solve, ms_noise and ms_readout of both calls:
the two differ in the read-out alone (k_lev_acc / k_lev_acc_lm_prior per batch, one [E][8] copy back and the host's fold).  Prints one
JSON line per call.  A K = 1 call of each goes first (it loads the kernels and uploads the maps).

    python tools/research/edge_leverage_timing.py [workload] [--out FILE]
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
        o.edge_leverage(1)
        for K in (16, 64):
            for call in ("tsgo_sample_marginals", "tsgo_edge_leverage"):
                t0 = time.perf_counter()
                st = (o.sample_marginals(K, seed=1) if call == "tsgo_sample_marginals" else o.edge_leverage(K, seed=1))["stats"]
                wall = time.perf_counter() - t0
                sv = st["solve"]
                rec = dict(workload=name, call=call, samples=K, vertices=len(g.v_id), edges=len(g.e_type), width=sv["batch_width"], batches=sv["batches"],
                           pcg_iters_per_sample=round(sv["pcg_iters_total"] / K, 2), fallbacks=sv["fallbacks"], ms_total=round(st["ms_total"], 3),
                           ms_solve=round(sv["ms_solve"], 3), ms_noise=round(st["ms_noise"], 3), ms_readout=round(st["ms_readout"], 3),
                           ms_readout_per_batch=round(st["ms_readout"] / sv["batches"], 3), wall_s=round(wall, 4))
                if call == "tsgo_edge_leverage":
                    rec.update(trace=round(st["trace"], 3), unknowns=st["unknowns"], h_gauge=round(st["h_gauge"], 4))
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
