"""Timing of tsgo_gate_edges at config 3 (c3_100k), multigrid preconditioner, default batch width: K = 64, 1 024 and 16 384 candidate edges
(three ODOM candidates to one LM candidate) over 64 and 1 024 vertices near the end of the trajectory (three poses to one landmark), and in
the same run tsgo_joint_marginals of the distinct vertices those candidates touch (the same PCG columns; a D x D result instead of K
records).  K = 64 touches at most 128 vertices, so its second case solves fewer columns than the others.  Prints one JSON line per call.
A call on two candidates goes first (it loads the kernels).

    python tools/research/gate_timing.py [workload] [--out FILE]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np  # noqa: E402

from toyslam_amd import synth  # noqa: E402
from toyslam_amd.optimizer import HipOptimizer  # noqa: E402


def candidates(K, poses, lms, rng):
    """K candidates whose vertices cycle through the pool: every pose is touched once K >= len(poses), every landmark once K >= 4 len(lms)."""
    e_type = np.zeros(K, np.uint32); e_ids = np.zeros((K, 2), np.uint32); e_meas = np.zeros((K, 9)); e_inf = np.full((K, 3), 100.0)
    n_p, n_l = len(poses), len(lms)
    for k in range(K):
        a = poses[k % n_p]
        if k % 4 == 3:
            e_type[k] = 1; e_ids[k] = (a, lms[(k // 4) % n_l]); e_meas[k, :2] = (rng.uniform(1, 10), rng.uniform(-3, 3))
        else:
            b = poses[(k % n_p + 1 + (7 * (k // n_p)) % (n_p - 1)) % n_p]
            th = rng.uniform(-3, 3)
            e_ids[k] = (a, b); e_meas[k] = (np.cos(th), -np.sin(th), rng.uniform(-2, 2), np.sin(th), np.cos(th), rng.uniform(-2, 2), 0, 0, 1)
    return e_type, e_ids, e_meas, e_inf


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
    rng = np.random.default_rng(0)
    lines = []
    o = HipOptimizer()
    try:
        o.set_graph(g)
        o.optimize(3)
        o.gate_edges(*candidates(2, poses[-2:], lms[-1:], rng))
        o.joint_marginals(poses[-2:])
        for n_p, n_l in ((48, 16), (768, 256)):
            for K in (64, 1024, 16384):
                c = candidates(K, poses[-n_p:], lms[-n_l:], rng)
                t0 = time.perf_counter()
                _res, st = o.gate_edges(*c)
                wall = time.perf_counter() - t0
                s = st["solve"]
                rec = dict(workload=name, call="tsgo_gate_edges", pool_vertices=n_p + n_l, candidates=K, vertices=st["vertices"], width=s["batch_width"],
                           columns=s["columns"], batches=s["batches"], pcg_iters_max=s["pcg_iters_max"], fallbacks=s["fallbacks"],
                           ms_total=round(st["ms_total"], 3), ms_solve=round(s["ms_solve"], 3), ms_readout=round(st["ms_readout"], 3),
                           readout_share=round(st["ms_readout"] / st["ms_total"], 5), wall_s=round(wall, 4),
                           columns_per_s=round(s["columns"] / (s["ms_solve"] / 1e3), 1), not_pd=st["not_pd"])
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                ids = np.unique(c[1])
                t0 = time.perf_counter()
                _cov, _off, js = o.joint_marginals(ids)
                wall = time.perf_counter() - t0
                rec = dict(workload=name, call="tsgo_joint_marginals", pool_vertices=n_p + n_l, candidates=K, vertices=len(ids), width=js["batch_width"],
                           columns=js["columns"], batches=js["batches"], pcg_iters_max=js["pcg_iters_max"], fallbacks=js["fallbacks"],
                           ms_total=round(js["ms_total"], 3), ms_solve=round(js["ms_solve"], 3), wall_s=round(wall, 4),
                           columns_per_s=round(js["columns"] / (js["ms_solve"] / 1e3), 1))
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
