"""What one round of GNC reweighting costs at config 3 (c3_100k), on ONE handle in ONE build, two ways:
  device        tsgo_gnc with inner_iterations = 0: per round one pass of k_gnc_reweight over the tables (evaluate, weight, scatter); nothing
                but the workgroup partials comes back.  ms_reweight is the hipEvent time of the passes, the probe included, so one round is
                (ms_reweight at R rounds - ms_reweight at 1 round) / (R - 1); the whole call at 1 round (probe + round + restore) is given too.
  caller_side   the round built from the calls that existed before: edge_report with records (48 B per edge back), the weights in numpy,
                tsgo_set_edge_information with the subject edges' new rows (32 B per listed edge up).  Host clock of the three steps.
for two subject sets: the whole LM class (about 1 M edges), and 1000 random ODOM edges — c3_100k has no loop closures, so these stand in
for a closure-sized set.  Every figure is the median of `--repeats` measurements after one warm-up, with the smallest and largest beside it.
One JSON line per case.

    python tools/research/gnc_timing.py [workload] [--repeats N] [--rounds R] [--out FILE]
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

BARC2 = np.array([11.345, 9.210, 9.210, 11.345, 9.210])


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def tls_weight(q, mu):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mid = np.sqrt(mu * (mu + 1.0) / q) - mu
    return np.where(q <= mu / (mu + 1.0), 1.0, np.where(q >= (mu + 1.0) / mu, 0.0, mid))


def main():
    argv = sys.argv[1:]
    opt = {"--repeats": "9", "--rounds": "9", "--out": ""}
    for k in list(opt):
        if k in argv:
            i = argv.index(k)
            opt[k] = argv[i + 1]
            del argv[i:i + 2]
    name = argv[0] if argv else "c3_100k"
    repeats, rounds = int(opt["--repeats"]), int(opt["--rounds"])
    g = synth.make_config(name)
    E = g.n_edges
    rng = np.random.default_rng(0)
    lines = []

    def emit(case, rec):
        lines.append(json.dumps(dict(workload=name, edges=E, case=case, repeats=repeats, **rec)))
        print(lines[-1], flush=True)

    subjects = {"lm_class": g.e_type == 1, "odom_1000": np.zeros(E, bool)}
    subjects["odom_1000"][rng.choice(np.where(g.e_type == 0)[0], 1000, replace=False)] = True
    o = HipOptimizer()
    try:
        o.set_robust(all="none"); o.set_graph(g); o.optimize(2)
        base = o.edge_information()
        for what, subj in subjects.items():
            mask = subj.astype(np.uint8)
            idx = np.where(subj)[0].astype(np.int64)
            # thresholds: the defaults, lowered where the subject set would otherwise be all inliers at these estimates (the largest q is at
            # least 4, so rounds run; what a pass costs does not depend on the value); mu_step 1.05 keeps that edge inside the band
            s_max = float(o.edge_report()[0]["s"][idx].max())
            barc2 = [float(min(v, s_max / 4.0)) if (g.e_type[idx] == t).any() else float(v) for t, v in enumerate(BARC2)]
            b = np.array(barc2)[g.e_type[idx]]

            def device(r):
                t0 = time.perf_counter()
                st = o.gnc(barc2=barc2, subject=mask, inner_iterations=0, rounds_max=r, mu_step=1.05, keep_weights=False, weights=False)
                assert st["rounds"] == r, (what, st["rounds"], st["stop"])
                return 1e3 * (time.perf_counter() - t0), st

            device(1); device(rounds)      # warm-up: the maps of the structure are built by the first call
            one = [device(1) for _ in range(repeats)]
            many = [device(rounds) for _ in range(repeats)]
            per_round = [(m[1]["ms_reweight"] - a[1]["ms_reweight"]) / (rounds - 1) for a, m in zip(one, many)]
            emit("device_" + what, dict(subject=int(subj.sum()), rounds=rounds, ms_reweight_per_round=spread(per_round),
                                        ms_reweight_probe_and_one_round=spread([st["ms_reweight"] for _ms, st in one]),
                                        call_ms_one_round=spread([ms for ms, _st in one]), q_max=one[0][1]["q_max"], barc2=barc2))
            mu = float(one[0][1]["mu"][0])

            def caller_side():
                t0 = time.perf_counter()
                rec, _summary = o.edge_report()
                t1 = time.perf_counter()
                w = tls_weight(rec["s"][idx] / b, mu)
                rows = base[idx] * w[:, None]
                t2 = time.perf_counter()
                o.set_edge_information(rows, idx)
                t3 = time.perf_counter()
                return [1e3 * (t3 - t0), 1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t3 - t2)], w

            caller_side()
            runs = []
            for _ in range(repeats):
                o.set_edge_information(base[idx], idx)      # (untimed: the base information again, as the device call leaves it)
                runs.append(caller_side()[0])
            o.set_edge_information(base[idx], idx)
            w = caller_side()[1]
            held = o.edge_information()
            o.set_edge_information(base[idx], idx)
            st = o.gnc(barc2=barc2, subject=mask, inner_iterations=0, rounds_max=1)      # the two ways give the same weights and the same tables
            agree = bool(np.allclose(st["w"][idx], w, rtol=1e-12, atol=0) and np.allclose(o.edge_information(), held, rtol=1e-12, atol=0))
            o.set_edge_information(base[idx], idx)
            emit("caller_side_" + what, dict(subject=int(subj.sum()), round_ms=spread([r[0] for r in runs]), edge_report_ms=spread([r[1] for r in runs]),
                                             numpy_ms=spread([r[2] for r in runs]), set_edge_information_ms=spread([r[3] for r in runs]), same_weights=agree))
    finally:
        o.close()
    if opt["--out"]:
        with open(opt["--out"], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
