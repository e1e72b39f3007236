"""The (name, where, bytes) list of tsgo_profile_iteration for every (case, rung) of tests/precond_cases.PAIRS — each branch of the
V-cycle, every cycle vector type and cycle storage — and for config 3 of bench.py (100 000 poses: 16-lane rows, the XCD-aware workgroup
map).  Graphs and handles are made as the tests and the benchmark make them, so two builds of the library can be compared line by line:
    python tools/research/profile_names.py > names.txt
The launch layer formats these names from the template arguments of each launch (pick() / kernel_name(), tsgo_hip.hip)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests import precond_cases as pc
from toyslam_amd import synth
from toyslam_amd.optimizer import HipOptimizer


def show(title, o):
    print("== %s" % title)
    for e in o.profile_iteration(2):
        print("%-52s | %-36s | %.17g" % (e["name"], e["where"], e["bytes"]))


for case, rung in pc.PAIRS:
    c, r = pc.CASES[case], pc.RUNGS[rung]
    kw = dict(pcg_rel_tol=1e-10, testing=True)
    kw.update(c["kw"])
    kw.update(cycle_storage=r["storage"], precision=r["precision"])
    env = dict(c["env"])
    if r["vec64"]:
        env["TSGO_CYCLE_VEC64"] = "1"
    with pc.Env(env):
        o = HipOptimizer(**kw)
        try:
            o.set_graph(c["graph"]())
            show("%s / %s" % (case, rung), o)
        finally:
            o.close()

o = HipOptimizer(precision=64, pcg_rel_tol=1e-10, use_graphs="auto", preconditioner="amg", cycle_level0="implicit", cycle_storage=16)
try:
    o.set_graph(synth.make_config("c3_100k", seed=0))
    o.optimize(2)
    show("c3_100k", o)
finally:
    o.close()
