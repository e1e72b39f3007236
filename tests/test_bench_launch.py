"""`bench.py --gpus N` started like the N = 1 line (no launcher around it) starts its own ranks, fails loudly without GPUs, and cannot
hang: every rank's watchdog names the phase it is stuck in, and the parent kills the process group at its deadline.  The same
spawn path is rehearsed end to end over gloo + the CPU twin (tests/bench_dry_run.py)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def bench(*args, env=None, timeout=240):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None); e.pop("RANK", None); e.pop("LOCAL_RANK", None)
    e["OMP_WAIT_POLICY"] = "PASSIVE"
    e.update(env or {})
    t0 = time.time()
    p = subprocess.run([sys.executable, BENCH] + list(args), cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    return p.returncode, p.stdout, p.stderr, time.time() - t0


@pytest.mark.skipif(torch.cuda.device_count() >= 2, reason="needs a box with fewer than 2 GPUs")
def test_two_gpus_asked_for_on_a_box_without_them_fails_in_seconds_and_says_why():
    rc, out, err, dt = bench("--gpus", "2", "--steps", "2", "--warmup", "1")
    assert rc != 0
    assert "2 GPUs needed, %d visible" % torch.cuda.device_count() in err, err[-2000:]
    assert out.strip() == ""                      # no JSON line from a run that did not happen
    assert dt < 90, dt


def test_dry_run_of_the_two_rank_launch_path_prints_one_json_line():
    rc, out, err, _ = bench("--gpus", "2", "--steps", "2", "--warmup", "1", "--dry-run-cpu")
    assert rc == 0, err[-3000:]
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out
    d = json.loads(lines[0])
    assert d["ranks"] == 2 and d["value"] is None and "dry_run" in d
    assert d["all_reduce_calls"] > 10 and d["chi2_first_last"][1] < d["chi2_first_last"][0]


def test_a_rank_that_never_reaches_the_first_all_reduce_is_named_and_the_run_ends_non_zero():
    rc, out, err, dt = bench("--gpus", "2", "--steps", "2", "--warmup", "1", "--dry-run-cpu", "--phase-timeout", "5", env={"TSGO_DRY_RUN_STALL_RANK": "1"})
    assert rc != 0
    assert "phase 'first all-reduce on the data path' has not ended after 5 s" in err, err[-3000:]
    assert "STUCK in first all-reduce" in err
    assert out.strip() == ""
    assert dt < 120, dt


def test_the_parent_kills_its_ranks_at_the_launch_deadline():
    # the ranks' own watchdogs are set far out: the parent's deadline is what ends this run
    rc, out, err, dt = bench("--gpus", "2", "--steps", "2", "--warmup", "1", "--dry-run-cpu", "--phase-timeout", "600", "--launch-timeout", "12",
                             env={"TSGO_DRY_RUN_STALL_RANK": "0"})
    assert rc == 4, (rc, err[-3000:])
    assert "killing the process group" in err and "first all-reduce on the data path" in err
    assert dt < 120, dt
    # nothing of the run is left behind
    time.sleep(1.0)
    left = subprocess.run(["pgrep", "-f", "bench.py --gpus 2 --steps 2 --warmup 1 --dry-run-cpu --phase-timeout 600"], capture_output=True, text=True).stdout.split()
    assert not left, left


@pytest.mark.gpu
def test_the_bench_line_keeps_its_contract_on_one_gpu():
    """One small run of bench.py --full as the driver starts it (no launcher, N = 1), and one with the collective code path forced (a one-rank
    RCCL communicator, tsgo_comm_selftest): ONE JSON line on stdout with the fields the driver and the judge read, `value` consistent
    with the timed region, `roofline` and `cpu_baseline` objects present and complete."""
    rc, out, err, _ = bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "c2_10k", "--full", timeout=600)
    assert rc == 0, err[-3000:]
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and d["config"]["workload"].startswith("c2_10k") and "model" not in d["config"]
    n_edges = 109999
    assert abs(d["value"] - n_edges / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0 < r["frac"] < 1
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["us_per_launch"] * 1e-6) / 1e9) <= 1e-6 * r["achieved"]
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample", "host", "all_cores", "one_thread", "reference_dense_c1"):
        assert k in c, k
    assert c["kind"] == "port" and c["one_thread"]["cores"] == 1 and c["host"]["nproc"] >= 1 and c["host"]["model"]
    for prec in ("f32", "f64"):
        ph = c["reference_dense_c1"][prec]
        assert ph["ms_dense_solve"] > 10 * ph["ms_linearize"] > 0 and ph["ms_update"] >= 0
    assert d["rccl_ranks"] == 1 and d["request_parallel"] is None
    rc, out, err, _ = bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--workload", "c2_10k", "--full", "--no-cpu", "--no-conv", "--force-collective", timeout=600)
    assert rc == 0, err[-3000:]
    d2 = json.loads([l for l in out.splitlines() if l.strip()][-1])
    assert d2["rccl_ranks"] == 1 and "collective code path forced" in d2["config"]["parallelism"]
    assert d["allreduce_us"] is None and set(d2["allreduce_us"]) == {"product_3P", "linearisation_18P", "level0_blocks_60MB"}      # tsgo_comm_time_allreduce: RCCL calls of the solver's three buffer sizes
    assert all(v["us"] > 0 and v["bytes"] > 0 for v in d2["allreduce_us"].values()), d2["allreduce_us"]
    assert abs(d2["chi2_first_last"][0] - d["chi2_first_last"][0]) <= 1e-9 * d["chi2_first_last"][0]


@pytest.mark.gpu
def test_a_plain_bench_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """bench.py without --full: the headline line alone (no probe, convergence or CPU leg after the timed region), and --dump-outputs
    writes what the last timed step left: every vertex, its chi^2 and ||delta||, as float64."""
    rc, out, err, _ = bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "c2_10k", "--dump-outputs", str(tmp_path / "out"), timeout=600)
    assert rc == 0, err[-3000:]
    lines = [l for l in out.splitlines() if l.strip()]
    assert len(lines) == 1, out[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["metric"] == "edges/sec per GN iter" and d["unit"] == "edges/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 3 and d["warmup"] == 1
    assert abs(d["value"] - 109999 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    for k in ("roofline", "iters_to_chi2_tol", "cpu_baseline"):
        assert k not in d, k
    assert d["allreduce_us"] is None and d["request_parallel"] is None
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == ["chi2.npy", "delta_norm.npy", "vertices.npy"], files
    v = np.load(tmp_path / "out" / "vertices.npy")
    chi2 = np.load(tmp_path / "out" / "chi2.npy")
    dn = np.load(tmp_path / "out" / "delta_norm.npy")
    assert v.dtype == chi2.dtype == dn.dtype == np.float64
    assert v.ndim == 2 and v.shape[1] == 3 and v.shape[0] > 10000 and np.isfinite(v).all()
    assert chi2.shape == (1,) and abs(chi2[0] - d["chi2_first_last"][1]) <= 1e-12 * chi2[0]       # the last timed step's linearisation
    assert dn.shape == (1,) and dn[0] > 0
    # the vertices are those of the LAST timed step: the same 1 + 3 iterations replayed here through the same C ABI, and not the input
    from toyslam_amd import synth
    from toyslam_amd.optimizer import HipOptimizer
    g = synth.make_config("c2_10k")
    assert v.shape == g.v_pos.shape and (v != g.v_pos).any(axis=1).mean() > 0.9
    o = HipOptimizer(pcg_rel_tol=1e-10)
    try:
        o.set_graph(g)
        for _ in range(1 + 3):
            r = o.optimize(1)
        v_here = o.vertices()
    finally:
        o.close()
    assert abs(r["chi2_last"] - chi2[0]) <= 1e-9 * chi2[0] and np.abs(v - v_here).max() <= 1e-9 * np.abs(v_here).max()
    # same arguments, same inputs: a second run dumps the same arrays, bit for bit
    rc, out, err, _ = bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "c2_10k", "--dump-outputs", str(tmp_path / "again"), timeout=600)
    assert rc == 0, err[-3000:]
    for name in files:
        assert np.array_equal(np.load(tmp_path / "out" / name), np.load(tmp_path / "again" / name)), name


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_outputs_gathers_a_sharded_run_from_the_owners_and_samples_large_graphs(tmp_path, monkeypatch):
    """bench.dump_outputs without a device: three shards as HipOptimizer.vertices() returns them (replicated poses, its own landmark
    range, the input everywhere else) merge into the full state on rank 0 only; above DUMP_MAX_ROWS a fixed seeded sample is written
    with the rows it kept."""
    bench_m = _bench_module()
    rng = np.random.default_rng(1)
    n, n_poses = 60, 20
    v_in = rng.normal(size=(n, 3))
    truth = v_in + rng.normal(size=(n, 3))
    shards = []
    for own in np.array_split(np.arange(n_poses, n), 3):
        v = v_in.copy(); v[:n_poses] = truth[:n_poses]; v[own] = truth[own]
        shards.append(v)

    class Shard:
        def __init__(self, r):
            self.r = r

        def vertices(self):
            return shards[self.r].copy()

    g = type("G", (), {"v_pos": v_in})()
    last = {"chi2_last": 5.0, "delta_norm": 0.5}
    for r in (1, 2, 0):           # every rank calls it; only rank 0 writes
        bench_m.dump_outputs(str(tmp_path / "sharded"), Shard(r), last, g, r, gather=lambda v: [s.copy() for s in shards])
    assert sorted(os.listdir(tmp_path / "sharded")) == ["chi2.npy", "delta_norm.npy", "vertices.npy"]
    assert np.array_equal(np.load(tmp_path / "sharded" / "vertices.npy"), truth)
    assert np.load(tmp_path / "sharded" / "chi2.npy").tolist() == [5.0] and np.load(tmp_path / "sharded" / "delta_norm.npy").tolist() == [0.5]
    assert np.array_equal(bench_m.merge_shards(v_in, shards), truth)

    monkeypatch.setattr(bench_m, "DUMP_MAX_ROWS", 25)
    for k in ("a", "b"):
        bench_m.dump_outputs(str(tmp_path / k), Shard(0), last, g, 0)
    rows = np.load(tmp_path / "a" / "vertex_rows.npy")
    assert rows.dtype == np.float64 and len(rows) == 25 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "vertices.npy"), shards[0][rows.astype(int)])
    assert np.array_equal(rows, np.load(tmp_path / "b" / "vertex_rows.npy"))                      # the same sample every run
