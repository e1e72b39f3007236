"""OptimizerHip::EdgeLeverage (include/tsgo.hpp): tests/cpp/edge_leverage_demo.cpp compiles against the wrapper with -Wall -Wextra
-Werror and runs — through where a GPU is visible, to the constructor's error where none is."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_cpp_demo_compiles_and_fails_loudly_without_a_device(tmp_path):
    import torch
    lib_dir = os.path.join(ROOT, "toyslam_amd")
    if not os.path.exists(os.path.join(lib_dir, "libtsgo_hip.so")):
        pytest.fail("toyslam_amd/libtsgo_hip.so is not built (run __graft_entry__.build())")
    exe = str(tmp_path / "edge_leverage_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "edge_leverage_demo.cpp"), "-o", exe, "-L" + lib_dir, "-ltsgo_hip", "-Wl,-rpath," + lib_dir])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    if torch.cuda.is_available() or torch.cuda.device_count() > 0:
        assert p.returncode == 0, p.stderr      # a GPU is visible: the demo runs through
        assert "15 edges (12 odometry, 3 landmark), 40 unknowns, 256 samples; the last edge weights 2 axes" in p.stdout, p.stdout
    else:
        assert p.returncode == 1
        assert "no CPU fallback" in p.stderr
