"""tsgo_joint_marginals at the boundary, without a device: declared, bound, exported, safe on a NULL handle, and reachable from the C++
wrapper."""
import ctypes as C
import os
import re
import subprocess

from toyslam_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_in_the_header_and_listed_in_the_bindings():
    h = open(os.path.join(ROOT, "include", "tsgo.h")).read()
    assert re.search(r"\bint\s+tsgo_joint_marginals\s*\(", h)
    assert "tsgo_joint_marginals" in _lib.DEVICE_SYMBOLS


def test_the_library_exports_it():
    so = build.build_hip()
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT tsgo_joint_marginals\b", out)


def test_null_handle_returns_an_error():
    L = _lib.hip_lib()
    ids = (C.c_uint32 * 1)(0)
    dim = C.c_int32(-1)
    st = _lib.tsgo_marginal_stats()
    assert L.tsgo_joint_marginals(None, C.cast(ids, C.c_void_p), 1, 0.0, None, 0, C.byref(dim), C.byref(st)) < 0
    assert b"null" in L.tsgo_last_error()
    cov = (C.c_double * 9)()
    assert L.tsgo_joint_marginals(None, C.cast(ids, C.c_void_p), 1, 0.0, C.cast(cov, C.c_void_p), 9, None, None) < 0


def test_the_wrapper_has_the_method():
    from toyslam_amd.optimizer import HipOptimizer
    assert callable(getattr(HipOptimizer, "joint_marginals", None))


def test_the_cpp_wrapper_compiles_a_call(tmp_path):
    src = tmp_path / "joint.cpp"
    src.write_text("#include <tsgo.hpp>\n"
                   "#include <cstdio>\n"
                   "int main() {\n"
                   "    tsgo::OptimizerHip opt(5);\n"
                   "    int dim = 0;\n"
                   "    const std::vector<double> cov = opt.JointMarginals({0u, 1u}, &dim);\n"
                   "    const std::vector<double> again = opt.JointMarginals({0u});\n"
                   "    std::printf(\"%d %zu %zu\\n\", dim, cov.size(), again.size());\n"
                   "    return 0;\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src)])
