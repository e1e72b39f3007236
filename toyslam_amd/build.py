"""In-tree builds: libtsgo_hip.so (hipcc, gfx950), libtsgo_host.so (g++), graph_optimizer (server) — the product — and
libtsgo_hip_testing.so: the same sources with -DTSGO_TESTING (test hooks, research variables, the in-process all-reduce group:
csrc/host/knobs.h, include/tsgo_testing.h), loaded only by the tests that need a hook."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
HOST_SRC = ["host/problem.cpp", "host/amg.cpp", "host/codec.cpp", "host/synth.cpp", "host/host_api.cpp", "host/errors.cpp"]
HIP_SO = os.path.join(HERE, "libtsgo_hip.so")
HOST_SO = os.path.join(HERE, "libtsgo_host.so")
HIP_TESTING_SO = os.path.join(HERE, "libtsgo_hip_testing.so")
HIP_PLAIN_SO = os.path.join(HERE, "libtsgo_hip_plain.so")
# Kernarg preload (gfx950): the command processor hands the first dwords of a kernel's arguments over in SGPRs before the wave starts
# (the compiler clamps 16 to the 14 dwords left beside the kernarg pointer); csrc/tsgo_kernels.h, "Argument heads".
PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=16"]
SERVER = os.path.join(HERE, "graph_optimizer")


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def _all_sources():
    out = []
    for root, _d, files in os.walk(CSRC):
        out += [os.path.join(root, f) for f in files if f.endswith((".h", ".hip", ".cpp", ".inc"))]
    out.append(os.path.join(os.path.dirname(HERE), "include", "tsgo.h"))
    out.append(os.path.join(os.path.dirname(HERE), "include", "tsgo_testing.h"))
    return out


def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def build_host(force=False):
    if force or _newer(HOST_SO, _all_sources()):
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-pthread", "-shared", "-o", HOST_SO] + HOST_SRC
        subprocess.check_call(cmd, cwd=CSRC)
    return HOST_SO


def _hip_library(out, extra, force):
    """One hipcc command line for every build of the device library: `extra` is all that tells them apart."""
    if force or _newer(out, _all_sources()):
        cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-result"] + extra + [
               "-o", out, "tsgo_hip.hip"] + HOST_SRC + ["-lrccl", "-lpthread"]
        subprocess.check_call(cmd, cwd=CSRC)
    return out


def build_hip(force=False):
    return _hip_library(HIP_SO, PRELOAD, force)


def build_hip_testing(force=False):
    return _hip_library(HIP_TESTING_SO, ["-DTSGO_TESTING"] + PRELOAD, force)


def build_hip_plain(force=False):
    """The product library's sources WITHOUT either latency measure — no kernarg preload, and TSGO_SHUFFLE_SUMS: lane sums through
    __shfl_xor, k_cg_step's and the gates' sums one after the other (csrc/tsgo_kernels.h: lane_xor) — the B side of the bitwise
    comparisons (tests/test_gpu_kernarg_preload.py, tests/test_gpu_lane_sums.py, tests/test_kernarg_heads.py).  Not a product binary:
    build_all does not build it."""
    return _hip_library(HIP_PLAIN_SO, ["-DTSGO_SHUFFLE_SUMS"], force)


def build_server(force=False):
    src = os.path.join(CSRC, "host", "server.cpp")
    if not os.path.exists(src):
        return None
    if force or _newer(SERVER, _all_sources()):
        cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-result"] + PRELOAD + ["-o", SERVER,
               "host/server.cpp", "tsgo_hip.hip"] + HOST_SRC + ["-lrccl", "-lpthread"]
        subprocess.check_call(cmd, cwd=CSRC)
    return SERVER


def build_all(force=False):
    """The three product binaries (returned) and the testing twin of the HIP library; the two hipcc jobs of the libraries run side by side."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(3) as ex:
        jobs = [ex.submit(f, force) for f in (build_hip, build_hip_testing, build_server)]
        host = build_host(force)
        hip, _testing, server = [j.result() for j in jobs]
    return host, hip, server


if __name__ == "__main__":
    print(build_all(force=True), build_hip_plain(force=True))
