// knobs.h — what the environment may and may not change.
//
// OPERATIONAL variables (thread count, message cap, verbosity and phase timings on stderr) are read by the shipped library and
// server.  Variables that change NUMERICS, pick research variants or inject failures exist only in builds made with
// -DTSGO_TESTING — libtsgo_hip_testing.so (what the hook-using tests load, toyslam_amd/build.py) and the CPU twin (oracle/Makefile):
// the shipped libtsgo_hip.so / libtsgo_host.so / graph_optimizer do not even contain their names, so a production process cannot
// change its answers, or declare a solver failure, because of an environment it inherited.
#pragma once
#include <cstdlib>

#ifdef TSGO_TESTING
#define TSGO_RESEARCH_ENV(name) std::getenv(name)
#define TSGO_RESEARCH_INT(name, dflt) (std::getenv(name) ? std::atoi(std::getenv(name)) : (dflt))
#define TSGO_RESEARCH_FLOAT(name, dflt) (std::getenv(name) ? std::atof(std::getenv(name)) : (double)(dflt))
#else
#define TSGO_RESEARCH_ENV(name) (static_cast<const char*>(nullptr))
#define TSGO_RESEARCH_INT(name, dflt) (dflt)
#define TSGO_RESEARCH_FLOAT(name, dflt) ((double)(dflt))
#endif

// TSGO_CYCLE_VEC64=1: the multigrid cycle's vectors below level 0 in the engine's own type (f64) instead of CycVec (f32) —
// the A/B of that choice (tests/test_gpu_cycle_f32_vectors.py, tests/research/bench_with_lib.py).  Testing builds only.
#ifdef TSGO_TESTING
#define TSGO_CYCLE_VEC64() (TSGO_RESEARCH_INT("TSGO_CYCLE_VEC64", 0) != 0)
#else
#define TSGO_CYCLE_VEC64() false
#endif

// The A/B switch of how the host thread follows the device through a Gauss-Newton step (engine/engine_solve.inc).
// It changes no result: every build reads it, once per handle (tsgo_create), so that the product library can be measured both ways.
//   TSGO_STEP_DRAINS=1  chi^2 and ||delta|| come back by copy command + stream synchronisation, k_save_x and k_pose_update are two launches
//                       (default: the device reports them into pinned memory, k_report, and the host polls; one launch, k_save_update)
inline bool tsgo_step_drains() { const char* e = std::getenv("TSGO_STEP_DRAINS"); return e && std::atoi(e) != 0; }
