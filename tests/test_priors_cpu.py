"""Unary priors (edge types 3 and 4, include/tsgo.h) on the host side: validation, the wire codec's refusal, the slot tables and
multigrid patterns they leave alone, and the Python and C++ graph builders."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import priors, util
from toyslam_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layout(g):
    lib = _lib.host_lib(); info = _lib.tsgo_layout_info(); cg = g.c_struct()
    rc = lib.tsgo_layout_probe(C.byref(cg), 0, 1, 0, 0, C.byref(info))
    return rc, lib.tsgo_last_error().decode(), info


def _amg_checksum(g):
    lib = _lib.host_lib(); info = _lib.tsgo_amg_info(); cg = g.c_struct()
    _lib.check(lib, lib.tsgo_amg_probe(C.byref(cg), C.byref(info)), "tsgo_amg_probe")
    return info.checksum


def test_priors_take_no_slot():
    g = synth.make(500, 6, seed=2)
    gp = priors.with_priors(g, seed=1)
    assert (gp.e_type == 3).sum() > 50 and (gp.e_type == 4).sum() > 50
    rc0, _, a = _layout(g)
    rc1, err, b = _layout(gp)
    assert rc0 == 0 and rc1 == 0, err
    fields = ("n_pose", "n_lm_local", "n_lm_edges_local", "n_odom_slots", "rows_by_pose", "rows_by_lm", "rows_odom")
    assert [getattr(a, f) for f in fields] == [getattr(b, f) for f in fields]


@pytest.mark.parametrize("case", ["pose_prior_on_a_landmark", "landmark_prior_on_a_pose", "pose_prior_with_two_ids", "landmark_prior_with_two_ids"])
def test_invalid_priors_are_rejected(case):
    g = synth.make(60, 4, seed=1)
    poses, lms = g.v_id[g.v_type == 0], g.v_id[g.v_type == 1]
    t, a, b, msg = {"pose_prior_on_a_landmark": (3, lms[2], lms[2], "must sit on an Se2 vertex"),
                    "landmark_prior_on_a_pose": (4, poses[3], poses[3], "must sit on a Point2 vertex"),
                    "pose_prior_with_two_ids": (3, poses[3], poses[4], "must give the same vertex id twice"),
                    "landmark_prior_with_two_ids": (4, lms[2], lms[3], "must give the same vertex id twice")}[case]
    bad = priors.append_edges(g, [t], [[a, b]], [np.r_[1.0, 2.0, 0.3, np.zeros(6)]], [[1.0, 1.0, 1.0]])
    rc, err, _ = _layout(bad)
    assert rc != 0 and msg in err, err
    assert ("pose prior" if t == 3 else "landmark prior") in err


def test_the_wire_codec_refuses_priors():
    g = synth.make(30, 4, seed=1)
    lib = _lib.host_lib()
    for t in (3, 4):
        gp = priors.with_priors(g, frac_pose=0.3 if t == 3 else 0.0, frac_lm=0.3 if t == 4 else 0.0, seed=2, n_far=0, n_dup=0)
        assert (gp.e_type == t).sum() > 0 and not np.any(gp.e_type == 7 - t)
        cg = gp.c_struct()
        n = lib.tsgo_wire_encode_request(C.byref(cg), None, 0)
        err = lib.tsgo_last_error()
        assert n < 0 and b"ODOM (0) and LM (1) edges only" in err and b"priors (3, 4)" in err, err
    # the decoder: a request whose first edge says type 3 / 4
    cg = g.c_struct()
    n = lib.tsgo_wire_encode_request(C.byref(cg), None, 0)
    buf = (C.c_uint8 * n)()
    assert lib.tsgo_wire_encode_request(C.byref(cg), buf, n) == n
    payload = bytearray(bytes(buf)[4:])
    off = 4 + sum(20 if t == 0 else 16 for t in g.v_type) + 4          # vertex count, vertices, edge count
    for t, name in ((3, b"pose prior"), (4, b"landmark prior")):
        p = bytearray(payload); p[off:off + 4] = struct.pack("<I", t)
        h = C.c_void_p()
        rc = lib.tsgo_wire_decode(bytes(p), len(p), C.byref(h))
        err = lib.tsgo_last_error()
        if h.value:
            lib.tsgo_wire_free(h)
        assert rc != 0 and name in err and b"behind the C ABI only" in err, err


def test_priors_change_no_pattern():
    """Priors enter the diagonal blocks only: the slot tables, numbering and multigrid patterns handed to the device are the same bytes."""
    for g in (util.c1_arrays(), synth.make(3000, 8, loop_closures=10, seed=5)):
        gp = priors.with_priors(g, seed=3)
        assert _amg_checksum(gp) == _amg_checksum(g)
        free = priors.append_edges(g, [], [], [], [], fixed=[])
        assert _amg_checksum(priors.with_priors(g, seed=3, fixed=[])) == _amg_checksum(free)


def test_python_and_cpp_builders_give_the_same_arrays(tmp_path):
    from toyslam_amd.graph import (EdgeLandmark2d, EdgeLandmarkPrior2d, EdgeOdometry2d, EdgePosePrior2d, GraphArrays, OptGraph, Vertex2d,
                                   VertexPose2d)
    exe = str(tmp_path / "prior_graph_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "prior_graph_dump.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    v = [ln.split()[1:] for ln in out if ln.startswith("v ")]
    e = [ln.split()[1:] for ln in out if ln.startswith("e ")]
    f = [int(ln.split()[1]) for ln in out if ln.startswith("f ")]

    def pose(x, y, t):
        c, s = np.cos(t), np.sin(t)
        return VertexPose2d(np.array([[c, -s, x], [s, c, y], [0, 0, 1.0]]))
    og = OptGraph()
    og.add_vertex(0, pose(1.0, 2.0, 0.3), fixed=True); og.add_vertex(1, pose(2.0, 2.5, 0.4)); og.add_vertex(2, Vertex2d([3.0, 1.0]))
    c, s = np.cos(0.1), np.sin(0.1)
    og.add_edge(EdgeOdometry2d(0, 1, np.array([[c, -s, 1.0], [s, c, 0.5], [0, 0, 1.0]]), np.diag([4.0, 4.0, 65.0])))
    og.add_edge(EdgeLandmark2d(0, 2, np.array([2.2, 0.4]), np.diag([44.0, 44.0])))
    og.add_edge(EdgePosePrior2d(1, np.array([1.9, 2.4, 0.35]), np.diag([10.0, 20.0, 30.0])))
    og.add_edge(EdgeLandmarkPrior2d(2, np.array([3.1, 0.9]), np.diag([5.0, 6.0])))
    pe, le = og.get_edges()[2], og.get_edges()[3]
    assert (pe.get_type(), pe.get_id(0), pe.get_id(1), le.get_type(), le.get_id(0), le.get_id(1)) == (3, 1, 1, 4, 2, 2)
    a = GraphArrays.from_optgraph(og)
    np.testing.assert_array_equal(a.v_id, [int(r[0]) for r in v]); np.testing.assert_array_equal(a.v_type, [int(r[1]) for r in v])
    np.testing.assert_allclose(a.v_pos, np.array([[float(x) for x in r[2:]] for r in v]), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(a.e_type, [int(r[0]) for r in e])
    np.testing.assert_array_equal(a.e_ids, np.array([[int(r[1]), int(r[2])] for r in e]))
    np.testing.assert_allclose(a.e_meas, np.array([[float(x) for x in r[3:12]] for r in e]), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(a.e_inf, np.array([[float(x) for x in r[12:15]] for r in e]))
    np.testing.assert_array_equal(a.fixed, f)
    # a pose prior given as a 3x3 transform flattens to the same (x, y, theta)
    t = np.array([[np.cos(0.35), -np.sin(0.35), 1.9], [np.sin(0.35), np.cos(0.35), 2.4], [0, 0, 1.0]])
    np.testing.assert_allclose(EdgePosePrior2d(1, t, np.eye(3)).measurement, [1.9, 2.4, 0.35], rtol=0, atol=1e-15)


def test_the_python_encoder_refuses_prior_edges():
    from toyslam_amd import remote
    from toyslam_amd.graph import EdgePosePrior2d, OptGraph, VertexPose2d
    og = OptGraph()
    og.add_vertex(0, VertexPose2d(np.eye(3)))
    og.add_edge(EdgePosePrior2d(0, [0.1, 0.2, 0.0], np.eye(3)))
    with pytest.raises(RuntimeError, match="priors"):
        remote.graph_to_bytes(og)
