"""The device pattern builders (toyslam_amd/csrc/tsgo_sym_kernels.h) list by list at their table edges: every kernel of that file run on
caller-given integer arrays through the testing library (include/tsgo_testing.h: tsgo_testing_sym_scan, tsgo_testing_sym_product,
tsgo_testing_schur_pattern — the engine's own launch helpers) and compared, with exact equality on every array it returns, with the
reference of tests/sym_patterns.py and, for the products, with the host builder run in the same process on the same arrays: the
"identical, entry by entry" of the kernels' header.  Integer arrays only: no tolerance."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import sym_patterns as sp
from toyslam_amd import _lib

pytestmark = pytest.mark.gpu

PRODUCT_RUNS = [(name, upper) for name, p in sp.product_cases().items() for upper in ((0, 1) if p.square else (0,))]
PRODUCT_IDS = ["%s-upper%d" % r for r in PRODUCT_RUNS]
GUARD = 16                               # entries past every capacity that must stay untouched
SENTINEL = -123456789


def _i32(values):
    return np.ascontiguousarray(np.asarray(values, dtype=np.int64).astype(np.int32))


def _u32(values):
    return np.ascontiguousarray(np.asarray(values, dtype=np.int64).astype(np.uint32))


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _out(count, dtype=np.int32):
    return np.full(count + GUARD, SENTINEL, dtype=np.int64).astype(dtype)


def _untouched(a, count):
    return bool(np.all(a[count:] == np.int64(SENTINEL).astype(a.dtype)))


def run_product(builder, p, upper, cap_blocks=None, cap_pairs=None):
    """(rc, flags, arrays): the arrays cut to what the call says it wrote; every guard zone checked."""
    lib = _lib.hip_testing_lib()
    ref = sp.product_reference(p.name, upper)
    cb = len(ref["zcol"]) if cap_blocks is None else cap_blocks
    cp = len(ref["px"]) if cap_pairs is None else cap_pairs
    bufs = dict(zptr=_out(p.n + 1), zcol=_out(cb), pl_ptr=_out(cb + 1), px=_out(cp), py=_out(cp), mirror=_out(cb), upper=_out(cb), n_upper=_out(p.n))
    o = _lib.tsgo_testing_sym_out()
    o.cap_blocks, o.cap_pairs = cb, cp
    for k, a in bufs.items():
        setattr(o, k, _ptr(a))
    x = [_i32(p.xptr), _i32(p.xcol), None if p.alias is None else _i32(p.alias), _i32(p.yptr), _i32(p.ycol)]
    rc = lib.tsgo_testing_sym_product(builder, upper, p.n, _ptr(x[0]), _ptr(x[1]), _ptr(x[2]), p.ny, p.nc, _ptr(x[3]), _ptr(x[4]), C.byref(o))
    sizes = dict(zptr=p.n + 1, zcol=cb, pl_ptr=cb + 1, px=cp, py=cp, mirror=cb, upper=cb, n_upper=p.n)
    for k, a in bufs.items():
        assert _untouched(a, sizes[k]), "written past the capacity of " + k
    flags = dict(declined=o.declined, not_symmetric=o.not_symmetric)
    if rc != 0 or o.declined:
        return rc, flags, {}
    wrote = dict(zptr=p.n + 1, zcol=o.nnz, pl_ptr=o.nnz + 1, px=o.pairs, py=o.pairs)
    if upper:
        wrote.update(mirror=o.nnz, upper=o.upper_blocks, n_upper=p.n)
    return rc, flags, {k: bufs[k][:n] for k, n in wrote.items()}


@functools.lru_cache(maxsize=None)
def device_product(name, upper):
    return run_product(1, sp.product_cases()[name], upper)


def _assert_equals_reference(arrays, ref):
    assert sorted(arrays) == sorted(k for k in ref if k != "not_symmetric")
    for k in arrays:
        np.testing.assert_array_equal(arrays[k], np.asarray(ref[k], dtype=np.int64), err_msg=k)


# ---- k_sym_scan --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sp.SCAN_SIZES)
def test_scan_against_cumsum(n):
    values = _i32(sp.scan_input(n))
    assert len(values) == n and (n < 100 or (values == 0).sum() > n // 10)
    out = _out(n + 1)
    assert _lib.hip_testing_lib().tsgo_testing_sym_scan(n, _ptr(values), _ptr(out)) == 0
    want = np.concatenate([[0], np.cumsum(values.astype(np.int64))])
    assert want[-1] < 2 ** 31
    np.testing.assert_array_equal(out[:n + 1], want)
    assert _untouched(out, n + 1)


def test_scan_refuses_a_total_beyond_int():
    lib = _lib.hip_testing_lib()
    values = _i32([2 ** 30, 2 ** 30])
    out = _out(3)
    assert lib.tsgo_testing_sym_scan(2, _ptr(values), _ptr(out)) != 0 and b"2^31" in lib.tsgo_last_error()
    assert lib.tsgo_testing_sym_scan(2, _ptr(_i32([1, -1])), _ptr(out)) != 0
    assert _untouched(out, 0)


# ---- the products ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,upper", PRODUCT_RUNS, ids=PRODUCT_IDS)
def test_device_product_equals_the_reference(name, upper):
    p = sp.product_cases()[name]
    rc, flags, arrays = device_product(name, upper)
    assert rc == 0, _lib.hip_testing_lib().tsgo_last_error()
    assert flags["declined"] == int(p.declined)
    if p.declined:
        assert arrays == {}                                  # only the flag: nothing else was launched
        return
    ref = sp.product_reference(name, upper)
    assert flags["not_symmetric"] == ref.get("not_symmetric", 0)
    _assert_equals_reference(arrays, ref)


@pytest.mark.parametrize("name,upper", PRODUCT_RUNS, ids=PRODUCT_IDS)
def test_host_builder_in_process_equals_the_device_builder(name, upper):
    p = sp.product_cases()[name]
    rc, flags, host = run_product(0, p, upper)
    assert rc == 0, _lib.hip_testing_lib().tsgo_last_error()
    ref = sp.product_reference(name, upper)
    assert flags == dict(declined=0, not_symmetric=ref.get("not_symmetric", 0))      # the host builder takes every row
    _assert_equals_reference(host, ref)
    rc_d, flags_d, dev = device_product(name, upper)
    assert rc_d == 0
    if p.declined:
        assert flags_d["declined"] == 1
        return
    assert flags_d == flags and sorted(dev) == sorted(host)
    for k in host:
        np.testing.assert_array_equal(dev[k], host[k], err_msg=k)


def test_product_refusals():
    lib = _lib.hip_testing_lib()
    for builder in (0, 1):
        rc, _f, _a = run_product(builder, sp.product_cases()["ylen_65"], 1)                # upper with nc != n
        assert rc != 0 and b"square" in lib.tsgo_last_error()
        small = sp.product_cases()["distinct_65"]
        ref = sp.product_reference("distinct_65", 0)
        rc, _f, _a = run_product(builder, small, 0, cap_blocks=len(ref["zcol"]) - 1)       # the guard zones are checked inside
        assert rc != 0 and b"capacities" in lib.tsgo_last_error()
        rc, _f, _a = run_product(builder, small, 0, cap_pairs=len(ref["px"]) - 1)
        assert rc != 0 and b"capacities" in lib.tsgo_last_error()

    class Raw:
        """A case the Product class itself would refuse."""
        def __init__(self, name, x_rows, y_rows, nc):
            self.name, self.n, self.ny, self.nc, self.alias = name, len(x_rows), len(y_rows), nc, None
            (self.xptr, self.xcol), (self.yptr, self.ycol) = sp.csr(x_rows), sp.csr(y_rows)

    for raw, text in ((Raw("empty_rows", [[0]], [[1, 2, 1]], 3), b"twice"), (Raw("empty_rows", [[0]], [[1, 3]], 3), b"[0, nc)"),
                      (Raw("empty_rows", [[0, 1]], [[1]], 3), b"[0, ny)"), (Raw("empty_rows", [[0]], [[-1]], 3), b"[0, nc)")):
        for builder in (0, 1):
            rc, _f, _a = run_product(builder, raw, 0)          # (the name only picks capacities)
            assert rc != 0 and text in lib.tsgo_last_error(), text


# ---- level 0 -----------------------------------------------------------------------------------------------------------------------------
def run_schur(s, cap=None):
    lib = _lib.hip_testing_lib()
    ref = sp.ref_schur(s) if cap is None else None
    cb, cp, co = (len(ref["zcol"]), len(ref["slot_i"]), len(ref["os"])) if cap is None else cap
    bufs = dict(zptr=_out(s.P + 1), zcol=_out(cb), sc_ptr=_out(cb + 1), sc_optr=_out(cb + 1), slot_i=_out(cp, np.uint32), slot_k=_out(cp, np.uint32), os=_out(co, np.uint32))
    o = _lib.tsgo_testing_schur_out()
    o.cap_blocks, o.cap_pairs, o.cap_od = cb, cp, co
    for k, a in bufs.items():
        setattr(o, k, _ptr(a))
    arrays = [_i32(s.pp_ptr), _i32(s.pp_lm), _u32(s.pp_slot), _i32(s.obs_ptr), _i32(s.obs_pose), _u32(s.obs_slot), _i32(s.od_ptr), _i32(s.od_col), _u32(s.od_slot)]
    rc = lib.tsgo_testing_schur_pattern(1, s.P, s.L, *[_ptr(a) for a in arrays], s.max_pair_degree, C.byref(o))
    sizes = dict(zptr=s.P + 1, zcol=cb, sc_ptr=cb + 1, sc_optr=cb + 1, slot_i=cp, slot_k=cp, os=co)
    for k, a in bufs.items():
        assert _untouched(a, sizes[k]), "written past the capacity of " + k
    if rc != 0 or o.declined:
        return rc, o.declined, {}
    wrote = dict(zptr=s.P + 1, zcol=o.nnz, sc_ptr=o.nnz + 1, sc_optr=o.nnz + 1, slot_i=o.pairs, slot_k=o.pairs, os=o.od)
    return rc, o.declined, {k: bufs[k][:n] for k, n in wrote.items()}


@pytest.mark.parametrize("name", list(sp.schur_cases()))
def test_device_level0_equals_the_reference(name):
    s = sp.schur_cases()[name]
    if s.declined:
        rc, declined, arrays = run_schur(s, cap=(0, 0, 0))   # only the flag is asked for: the fill pass is never launched
        assert rc == 0 and declined == 1 and arrays == {}
        return
    rc, declined, arrays = run_schur(s)
    assert rc == 0, _lib.hip_testing_lib().tsgo_last_error()
    assert declined == 0
    ref = sp.schur_reference(name)
    assert sorted(arrays) == sorted(ref)
    for k in arrays:
        np.testing.assert_array_equal(arrays[k].astype(np.int64), np.asarray(ref[k], dtype=np.int64), err_msg=k)


def test_level0_refusals():
    """host/problem.cpp fills by_pose and by_lm in edge order and a pose's slots rise with an entry's rank, so the two entries of one pose
    in one observer list always come with rising slots: that is k_s0_fill's stated contract, and the entry point refuses anything else."""
    lib = _lib.hip_testing_lib()
    rc, _d, _a = run_schur(sp.descending_repeat())
    assert rc != 0 and b"rising slots" in lib.tsgo_last_error()
    ok = sp.schur_cases()["repeated_observers"]
    ref = sp.schur_reference("repeated_observers")
    full = (len(ref["zcol"]), len(ref["slot_i"]), len(ref["os"]))
    for k in range(3):
        cap = tuple(v - 1 if j == k else v for j, v in enumerate(full))
        rc, _d, _a = run_schur(ok, cap=cap)
        assert rc != 0 and b"capacities" in lib.tsgo_last_error()
