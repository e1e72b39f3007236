"""The host builder of the multigrid hierarchy's pair-list products (toyslam_amd/csrc/host/amg.cpp: spgemm_sym), compiled for the host
(tests/cpp/sym_product_dump.cpp) and compared, array by array and with exact equality, with the reference of tests/sym_patterns.py on every
product case; the reference itself against hand-written arrays; and the case generators against what their names claim.  The device
builders run the same cases in tests/test_gpu_sym_patterns.py."""
import os
import subprocess

import pytest

from tests import sym_patterns as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = [(name, upper) for name, p in sp.product_cases().items() for upper in ((0, 1) if p.square else (0,))]


@pytest.fixture(scope="module")
def host_rows(tmp_path_factory):
    """{(case, upper): the dump program's integers}, compiled and run once."""
    exe = str(tmp_path_factory.mktemp("sym_product") / "sym_product_dump")
    csrc = os.path.join(ROOT, "toyslam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I" + csrc, os.path.join(ROOT, "tests", "cpp", "sym_product_dump.cpp"),
                           os.path.join(csrc, "host", "amg.cpp"), os.path.join(csrc, "host", "problem.cpp"), "-o", exe])
    text = "\n".join(sp.product_cases()[name].text(upper) for name, upper in RUNS) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    got = [[int(x) for x in ln.split()] for ln in out if ln]
    assert len(got) == len(RUNS)
    return dict(zip(RUNS, got))


def parse_host_row(row, n, upper):
    not_symmetric, nnz, pairs = row[:3]
    at, out = 3, dict(not_symmetric=not_symmetric)
    for key, count in (("zptr", n + 1), ("zcol", nnz), ("pl_ptr", nnz + 1), ("px", pairs), ("py", pairs)) + ((("mirror", nnz),) if upper else ()):
        out[key] = row[at:at + count]
        assert len(out[key]) == count
        at += count
    assert at == len(row)
    return out


@pytest.mark.parametrize("name,upper", RUNS, ids=["%s-upper%d" % r for r in RUNS])
def test_host_builder_equals_the_reference(host_rows, name, upper):
    p = sp.product_cases()[name]
    got = parse_host_row(host_rows[(name, upper)], p.n, upper)
    want = sp.product_reference(name, upper)
    assert got.pop("not_symmetric") == want.get("not_symmetric", 0)
    for key in got:
        assert got[key] == want[key], key


# ---- the reference against arrays written by hand ------------------------------------------------------------------------------------------
def test_reference_product_by_hand():
    #      Y: row 0 = (2, 0), row 1 = (1), row 2 = (0, 1)         X: row 0 = (Y0, Y2), row 1 = (Y1, Y1)
    p = sp.Product("hand", [[0, 2], [1, 1]], [[2, 0], [1], [0, 1]], 3)
    # row 0 walks (c, x, y): (2,0,0) (0,0,1) (0,1,3) (1,1,4); row 1: (1,2,2) (1,3,2)
    assert sp.ref_product(p, 0) == dict(zptr=[0, 3, 4], zcol=[0, 1, 2, 1], pl_ptr=[0, 2, 3, 4, 6], px=[0, 1, 1, 0, 2, 3], py=[1, 3, 4, 0, 2, 2])
    q = sp.Product("hand_alias", [[0, 2], [1, 1]], [[2, 0], [1], [0, 1]], 3, alias=[9, 8, 7, 6])
    assert sp.ref_product(q, 0)["px"] == [9, 8, 8, 9, 7, 6]


def test_reference_upper_product_by_hand():
    # Z (= X, as Y is the identity): row 0 = (0, 1), row 1 = (0, 1, 2), row 2 = (1, 2): symmetric
    p = sp.Product("hand_upper", [[1, 0], [2, 0, 1], [2, 1]], [[0], [1], [2]], 3)
    assert sp.ref_product(p, 1) == dict(zptr=[0, 2, 5, 7], zcol=[0, 1, 0, 1, 2, 1, 2], pl_ptr=[0, 1, 2, 2, 3, 4, 4, 5], px=[1, 0, 4, 2, 5], py=[0, 1, 1, 2, 2],
                                        mirror=[-1, -1, 1, -1, -1, 4, -1], upper=[0, 1, 3, 4, 6], n_upper=[2, 2, 1], not_symmetric=0)
    # without block (1, 2): block (2, 1) has no mirror
    q = sp.Product("hand_bad", [[1, 0], [0, 1], [2, 1]], [[0], [1], [2]], 3)
    r = sp.ref_product(q, 1)
    assert r["not_symmetric"] == 1 and r["mirror"] == [-1, -1, 1, -1, -1, -1] and r["upper"] == [0, 1, 3, 5]


def test_reference_level0_by_hand():
    # edges in order: e0 (pose 0, lm 0), e1 (1, 0), e2 (1, 0) again, e3 (2, 0); by_pose slots: pose 0: 1; pose 1: 4, 7; pose 2: 10.
    # odometry entries (sorted by pose, slots 2, 7, 12, ...): pose 0 -> 1 (2), 0 -> 1 again (7), 1 -> 0 (12), 2 -> 0 (17)
    s = sp.Schur("hand", 3, 1, [(0, 0), (1, 0), (1, 0), (2, 0)], [(0, 1), (1, 0), (0, 1), (2, 0)])
    assert (s.pp_ptr, s.pp_slot, s.obs_pose, s.obs_slot) == ([0, 1, 3, 4], [1, 4, 7, 10], [0, 1, 1, 2], [1, 4, 7, 10])
    assert (s.od_ptr, s.od_col, s.od_slot) == ([0, 2, 3, 4], [1, 1, 0, 0], [2, 7, 12, 17])
    assert sp.ref_schur(s) == dict(zptr=[0, 3, 6, 9], zcol=[0, 1, 2, 0, 1, 2, 0, 1, 2],
                                   sc_ptr=[0, 0, 2, 3, 5, 5, 7, 8, 10, 10], slot_i=[1, 1, 1, 4, 7, 4, 7, 10, 10, 10], slot_k=[4, 7, 10, 1, 1, 10, 10, 1, 4, 7],
                                   sc_optr=[0, 0, 2, 2, 3, 3, 3, 4, 4, 4], os=[2, 7, 12, 17])
    # the same landmark with max_pair_degree = 3 < its 4 observers: no pair, no block beyond the diagonal and the odometry neighbours
    t = sp.Schur("hand_hub", 3, 1, [(0, 0), (1, 0), (1, 0), (2, 0)], [(0, 1), (1, 0), (0, 1), (2, 0)], max_pair_degree=3)
    assert sp.ref_schur(t) == dict(zptr=[0, 2, 4, 6], zcol=[0, 1, 0, 1, 0, 2], sc_ptr=[0] * 7, slot_i=[], slot_k=[], sc_optr=[0, 0, 2, 3, 3, 4, 4], os=[2, 7, 12, 17])


# ---- the generators produce what they claim -----------------------------------------------------------------------------------------------
def test_distinct_and_declined_cases_have_the_columns_their_names_say():
    cases = sp.product_cases()
    for D in (1, 2, 3, 5, 64, 65, 127, 128, 129, 513, 1023, 1024):
        p = cases["distinct_%d" % D]
        assert p.distinct(p.big_row) == D and not p.declined
        assert max(p.distinct(i) for i in range(p.n) if i != p.big_row) < 64
    for D in (1023, 1024):                                   # reached over several X blocks, not in ascending input order
        p = cases["distinct_%d" % D]
        cols = [c for c, _x, _y in p.row_triples(p.big_row)]
        assert p.xptr[p.big_row + 1] - p.xptr[p.big_row] >= 4 and cols != sorted(cols) and len(cols) > D
    for name, D, at in (("declined_1025_first", 1025, "first"), ("declined_1025_last", 1025, "last"), ("declined_1025_middle", 1025, "middle"), ("declined_1500", 1500, "middle")):
        p = cases[name]
        assert p.distinct(p.big_row) == D and p.declined and p.xptr[p.big_row + 1] - p.xptr[p.big_row] >= 4
        assert dict(first=p.big_row == 0, last=p.big_row == p.n - 1, middle=0 < p.big_row < p.n - 1)[at] and p.n >= 4
        assert [i for i in range(p.n) if p.distinct(i) > sp.MAX_DISTINCT] == [p.big_row]
    for L in (2049, 3000):
        p = cases["declined_yrow_%d" % L]
        assert max(p.yptr[k + 1] - p.yptr[k] for k in range(p.ny)) == L > sp.TABLE and p.declined
        assert [p.distinct(i) > sp.MAX_DISTINCT for i in range(p.n)] == [False, True, False]
    assert [name for name, p in cases.items() if p.declined] == [n for n in cases if n.startswith("declined_")]
    for L in (1, 63, 64, 65, 129, 200):
        p = cases["ylen_%d" % L]
        assert p.yptr[1] - p.yptr[0] == L
    assert all(p.n <= 64 for p in cases.values())


def _slots_after_inserting(cols):
    """Linear probing with wrap-around, as tsgo_sym_kernels.h: sym_insert does it (one insert after the other)."""
    keys = {}
    for c in cols:
        h = sp.sym_hash(c)
        while h in keys and keys[h] != c:
            h = (h + 1) & (sp.TABLE - 1)
        keys[h] = c
    return keys


def test_hash_cases_cluster_and_wrap():
    cases = sp.product_cases()
    assert sp.sym_hash(0) == 0 and sp.sym_hash(1) == 2654435761 >> 21 and sp.sym_hash(1 << 19) == ((2654435761 << 19) & 0xFFFFFFFF) >> 21
    one = cases["hash_one_bucket"]
    cols = {c for c, _x, _y in one.row_triples(0)}
    assert len(cols) == 200 and {sp.sym_hash(c) for c in cols} == {777}
    assert sorted(_slots_after_inserting(cols)) == list(range(777, 977))          # one chain of 200
    wrap = cases["hash_wrap_2047"]
    cols = {c for c, _x, _y in wrap.row_triples(0)}
    assert len(cols) == 150 and {sp.sym_hash(c) for c in cols} == {sp.TABLE - 1}
    assert sorted(_slots_after_inserting(cols)) == list(range(149)) + [sp.TABLE - 1]      # probing wraps past slot 2047 to slot 0
    mixed = cases["hash_mixed"]
    cols = {c for c, _x, _y in mixed.row_triples(1)}
    by_bucket = [sum(1 for c in cols if sp.sym_hash(c) == b) for b in (777, sp.TABLE - 1)]
    assert by_bucket == [120, 100] and len(cols) == 340 and max(cols) > 1 << 19 and mixed.nc == 1 << 20
    assert 0 in _slots_after_inserting(cols)


def test_many_pairs_and_galerkin_cases():
    cases = sp.product_cases()
    many = sp.product_reference("many_pairs", 0)
    z = many["zcol"].index(7)
    assert many["pl_ptr"][z + 1] - many["pl_ptr"][z] == 40 and many["zcol"][z + 1] == 8 and many["pl_ptr"][z + 2] - many["pl_ptr"][z + 1] == 1
    assert sorted(cases["many_pairs"].alias) == list(range(42)) and cases["many_pairs"].alias != list(range(42))
    t, a = cases["galerkin_T"], cases["galerkin_A"]
    assert t.n == 60 and a.square and a.n == t.nc and a.alias is not None and sorted(a.alias) == list(range(len(a.alias)))
    sizes = [t.ycol.count(g) for g in range(t.nc)]           # P has at least its aggregate's own rows per column
    assert min(sizes) >= 2
    r = sp.product_reference("galerkin_A", 1)
    assert r["not_symmetric"] == 0
    last = r["zcol"][r["zptr"][a.n - 1]:r["zptr"][a.n]]
    assert last == list(range(a.n)) and r["n_upper"][a.n - 1] == 1          # every column below the diagonal except the diagonal
    assert r["zcol"][0] == 0 and r["n_upper"][0] == r["zptr"][1]              # none below
    assert sp.product_reference("not_symmetric", 1)["not_symmetric"] == 1
    assert sum(sp.product_reference(n, 1)["not_symmetric"] for n, p in cases.items() if p.square and n.startswith("random_")) >= 3


def test_level0_cases_hold_what_their_names_say():
    cases = sp.schur_cases()
    lonely = cases["lonely"]
    assert lonely.distinct(3) == 1 and lonely.pp_ptr[3] == lonely.pp_ptr[4] and lonely.od_ptr[3] == lonely.od_ptr[4] and lonely.degree(1) == 1 and lonely.degree(2) == 0
    deg = cases["degree_64_in_65_out"]
    assert (deg.degree(0), deg.degree(1)) == (64, 65)
    assert deg.distinct(0) == 64 and deg.distinct(64) == 1 and deg.distinct(65) == 1
    assert len(sp.schur_reference("degree_64_in_65_out")["slot_i"]) == 64 * 63
    rep = cases["repeated_observers"]
    assert rep.obs_pose[rep.obs_ptr[0]:rep.obs_ptr[1]].count(1) == 2 and rep.obs_pose[rep.obs_ptr[0]:rep.obs_ptr[1]].count(0) == 2
    od = cases["odometry_repeats"].row(0)
    assert len(od[1][1]) == 2 and not od[1][0] and od[2][0] and od[2][1] and od[3][1] and not od[3][0] and od[4][0] and not od[4][1]
    for count in (65, 130):
        assert cases["odometry_list_%d" % count].od_ptr[1] == count
    for through in ("landmarks", "mixed", "odometry"):
        ok, over = cases["crowd_1024_%s" % through], cases["declined_1025_%s" % through]
        assert ok.distinct(0) == 1024 and not ok.declined and over.distinct(0) == 1025 and over.declined
        assert max(ok.degree(l) for l in range(ok.L)) <= 64 and max(over.degree(l) for l in range(over.L)) <= 64
        assert [i for i in range(over.P) if over.distinct(i) > sp.MAX_DISTINCT] == [0]
    mixed = cases["crowd_1024_mixed"].row(0)
    assert sum(1 for k, (pairs, _o) in mixed.items() if pairs) == 1000 and sum(1 for k, (pairs, o) in mixed.items() if o and not pairs) == 23
    assert sum(1 for k, (pairs, o) in mixed.items() if o and pairs) == 2
    assert cases["crowd_1024_odometry"].pp_ptr[-1] == 0 and cases["crowd_1024_landmarks"].od_ptr[-1] == 0
    for length in (65, 128, 200):
        s = cases["trips_%d_degree_200" % length]
        assert s.degree(0) == length and s.max_pair_degree == 200
        seen = s.obs_pose[:length]
        assert seen.count(2) == 2 and seen.index(2) // 64 == (seen.index(2, 3)) // 64           # twice within one trip
        if length > 67:
            assert [k // 64 for k, p in enumerate(seen) if p == 3] == [0, 1]                     # repeated across two trips
    assert all(s.max_pair_degree == 64 for n, s in cases.items() if not n.startswith("trips_"))
    bad = sp.descending_repeat()
    q = [k for k in range(bad.obs_ptr[0], bad.obs_ptr[1]) if bad.obs_pose[k] == 1]
    assert bad.obs_slot[q[0]] > bad.obs_slot[q[1]]
