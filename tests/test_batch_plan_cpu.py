"""The batch planning of the H^-1 readers (toyslam_amd/csrc/host/batch_plan.h: whole_query_batches, full_batches, gate_batch_lists), compiled
for the host (tests/cpp/batch_plan_dump.cpp) and checked against brute-force restatements: which columns a batch solves, which queries /
candidates it reads out, and where their rows lie."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, L = 0, 1                                  # vertex kinds
NEED = {P: 3, L: 2}                          # columns of a pose / a landmark
KINDS = [P, P, L, P, L, L, P]


def _gate_case(kinds, cands, nv):
    """Distinct vertices in order (idx = place, col0 = running column count) and 2 vertex numbers per candidate."""
    col0 = np.concatenate([[0], np.cumsum([NEED[k] for k in kinds])[:-1]]).astype(int)
    return dict(nv=nv, kinds=list(kinds), col0=[int(c) for c in col0], cands=[(int(a), int(b)) for a, b in cands])


def _gate_cases():
    rng = np.random.default_rng(11)
    kinds = rng.integers(0, 2, 12)
    pairs = rng.integers(0, 12, (40, 2))
    pairs[::7, 1] = pairs[::7, 0]            # some unary candidates
    return {
        # tests/test_gpu_gate.py::test_read_out_shapes: poses fill columns 0 .. 14, the sixth pose straddles two batches (15 | 16, 17), the
        # landmark of the fourth candidate lies in the second batch and its pose in the first, the last batch is partial
        "straddle": _gate_case([P] * 6 + [L, P], [(0, 1), (2, 3), (4, 5), (0, 6), (1, 7)], 16),
        "unary": _gate_case([P, L], [(0, 0), (1, 1), (0, 1)], 16),
        "different_batches": _gate_case([P] * 6, [(0, 5), (2, 2)], 8),
        "random": _gate_case(kinds, pairs, 8),
    }


WHOLE = [(8, KINDS), (16, KINDS), (1, KINDS), (8, []), (16, [L] * 9), (8, [P] * 5)]
FULL = [(d, nv) for d in (1, 15, 16, 17, 23) for nv in (16, 8, 1)]


def input_text():
    lines = ["W %d %d %s" % (nv, len(k), " ".join(map(str, k))) for nv, k in WHOLE]
    lines += ["F %d %d" % c for c in FULL]
    for c in _gate_cases().values():
        verts = " ".join("%d %d %d" % (k, v, c0) for v, (k, c0) in enumerate(zip(c["kinds"], c["col0"])))
        lines.append("G %d %d %s %d %s" % (c["nv"], len(c["kinds"]), verts, len(c["cands"]), " ".join("%d %d" % p for p in c["cands"])))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """One row of integers per case of input_text(), compiled and run once."""
    exe = str(tmp_path_factory.mktemp("batch_plan") / "batch_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "toyslam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "batch_plan_dump.cpp"), "-o", exe])
    out = subprocess.run([exe], input=input_text(), capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [[int(x) for x in ln.split()] for ln in out if ln]
    assert len(rows) == len(WHOLE) + len(FULL) + len(_gate_cases())
    return rows


class _Reader:
    def __init__(self, row):
        self.row, self.at = row, 0

    def take(self, n=1, width=None):
        n_int = n * (width or 1)
        out = self.row[self.at:self.at + n_int]
        assert len(out) == n_int
        self.at += n_int
        return [tuple(out[i * width:(i + 1) * width]) for i in range(n)] if width else out

    def done(self):
        return self.at == len(self.row)


def _read_whole(row):
    r = _Reader(row)
    narrow, nb = r.take(2)
    out = dict(narrow=narrow, ranges=r.take(nb, 2), q_off=r.take(nb + 1))
    out["items"] = r.take(r.take()[0], 3)
    out["all"] = r.take(r.take()[0], 3)
    assert r.done()
    return out


@pytest.mark.parametrize("case", range(len(WHOLE)))
def test_whole_query_batches(plans, case):
    nv, kinds = WHOLE[case]
    pl = _read_whole(plans[case])
    if any(NEED[k] > nv for k in kinds):
        assert pl["narrow"] == 1 and pl["ranges"] == [] and pl["all"] == [] and pl["items"] == []
        return
    # brute force: a batch is closed when the next query would not fit; a query is never split
    batches, cur = [], []
    for q, k in enumerate(kinds):
        if cur and sum(NEED[kinds[i]] for i in cur) + NEED[k] > nv:
            batches.append(cur); cur = []
        cur.append(q)
    if cur:
        batches.append(cur)
    assert pl["narrow"] == 0 and len(pl["ranges"]) == len(batches)
    assert pl["all"] == [(k, q, c) for q, k in enumerate(kinds) for c in range(NEED[k])]
    assert pl["q_off"] == [0] + [b[-1] + 1 for b in batches]
    j = 0
    for b, (j0, nc) in zip(batches, pl["ranges"]):
        assert (j0, nc) == (j, sum(NEED[kinds[q]] for q in b)) and 0 < nc <= nv
        at = 0
        for q in b:                          # the item of a query: its first column within the batch
            assert pl["items"][q] == (kinds[q], q, at)
            at += NEED[kinds[q]]
        j += nc
    assert j == len(pl["all"]) and len(pl["items"]) == len(kinds)


def test_whole_query_batch_counts(plans):
    """[P, P, L, P, L, L, P] = 3 3 2 | 3 2 2 | 3 at 8 columns and 3 3 2 3 2 2 | 3 at 16; width 1 is narrow; no query, no batch."""
    got = [_read_whole(plans[c]) for c in range(4)]
    assert [len(g["ranges"]) for g in got] == [3, 2, 0, 0]
    assert [g["narrow"] for g in got] == [0, 0, 1, 0]
    assert got[3]["q_off"] == [0]


@pytest.mark.parametrize("case", range(len(FULL)))
def test_full_batches(plans, case):
    d, nv = FULL[case]
    r = _Reader(plans[len(WHOLE) + case])
    nb = r.take()[0]
    ranges = r.take(nb, 2)
    assert r.done()
    assert nb == -(-d // nv)
    assert all(nc == nv for _j0, nc in ranges[:-1]) and 0 < ranges[-1][1] <= nv
    assert [j0 for j0, _nc in ranges] == [b * nv for b in range(nb)] and sum(nc for _j0, nc in ranges) == d


@pytest.mark.parametrize("name", list(_gate_cases()))
def test_gate_batch_lists(plans, name):
    cases = _gate_cases()
    c = cases[name]
    r = _Reader(plans[len(WHOLE) + len(FULL) + list(cases).index(name)])
    nb, max_rows = r.take(2)
    item_off, job_off = r.take(nb + 1), r.take(nb + 1)
    items = r.take(r.take()[0], 3)
    jobs = r.take(r.take()[0], 3)
    assert r.done()
    nv, kinds, col0, cands = c["nv"], c["kinds"], c["col0"], c["cands"]
    D = col0[-1] + NEED[kinds[-1]]
    assert nb == -(-D // nv) and item_off[0] == job_off[0] == 0 and item_off[-1] == len(items) and job_off[-1] == len(jobs)
    if name == "straddle":
        assert (D, nb) == (23, 2)
    tallest = 1
    for b in range(nb):
        cols = set(range(b * nv, min(D, (b + 1) * nv)))
        inside = [v for v in range(len(kinds)) if cols & set(range(col0[v], col0[v] + NEED[kinds[v]]))]
        b_items, b_jobs = items[item_off[b]:item_off[b + 1]], jobs[job_off[b]:job_off[b + 1]]
        # every candidate with a vertex column in this batch exactly once, nobody else
        assert sorted(k for k, _r0, _r1 in b_jobs) == [k for k, (va, vb) in enumerate(cands) if va in inside or vb in inside]
        # the items: every vertex once, rows one after the other
        assert len({(k, i) for k, i, _row in b_items}) == len(b_items)
        row = {}
        at = 0
        for k, i, r0 in b_items:
            assert k == kinds[i] and r0 == at
            row[i] = r0
            at += NEED[k]
        tallest = max(tallest, at)
        # r0 / r1: the rows of the candidate's vertices in these items; and no item without a job that reads it
        for k, r0, r1 in b_jobs:
            assert (r0, r1) == (row[cands[k][0]], row[cands[k][1]])
        assert set(row) == {v for k, _r0, _r1 in b_jobs for v in cands[k]}
        # the order: vertices by column, a vertex's candidates by number, a candidate's vertices first slot first
        want_jobs, want_items = [], []
        for v in inside:
            for k, pair in enumerate(cands):
                if v in pair and k not in want_jobs:
                    want_jobs.append(k)
                    want_items += [u for u in dict.fromkeys(pair) if u not in want_items]
        assert [k for k, _r0, _r1 in b_jobs] == want_jobs and [i for _k, i, _row in b_items] == want_items
    assert max_rows == tallest
    if name == "different_batches":          # candidate 0 = (vertex 0, vertex 5): columns 0 .. 2 | 15 | 16, 17; candidate 1 on vertex 2: 6, 7 | 8
        assert nb == 3 and [k for k, _r0, _r1 in jobs] == [0, 1, 1, 0, 0]
