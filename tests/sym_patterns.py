"""The symbolic side of the multigrid hierarchy, restated from its DEFINITION in plain Python (Python ints, no numpy arithmetic), and the
cases on which the two builders — the host's (toyslam_amd/csrc/host/amg.cpp: spgemm_sym) and the device's (toyslam_amd/csrc/tsgo_sym_kernels.h) —
are compared with it, list by list: tests/test_sym_patterns_cpu.py (host builder, no GPU), tests/test_gpu_sym_patterns.py (both).

Everything here is integer-exact; no tolerance exists.  The constants restate tsgo_sym_kernels.h: one wavefront of 64 lanes per row, a hash
set of 2048 LDS slots per row (hash = (c * 2654435761 mod 2^32) >> 21, linear probing with wrap-around), at most 1024 distinct columns per
row — a row with more is DECLINED (the engine hands the level to the host builder)."""
import functools
import random

WAVE, TABLE, MAX_DISTINCT = 64, 2048, 1024
MAX_PAIR_DEGREE = 64                     # host/amg.h: kMaxPairDegree


def sym_hash(c):
    return ((c * 2654435761) & 0xFFFFFFFF) >> 21


def csr(rows):
    """(ptr, col) of a list of rows."""
    ptr, col = [0], []
    for r in rows:
        col += list(r)
        ptr.append(len(col))
    return ptr, col


def rows_of(ptr, col):
    return [col[ptr[i]:ptr[i + 1]] for i in range(len(ptr) - 1)]


# ---- the product: reference -------------------------------------------------------------------------------------------------------------
class Product:
    """Z = X * Y on patterns.  X: n rows (columns = rows of Y), Y: ny rows, nc columns; alias: per X block, or None."""

    def __init__(self, name, x_rows, y_rows, nc, alias=None):
        self.name, self.n, self.ny, self.nc = name, len(x_rows), len(y_rows), nc
        self.xptr, self.xcol = csr(x_rows)
        self.yptr, self.ycol = csr(y_rows)
        self.alias = None if alias is None else list(alias)
        assert self.alias is None or len(self.alias) == len(self.xcol)
        assert all(0 <= k < self.ny for k in self.xcol) and all(0 <= c < nc for c in self.ycol)
        assert all(len(set(r)) == len(r) for r in y_rows), "a Y row has every column once"

    @property
    def square(self):
        return self.nc == self.n

    def row_triples(self, i):
        """(c, x, y) of row i in walking order: a over X's row, q over Y's row xcol[a]."""
        out = []
        for a in range(self.xptr[i], self.xptr[i + 1]):
            k = self.xcol[a]
            x = self.alias[a] if self.alias is not None else a
            out += [(self.ycol[q], x, q) for q in range(self.yptr[k], self.yptr[k + 1])]
        return out

    def distinct(self, i):
        return len({c for c, _x, _y in self.row_triples(i)})

    @property
    def declined(self):
        """What the device builder must answer: some row has more distinct columns than its table takes."""
        return any(self.distinct(i) > MAX_DISTINCT for i in range(self.n))

    def text(self, upper):
        """One line of tests/cpp/sym_product_dump.cpp's input."""
        out = [upper, self.n, self.ny, self.nc, 0 if self.alias is None else 1] + self.xptr + self.xcol + (self.alias or []) + self.yptr + self.ycol
        return " ".join(map(str, out))


def ref_product(p, upper):
    """dict of lists: zptr, zcol, pl_ptr, px, py; upper: mirror, upper, n_upper, not_symmetric."""
    zptr, zcol, pl_ptr, px, py = [0], [], [], [], []
    for i in range(p.n):
        lists = {}
        for c, x, y in p.row_triples(i):
            lists.setdefault(c, [])
            if not upper or c >= i:
                lists[c].append((x, y))              # walking order within a block: a stable grouping
        for c in sorted(lists):
            zcol.append(c)
            pl_ptr.append(len(px))
            px += [x for x, _y in lists[c]]
            py += [y for _x, y in lists[c]]
        zptr.append(len(zcol))
    pl_ptr.append(len(px))
    out = dict(zptr=zptr, zcol=zcol, pl_ptr=pl_ptr, px=px, py=py)
    if upper:
        where = {(i, zcol[z]): z for i in range(p.n) for z in range(zptr[i], zptr[i + 1])}
        mirror, up, n_upper, bad = [], [], [0] * p.n, 0
        for i in range(p.n):
            for z in range(zptr[i], zptr[i + 1]):
                c = zcol[z]
                if c >= i:
                    mirror.append(-1)
                    up.append(z)
                    n_upper[i] += 1
                else:
                    mirror.append(where.get((c, i), -1))
                    bad |= (c, i) not in where
        out.update(mirror=mirror, upper=up, n_upper=n_upper, not_symmetric=int(bad))
    return out


@functools.lru_cache(maxsize=None)
def product_reference(name, upper):
    return ref_product(product_cases()[name], upper)


# ---- the product: cases -----------------------------------------------------------------------------------------------------------------
def _spread(rng, cols, n_rows, longest=300):
    """Y rows (each at most `longest` long, no column twice in a row) whose union is exactly `cols`, overlapping, in shuffled order."""
    cols = list(cols)
    rows, at = [], 0
    per = max(1, min(longest, -(-len(cols) // n_rows)))
    while at < len(cols):
        part = cols[at:at + per]
        extra = rng.sample(cols[:at], min(at, per // 3)) if at else []       # columns an earlier block reached already
        row = part + [c for c in extra if c not in part]
        rng.shuffle(row)
        rows.append(row)
        at += per
    return rows


def _distinct_case(name, D, where="first", ordinary=3, seed=0):
    """One row with exactly D distinct columns out of 4096, reached over several X blocks, columns not in ascending input order;
    `ordinary` small rows around it (the row is first, last or in the middle)."""
    rng = random.Random(1000 + D + seed)
    nc = 4096
    cols = rng.sample(range(nc), D)
    y_rows = _spread(rng, cols, max(1, min(7, D)))
    big = list(range(len(y_rows)))
    small_y = [sorted(rng.sample(range(nc), rng.randint(1, 9)), reverse=True) for _ in range(4)]
    base = len(y_rows)
    y_rows += small_y
    small = [[base + rng.randrange(4) for _ in range(rng.randint(1, 3))] for _ in range(ordinary)]
    small = [sorted(set(r)) for r in small]
    at = dict(first=0, last=len(small), middle=len(small) // 2)[where]
    x_rows = small[:at] + [big] + small[at:]
    p = Product(name, x_rows, y_rows, nc)
    p.big_row = at
    return p


def _ylen_case(L):
    rng = random.Random(2000 + L)
    nc = 256
    long_row = rng.sample(range(nc), L)
    other = rng.sample(range(nc), 3)
    return Product("ylen_%d" % L, [[0, 1], [1], [0]], [long_row, other], nc)


def _bucket(b, count, rng, limit=1 << 20):
    cols = [c for c in range(limit) if sym_hash(c) == b]
    return rng.sample(cols, count)


def _hash_cases():
    rng = random.Random(3000)
    nc = 1 << 20
    one = _bucket(777, 200, rng)
    wrap = _bucket(TABLE - 1, 150, rng)
    ordinary = rng.sample(range(nc), 120)
    out = {}
    # each cluster over two Y rows (a Y row of 200 is also a multi-trip row) and one more X block that repeats a part of it
    out["hash_one_bucket"] = Product("hash_one_bucket", [[0, 1], [1]], [one, one[50:90][::-1]], nc)
    out["hash_wrap_2047"] = Product("hash_wrap_2047", [[0, 1], [0]], [wrap[:100], wrap[60:]], nc)
    mixed = one[:120] + wrap[:100] + ordinary
    rng.shuffle(mixed)
    out["hash_mixed"] = Product("hash_mixed", [[2], [0, 1, 2], [1]], [mixed[:170], mixed[170:], mixed[100:240][::-1]], nc)
    for p, b, k in ((out["hash_one_bucket"], 777, 200), (out["hash_wrap_2047"], TABLE - 1, 150)):
        p.bucket, p.cluster = b, k
    return out


def _many_pairs_case():
    rng = random.Random(4000)
    nc, blocks = 64, 40
    y_rows = [[7] + rng.sample([c for c in range(nc) if c not in (7, 8)], rng.randint(0, 4)) for _ in range(blocks)]
    for r in y_rows:
        rng.shuffle(r)
    y_rows[17].append(8)                                       # the neighbour: reached through ONE X block
    x_rows = [list(range(blocks)), [3, 5]]
    alias = list(range(blocks + 2))
    rng.shuffle(alias)
    return Product("many_pairs", x_rows, y_rows, nc, alias)


def _transpose(rows, n_cols):
    """(rows of the transpose, for each of its blocks the index of the block it transposes) — R and r_to_p of P."""
    ptr, _col = csr(rows)
    t_rows, to_src = [[] for _ in range(n_cols)], [[] for _ in range(n_cols)]
    for i, r in enumerate(rows):
        for k, c in enumerate(r):
            t_rows[c].append(i)
            to_src[c].append(ptr[i] + k)
    return t_rows, [s for r in to_src for s in r]


def _galerkin_cases():
    """A: random structurally symmetric with diagonal, 60 rows; P from random aggregates of 2 to 8 plus a few smoothed extra entries;
    T = A P; A' = R T with R = P^T and x_alias = r_to_p."""
    rng = random.Random(5000)
    n = 60
    adj = [{i} for i in range(n)]
    for i in range(n):
        for j in rng.sample(range(n), 3):
            adj[i].add(j)
            adj[j].add(i)
    for j in range(n):                                         # the last row couples to everything: all below the diagonal but the diagonal
        adj[n - 1].add(j)
        adj[j].add(n - 1)
    a_rows = [sorted(s) for s in adj]
    agg, na = [], 0
    while len(agg) < n:
        size = min(rng.randint(2, 8), n - len(agg))
        agg += [na] * size
        na += 1
    p_rows = []
    for i in range(n):
        cols = {agg[i]} | {agg[k] for k in rng.sample(a_rows[i], min(2, len(a_rows[i])))}      # smoothed: aggregates of some neighbours
        p_rows.append(sorted(cols))
    t_case = Product("galerkin_T", a_rows, p_rows, na)
    t = ref_product(t_case, 0)
    t_rows = rows_of(t["zptr"], t["zcol"])
    r_rows, r_to_p = _transpose(p_rows, na)
    a_case = Product("galerkin_A", r_rows, t_rows, na, r_to_p)
    return {"galerkin_T": t_case, "galerkin_A": a_case}


def _random_case(seed):
    rng = random.Random(6000 + seed)
    n = rng.randint(1, 40)
    ny = rng.randint(1, 40)
    nc = n if seed % 2 else rng.choice([1, 5, 70, 300, 5000])
    lens = [0, 1, 2, 5, 30, 63, 64, 65, 130]
    y_rows = [rng.sample(range(nc), min(nc, rng.choice(lens))) for _ in range(ny)]
    x_rows = [[rng.randrange(ny) for _ in range(rng.choice([0, 1, 2, 3, 8, 20]))] for _ in range(n)]
    alias = None
    if seed % 3 == 0:
        alias = list(range(sum(len(r) for r in x_rows)))
        rng.shuffle(alias)
    return Product("random_%02d" % seed, x_rows, y_rows, nc, alias)


@functools.lru_cache(maxsize=None)
def product_cases():
    out = {}

    def add(p):
        assert p.name not in out
        out[p.name] = p

    # empty shapes
    add(Product("empty_n1", [[]], [], 1))
    add(Product("empty_n1_with_y", [[]], [[0]], 1))
    # X rows without entries (0, 3), Y rows without entries (1, 4), a row whose product is empty (2: its X blocks lead to empty Y rows)
    add(Product("empty_rows", [[], [0, 2], [1, 4], [], [2, 1, 3], [5]], [[1, 4], [], [4, 2, 1], [5, 0], [], [5]], 6))
    for L in (1, 63, 64, 65, 129, 200):
        add(_ylen_case(L))
    for D in (1, 2, 3, 5, 64, 65, 127, 128, 129, 513, 1023, 1024):
        add(_distinct_case("distinct_%d" % D, D))
    # declined: more than 1024 distinct columns
    add(_distinct_case("declined_1025_first", 1025, "first"))
    add(_distinct_case("declined_1025_last", 1025, "last", seed=1))
    add(_distinct_case("declined_1025_middle", 1025, "middle", ordinary=4, seed=2))
    add(_distinct_case("declined_1500", 1500, "middle", seed=3))
    for L in (2049, 3000):                                   # ONE Y row longer than the whole table: the insert itself reports "full"
        rng = random.Random(7000 + L)
        add(Product("declined_yrow_%d" % L, [[1], [0, 1], [1]], [rng.sample(range(4096), L), [5, 2]], 4096))
    for p in _hash_cases().values():
        add(p)
    add(_many_pairs_case())
    for p in _galerkin_cases().values():
        add(p)
    # square, not structurally symmetric: block (2, 0) exists, block (0, 2) does not
    add(Product("not_symmetric", [[0], [1, 0], [2, 0], [1, 3]], [[0, 1], [1], [2], [3, 1]], 4))
    for seed in range(30):
        add(_random_case(seed))
    return out


# ---- level 0: reference -----------------------------------------------------------------------------------------------------------------
class Schur:
    """Level 0's inputs (host/amg.h: SchurCsr) from a graph in edge order: lm_edges = [(pose, landmark)], odom = [(pose, neighbour)] (one
    entry per side the caller wants).  Slots rise with an entry's rank in its pose's list, as the host's tables give them, with gaps."""

    def __init__(self, name, P, L, lm_edges, odom, max_pair_degree=MAX_PAIR_DEGREE):
        self.name, self.P, self.L, self.max_pair_degree = name, P, L, max_pair_degree
        order = sorted(range(len(lm_edges)), key=lambda e: (lm_edges[e][0], e))
        slot = {e: 3 * r + 1 for r, e in enumerate(order)}      # by_pose slot of every LM edge
        pp = [[] for _ in range(P)]
        obs = [[] for _ in range(L)]
        for e, (p, l) in enumerate(lm_edges):
            assert 0 <= p < P and 0 <= l < L
            pp[p].append((l, slot[e]))
            obs[l].append((p, slot[e]))
        od = [[] for _ in range(P)]
        for r, (p, k) in enumerate(sorted(odom, key=lambda t: t[0])):      # stable: a pose's entries keep their order
            assert p != k and 0 <= p < P and 0 <= k < P
            od[p].append((k, 5 * r + 2))
        self.pp_ptr, flat = csr(pp)
        self.pp_lm, self.pp_slot = [a for a, _b in flat], [b for _a, b in flat]
        self.obs_ptr, flat = csr(obs)
        self.obs_pose, self.obs_slot = [a for a, _b in flat], [b for _a, b in flat]
        self.od_ptr, flat = csr(od)
        self.od_col, self.od_slot = [a for a, _b in flat], [b for _a, b in flat]

    def degree(self, l):
        return self.obs_ptr[l + 1] - self.obs_ptr[l]

    def row(self, i):
        """{k: (pairs, odometry slots)} of pose i, from the definition."""
        blocks = {i: ([], [])}
        for a in range(self.pp_ptr[i], self.pp_ptr[i + 1]):
            l = self.pp_lm[a]
            if self.degree(l) > self.max_pair_degree:
                continue
            for q in range(self.obs_ptr[l], self.obs_ptr[l + 1]):
                k = self.obs_pose[q]
                if k != i:
                    blocks.setdefault(k, ([], []))[0].append((self.pp_slot[a], self.obs_slot[q]))
        for e in range(self.od_ptr[i], self.od_ptr[i + 1]):
            blocks.setdefault(self.od_col[e], ([], []))[1].append(self.od_slot[e])
        return blocks

    def distinct(self, i):
        return len(self.row(i))

    @property
    def declined(self):
        return any(self.distinct(i) > MAX_DISTINCT for i in range(self.P))


def ref_schur(s):
    zptr, zcol, sc_ptr, sc_optr, slot_i, slot_k, os_ = [0], [], [], [], [], [], []
    for i in range(s.P):
        blocks = s.row(i)
        for k in sorted(blocks):
            pairs, od = blocks[k]
            zcol.append(k)
            sc_ptr.append(len(slot_i))
            sc_optr.append(len(os_))
            for a, b in sorted(pairs):                       # the host's sort key: (slot of i, slot of k)
                slot_i.append(a)
                slot_k.append(b)
            os_ += sorted(od)
        zptr.append(len(zcol))
    sc_ptr.append(len(slot_i))
    sc_optr.append(len(os_))
    return dict(zptr=zptr, zcol=zcol, sc_ptr=sc_ptr, sc_optr=sc_optr, slot_i=slot_i, slot_k=slot_k, os=os_)


@functools.lru_cache(maxsize=None)
def schur_reference(name):
    return ref_schur(schur_cases()[name])


# ---- level 0: cases ---------------------------------------------------------------------------------------------------------------------
def _chain(P):
    return [(i, i + 1) for i in range(P - 1)] + [(i + 1, i) for i in range(P - 1)]


def _crowd(name, through, extra):
    """Pose 0 with 1023 + extra other columns (1024 + extra with itself), reached through `through`:
    'landmarks' (each seen by pose 0 and 63 others), 'mixed' (1000 co-observers plus odometry neighbours that are not among them),
    'odometry' (alone)."""
    others = 1023 + extra
    P = others + 1
    lm_edges, odom = [], []
    n_lm_others = dict(landmarks=others, mixed=1000, odometry=0)[through]
    L, k = 0, 1
    while k <= n_lm_others:
        group = list(range(k, min(k + 63, n_lm_others + 1)))
        lm_edges += [(0, L)] + [(p, L) for p in group]
        k += len(group)
        L += 1
    odom += [(0, p) for p in range(n_lm_others + 1, P)]
    if through == "mixed":
        odom += [(0, 5), (0, 990)]                          # two neighbours that ARE co-observers: no new column
    s = Schur(name, P, max(L, 1), lm_edges, odom)
    return s


def _multi_trip(name, length, max_deg):
    """One landmark whose observer list has `length` entries: pose 0 first, then poses 1 .. , with pose 3 once more at entry 3 + 64 (a pose
    repeated across two trips of 64 lanes) where the list is long enough, and pose 2 twice within the first trip; a second, short landmark."""
    lm_edges = [(0, 0)]
    p = 1
    while len(lm_edges) < length:
        at = len(lm_edges)
        if at == 67 and length > 67:
            lm_edges.append((3, 0))
        elif at == 20:
            lm_edges.append((2, 0))
        else:
            lm_edges.append((p, 0))
            p += 1
    P = p + 1
    lm_edges += [(0, 1), (1, 1), (P - 1, 1)]
    return Schur(name, P, 2, lm_edges, _chain(P), max_deg)


@functools.lru_cache(maxsize=None)
def schur_cases():
    out = {}

    def add(s):
        assert s.name not in out
        out[s.name] = s

    # pose 3 has no edge at all; landmark 1 is seen by pose 2 only; landmark 2 by nobody
    add(Schur("lonely", 4, 3, [(0, 0), (1, 0), (2, 1), (2, 0)], [(0, 1), (1, 0), (1, 2), (2, 1)]))
    # landmark 0: 64 observers (poses 0 .. 63), in; landmark 1: 65 observers (poses 0 .. 64), out: pose 64 sees nothing else
    add(Schur("degree_64_in_65_out", 66, 2, [(p, 0) for p in range(64)] + [(p, 1) for p in range(65)], []))
    # landmark 0 observed twice by pose 1 and twice by pose 0 itself; landmark 1 twice by pose 2, with another edge of pose 2 in between
    add(Schur("repeated_observers", 4, 3, [(0, 0), (1, 0), (2, 1), (1, 0), (0, 0), (2, 2), (2, 1), (3, 1), (0, 1), (3, 0)], _chain(4)))
    # pose 0: two ODOM entries to pose 1, pose 2 is an odometry neighbour AND a co-observer, pose 3 an odometry neighbour only, pose 4 a co-observer only
    add(Schur("odometry_repeats", 5, 2, [(0, 0), (2, 0), (4, 0), (2, 1), (0, 1)], [(0, 1), (0, 2), (0, 1), (0, 3), (1, 0), (2, 0), (3, 0), (1, 0)]))
    for count in (65, 130):                                  # an odometry list longer than one trip of the wavefront, neighbours repeating
        rng = random.Random(8000 + count)
        add(Schur("odometry_list_%d" % count, 40, 1, [(0, 0), (7, 0), (9, 0)], [(0, rng.randint(1, 39)) for _ in range(count)] + [(5, 0), (5, 6)]))
    for through in ("landmarks", "mixed", "odometry"):
        add(_crowd("crowd_1024_%s" % through, through, 0))
        add(_crowd("declined_1025_%s" % through, through, 1))
    for length in (65, 128, 200):
        add(_multi_trip("trips_%d_degree_200" % length, length, 200))
    return out


def descending_repeat():
    """`repeated_observers` with pose 1's two entries in landmark 0's observer list swapped: descending slots.  host/problem.cpp cannot lay
    a graph out like this (both tables are filled in edge order and a pose's slots rise with the entry's rank); the entry point refuses it."""
    s = Schur("repeated_observers_descending", 4, 3, [(0, 0), (1, 0), (2, 1), (1, 0), (0, 0), (2, 2), (2, 1), (3, 1), (0, 1), (3, 0)], _chain(4))
    q = [k for k in range(s.obs_ptr[0], s.obs_ptr[1]) if s.obs_pose[k] == 1]
    assert len(q) == 2 and s.obs_slot[q[0]] < s.obs_slot[q[1]]
    s.obs_slot[q[0]], s.obs_slot[q[1]] = s.obs_slot[q[1]], s.obs_slot[q[0]]
    return s


# ---- k_sym_scan -------------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = (0, 1, 2, 1023, 1024, 1025, 2047, 2049, 100003)


def scan_input(n):
    """Entries in [0, 50] with runs of zeros."""
    rng = random.Random(9000 + n)
    out = []
    while len(out) < n:
        if rng.random() < 0.3:
            out += [0] * rng.randint(1, 40)
        else:
            out += [rng.randint(0, 50) for _ in range(rng.randint(1, 40))]
    return out[:n]
