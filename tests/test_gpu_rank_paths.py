"""Every top-k path of the ranking stage (rank.hip, sort.hip, sort_small.h, small.hip) against the exact NumPy reference of
tests/rank_reference.py, at the boundaries where integer key arithmetic goes wrong: ids, counts and score BITS must match.

Paths, as the library picks them (n_items = m, tile width G, tile group tg):
  * select (top_n <= SEL_MAX_K): MSD radix select on the 128-bit key (score, id), then a bitonic sort of the collected
    candidates.  tg*G <= 64: k_sel_hist with the last-workgroup ticket for levels 0 .. SEL_FUSED_LEVELS-1, then k_sel_tail
    (one workgroup per tile walks every row block); tg*G > 64: k_sel_hist + k_sel_decide for all 16 levels.  One k_sel_hist
    workgroup per SEL_ROWS_PER_BLOCK items of a tile.
  * sort (top_n > SEL_MAX_K): m <= SEL_SLOTS: k_rank_small; else k_rank_keys, then G == 1 and m <= SMALL_SORT_MAX:
    k_sort_small; G == 1 beyond: the multi-block radix sort, one segment; G > 1: the segmented radix sort (nseg = G),
    whose scan carries across chunks of 256 sort blocks once a segment has more of them.
  * ego networks (one seed, m <= SM_MAX_ITEMS and the other small.hip limits): the in-launch bitonic sort.

Part A drives the select path with rank vectors chosen here: rwr_part_begin on the whole slab, the device x overwritten
from torch, rwr_part_rank.  Part B goes through the public entry points; its reference rank vectors come from
Model.RunBatch (pinned bitwise to rwr_model_run and the oracle elsewhere), so the reference cost stays a NumPy sort.
"""
import numpy as np
import pytest

from oracle import rwr_oracle as po
from oracle.c_oracle import FlatGraph, evaluate
from tests import graphgen as gg
from tests.rank_reference import candidate_rows, reference_batch, reference_ranking

pytestmark = pytest.mark.gpu

# the dispatch constants the cases below are built around (tests/test_rank_constants.py reads them out of the sources)
EXPECTED_CONSTANTS = dict(SEL_MAX_K=1024, SEL_CAP=3072, SEL_SLOTS=4096, SEL_ROWS_PER_BLOCK=4096, SEL_FUSED_LEVELS=3,
                          SORT_CHUNK=4096, SMALL_SORT_MAX=20480, SM_MAX_ITEMS=4096)
SEL_MAX_K = EXPECTED_CONSTANTS["SEL_MAX_K"]
SEL_CAP = EXPECTED_CONSTANTS["SEL_CAP"]
SEL_SLOTS = EXPECTED_CONSTANTS["SEL_SLOTS"]
SEL_ROWS = EXPECTED_CONSTANTS["SEL_ROWS_PER_BLOCK"]
SORT_CHUNK = EXPECTED_CONSTANTS["SORT_CHUNK"]
SMALL_SORT_MAX = EXPECTED_CONSTANTS["SMALL_SORT_MAX"]
SM_MAX_ITEMS = EXPECTED_CONSTANTS["SM_MAX_ITEMS"]

I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
D = 0.15
DW = po.widen_float(D)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same(ids, sc, cnt, ri, rs, rc, what):
    ids, sc, cnt = np.asarray(ids), np.asarray(sc), np.asarray(cnt)
    assert (cnt == rc).all(), (what, "counts", cnt, rc)
    for k in range(len(rc)):
        c = int(rc[k])
        bad = np.flatnonzero((ids[k, :c] != ri[k, :c]) | (bits(sc[k, :c]) != bits(rs[k, :c])))
        assert bad.size == 0, (what, "row", k, "first difference at", int(bad[0]), int(ids[k, bad[0]]), int(ri[k, bad[0]]),
                               float(sc[k, bad[0]]), float(rs[k, bad[0]]))


@pytest.fixture(scope="module")
def amd():
    import recommendersystems_amd as amd
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    return amd


def f64_from_bits(u):
    return np.asarray(u, dtype=np.uint64).view(np.float64)


def full_range_ids(rng, m):
    """m unique int64 ids over the whole range, both extremes and -1 / 0 / 1 included, in random order."""
    fixed = [I64_MIN, I64_MAX, -1, 0, 1]
    s = set(fixed)
    while len(s) < m:
        s.update(int(x) for x in rng.integers(I64_MIN, I64_MAX, size=m - len(s) + 8, dtype=np.int64, endpoint=True))
    rest = np.array(sorted(s - set(fixed)), dtype=np.int64)[:m - len(fixed)]
    return np.concatenate([np.array(fixed, dtype=np.int64), rest])[rng.permutation(m)]


# ============================================================================================ A. vector-driven (select path)

N_USERS_A = 64          # the seeds of part A: user u LIKEs one item (row N_USERS_A + m - 1 - u % 3)


def item_ids(pattern: str, m: int, rng) -> np.ndarray:
    """Unique item ids whose byte structure makes a given select level settle an all-equal-score tie."""
    i = np.arange(m, dtype=np.int64)
    if pattern == "top":            # (b << 56) | j: the id's top byte (level 8) splits the tie
        iu = i.astype(np.uint64)
        ids = ((iu % np.uint64(256)) << np.uint64(56) | (iu // np.uint64(256))).view(np.int64)
    elif pattern == "low":          # consecutive: only the two lowest bytes differ (levels 13-14)
        ids = np.int64(0x1234_5678_9ABC_0000) + i
    elif pattern == "sign":         # across -1 / 0 / 1: the sign bit of the id key
        ids = i - m // 2
    elif pattern == "p53":          # across 2^53 (0x001F... -> 0x0020...)
        ids = np.int64(2 ** 53) - m // 2 + i
    elif pattern == "m53":          # across -2^53
        ids = np.int64(-(2 ** 53)) - m // 2 + i
    elif pattern == "full":
        ids = full_range_ids(rng, m)
    else:
        raise ValueError(pattern)
    assert len(np.unique(ids)) == m
    return ids[rng.permutation(m)]


def vector_graph(m: int, pattern: str, seed: int = 0):
    rng = np.random.default_rng(seed)
    n = N_USERS_A + m
    node_type = np.array([gg.NODE_USER] * N_USERS_A + [gg.NODE_ITEM] * m, dtype=np.uint8)
    iid = item_ids(pattern, m, rng)
    uid = np.int64(0x0707_0707_0707_0000) + np.arange(N_USERS_A, dtype=np.int64)
    node_id = np.concatenate([uid, iid])
    lists = {v: [] for v in range(n)}
    for u in range(N_USERS_A):
        it = N_USERS_A + m - 1 - u % 3
        lists[u].append(it)
        lists[it].append(u)
    return gg._from_lists(node_id, node_type, lists)


# --- column scenarios: values for the c_total candidates of a column, for a given top_n (None: does not fit)
def _bits_with(level_byte, low_vals, level):
    """bit patterns: bytes 0 .. level-1 from PREFIX, byte `level` = level_byte, the bytes below from low_vals with byte
    level+1 varying fastest (so that the next level splits a bin)."""
    u = np.zeros(len(low_vals), dtype=np.uint64)
    for b in range(level):
        u |= np.uint64(PREFIX[b]) << np.uint64(56 - 8 * b)
    u |= np.uint64(level_byte) << np.uint64(56 - 8 * level)
    low = np.asarray(low_vals, dtype=np.uint64)
    for q in range(7 - level):
        u |= ((low >> np.uint64(8 * q)) & np.uint64(255)) << np.uint64(56 - 8 * (level + 1 + q))
    return u


PREFIX = [0x3F, 0xF4, 0x56, 0x78, 0x9A, 0xBC, 0xDE]      # bytes of a double near 1.27


def scen_cap(level: int, C: int, pos: str):
    """The k-th entry's bin at select level `level` holds exactly C members, the k-th entry its first or its last member.
    The entries above the bin and 50 (+ SEL_CAP) decoys just below it share its first `level` bytes, so that the bin of
    every earlier level is larger than SEL_CAP; the other candidates lie below at level 0."""
    def make(c_total, top_n, rng):
        A = top_n - 1 if pos == "first" else top_n - C
        if A < 0:
            return None
        nd = 0 if level == 0 else 50 + (SEL_CAP if C <= SEL_CAP and pos == "last" else 0)
        if A + C + nd > c_total:
            return None
        b0 = PREFIX[level]
        parts = [_bits_with(b0 + 1, rng.permutation(1 << 16)[:A], level), _bits_with(b0, rng.permutation(1 << 16)[:C], level),
                 _bits_with(b0 - 1, rng.permutation(1 << 16)[:nd], level)]
        vals = f64_from_bits(np.concatenate(parts))
        rest = c_total - len(vals)
        tail = np.where(rng.random(rest) < 0.5, 0.0, rng.random(rest) * 1e-300)
        return np.concatenate([vals, tail])
    make.__name__ = f"cap_L{level}_{C}_{pos}"
    return make


def scen_tie(value: float):
    def make(c_total, top_n, rng):
        return np.full(c_total, value)
    make.__name__ = f"tie_{value!r}"
    return make


def scen_tie_above(n_above: int, value: float):
    """n_above distinct larger scores, every other candidate at `value`: the k-th entry sits inside the tie."""
    def make(c_total, top_n, rng):
        v = np.full(c_total, value)
        v[:n_above] = value + 1.0 + rng.permutation(n_above)
        return v
    make.__name__ = f"tie_above_{n_above}_{value!r}"
    return make


SPECIAL = np.array([0.0, 5e-324, 1e-323, 2.2250738585072014e-308, np.nextafter(2.2250738585072014e-308, 0.0),
                    np.nextafter(1.0, 0.0), 1.0, np.nextafter(1.0, 2.0), 2.0, 1.7976931348623157e308,
                    np.nextafter(1.7976931348623157e308, 0.0)])


def scen_special(c_total, top_n, rng):
    """+0.0, the two smallest subnormals, DBL_MIN and its lower neighbour, 1.0 and its neighbours, DBL_MAX and its lower
    neighbour, and 256 values equal in their top 7 bytes: each repeated (ties), every other candidate +0.0."""
    top7 = f64_from_bits(np.uint64(0x3FF0_0000_0000_0100) | np.arange(256, dtype=np.uint64))
    pool = np.concatenate([np.repeat(SPECIAL, 40), np.repeat(top7, 3)])
    v = np.zeros(c_total)
    k = min(len(pool), c_total)
    v[:k] = pool[rng.permutation(len(pool))[:k]]
    return v


def scen_natural(c_total, top_n, rng):
    return rng.exponential(size=c_total) * np.where(rng.random(c_total) < 0.3, 0.0, 1.0)


COLS_DEEP = [scen_tie(0.0), scen_tie(1.0), scen_tie_above(700, 0.0), scen_tie_above(2000, 2.5), scen_special, scen_natural]
COLS_CAP = [scen_cap(0, SEL_CAP, "first"), scen_cap(0, SEL_CAP + 1, "first"), scen_cap(1, SEL_CAP, "first"),
            scen_cap(1, SEL_CAP + 1, "first"), scen_cap(4, SEL_CAP, "first"), scen_cap(4, SEL_CAP + 1, "first"),
            scen_cap(1, 1000, "last"), scen_cap(4, 1000, "last"), scen_cap(0, 1000, "last")]


@pytest.fixture(scope="module")
def part_backends(amd):
    from recommendersystems_amd import partitioned as pt
    cache = {}

    def get(m, pattern):
        if (m, pattern) not in cache:
            g = vector_graph(m, pattern, seed=m)
            n = len(g["node_id"])
            cache[(m, pattern)] = (g, pt.HipSlabBackend(pt.slab_graph(g, 0, n), 0, n))
        return cache[(m, pattern)]
    yield get
    for _, be in cache.values():
        be.graph.close()


def run_vector_case(part_backends, m, pattern, K, top_n, scenarios, seed):
    """One rwr_part_rank call: column k of x holds the first scenario from k % len(scenarios) on that fits top_n, over its
    seed's candidates in a random row order; the seed's excluded item and every user row hold 1e300, which must never
    show.  Returns the scenario names used."""
    import torch
    g, be = part_backends(m, pattern)
    n = len(g["node_id"])
    rng = np.random.default_rng(seed)
    seeds = np.arange(K, dtype=np.int32)            # users 0 .. K-1
    x, _, _ = be.begin(seeds, D)
    G = be.G
    # rwr_part_rank ranks one tile (tg = 1) of G <= 64 seeds: the fused select (ticket + k_sel_tail) always
    assert G <= 64 and top_n <= SEL_MAX_K
    X = np.full((n, G), 1e300)
    ranks = np.zeros((K, n))
    used = []
    for k in range(G):
        if k >= K:
            X[N_USERS_A:, k] = rng.random(m)        # padded slot: no seed, never ranked
            continue
        rows = candidate_rows(g["node_type"], g["rowptr"], g["dst"], g["etype"], int(seeds[k]))
        vals = None
        for q in range(len(scenarios)):
            sc = scenarios[(k + q) % len(scenarios)]
            vals = sc(len(rows), top_n, rng)
            if vals is not None:
                used.append(sc.__name__)
                break
        assert vals is not None
        assert (vals >= 0).all() and np.isfinite(vals).all()
        X[rows[rng.permutation(len(rows))], k] = vals
        ranks[k] = X[:, k]
    x.view(n, G).copy_(torch.from_numpy(X).to(x.device))
    torch.cuda.synchronize()
    ids, sc, cnt = be.rank(x, top_n)
    ri, rs, rc = reference_batch(ranks, g["node_id"], g["node_type"], g["rowptr"], g["dst"], g["etype"], seeds, top_n)
    assert_same(ids, sc, cnt, ri, rs, rc, (m, pattern, K, top_n, used))
    return used


@pytest.mark.parametrize("m", [4095, 4096, 4097, 3 * 4096 + 1])
@pytest.mark.parametrize("K", [1, 3, 7, 64])
@pytest.mark.parametrize("top_n", [1, 1023, 1024])
def test_select_deep_ties_and_byte_boundaries(part_backends, m, K, top_n):
    """Deep ties settled by the id alone and values across the key's byte boundaries; m covers one and several k_sel_hist
    workgroups per tile, and a k_sel_tail that walks one or several row blocks."""
    assert (m > SEL_ROWS) == (m in (4097, 3 * 4096 + 1))
    run_vector_case(part_backends, m, "full", K, top_n, COLS_DEEP, seed=m * 7 + K * 3 + top_n)


@pytest.mark.parametrize("pattern", ["top", "low", "sign", "p53", "m53", "full"])
@pytest.mark.parametrize("m", [4097, 3 * 4096 + 1])
def test_select_id_decides_at_every_byte(part_backends, pattern, m):
    """All-equal scores (+0.0, 3.0, and +0.0 below 700 larger scores): only the id orders them; the id patterns make the
    top byte, the lowest bytes, the sign bit and the +-2^53 boundaries decide.  K = 7: one padded slot."""
    for top_n in (1, 2, 1023, 1024):
        run_vector_case(part_backends, m, pattern, 7, top_n, [scen_tie(0.0), scen_tie_above(700, 0.0), scen_tie(3.0)],
                        seed=top_n)


@pytest.mark.parametrize("m", [4096, 4097, 3 * 4096 + 1])
@pytest.mark.parametrize("K", [1, 3, 64])
@pytest.mark.parametrize("top_n", [1, 2, 1000, 1023, 1024])
def test_select_cap_boundaries(part_backends, m, K, top_n):
    """The k-th entry's bin holds exactly SEL_CAP or SEL_CAP + 1 members at level 0, 1 and 4 with the k-th entry its first
    member, or it is the last member of a smaller bin.  Columns of one tile stop at different levels."""
    used = run_vector_case(part_backends, m, "full", K, top_n, COLS_CAP, seed=m + K + top_n)
    assert any(u.startswith("cap_") for u in used)


def test_select_collects_sel_slots_minus_one(part_backends):
    """top_n = 1024 with 1023 entries above a level-0 bin of exactly SEL_CAP members: SEL_SLOTS - 1 = 4095 candidates are
    collected, on 4096 items (one row block) and on 4097 (two)."""
    assert SEL_MAX_K - 1 + SEL_CAP == SEL_SLOTS - 1
    for m in (4096, 4097):
        used = run_vector_case(part_backends, m, "full", 1, 1024, [scen_cap(0, SEL_CAP, "first")], seed=5)
        assert used == [f"cap_L0_{SEL_CAP}_first"]


# ============================================================================================ B. graph-driven, public entry points

def graph_b(n_items: int, n_users: int, seed: int, likes_per_user=(2, 12), tie_groups=40, tie_size=30):
    """Users and items, built vectorised: users LIKE a few random items and have two FRIENDSHIPs; `tie_groups` groups of
    `tie_size` items are each LIKEd by exactly the same two users and nobody else (structural ties: bitwise-equal scores);
    most items are LIKEd by nobody (+0.0 after any number of steps).  Ids: unique, full int64 range, shuffled."""
    rng = np.random.default_rng(seed)
    n = n_users + n_items
    reserved = tie_groups * tie_size
    free_items = n_items - reserved
    deg = rng.integers(likes_per_user[0], likes_per_user[1] + 1, size=n_users)
    us = np.repeat(np.arange(n_users), deg)
    its = (rng.random(len(us)) ** 3 * free_items).astype(np.int64) + reserved    # skewed
    pairs = set(zip(us.tolist(), its.tolist()))
    for t in range(tie_groups):
        a, b = rng.choice(n_users, 2, replace=False)
        for j in range(tie_size):
            pairs.add((int(a), t * tie_size + j))
            pairs.add((int(b), t * tie_size + j))
    pairs = sorted(pairs)
    pu = np.array([p[0] for p in pairs], dtype=np.int64)
    pi = np.array([p[1] for p in pairs], dtype=np.int64) + n_users
    # two FRIENDSHIP links per user (both ways): after two steps a seed reaches the items its friends LIKE
    fa = np.repeat(np.arange(n_users), 2)
    fb = (fa + rng.integers(1, n_users, size=len(fa))) % n_users
    fr = sorted(set(zip(fa.tolist(), fb.tolist())) | set(zip(fb.tolist(), fa.tolist())))
    fa = np.array([p[0] for p in fr], dtype=np.int64)
    fb = np.array([p[1] for p in fr], dtype=np.int64)
    src = np.concatenate([pu, pi, fa])
    dst = np.concatenate([pi, pu, fb])
    ety = np.concatenate([np.full(2 * len(pu), gg.EDGE_LIKE), np.full(len(fa), gg.EDGE_FRIENDSHIP)]).astype(np.uint8)
    order = np.lexsort((rng.random(len(src)), src))           # random list order inside a row
    src, dst, ety = src[order], dst[order], ety[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=rowptr[1:])
    node_type = np.array([gg.NODE_USER] * n_users + [gg.NODE_ITEM] * n_items, dtype=np.uint8)
    return dict(node_id=full_range_ids(rng, n), node_type=node_type, rowptr=rowptr, dst=dst.astype(np.int32),
                etype=ety, w=np.ones(len(dst)))


def live_seeds(g, count, rng, with_item=True):
    """Seeds with out-links (dangling seeds take k_emit_dangling, not the ranking kernels): users, and one LIKEd item."""
    deg = np.diff(g["rowptr"])
    users = np.flatnonzero((g["node_type"] == gg.NODE_USER) & (deg > 0))
    s = [int(v) for v in rng.choice(users, count, replace=False)]
    if with_item and count > 1:
        items = np.flatnonzero((g["node_type"] == gg.NODE_ITEM) & (deg > 0))
        s[-1] = int(items[rng.integers(0, len(items))])
    return np.array(s, dtype=np.int32)


class GraphB:
    def __init__(self, amd, n_items, n_users, seed):
        self.amd = amd
        self.g = graph_b(n_items, n_users, seed)
        self.n_items = n_items
        self.handles = {}
        self._ranks = {}
        self._flat = None

    def handle(self, tile_seeds=0, tile_group=0):
        key = (tile_seeds, tile_group)
        if key not in self.handles:
            G = self.amd.Graph.from_flat(**self.g, tile_seeds=tile_seeds, tile_group=tile_group)
            G.buildGraph()
            self.handles[key] = G
        return self.handles[key]

    def flat(self):
        if self._flat is None:
            self._flat = FlatGraph(**self.g)
        return self._flat

    def ranks(self, seeds, T):
        """Model.RunBatch rows: the reference's rank vectors after T steps (widened damping factor), on a handle of
        its own."""
        todo = sorted(set(int(s) for s in seeds if (int(s), T) not in self._ranks))
        if todo:
            r, _ = self.amd.Model.RunBatch(self.handle(), DW,np.array(todo, dtype=np.int32), T)
            for s, row in zip(todo, r):
                self._ranks[(s, T)] = row
        return np.stack([self._ranks[(int(s), T)] for s in seeds])

    def reference(self, seeds, T, top_n):
        g = self.g
        return reference_batch(self.ranks(seeds, T), g["node_id"], g["node_type"], g["rowptr"], g["dst"], g["etype"], seeds, top_n)

    def close(self):
        for G in self.handles.values():
            G.close()
        self.handles.clear()


@pytest.fixture(scope="module")
def graphs_b(amd):
    made = {}

    def get(n_items):
        if n_items not in made:
            made[n_items] = GraphB(amd, n_items, n_users=max(300, n_items // 30), seed=n_items)
        return made[n_items]
    yield get
    for gb in made.values():
        gb.close()


@pytest.mark.parametrize("n_items", [4097, 9000])
@pytest.mark.parametrize("T", [0, 1, 2])
def test_batch_select_both_forms_in_deep_ties(amd, graphs_b, n_items, T):
    """RecommendationBatch, top_n in {1, 1023, 1024}: K = 5 at G = 8 (tg*G <= 64: ticket + k_sel_tail) and K = 100 at
    G = 16 with tile group 7 (tg*G = 112 > 64: k_sel_hist + k_sel_decide), both inside the +0.0 tie of T <= 2."""
    gb = graphs_b(n_items)
    rng = np.random.default_rng(n_items + T)
    for K, ts, tgrp, fused in ((5, 8, 0, True), (100, 16, 7, False)):
        seeds = live_seeds(gb.g, K, rng)
        G = gb.handle(ts, tgrp)
        rec = amd.Recommender(G)
        for top_n in (1, 1023, 1024):
            ids, sc, cnt = rec.RecommendationBatch(seeds, D, T, top_n)
            st = G.stats()
            assert st["tile_seeds"] == ts and top_n <= SEL_MAX_K and n_items > SEL_ROWS
            assert (st["tile_seeds"] * st["tile_group"] <= 64) == fused, st
            ri, rs, rc = gb.reference(seeds, T, top_n)
            assert_same(ids, sc, cnt, ri, rs, rc, ("select", n_items, T, K, top_n))
    # two seeds straight against the C oracle (its own iteration and ranking)
    seeds = live_seeds(gb.g, 2, rng)
    ids, sc, cnt = amd.Recommender(gb.handle(8, 0)).RecommendationBatch(seeds, D, T, 1024)
    oi, os_, oc = gb.flat().recommend_batch(seeds, D, T, 1024)
    assert (cnt == oc).all() and (ids == oi).all() and (bits(sc) == bits(os_)).all()


def sort_path(G, m):
    if m <= SEL_SLOTS:
        return "k_rank_small"
    if G == 1:
        return "k_sort_small" if m <= SMALL_SORT_MAX else "radix_one_segment"
    return "radix_segmented"


@pytest.mark.parametrize("n_items", [4097, 20480, 20481])
def test_batch_full_sort_paths(amd, graphs_b, n_items):
    """RecommendationBatch with top_n in {1025, m - 1, m, m + 5}: k_sort_small (G = 1, m <= SMALL_SORT_MAX), the
    single-segment multi-block sort (G = 1 beyond) and the segmented sort (G = 4, 16) with padded segments."""
    gb = graphs_b(n_items)
    rng = np.random.default_rng(n_items)
    seen = set()
    for ts, K in ((1, 1), (1, 2), (4, 5), (16, 2)):
        G = gb.handle(ts, 0)
        rec = amd.Recommender(G)
        for T in (0, 1, 2):
            seeds = live_seeds(gb.g, K, rng)
            for top_n in (1025, n_items - 1, n_items, n_items + 5):
                ids, sc, cnt = rec.RecommendationBatch(seeds, D, T, top_n)
                assert G.stats()["tile_seeds"] == ts and top_n > SEL_MAX_K
                seen.add(sort_path(ts, n_items))
                ri, rs, rc = gb.reference(seeds, T, top_n)
                assert_same(ids, sc, cnt, ri, rs, rc, ("sort", n_items, ts, K, T, top_n))
    expect = {4097: {"k_sort_small", "radix_segmented"}, 20480: {"k_sort_small", "radix_segmented"},
              20481: {"radix_one_segment", "radix_segmented"}}[n_items]
    assert seen == expect
    seeds = live_seeds(gb.g, 2, rng)
    ids, sc, cnt = amd.Recommender(gb.handle(1, 0)).RecommendationBatch(seeds, D, 2, n_items)
    oi, os_, oc = gb.flat().recommend_batch(seeds, D, 2, n_items)
    assert (cnt == oc).all() and (ids == oi).all() and (bits(sc) == bits(os_)).all()


def test_full_list_beyond_256_sort_blocks(amd):
    """A graph of a little over 2^20 items with few links: one segment needs more than 256 sort blocks, so the scan of
    k_sort_scan_rows carries across chunks.  K = 2, full lists, T = 1, at G = 2 (segmented) and G = 1 (one segment);
    nearly every item sits in the +0.0 tie, which only the id order (item_order, built by the same sort) settles."""
    n_items = (1 << 20) + 3000
    assert n_items > 256 * SORT_CHUNK
    gb = GraphB(amd, n_items, n_users=3000, seed=20)
    try:
        rng = np.random.default_rng(1)
        seeds = live_seeds(gb.g, 2, rng)
        ri, rs, rc = gb.reference(seeds, 1, n_items)
        for ts in (2, 1):
            G = gb.handle(ts, 0)
            ids, sc, cnt = amd.Recommender(G).RecommendationBatch(seeds, D, 1, n_items)
            assert G.stats()["tile_seeds"] == ts
            assert_same(ids, sc, cnt, ri, rs, rc, ("2^20", ts))
        oi, os_ = gb.flat().recommend(int(seeds[0]), D, 1)
        assert (oi == ri[0, :rc[0]]).all() and (bits(os_) == bits(rs[0, :rc[0]])).all()
    finally:
        gb.close()


def eval_sets(gb, seed, T, rng):
    """Test sets for `seed`: hits before and past position 1024, inside the +0.0 tie and at the last entry, duplicates,
    a non-item id and an id of no node; an empty set; the hits past 1024 alone.  Also returns the reference list."""
    ri, rs, rc = gb.reference(np.array([seed], dtype=np.int32), T, gb.n_items)
    c = int(rc[0])
    lst = ri[0, :c]
    zero = np.flatnonzero(rs[0, :c] == 0.0)
    pos = [0, 3, 1023, 1024, 1025, 2000, c - 1]
    if len(zero) >= 5:
        pos += [int(p) for p in rng.choice(zero, 5, replace=False)]
    pos = [p for p in pos if p < c]
    users = gb.g["node_id"][gb.g["node_type"] == gg.NODE_USER]
    missing = int(np.setdiff1d(np.array([7, 8, 9], dtype=np.int64), gb.g["node_id"])[0])
    s1 = [int(lst[p]) for p in pos] + [int(lst[pos[1]]), int(lst[pos[-1]]), int(users[0]), missing]
    s3 = [int(lst[p]) for p in pos if p >= 1024] or [int(lst[-1])]
    return [s1, [], s3], lst


@pytest.mark.parametrize("n_items", [9000, 20481])
@pytest.mark.parametrize("T", [0, 1, 2])
def test_eval_and_eval_batch(amd, graphs_b, n_items, T):
    """RecommendationEval / RecommendationEvalBatch against oracle.c_oracle.evaluate over the reference list: hits, list
    length and sumPrecision bitwise."""
    gb = graphs_b(n_items)
    rng = np.random.default_rng(T + n_items)
    seeds = live_seeds(gb.g, 3, rng)
    rec = amd.Recommender(gb.handle())
    all_sets, expect = [], []
    for s in seeds:
        sets, lst = eval_sets(gb, int(s), T, rng)
        for t in sets:
            h, sp = evaluate(lst, np.unique(np.array(t, dtype=np.int64)))
            gh, gsp, gln = rec.RecommendationEval(int(s), D, T, set(t))
            assert (gh, gln) == (h, len(lst)), (int(s), T)
            assert bits([gsp]) == bits([sp]), (int(s), T, gsp, sp)
            all_sets.append(t)
            expect.append((int(s), h, sp, len(lst)))
    hits, sps, lns = rec.RecommendationEvalBatch(np.array([e[0] for e in expect], dtype=np.int32), D, T, all_sets)
    assert hits.tolist() == [e[1] for e in expect]
    assert lns.tolist() == [e[3] for e in expect]
    assert (bits(sps) == bits([e[2] for e in expect])).all()


@pytest.mark.parametrize("n_items", [4095, 4096])
def test_small_path_at_its_edge(amd, n_items):
    """Recommendation(seed, ...) without top_n on graphs of exactly 4096 and 4095 items (within small_path_ok: the
    one-launch call and its LDS bitonic sort), full-range ids, T = 0 and 1; then the same graphs through EvaluateGraphs."""
    g = graph_b(n_items, n_users=200, seed=n_items, likes_per_user=(1, 4), tie_groups=10, tie_size=20)
    assert len(g["node_id"]) <= 6144 and len(g["dst"]) <= 65536 and n_items <= SM_MAX_ITEMS
    G = amd.Graph.from_flat(**g)
    G.buildGraph()
    Gr = amd.Graph.from_flat(**g)       # reference rank vectors on a handle of their own
    Gr.buildGraph()
    try:
        rng = np.random.default_rng(n_items)
        seeds = live_seeds(g, 4, rng)
        rec = amd.Recommender(G)
        ev_seeds, ev_sets, ev_expect = [], [], []
        for T in (0, 1):
            r, _ = amd.Model.RunBatch(Gr, DW, seeds, T)
            for k, s in enumerate(seeds):
                got = rec.Recommendation(int(s), D, T)
                ri, rs, rc = reference_ranking(r[k], g["node_id"], g["node_type"], g["rowptr"], g["dst"], g["etype"], int(s))
                assert len(got) == rc
                assert [x[0] for x in got] == ri.tolist(), (T, int(s))
                assert (bits([x[1] for x in got]) == bits(rs)).all(), (T, int(s))
                if T == 1:
                    t = [int(ri[p]) for p in (0, 10, rc // 2, rc - 1)] + [int(ri[0])]
                    ev_seeds.append(int(s))
                    ev_sets.append(t)
                    ev_expect.append(evaluate(ri, np.unique(np.array(t, dtype=np.int64))) + (rc,))
        assert G.stats()["tile_seeds"] == 0, "a general-path call ran: the small path was not taken"
        ev_graphs = [amd.Graph.from_flat(**g) for _ in ev_seeds]
        hits, sps, lns = amd.EvaluateGraphs(ev_graphs, ev_seeds, D, 1, ev_sets)
        assert hits.tolist() == [e[0] for e in ev_expect]
        assert (bits(sps) == bits([e[1] for e in ev_expect])).all()
        assert lns.tolist() == [e[2] for e in ev_expect]
        oi, os_ = FlatGraph(**g).recommend(int(seeds[0]), D, 1)
        got = rec.Recommendation(int(seeds[0]), D, 1)
        assert [x[0] for x in got] == oi.tolist() and (bits([x[1] for x in got]) == bits(os_)).all()
    finally:
        G.close()
        Gr.close()
