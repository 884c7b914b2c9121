"""Positions and scores of held-out ids in whole typed lists (rwr_recommend_typed_positions_batch /
rwr_recommend_restart_typed_positions_batch).  The expectation is never the code under test: the rank row comes
from oracle/rwr_oracle.py's Model (tests/test_gpu_typed.py's oracle_row; for restart vectors the sparse-restart idiom of
tests/test_gpu_restart_batch.py), the WHOLE list is filtered and sorted in Python with sorted(key=(-score, -id)), and the
position of a test id is the first index of that id in it.  Positions and list_len must be equal, scores bitwise equal.

Graphs: tests/test_gpu_typed.py's mixed graphs (about 330 nodes, weighted and unit-weight) at tile_seeds = 4, tile_group = 2 --
K = 9 is three tiles in two groups, the last with padding slots -- and boundary graphs as small as their boundary allows:
257 users (255 / 256 / 257 hits in a slot: the finishing prefix sum's chunk; 256 / 257 candidates: the compaction's block),
4 100 users (4 096 / 4 097 hits: the one-workgroup sort against the radix sort, past the counting kernel's LDS budget)."""
import ctypes as C

import numpy as np
import pytest

from tests import graphgen as gg
from tests.test_gpu_typed import CAND_BLOCK, D, PD, PI32, PI64, _mixed, bits, built, expected_list, oracle_row
from tests.test_gpu_typed_eval import EVAL_SORT_SLOTS, typed_eval

pytestmark = pytest.mark.gpu

OPTS = dict(tile_seeds=4, tile_group=2)
FOLLOWS = (gg.EDGE_FRIENDSHIP, gg.EDGE_FOLLOW)
PREFIX_CHUNK = 256         # eval_count.h: counters the finishing workgroup sums per trip (one more than hits)
EXACT_MAX = 256            # RWR_RESTART_EXACT_MAX


@pytest.fixture(scope="module")
def amd():
    import recommendersystems_amd as m
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    return m


@pytest.fixture(scope="module")
def mixed():
    return _mixed(11, uniform=False)


@pytest.fixture(scope="module")
def unit():
    return _mixed(12, uniform=True)


# ---- the expectation -----------------------------------------------------------------------------------------------------------

def first_places(L, test):
    """L = [(id, score), ...] whole and in order: for every test entry the first index of its id and that entry's score"""
    first = {}
    for i, (node_id, score) in enumerate(L):
        first.setdefault(node_id, (i, score))
    pos = np.array([first.get(int(t), (-1, 0.0))[0] for t in test], dtype=np.int64)
    sc = np.array([first.get(int(t), (-1, 0.0))[1] for t in test], dtype=np.float64)
    return pos, sc


def expected_positions(g, seeds, T, tests, cand_type, edge_types, exclude_self):
    lists = [expected_list(g, oracle_row(g, int(s), T), int(s), cand_type, set(edge_types), exclude_self) for s in seeds]
    out = [first_places(L, t) for L, t in zip(lists, tests)]
    return [o[0] for o in out], [o[1] for o in out], np.array([len(L) for L in lists], dtype=np.int64)


def typed_positions(amd, G, seeds, T, tests, cand_type, edge_types=(), exclude_self=False):
    return amd.Recommender(G).RecommendationTypedPositionsBatch(np.asarray(seeds, dtype=np.int32), D, T, tests, cand_type,
                                                                edge_types, exclude_self)


def check(got, want, what):
    pos, sc, ln = got
    wp, ws, wl = want
    print(what, "len", ln.tolist()[:9], "want", wl.tolist()[:9], "pos", [p.tolist()[:6] for p in pos[:3]], "want",
          [p.tolist()[:6] for p in wp[:3]])
    assert (ln == wl).all(), (what, "list_len", ln.tolist(), wl.tolist())
    assert len(pos) == len(wp) and len(sc) == len(ws)
    for k in range(len(wp)):
        assert pos[k].dtype == np.int64 and pos[k].tolist() == wp[k].tolist(), (what, "positions of batch position", k,
                                                                               pos[k].tolist()[:20], wp[k].tolist()[:20])
        assert (bits(sc[k]) == bits(ws[k])).all(), (what, "scores not bitwise equal at batch position", k)


def same(a, b):
    return (all(x.tolist() == y.tolist() for x, y in zip(a[0], b[0])) and all((bits(x) == bits(y)).all() for x, y in zip(a[1], b[1]))
            and (a[2] == b[2]).all())


def make_sets(g, seeds, rng, cand_type, edge_types):
    """one list of test entries per seed, in an order of their own: ids of the type with duplicates, absent ids, an id that only a
    node of another type carries, the id of an excluded target, the seed's own id, an empty list, every candidate's id"""
    ids = g["node_id"][g["node_type"] == cand_type]
    other = g["node_id"][g["node_type"] != cand_type]
    sets = []
    for k, s in enumerate(seeds):
        lo, hi = int(g["rowptr"][s]), int(g["rowptr"][s + 1])
        masked = [int(g["node_id"][g["dst"][p]]) for p in range(lo, hi) if int(g["etype"][p]) in edge_types]
        own = int(g["node_id"][s])
        pick = rng.choice(ids, min(len(ids), 12), replace=False).tolist() if len(ids) else []
        if k % 5 == 0:
            sets.append(pick + [own] + pick[:4] + [-3, 10 ** 12, int(other[k])] + masked[:2] + [own])
        elif k % 5 == 1:
            sets.append([])
        elif k % 5 == 2:
            sets.append(rng.permutation(ids).tolist() + [17, own])         # every candidate, in no order
        elif k % 5 == 3:
            sets.append([5, 6, 999999, int(other[0])])                     # nothing the list could hold
        else:
            sets.append(masked[:3] + pick[:3] + [24, 24, own])
    return sets


def ap_from_positions(pos):
    """Experiment.cs:121-128 from the positions of the distinct hits (unique node ids): the same divisions in the same order"""
    hits = sorted(set(int(p) for p in pos if p >= 0))
    total = 0.0
    for i, p in enumerate(hits):
        total += float(i + 1) / (p + 1)
    return len(hits), total


# ---- 1. who to follow ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["weighted", "value_free"])
def test_who_to_follow_positions(amd, mixed, unit, which):
    g, (linkless, undef_only) = mixed if which == "weighted" else unit
    G = built(amd, g, **OPTS)
    item_seed = 120 + 3
    assert g["node_type"][item_seed] == gg.NODE_ITEM
    # users, one of them twice (with different test entries), an ITEM seed, the user without raw links, the dangling user with
    # UNDEFINED links only
    all_seeds = [0, 5, 5, item_seed, linkless, undef_only, 7, 9, 21]
    rng = np.random.default_rng(3)
    for K in (1, 3, 9):
        seeds = all_seeds[:K] if K > 1 else [5]
        tests = make_sets(g, seeds, rng, gg.NODE_USER, FOLLOWS)
        if K > 2:
            tests[2] = tests[1] + [int(g["node_id"][7]), int(g["node_id"][5])]      # the duplicate seed asks something else
            assert seeds[1] == seeds[2] and tests[1] != tests[2]
        for T in (0, 1, 10):
            for self_ in (False, True):
                want = expected_positions(g, seeds, T, tests, gg.NODE_USER, FOLLOWS, self_)
                got = typed_positions(amd, G, seeds, T, tests, gg.NODE_USER, FOLLOWS, self_)
                check(got, want, (which, K, T, self_))
                assert same(got, typed_positions(amd, G, seeds, T, tests, gg.NODE_USER, FOLLOWS, self_)), "two calls differ"
                # the seed's own id: in the list exactly when the seed is a candidate and exclude_self is off
                for k, s in enumerate(seeds):
                    own = [j for j, t in enumerate(tests[k]) if t == int(g["node_id"][s])]
                    if own:
                        in_list = g["node_type"][s] == gg.NODE_USER and not self_
                        assert all((got[0][k][j] >= 0) == in_list for j in own), (K, T, self_, k)
                # against what exists: the evaluating entry's Hits, its sum bit for bit, its list lengths (node ids are unique here)
                h, sp, ln = typed_eval(amd, G, seeds, T, tests, gg.NODE_USER, FOLLOWS, self_, 0)
                assert (ln == got[2]).all()
                for k in range(len(seeds)):
                    n_hits, total = ap_from_positions(got[0][k])
                    assert n_hits == h[k] and bits([total])[0] == bits(sp[k:k + 1])[0], (which, K, T, self_, k)
            if T == 0:                                   # every score but the seed's is +0.0: the order is the id order alone
                pos, sc, _ = got
                assert all(not bits(sc[k][(pos[k] > 0)]).any() for k in range(len(seeds)))
    G.close()


def test_items_like_is_the_single_seed_whole_list(amd, mixed):
    """ITEM / {LIKE} / no self: the positions in rwr_recommend's whole list (top_n <= 0), and the oracle's"""
    g, _ = mixed
    G = built(amd, g, **OPTS)
    rec = amd.Recommender(G)
    rng = np.random.default_rng(4)
    seeds = [0, 5, 0, 123, 7, 9, 21]                                    # users (one twice) and an item
    tests = make_sets(g, seeds, rng, gg.NODE_ITEM, (gg.EDGE_LIKE,))
    for T in (0, 1, 10):
        got = typed_positions(amd, G, seeds, T, tests, gg.NODE_ITEM, (gg.EDGE_LIKE,), False)
        check(got, expected_positions(g, seeds, T, tests, gg.NODE_ITEM, (gg.EDGE_LIKE,), False), ("items", T))
        singles = [rec.Recommendation(int(s), D, T, 0) for s in seeds]
        want = [first_places(L, t) for L, t in zip(singles, tests)]
        check(got, ([w[0] for w in want], [w[1] for w in want], np.array([len(L) for L in singles], dtype=np.int64)), ("rwr_recommend", T))
    # the one-seed mirror
    p, s, n = rec.RecommendationTypedPositions(5, D, 10, tests[0], amd.NodeType.ITEM, (amd.EdgeType.LIKE,), False)
    wp, ws = first_places(rec.Recommendation(5, D, 10, 0), tests[0])
    assert p.tolist() == wp.tolist() and (bits(s) == bits(ws)).all() and n == len(rec.Recommendation(5, D, 10, 0))
    G.close()


# ---- 2. boundaries ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [CAND_BLOCK, CAND_BLOCK + 1])
def test_prefix_chunk_and_a_block_of_candidates(amd, m):
    """256 / 257 nodes of the candidate type (one block of the compaction, and a row more); 255 / 256 / 257 hits in a slot: the
    finishing workgroup sums hits + 1 counters, 256 per trip"""
    g = gg.random_graph(52, n_users=m, n_items=90, n_likes=800, n_friend=300)
    G = built(amd, g, **OPTS)
    user_ids = g["node_id"][:m]
    seeds = [0, m - 1, m + 5, 3, 3]
    tests = [user_ids[:PREFIX_CHUNK - 1].tolist(), user_ids[:PREFIX_CHUNK].tolist(), user_ids.tolist()[::-1],
             user_ids[1:PREFIX_CHUNK].tolist() + [int(user_ids[0])], []]
    for mask, self_ in (((), False), (FOLLOWS, True)):
        want = expected_positions(g, seeds, 4, tests, gg.NODE_USER, mask, self_)
        if not mask:
            assert [int((p >= 0).sum()) for p in want[0]] == [PREFIX_CHUNK - 1, PREFIX_CHUNK, m, PREFIX_CHUNK, 0]
            assert want[2].tolist() == [m] * 5
        check(typed_positions(amd, G, seeds, 4, tests, gg.NODE_USER, mask, self_), want, ("block", m, mask))
    G.close()


def test_sort_boundary_and_global_counters(amd):
    """4 096 hits in one slot (the one-workgroup sort) and 4 097 in the other (the radix sort); 8 193 keys of the tile are past
    the counting kernel's LDS budget, so its global counters run"""
    g = gg.random_graph(51, n_users=EVAL_SORT_SLOTS + 4, n_items=12, n_likes=260, n_friend=220)
    G = built(amd, g, **OPTS)
    user_ids = g["node_id"][:EVAL_SORT_SLOTS + 4]
    seeds = [2, 7]
    tests = [user_ids[:EVAL_SORT_SLOTS].tolist(), user_ids[:EVAL_SORT_SLOTS + 1].tolist()[::-1]]
    want = expected_positions(g, seeds, 3, tests, gg.NODE_USER, (), False)
    assert [int((p >= 0).sum()) for p in want[0]] == [EVAL_SORT_SLOTS, EVAL_SORT_SLOTS + 1]
    assert want[2].tolist() == [EVAL_SORT_SLOTS + 4] * 2
    got = typed_positions(amd, G, seeds, 3, tests, gg.NODE_USER, (), False)
    check(got, want, "4096 / 4097 hits")
    assert same(got, typed_positions(amd, G, seeds, 3, tests, gg.NODE_USER, (), False)), "two calls differ"
    check(typed_positions(amd, G, seeds, 3, tests, gg.NODE_USER, FOLLOWS, True),
          expected_positions(g, seeds, 3, tests, gg.NODE_USER, FOLLOWS, True), "4096 / 4097 hits, masked")
    G.close()


def test_a_type_no_node_carries(amd, mixed):
    g, _ = mixed
    G = built(amd, g, **OPTS)
    assert not (g["node_type"] == 77).any()
    seeds = [0, 5, 123]
    tests = [g["node_id"][:9].tolist(), [], [17, 17]]
    pos, sc, ln = typed_positions(amd, G, seeds, 3, tests, 77, FOLLOWS, True)
    assert [p.tolist() for p in pos] == [[-1] * 9, [], [-1, -1]] and not ln.any()
    assert all(not bits(s).any() for s in sc)                           # +0.0, not -0.0
    G.close()


# ---- 3. node ids need not be unique ------------------------------------------------------------------------------------------------

def test_two_candidates_share_an_id(amd, mixed):
    """rwr_graph_append_nodes may repeat an id: the best-ranked candidate that carries it answers"""
    g0, _ = mixed
    n = len(g0["node_id"])
    G = built(amd, g0, **OPTS)
    twin = int(g0["node_id"][3])
    # n: a second user with user 3's id, mentioned by user 5 (another score than user 3's)
    # n + 1, n + 2: two users with the id 777 and no link at all (one score: equal 128-bit keys)
    # n + 3, n + 4: two users with the id 888; user 9 follows the first, user 0 mentions the second
    G.appendNodes([(twin, gg.NODE_USER), (777, gg.NODE_USER), (777, gg.NODE_USER), (888, gg.NODE_USER), (888, gg.NODE_USER)],
                  src=[5, 9, 0], dst=[n, n + 3, n + 4], etype=[gg.EDGE_MENTION, gg.EDGE_FOLLOW, gg.EDGE_MENTION], w=[2.0, 1.0, 1.5])
    g = dict(zip(("node_id", "node_type", "rowptr", "dst", "etype", "w"), G._flat))
    assert (g["node_id"] == twin).sum() == 2 and (g["node_id"] == 777).sum() == 2 and (g["node_id"] == 888).sum() == 2
    seeds = [0, 5, 9, 9, 21]
    tests = [[twin, 777, 888, 777], [888, twin], [888, 777, twin], [], [777, int(g["node_id"][7]), twin, 888]]
    for T in (0, 1, 10):
        for self_ in (False, True):
            want = expected_positions(g, seeds, T, tests, gg.NODE_USER, FOLLOWS, self_)
            check(typed_positions(amd, G, seeds, T, tests, gg.NODE_USER, FOLLOWS, self_), want, ("shared ids", T, self_))
    # the three cases hold what they claim, in the oracle's lists at T = 10
    L = expected_list(g, oracle_row(g, 5, 10), 5, gg.NODE_USER, set(FOLLOWS), True)
    at = [i for i, c in enumerate(L) if c[0] == twin]
    assert len(at) == 2 and L[at[0]][1] > L[at[1]][1]                   # two scores: the better one answers
    at = [i for i, c in enumerate(L) if c[0] == 777]
    assert len(at) == 2 and at[1] == at[0] + 1 and L[at[0]] == L[at[1]]  # equal keys: f, not f + 1
    assert first_places(L, [777])[0][0] == at[0]
    L9 = expected_list(g, oracle_row(g, 9, 10), 9, gg.NODE_USER, set(FOLLOWS), True)
    assert [c[0] for c in L9].count(888) == 1 and [c[0] for c in L].count(888) == 2     # seed 9 follows one of the pair
    G.close()


# ---- 4. the restart-vector driver --------------------------------------------------------------------------------------------------

def restart_list(g, row, members, cand_type, edge_types, exclude_members):
    out = set()
    for m in members:
        for p in range(int(g["rowptr"][m]), int(g["rowptr"][m + 1])):
            if int(g["etype"][p]) in edge_types:
                out.add(int(g["dst"][p]))
    if exclude_members:
        out |= {int(m) for m in members}
    cand = [(int(g["node_id"][i]), float(row[i])) for i in range(len(row)) if g["node_type"][i] == cand_type and i not in out]
    return sorted(cand, key=lambda c: (-c[1], -c[0]))


class RestartCase:
    def __init__(self, amd, g, linkless):
        from tests.test_gpu_restart_batch import _oracle_graph
        self.amd, self.g, self.n = amd, g, len(g["node_id"])
        self.G = built(amd, g, **OPTS)
        self.PG = _oracle_graph(g)
        rng = np.random.default_rng(8)
        sizes = [8, 1, 3, 2, 5, 8, 4, 1, 6]                              # 1 to 8 support rows
        self.restarts = []
        for k, m in enumerate(sizes):
            idx = rng.choice(120, m, replace=False).astype(np.int32)
            if m >= 3 and k % 3 == 2:
                idx[1] = 120 + int(rng.integers(0, 200))                 # an ITEM node in the support
            self.restarts.append((idx, rng.random(m) + 0.05))
        self.restarts[4] = (np.array([linkless, 3, 9, 40, 41], dtype=np.int32), np.array([0.5, 1.0, 0.25, 2.0, 0.125]))
        self.starts = np.array([-1, 7, 3, -1, 3, 11, 130, -1, 0], dtype=np.int32)
        self.sets = [np.zeros(0, dtype=np.int32), np.array([5, 9, 5], dtype=np.int32), np.array([0, 1, 33], dtype=np.int32),
                     np.array([7, 125], dtype=np.int32), np.array([linkless, 5], dtype=np.int32), np.array([21], dtype=np.int32),
                     np.array([2, 3, 4], dtype=np.int32), np.zeros(0, dtype=np.int32), np.array([9], dtype=np.int32)]
        self._rows = {}

    def close(self):
        self.G.close()

    def row(self, k, T):
        """the oracle's Model with vector k as its restart field, after T steps"""
        from tests.test_gpu_restart_batch import _oracle_model
        if (k, T) not in self._rows:
            idx, val = self.restarts[k]
            m = _oracle_model(self.PG, D, int(self.starts[k]), idx, val)
            for _ in range(T):
                m.deliverRanks()
                m.updateRanks()
            self._rows[(k, T)] = np.array(m.rank, dtype=np.float64)
        return self._rows[(k, T)]

    def members(self, k, explicit):
        return self.sets[k] if explicit else self.restarts[k][0]

    def tests(self, ks, explicit, rng):
        ids = self.g["node_id"][self.g["node_type"] == gg.NODE_USER]
        out = []
        for j, k in enumerate(ks):
            mem = [int(self.g["node_id"][m]) for m in self.members(k, explicit)]
            pick = rng.choice(ids, 10, replace=False).tolist()
            out.append([] if j % 4 == 3 else rng.permutation(ids).tolist() if j % 4 == 2 else pick + mem + pick[:3] + [-3, 10 ** 12])
        return out

    def want(self, ks, T, tests, members, explicit, rows=None):
        lists = [restart_list(self.g, rows[j] if rows else self.row(k, T), self.members(k, explicit), gg.NODE_USER, set(FOLLOWS), members)
                 for j, k in enumerate(ks)]
        out = [first_places(L, t) for L, t in zip(lists, tests)]
        return [o[0] for o in out], [o[1] for o in out], np.array([len(L) for L in lists], dtype=np.int64)

    def call(self, ks, T, tests, members, explicit, restarts=None, starts=None):
        rec = self.amd.Recommender(self.G)
        return rec.RecommendationRestartTypedPositionsBatch(restarts or [self.restarts[k] for k in ks],
                                                            self.starts[list(ks)] if starts is None else starts, D, T, tests,
                                                            gg.NODE_USER, FOLLOWS, members,
                                                            exclude=[self.sets[k] for k in ks] if explicit else None)


@pytest.fixture(scope="module")
def restart_case(amd):
    g, (linkless, _) = _mixed(11, uniform=False)
    c = RestartCase(amd, g, linkless)
    yield c
    c.close()


@pytest.mark.parametrize("K", [3, 9])
def test_restart_vectors(restart_case, K):
    c = restart_case
    ks = list(range(K)) if K == 9 else [4, 1, 6]
    rng = np.random.default_rng(12)
    for T in (0, 1, 10):
        for members in (False, True):
            for explicit in (False, True):
                tests = c.tests(ks, explicit, rng)
                got = c.call(ks, T, tests, members, explicit)
                check(got, c.want(ks, T, tests, members, explicit), ("restart", K, T, members, explicit))
                if T == 10:
                    assert same(got, c.call(ks, T, tests, members, explicit)), "two calls differ"


def test_restart_fallback_classes(restart_case):
    """K == 1 and a vector of 257 support entries run vector by vector through rwr_model_run_restart, whose rank row is
    tolerance parity only for the wide vector: the expectation ranks THAT call's own row on the host (the composition the
    header states) instead of the oracle's"""
    from tests.test_gpu_restart_rank import _single_row
    c = restart_case
    rng = np.random.default_rng(13)
    for k in (0, 4):
        for members in (False, True):
            tests = c.tests([k], k == 4, rng)
            rows = [_single_row(c.G, c.n, *c.restarts[k], int(c.starts[k]), D, 10)]
            check(c.call([k], 10, tests, members, k == 4), c.want([k], 10, tests, members, k == 4, rows), ("K == 1", k, members))
            check(c.call([k], 10, tests, members, k == 4), c.want([k], 10, tests, members, k == 4), ("K == 1, oracle", k, members))
    wide_idx = rng.choice(c.n, EXACT_MAX + 1, replace=False).astype(np.int32)
    ks = [1, 2, 4]
    restarts = [c.restarts[1], (wide_idx, rng.random(EXACT_MAX + 1) + 0.1), c.restarts[4]]
    starts = np.array([-1, 7, 3], dtype=np.int32)
    for T in (1, 10):
        rows = [_single_row(c.G, c.n, *restarts[j], int(starts[j]), D, T) for j in range(3)]
        for members in (False, True):
            tests = c.tests(ks, True, rng)
            got = c.call(ks, T, tests, members, True, restarts=restarts, starts=starts)
            check(got, c.want(ks, T, tests, members, True, rows), ("wide", T, members))


# ---- 5. refusals on a live graph ---------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(amd, mixed):
    from recommendersystems_amd import _lib
    lib = _lib.load()
    name = b"rwr_recommend_typed_positions_batch"
    g, _ = mixed
    n = len(g["node_id"])
    G = built(amd, g, **OPTS)
    h = G._handle()
    K = 4
    seeds = np.array([0, 5, 9, 123], dtype=np.int32)
    tp = np.array([0, 2, 2, 3, 5], dtype=np.int64)
    ti = g["node_id"][[1, 2, 3, 4, 1]].astype(np.int64)
    pos, sc, ln = np.full(5, -77, dtype=np.int64), np.full(5, -7.5), np.full(K, -9, dtype=np.int64)
    ps, pp, pt = seeds.ctypes.data_as(PI32), tp.ctypes.data_as(PI64), ti.ctypes.data_as(PI64)
    po_, pq, pl = pos.ctypes.data_as(PI64), sc.ctypes.data_as(PD), ln.ctypes.data_as(PI64)

    def call(handle=h, s=ps, k=K, d=D, T=3, cand=gg.NODE_USER, mask=0x0c, self_=1, p=pp, t=pt, o=po_, q=pq, m=pl):
        return (lib.rwr_recommend_typed_positions_batch(handle, s, k, C.c_float(d), T, cand, mask, self_, p, t, o, q, m),
                lib.rwr_last_error())

    def untouched():
        return (pos == -77).all() and (sc == -7.5).all() and (ln == -9).all()

    st, msg = call(handle=None, k=-1, cand=999, p=None)               # a NULL graph is refused first
    assert st == _lib.RWR_E_INVALID and b"NULL graph" in msg
    assert call(k=0, s=None, cand=999, mask=1 << 9, p=None, t=None, o=None)[0] == _lib.RWR_OK and untouched()
    for kw, word in ((dict(k=-1), b"negative K"), (dict(s=None), b"seeds"), (dict(cand=256), b"cand_type"),
                     (dict(mask=1 << 8), b"excl_edge_mask")):
        for extra in (dict(), dict(p=None), dict(o=None)):
            st, msg = call(**kw, **extra)
            assert st == _lib.RWR_E_INVALID and name in msg and word in msg, (kw, extra, st, msg)
            assert untouched(), kw
    seeds[2] = n
    st, msg = call(o=None)
    assert st == _lib.RWR_E_RANGE and name in msg and b"batch position 2" in msg and untouched()
    seeds[2] = 9
    for kw, word in ((dict(p=None), b"NULL test_ptr"), (dict(o=None), b"NULL pos_out"), (dict(t=None), b"NULL test_ids")):
        st, msg = call(**kw)
        assert st == _lib.RWR_E_INVALID and name in msg and word in msg, (kw, st, msg)
        assert untouched(), kw
    tp[0] = 1
    st, msg = call()
    assert st == _lib.RWR_E_INVALID and b"test_ptr[0]" in msg and untouched()
    tp[0], tp[2] = 0, 1
    st, msg = call()
    assert st == _lib.RWR_E_INVALID and b"decreases at batch position 1" in msg and untouched()
    tp[2] = 2
    for d in (-0.25, 1.5, float("nan")):                               # the domain comes last
        st, msg = call(d=d)
        assert st == _lib.RWR_E_UNSUPPORTED and b"[0, 1]" in msg and untouched(), d
    # a correct call afterwards answers right; score_out and list_len may be NULL
    tests = [ti[0:2].tolist(), [], ti[2:3].tolist(), ti[3:5].tolist()]
    wp, ws, wl = expected_positions(g, seeds.tolist(), 3, tests, gg.NODE_USER, FOLLOWS, True)
    assert call()[0] == _lib.RWR_OK
    assert pos.tolist() == np.concatenate(wp).tolist() and (bits(sc) == bits(np.concatenate(ws))).all() and (ln == wl).all()
    pos[:], sc[:], ln[:] = -77, -7.5, -9
    assert call(q=None, m=None)[0] == _lib.RWR_OK
    assert pos.tolist() == np.concatenate(wp).tolist() and (sc == -7.5).all() and (ln == -9).all()
    G.close()
