"""Ranked walks within a caller-set candidate pool and with per-seed deny lists (rwr_recommend_filtered_batch,
rwr_recommend_filtered_positions_batch / Recommender.RecommendationFilteredBatch).  The expectation is never the
code under test: the rank row comes from oracle/rwr_oracle.py's Model (as in tests/test_gpu_typed.py, whose graphs and row cache
are shared), the candidates are filtered -- type, pool, masked link targets, the seed, the deny list -- and sorted here with
sorted(key=(-score, -id)).  Ids must be equal, scores bitwise equal.

Shapes: the mixed weighted and unit-weight graphs of a few hundred nodes; 256 / 257 nodes (the compaction's block) with pool
members on both sides of the bitmap's word edges; 1 025 pooled users for top-1024; K = 20 on tiles of 8 seeds, one tile a
group, so that the deny pairs of later groups start at an offset."""
import ctypes as C

import numpy as np
import pytest

from tests import graphgen as gg
from tests.test_gpu_typed import _flat, _lists, _mixed, bits, built, oracle_row

pytestmark = pytest.mark.gpu

D = 0.15
CAND_BLOCK = 256           # cand_plan.h
SEL_MAX_K = 1024           # rank_keys.h
PI64, PI32, PD = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
FOLLOWS = (gg.EDGE_FRIENDSHIP, gg.EDGE_FOLLOW)


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


# ---- the expectation -------------------------------------------------------------------------------------------------------------

def expected_list(g, row, seed, cand_type, edge_types, exclude_self, pool, deny):
    """the whole list the header defines for one seed: [(id, score), ...]; cand_type None: any type, pool None: no pool"""
    lo, hi = int(g["rowptr"][seed]), int(g["rowptr"][seed + 1])
    out = {int(g["dst"][p]) for p in range(lo, hi) if int(g["etype"][p]) in edge_types}
    if exclude_self:
        out.add(int(seed))
    out |= {int(x) for x in deny}
    inside = None if pool is None else {int(x) for x in pool}
    cand = [(int(g["node_id"][i]), float(row[i])) for i in range(len(row))
            if (cand_type is None or g["node_type"][i] == cand_type) and (inside is None or i in inside) and i not in out]
    return sorted(cand, key=lambda c: (-c[1], -c[0]))


def expected(g, seeds, T, top_n, cand_type, edge_types, exclude_self, pool, deny):
    K = len(seeds)
    ids, sc, cnt = np.zeros((K, top_n), dtype=np.int64), np.zeros((K, top_n)), np.zeros(K, dtype=np.int32)
    for k, s in enumerate(seeds):
        L = expected_list(g, oracle_row(g, int(s), T), int(s), cand_type, set(edge_types), exclude_self, pool,
                          () if deny is None else deny[k])[:top_n]
        cnt[k] = len(L)
        ids[k, :len(L)] = [c[0] for c in L]
        sc[k, :len(L)] = [c[1] for c in L]
    return ids, sc, cnt


def expected_positions(g, seeds, T, tests, cand_type, edge_types, exclude_self, pool, deny):
    pos, sc, ln = [], [], np.zeros(len(seeds), dtype=np.int64)
    for k, s in enumerate(seeds):
        L = expected_list(g, oracle_row(g, int(s), T), int(s), cand_type, set(edge_types), exclude_self, pool,
                          () if deny is None else deny[k])
        first = {}
        for at, (i, x) in enumerate(L):
            first.setdefault(i, (at, x))
        pos.append(np.array([first.get(int(t), (-1, 0.0))[0] for t in tests[k]], dtype=np.int64))
        sc.append(np.array([first.get(int(t), (-1, 0.0))[1] for t in tests[k]], dtype=np.float64))
        ln[k] = len(L)
    return pos, sc, ln


def check(got, want, what):
    ids, sc, cnt = got
    wi, ws, wc = want
    print(what, "counts", cnt.tolist()[:8], "want", wc.tolist()[:8])
    assert (cnt == wc).all(), (what, "counts", cnt.tolist(), wc.tolist())
    bad = np.flatnonzero((ids != wi).any(axis=1))
    assert bad.size == 0, (what, "ids differ in rows", bad.tolist(), ids[bad[0]].tolist()[:10], wi[bad[0]].tolist()[:10])
    bad = np.flatnonzero((bits(sc) != bits(ws)).any(axis=1))
    assert bad.size == 0, (what, "scores not bitwise equal in rows", bad.tolist())


def check_positions(got, want, what):
    pos, sc, ln = got
    wp, ws, wl = want
    print(what, "list_len", ln.tolist()[:8], "want", wl.tolist()[:8])
    assert (ln == wl).all(), (what, "list_len", ln.tolist(), wl.tolist())
    for k in range(len(wp)):
        assert pos[k].tolist() == wp[k].tolist(), (what, "positions of batch position", k, pos[k].tolist(), wp[k].tolist())
        assert (bits(sc[k]) == bits(ws[k])).all(), (what, "scores not bitwise equal at batch position", k)


def filtered(amd, G, seeds, T, top_n, cand_type, edge_types=(), exclude_self=False, pool=None, deny=None):
    return amd.Recommender(G).RecommendationFilteredBatch(np.asarray(seeds, dtype=np.int32), D, T, top_n, cand_type, edge_types,
                                                          exclude_self, pool, deny)


def rows_of(g, t):
    return np.flatnonzero(g["node_type"] == t)


# ---- 1. pools and deny lists on the mixed graphs ---------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["weighted", "value_free"])
def test_pool_and_deny_lists(amd, mixed, unit, which):
    g, (linkless, undef_only) = mixed if which == "weighted" else unit
    n = len(g["node_id"])
    G = built(amd, g)
    assert G.stats()["uniform_path"] == (0 if which == "weighted" else 1)
    rng = np.random.default_rng(3)
    items, users = rows_of(g, gg.NODE_ITEM), rows_of(g, gg.NODE_USER)
    # an unsorted pool with duplicates: a third of the items, some users (non-matching when the candidates are ITEM)
    pool = np.concatenate([rng.choice(items, 70, replace=False), rng.choice(users, 15, replace=False)])
    pool = rng.permutation(np.concatenate([pool, pool[:30]]))
    in_pool = [int(x) for x in np.unique(pool[np.isin(pool, items)])[:6]]      # six distinct pooled items
    off_pool = [int(x) for x in np.setdiff1d(items, pool)[:3]]
    # two positions hold seed 5 with different deny lists; the dangling seeds; an ITEM seed that denies itself
    item_seed = int(items[3])
    seeds = [0, 5, 5, item_seed, linkless, undef_only, 9]
    deny = [in_pool[:3] + in_pool[:3] + [0],                      # duplicates and the seed itself
            in_pool[3:6] + off_pool,                              # rows outside the pool
            [],                                                   # the same seed, nothing denied
            [item_seed] + [int(u) for u in users[:4]],            # the seed (a candidate of the pool or not) and other types
            [int(x) for x in np.unique(pool)],                    # the whole pool: nothing is left
            [int(x) for x in items],                              # every item
            [n - 1, n - 2]]
    for T in (0, 1, 5):
        for cand in (gg.NODE_ITEM, None):
            for mask, self_ in (((gg.EDGE_LIKE,), False), ((), True)):
                got = filtered(amd, G, seeds, T, 120, cand, mask, self_, pool, deny)       # (120: no list is cut)
                want = expected(g, seeds, T, 120, cand, mask, self_, pool, deny)
                assert want[2][4] == 0 and (cand is None or want[2][5] == 0)
                if not mask:                                      # no link exclusion: the three denied pool items are the difference
                    assert want[2][2] == want[2][1] + 3
                check(got, want, (which, T, cand, mask, self_))
    # the pool alone, the deny lists alone
    check(filtered(amd, G, seeds, 5, 40, gg.NODE_ITEM, (gg.EDGE_LIKE,), False, pool, None),
          expected(g, seeds, 5, 40, gg.NODE_ITEM, (gg.EDGE_LIKE,), False, pool, None), (which, "pool alone"))
    check(filtered(amd, G, seeds, 5, 40, gg.NODE_USER, FOLLOWS, True, None, deny),
          expected(g, seeds, 5, 40, gg.NODE_USER, FOLLOWS, True, None, deny), (which, "deny alone"))
    G.close()


def test_one_seed_mirror(amd, mixed):
    g, _ = mixed
    G = built(amd, g)
    pool = [int(x) for x in rows_of(g, gg.NODE_USER)[::2]]
    got = amd.Recommender(G).RecommendationFiltered(5, D, 3, 15, amd.NodeType.USER, (amd.EdgeType.FRIENDSHIP, amd.EdgeType.FOLLOW),
                                                    True, pool=pool, deny=pool[:4])
    want = expected_list(g, oracle_row(g, 5, 3), 5, gg.NODE_USER, set(FOLLOWS), True, pool, pool[:4])[:15]
    assert len(want) == 15 and [r[0] for r in got] == [w[0] for w in want]
    assert (bits([r[1] for r in got]) == bits([w[1] for w in want])).all()
    G.close()


# ---- 2. the list build at its edges ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [CAND_BLOCK, CAND_BLOCK + 1])
def test_block_and_word_edges(amd, n):
    g = gg.random_graph(21, n_users=100, n_items=n - 100, n_likes=900, n_friend=60)
    assert len(g["node_id"]) == n
    G = built(amd, g)
    seeds = [0, 4, 9, n - 1]
    edge = [31, 32, 33, n - 1]
    for pool in (edge, [n - 1], [33, n - 1, 31, 32, 32, 31, n - 1, 33], [255, 0, 63, 64, 255], list(range(n - 1, -1, -1)) * 2):
        for cand in (None, gg.NODE_USER, gg.NODE_ITEM):
            got = filtered(amd, G, seeds, 3, 6, cand, (), False, pool, None)
            want = expected(g, seeds, 3, 6, cand, (), False, pool, None)
            check(got, want, ("edges", n, pool[:8], cand))
    # every row but the last one denied: the last row of the last block is the one candidate
    deny = [list(range(n - 1))] * 4
    want = expected(g, seeds, 3, 6, None, (), False, None, deny)
    assert want[2].tolist() == [1, 1, 1, 1] and (want[0][:, 0] == g["node_id"][n - 1]).all()
    check(filtered(amd, G, seeds, 3, 6, None, (), False, None, deny), want, ("all but the last row denied", n))
    G.close()


def test_pool_shapes(amd, mixed):
    """a pool that is empty, that holds all nodes, that holds only nodes of another type; cand_type -1 with and without it"""
    g, _ = mixed
    n = len(g["node_id"])
    G = built(amd, g)
    seeds = [0, 5, 123, 9]
    users = [int(x) for x in rows_of(g, gg.NODE_USER)]
    for pool, cand, empty in (([], gg.NODE_ITEM, True), ([], None, True), (list(range(n)), gg.NODE_ITEM, False),
                              (list(range(n)), None, False), (users, gg.NODE_ITEM, True), (users, None, False),
                              (None, None, False)):
        got = filtered(amd, G, seeds, 4, 25, cand, (gg.EDGE_LIKE,), True, pool, None)
        want = expected(g, seeds, 4, 25, cand, (gg.EDGE_LIKE,), True, pool, None)
        assert (want[2] == 0).all() == empty
        check(got, want, ("pool shape", None if pool is None else len(pool), cand))
    # the whole-graph pool and no pool are one list; so is the ITEM pool under cand_type -1 and the ITEM type without a pool
    a = filtered(amd, G, seeds, 4, 25, gg.NODE_ITEM, (), False, None, None)
    b = filtered(amd, G, seeds, 4, 25, None, (), False, [int(x) for x in rows_of(g, gg.NODE_ITEM)], None)
    check(a, b, "ITEM by type and ITEM by pool")
    G.close()


def test_top_1024_of_a_pool_of_1025(amd):
    from recommendersystems_amd import _lib
    g = gg.random_graph(41, n_users=SEL_MAX_K + 40, n_items=60, n_likes=2500, n_friend=700)
    G = built(amd, g)
    seeds = [3, 1030]
    pool = [int(x) for x in np.random.default_rng(2).permutation(SEL_MAX_K + 40)[:SEL_MAX_K + 1]]
    got = filtered(amd, G, seeds, 3, SEL_MAX_K, gg.NODE_USER, (), False, pool, None)
    want = expected(g, seeds, 3, SEL_MAX_K, gg.NODE_USER, (), False, pool, None)
    assert want[2].tolist() == [SEL_MAX_K, SEL_MAX_K]
    check(got, want, "top-1024 of 1025 pooled")
    got = filtered(amd, G, seeds, 3, SEL_MAX_K, gg.NODE_USER, (gg.EDGE_FRIENDSHIP,), True, pool, [pool[:5], pool[5:9]])
    check(got, expected(g, seeds, 3, SEL_MAX_K, gg.NODE_USER, (gg.EDGE_FRIENDSHIP,), True, pool, [pool[:5], pool[5:9]]),
          "top-1024, exclusions")
    with pytest.raises(_lib.RwrError) as e:
        filtered(amd, G, seeds, 3, SEL_MAX_K + 1, gg.NODE_USER, (), False, pool, None)
    assert e.value.status == _lib.RWR_E_UNSUPPORTED and "1024" in str(e.value)
    G.close()


# ---- 3. tile groups, identity, determinism -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["weighted", "value_free"])
def test_deny_pairs_across_tile_groups(amd, mixed, unit, which):
    """K = 20 on tiles of 8 seeds, one tile a group: three groups, the last with four padding slots; every batch position has a
    deny list of its own length (0 .. 19 rows), so that the pairs of the second and third group start at an offset"""
    g, (linkless, _) = mixed if which == "weighted" else unit
    G = built(amd, g, tile_seeds=8, tile_group=1)
    items = [int(x) for x in rows_of(g, gg.NODE_ITEM)]
    seeds = [int(s) for s in (np.arange(20) * 5) % 120]
    seeds[7], seeds[13] = seeds[2], linkless                       # a repeated seed, a dangling one
    pool = items[::2] + items[:10]
    deny = [pool[k:2 * k] for k in range(20)]
    for T in (1, 5):
        got = filtered(amd, G, seeds, T, 30, gg.NODE_ITEM, (gg.EDGE_LIKE,), False, pool, deny)
        check(got, expected(g, seeds, T, 30, gg.NODE_ITEM, (gg.EDGE_LIKE,), False, pool, deny), ("groups", which, T))
    st = G.stats()
    assert st["tile_seeds"] == 8 and st["tile_group"] == 1
    tests = [[int(g["node_id"][r]) for r in pool[:12]] for _ in seeds]
    got = amd.Recommender(G).RecommendationFilteredPositionsBatch(seeds, D, 5, tests, gg.NODE_ITEM, (gg.EDGE_LIKE,), False, pool, deny)
    check_positions(got, expected_positions(g, seeds, 5, tests, gg.NODE_ITEM, (gg.EDGE_LIKE,), False, pool, deny), ("groups", which))
    G.close()


def test_identity_with_the_typed_entries(amd, mixed):
    """no pool, no deny lists, a node type: the typed entries' own arrays, from an actual call on the same handle"""
    g, (linkless, undef_only) = mixed
    G = built(amd, g)
    rec = amd.Recommender(G)
    seeds = np.array([0, 5, 5, 123, linkless, undef_only, 7, 9, 21, 33, 2], dtype=np.int32)
    tests = [[int(x) for x in g["node_id"][k:k + 9]] + [123456789] for k in range(len(seeds))]
    for cand, mask, self_ in ((gg.NODE_USER, FOLLOWS, True), (gg.NODE_ITEM, (gg.EDGE_LIKE,), False), (77, (), False)):
        for T in (0, 1, 5):
            want = rec.RecommendationTypedBatch(seeds, D, T, 20, cand, mask, self_)
            got = rec.RecommendationFilteredBatch(seeds, D, T, 20, cand, mask, self_)
            assert all((a == b).all() for a, b in zip(got[:1] + got[2:], want[:1] + want[2:])) and (bits(got[1]) == bits(want[1])).all()
            wp, ws, wl = rec.RecommendationTypedPositionsBatch(seeds, D, T, tests, cand, mask, self_)
            gp, gs, gl = rec.RecommendationFilteredPositionsBatch(seeds, D, T, tests, cand, mask, self_)
            check_positions((gp, gs, gl), (wp, ws, wl), ("identity", cand, T))
    G.close()


def test_the_same_call_twice(amd, unit):
    g, _ = unit
    G = built(amd, g)
    rng = np.random.default_rng(8)
    seeds = [0, 5, 9, 123, 40]
    pool = rng.integers(0, len(g["node_id"]), 400)
    deny = [rng.integers(0, len(g["node_id"]), 30) for _ in seeds]
    tests = [g["node_id"][rng.integers(0, len(g["node_id"]), 20)] for _ in seeds]
    rec = amd.Recommender(G)
    a = rec.RecommendationFilteredBatch(seeds, D, 4, 50, None, FOLLOWS, True, pool, deny)
    pa = rec.RecommendationFilteredPositionsBatch(seeds, D, 4, tests, None, FOLLOWS, True, pool, deny)
    rec.RecommendationTypedBatch(seeds, D, 4, 50, gg.NODE_USER)              # (another call in between)
    b = rec.RecommendationFilteredBatch(seeds, D, 4, 50, None, FOLLOWS, True, pool, deny)
    pb = rec.RecommendationFilteredPositionsBatch(seeds, D, 4, tests, None, FOLLOWS, True, pool, deny)
    assert (a[0] == b[0]).all() and (bits(a[1]) == bits(b[1])).all() and (a[2] == b[2]).all()
    check_positions(pa, pb, "twice")
    check(a, expected(g, seeds, 4, 50, None, FOLLOWS, True, pool, deny), "twice: the oracle")
    G.close()


def test_pooled_calls_leave_the_cached_lists_alone(amd, mixed):
    """typed calls before and after pooled ones of the same type, of type -1 and of four further types: equal, and the oracle's"""
    g, _ = mixed
    G = built(amd, g)
    seeds = [0, 5, 9]
    before = amd.Recommender(G).RecommendationTypedBatch(seeds, D, 3, 20, gg.NODE_USER, FOLLOWS, True)
    for cand in (gg.NODE_USER, None, 7, 8, 9, 10):
        filtered(amd, G, seeds, 3, 20, cand, (), False, [1, 2, 3, 200, 201], None)
    after = amd.Recommender(G).RecommendationTypedBatch(seeds, D, 3, 20, gg.NODE_USER, FOLLOWS, True)
    check(after, before, "typed after pooled")
    check(filtered(amd, G, seeds, 3, 20, gg.NODE_USER, FOLLOWS, True), before, "unpooled filtered takes the cached list")
    G.close()


# ---- 4. appended nodes ------------------------------------------------------------------------------------------------------------

def test_pool_names_appended_nodes(amd, mixed):
    from recommendersystems_amd import _lib
    g, _ = mixed
    n = len(g["node_id"])
    G = built(amd, g)
    seeds = [0, 5, 9, 123]
    pool = [n + 2, 3, n, 7, n + 3, 20, 21, n]
    with pytest.raises(_lib.RwrError) as e:                         # out of range before the append ...
        filtered(amd, G, seeds, 4, 10, gg.NODE_USER, FOLLOWS, True, pool, None)
    assert e.value.status == _lib.RWR_E_RANGE and "pool position 0" in str(e.value)
    with pytest.raises(_lib.RwrError) as e:
        filtered(amd, G, seeds, 4, 10, gg.NODE_USER, FOLLOWS, True, None, [[], [3, n], [], []])
    assert e.value.status == _lib.RWR_E_RANGE and "batch position 1" in str(e.value)
    G.appendNodes([(90001, gg.NODE_USER), (90002, gg.NODE_ITEM), (90003, gg.NODE_USER), (90004, gg.NODE_USER)],
                  src=[0, 5, n, n + 2, 9, n + 3], dst=[n, n + 2, 5, 0, n + 3, 9],
                  etype=[gg.EDGE_FOLLOW, gg.EDGE_MENTION, gg.EDGE_FRIENDSHIP, gg.EDGE_FOLLOW, gg.EDGE_MENTION, gg.EDGE_FOLLOW],
                  w=[1.0, 2.0, 1.0, 1.0, 0.5, 1.0])
    grown = dict(zip(("node_id", "node_type", "rowptr", "dst", "etype", "w"), G._flat))
    seeds2 = seeds + [n, n + 3]
    deny = [[], [n + 2], [n + 3, n + 3], [], [n], [3, 7]]
    for cand in (gg.NODE_USER, None):                               # ... and legal after it
        got = filtered(amd, G, seeds2, 4, 10, cand, (gg.EDGE_FRIENDSHIP,), True, pool, deny)
        want = expected(grown, seeds2, 4, 10, cand, (gg.EDGE_FRIENDSHIP,), True, pool, deny)
        check(got, want, ("after append_nodes", cand))
        assert any({90001, 90003, 90004} & set(got[0][k, :got[2][k]].tolist()) for k in range(len(seeds2))), "no new user in any list"
    with pytest.raises(_lib.RwrError) as e:
        filtered(amd, G, seeds2, 4, 10, gg.NODE_USER, (), False, [3, n + 4], None)
    assert e.value.status == _lib.RWR_E_RANGE and "pool position 1" in str(e.value)
    G.close()


# ---- 5. positions -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["weighted", "value_free"])
def test_positions_in_the_filtered_lists(amd, mixed, unit, which):
    g, (linkless, _) = mixed if which == "weighted" else unit
    G = built(amd, g)
    rec = amd.Recommender(G)
    items = [int(x) for x in rows_of(g, gg.NODE_ITEM)]
    pool = items[1::2] + items[1:9:2]
    outside = items[0::2]
    seeds = [0, 5, 5, linkless, 9]
    deny = [pool[:4], pool[4:8] + pool[4:8], [], pool, []]
    ident = lambda rows: [int(g["node_id"][r]) for r in rows]
    # a denied id, an id outside the pool, an id no node carries, ids of the list (one of them twice), a user's id
    tests = [ident(deny[0][:2]) + ident(outside[:2]) + [987654321] + ident(pool[10:14]) + ident(pool[10:11]) + ident([3]),
             ident(pool[:12]), ident(pool[:12]), ident(pool[:3]), []]
    for T in (0, 1, 5):
        got = rec.RecommendationFilteredPositionsBatch(seeds, D, T, tests, gg.NODE_ITEM, (gg.EDGE_LIKE,), False, pool, deny)
        want = expected_positions(g, seeds, T, tests, gg.NODE_ITEM, (gg.EDGE_LIKE,), False, pool, deny)
        check_positions(got, want, ("positions", which, T))
        assert got[0][0][:5].tolist() == [-1] * 5 and (bits(got[1][0][:5]) == 0).all()       # -1 / +0.0
        assert got[0][0][9] == got[0][0][5]                                                  # the duplicate entry
        assert got[2][3] == 0 and got[0][3].tolist() == [-1] * 3                             # the whole pool denied
        assert got[2][2] >= got[2][1] and got[2][2] <= len(set(pool))                        # list_len is the filtered length
    # an empty pool: every position -1, every list empty
    pos, sc, ln = rec.RecommendationFilteredPositionsBatch(seeds, D, 3, tests, None, (), False, [], None)
    assert (ln == 0).all() and all((p == -1).all() and (bits(s) == 0).all() for p, s in zip(pos, sc))
    G.close()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_in_their_order_write_nothing(amd, mixed):
    from recommendersystems_amd import _lib
    lib = _lib.load()
    g, _ = mixed
    n = len(g["node_id"])
    G = built(amd, g)
    h = G._handle()
    K, top_n = 4, 6
    seeds = np.array([0, 5, 9, 123], dtype=np.int32)
    pool = np.array([3, 200, 3, 7], dtype=np.int32)
    dp, di = np.array([0, 1, 1, 3, 3], dtype=np.int64), np.array([4, 5, 6], dtype=np.int32)
    tp, ti = np.array([0, 1, 1, 3, 3], dtype=np.int64), np.array([1007, 1014, 1021], dtype=np.int64)
    ids, sc, cnt = np.full((K, top_n), -77, dtype=np.int64), np.full((K, top_n), -7.5), np.full(K, -9, dtype=np.int32)
    pos, psc, ln = np.full(3, -77, dtype=np.int64), np.full(3, -7.5), np.full(K, -9, dtype=np.int64)
    like = 1 << gg.EDGE_LIKE
    P = lambda a, t: None if a is None else a.ctypes.data_as(t)

    def ranked(handle=h, s=seeds, k=K, d=D, top=top_n, cand=gg.NODE_USER, mask=like, pc=4, pi=pool, p=dp, i=di, o=(ids, sc, cnt)):
        st = lib.rwr_recommend_filtered_batch(handle, P(s, PI32), k, C.c_float(d), 3, top, cand, mask, 0, pc, P(pi, PI32), P(p, PI64),
                                              P(i, PI32), P(o[0], PI64), P(o[1], PD), P(o[2], PI32))
        return st, lib.rwr_last_error()

    def positions(handle=h, s=seeds, k=K, d=D, cand=gg.NODE_USER, mask=like, pc=4, pi=pool, p=dp, i=di, t=tp, ids_=ti, o=pos):
        st = lib.rwr_recommend_filtered_positions_batch(handle, P(s, PI32), k, C.c_float(d), 3, cand, mask, 0, pc, P(pi, PI32),
                                                        P(p, PI64), P(i, PI32), P(t, PI64), P(ids_, PI64), P(o, PI64), P(psc, PD),
                                                        P(ln, PI64))
        return st, lib.rwr_last_error()

    def untouched():
        return ((ids == -77).all() and (sc == -7.5).all() and (cnt == -9).all() and (pos == -77).all() and (psc == -7.5).all()
                and (ln == -9).all())

    INV, RNG, UNS = _lib.RWR_E_INVALID, _lib.RWR_E_RANGE, _lib.RWR_E_UNSUPPORTED
    bad_seeds = seeds.copy(); bad_seeds[2] = n
    bad_pool = pool.copy(); bad_pool[1] = n
    bad_di = di.copy(); bad_di[2] = -1
    # one fault per step of the documented order, first -> last; each call carries its own fault and EVERY later one
    steps = [(dict(handle=None), INV, b"NULL graph"), (dict(k=-1), INV, b"negative K"), (dict(s=None), INV, b"NULL"),
             (dict(cand=-2), INV, b"[-1, 255]"), (dict(mask=1 << 8), INV, b"excl_edge_mask"),
             (dict(s=bad_seeds), RNG, b"batch position 2"), (dict(pi=None), INV, b"NULL pool_idx"),
             (dict(pi=bad_pool), RNG, b"pool position 1"), (dict(p=np.array([1, 1, 1, 3, 3], dtype=np.int64)), INV, b"deny_ptr[0]"),
             (dict(p=np.array([0, 2, 1, 3, 3], dtype=np.int64)), INV, b"deny_ptr decreases at batch position 1"),
             (dict(i=None), INV, b"NULL deny_idx"), (dict(i=bad_di), RNG, b"batch position 2")]
    tail_ranked = [(dict(top=SEL_MAX_K + 1), UNS, b"1024"), (dict(d=1.5), UNS, b"[0, 1]")]
    tail_positions = [(dict(t=None), INV, b"NULL test_ptr"), (dict(o=None), INV, b"NULL pos_out"),
                      (dict(t=np.array([0, 2, 1, 3, 3], dtype=np.int64)), INV, b"test_ptr decreases"),
                      (dict(ids_=None), INV, b"NULL test_ids"), (dict(d=1.5), UNS, b"[0, 1]")]
    for call, name, order in ((ranked, b"rwr_recommend_filtered_batch", steps + tail_ranked),
                              (positions, b"rwr_recommend_filtered_positions_batch", steps + tail_positions)):
        for at, (kw, status, text) in enumerate(order):
            later = {}
            for kw2, _, _ in reversed(order[at + 1:]):
                later.update({k: v for k, v in kw2.items() if k not in kw})
            # (a later fault on the same argument cannot ride along: the argument holds this step's fault)
            st, msg = call(**dict(later, **kw))
            assert st == status and text in msg and name in msg, (name, at, kw.keys(), st, msg)
            assert untouched(), (name, at)
    # the ranked entry's own pointers and top_n's lower bound
    for kw in (dict(o=(None, sc, cnt)), dict(o=(ids, None, cnt)), dict(o=(ids, sc, None)), dict(top=0), dict(cand=256)):
        st, msg = ranked(**kw)
        assert st == INV and untouched(), kw
    # what is no fault: K == 0 (whatever else is there), an empty pool without an array, no pool, empty deny lists without an array
    assert ranked(k=0, s=None, pi=None, p=None, i=None, o=(None, None, None))[0] == _lib.RWR_OK and untouched()
    assert positions(k=0, s=None, t=None, o=None)[0] == _lib.RWR_OK and untouched()
    assert ranked(pc=0, pi=None)[0] == _lib.RWR_OK and (cnt == 0).all() and (ids == 0).all()
    assert ranked(pc=-1, pi=None, p=np.zeros(K + 1, dtype=np.int64), i=None, cand=-1, mask=0xFF)[0] == _lib.RWR_OK and (cnt == top_n).all()
    assert positions(pc=-7, pi=None, p=None, i=None, cand=255)[0] == _lib.RWR_OK and (pos == -1).all() and (ln == 0).all()
    G.close()
    neg = dict(g, w=g["w"].copy())
    neg["w"][3] = -1.0
    Gn = built(amd, neg)
    ids[:], sc[:], cnt[:], pos[:], psc[:], ln[:] = -77, -7.5, -9, -77, -7.5, -9
    for call in (ranked, positions):
        st, msg = call(handle=Gn._handle())
        assert st == UNS and b"non-negative" in msg and untouched()
    Gn.close()
