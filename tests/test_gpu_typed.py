"""Recommendation among the nodes of any node type (rwr_recommend_typed_batch / Recommender.RecommendationTypedBatch, DESIGN
§3.16).  The expectation is never the code under test: the rank row comes from oracle/rwr_oracle.py's Model (the literal
restatement, its zero restart addends skipped -- asserted bit-identical in tests/test_oracle.py), the candidates are filtered
and sorted here with sorted(key=(-score, -id)).  Ids must be equal, scores bitwise equal.

Graphs: a few hundred nodes of all four node types (and of types beyond them) with LIKE, FRIENDSHIP, FOLLOW, MENTION (weights
!= 1: the weighted matrix path), AUTHORSHIP and UNDEFINED links, and a unit-weight one (the value-free path).  The boundary
graphs are as small as their boundary allows: 256 / 257 nodes (the compaction's block), 1 025 users (top-1024), a hub with
4 096 / 4 097 raw links (one / two exclusion segments)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from oracle import rwr_oracle as po
from tests import graphgen as gg
from tests.test_golden import load as load_golden

pytestmark = pytest.mark.gpu

D = 0.15
CAND_BLOCK = 256           # cand_plan.h
EXCLUDE_SEG_MAX = 4096     # exclude_plan.h
SEL_MAX_K = 1024           # rank_keys.h
PI64, PI32, PD = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "*.json")))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def amd():
    import recommendersystems_amd as m
    from recommendersystems_amd import _lib
    assert _lib.load().rwr_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    return m


# ---- graphs ------------------------------------------------------------------------------------------------------------------

def _lists(g):
    rp = g["rowptr"]
    return [[(int(g["dst"][e]), int(g["etype"][e]), float(g["w"][e])) for e in range(int(rp[i]), int(rp[i + 1]))]
            for i in range(len(g["node_id"]))]


def _flat(node_id, node_type, lists):
    rowptr = np.zeros(len(lists) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(L) for L in lists])
    flat = [l for L in lists for l in L]
    return dict(node_id=np.asarray(node_id, dtype=np.int64), node_type=np.asarray(node_type, dtype=np.uint8), rowptr=rowptr,
                dst=np.array([l[0] for l in flat], dtype=np.int32), etype=np.array([l[1] for l in flat], dtype=np.uint8),
                w=np.array([l[2] for l in flat], dtype=np.float64))


def _mixed(seed, uniform):
    """users, items and ETC nodes; some users retagged UNDEFINED; half of the FRIENDSHIP links relabelled FOLLOW; behind them a
    user without any raw link and a user whose only links are UNDEFINED (both dangling).  Returns (graph, the two rows)."""
    g = gg.random_graph(seed, n_users=120, n_items=200, n_likes=1500, n_etc=6, n_friend=160, n_mention=0 if uniform else 90,
                        n_author=40, uniform=uniform)
    rng = np.random.default_rng(seed + 1)
    types = g["node_type"].copy()
    types[rng.choice(120, 5, replace=False)] = gg.NODE_UNDEFINED
    et = g["etype"].copy()
    fr = np.flatnonzero(et == gg.EDGE_FRIENDSHIP)
    et[fr[rng.random(fr.size) < 0.5]] = gg.EDGE_FOLLOW
    g = dict(g, node_type=types, etype=et)
    lists = _lists(g)
    n = len(lists)
    lists += [[], [(3, gg.EDGE_UNDEFINED, 1.0), (130, gg.EDGE_UNDEFINED, 1.0)]]
    lists[7].append((n, gg.EDGE_FOLLOW, 1.0))                      # somebody follows the linkless user
    ids = np.concatenate([g["node_id"], [17, 24]])
    return _flat(ids, np.concatenate([types, [gg.NODE_USER, gg.NODE_USER]]), lists), (n, n + 1)


@pytest.fixture(scope="module")
def mixed():
    return _mixed(11, uniform=False)


@pytest.fixture(scope="module")
def unit():
    return _mixed(12, uniform=True)


_oracle_graphs, _oracle_rows = {}, {}


def oracle_row(g, seed, T):
    """Model(graph, (double)(float)d, seed).run(T).rank of the literal restatement, cached per (graph, seed, T)"""
    key = id(g)
    if key not in _oracle_graphs:
        G = po.Graph(*po.from_flat(**g))
        G.buildGraph()
        _oracle_graphs[key] = (G, g)                               # (g kept alive: its id stays its own)
    if (key, seed, T) not in _oracle_rows:
        m = po.Model(_oracle_graphs[key][0], po.widen_float(D), int(seed), dense_restart=False)
        m.run(int(T))
        _oracle_rows[(key, seed, T)] = np.array(m.rank, dtype=np.float64)
    return _oracle_rows[(key, seed, T)]


def expected_list(g, row, seed, cand_type, edge_types, exclude_self):
    """the whole list the header defines for one seed: [(id, score), ...]"""
    lo, hi = int(g["rowptr"][seed]), int(g["rowptr"][seed + 1])
    out = {int(g["dst"][p]) for p in range(lo, hi) if int(g["etype"][p]) in edge_types}
    if exclude_self:
        out.add(int(seed))
    cand = [(int(g["node_id"][i]), float(row[i])) for i in range(len(row)) if g["node_type"][i] == cand_type and i not in out]
    return sorted(cand, key=lambda c: (-c[1], -c[0]))


def expected(g, seeds, T, top_n, cand_type, edge_types, exclude_self):
    K = len(seeds)
    ids, sc, cnt = np.zeros((K, top_n), dtype=np.int64), np.zeros((K, top_n)), np.zeros(K, dtype=np.int32)
    for k, s in enumerate(seeds):
        L = expected_list(g, oracle_row(g, int(s), T), int(s), cand_type, set(edge_types), exclude_self)[:top_n]
        cnt[k] = len(L)
        ids[k, :len(L)] = [c[0] for c in L]
        sc[k, :len(L)] = [c[1] for c in L]
    return ids, sc, cnt


def check(got, want, what):
    ids, sc, cnt = got
    wi, ws, wc = want
    print(what, "counts", cnt.tolist()[:8], "want", wc.tolist()[:8])
    assert (cnt == wc).all(), (what, "counts", cnt.tolist(), wc.tolist())
    bad = np.flatnonzero((ids != wi).any(axis=1))
    assert bad.size == 0, (what, "ids differ in rows", bad.tolist(), ids[bad[0]].tolist()[:10], wi[bad[0]].tolist()[:10])
    bad = np.flatnonzero((bits(sc) != bits(ws)).any(axis=1))
    assert bad.size == 0, (what, "scores not bitwise equal in rows", bad.tolist())


def built(amd, g, **opts):
    G = amd.Graph.from_flat(**g, **opts)
    G.buildGraph()
    return G


def typed(amd, G, seeds, T, top_n, cand_type, edge_types=(), exclude_self=False):
    return amd.Recommender(G).RecommendationTypedBatch(np.asarray(seeds, dtype=np.int32), D, T, top_n, cand_type, edge_types,
                                                       exclude_self)


# ---- 1. identity with rwr_recommend_batch ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[:-5])
def test_item_like_is_recommend_batch(amd, path):
    _, g = load_golden(path)
    n = len(g["node_id"])
    n_items = int((g["node_type"] == gg.NODE_ITEM).sum())
    top_n = max(1, min(7, n_items))
    for tile_seeds in (1, 8, 64):
        G = built(amd, g, tile_seeds=tile_seeds)
        rec = amd.Recommender(G)
        for K in (1, 3, 65):
            seeds = ((np.arange(K, dtype=np.int64) * 7 + 1) % n).astype(np.int32)
            for T in (0, 1, 2, 10):
                want = rec.RecommendationBatch(seeds, D, T, top_n)
                got = rec.RecommendationTypedBatch(seeds, D, T, top_n, gg.NODE_ITEM, (gg.EDGE_LIKE,), False)
                check(got, want, (os.path.basename(path), tile_seeds, K, T))
        G.close()


# ---- 2. who to follow ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["weighted", "value_free"])
@pytest.mark.parametrize("opts", [dict(), dict(tile_seeds=1, tile_group=1), dict(tile_seeds=8, tile_group=1)],
                         ids=["auto", "G1_groups", "G8_groups"])
def test_who_to_follow(amd, mixed, unit, which, opts):
    g, (linkless, undef_only) = mixed if which == "weighted" else unit
    G = built(amd, g, **opts)
    assert G.stats()["uniform_path"] == (0 if which == "weighted" else 1)
    item_seed = 120 + 3
    assert g["node_type"][item_seed] == gg.NODE_ITEM and g["rowptr"][linkless] == g["rowptr"][linkless + 1]
    # two users, one of them twice, an ITEM seed (no candidate itself), the user without raw links, the dangling user with
    # UNDEFINED links only, and enough further users for a second tile at G = 8
    seeds = [0, 5, 5, item_seed, linkless, undef_only, 7, 9, 21, 33, 2]
    mask = (gg.EDGE_FRIENDSHIP, gg.EDGE_FOLLOW)
    for T in (1, 10):
        got = typed(amd, G, seeds, T, 20, gg.NODE_USER, mask, True)
        check(got, expected(g, seeds, T, 20, gg.NODE_USER, mask, True), (which, opts, T))
    # the linkless seed holds all of its rank (n) and would lead its own list: with exclude_self its id is gone from it
    ids, sc, cnt = typed(amd, G, [linkless], 10, 20, gg.NODE_USER, mask, True)
    assert int(g["node_id"][linkless]) not in ids[0, :cnt[0]].tolist()
    ids, sc, cnt = typed(amd, G, [linkless], 10, 20, gg.NODE_USER, mask, False)
    assert ids[0, 0] == g["node_id"][linkless] and sc[0, 0] == float(len(g["node_id"]))
    G.close()


def test_one_seed_mirror(amd, mixed):
    g, _ = mixed
    G = built(amd, g)
    got = amd.Recommender(G).RecommendationTyped(5, D, 3, 15, amd.NodeType.USER, (amd.EdgeType.FRIENDSHIP, amd.EdgeType.FOLLOW), True)
    want = expected_list(g, oracle_row(g, 5, 3), 5, gg.NODE_USER, {gg.EDGE_FRIENDSHIP, gg.EDGE_FOLLOW}, True)[:15]
    assert [r[0] for r in got] == [w[0] for w in want]
    assert (bits([r[1] for r in got]) == bits([w[1] for w in want])).all()
    G.close()


@pytest.mark.parametrize("which", ["weighted", "value_free"])
def test_own_rows_with_a_padding_slot_and_a_repeated_seed(amd, mixed, unit, which):
    """exclude_self with an empty mask -- no link is looked at, the seeds' own rows are the whole exclusion -- at K = 3 on
    tiles of two slots (two tiles, one padding slot), two batch positions holding the same seed.  The rows are
    rwr_model_run_batch's, ranked here."""
    g, _ = mixed if which == "weighted" else unit
    G = built(amd, g, tile_seeds=2, tile_group=1)
    seeds, T, top_n = [5, 9, 5], 6, int((g["node_type"] == gg.NODE_USER).sum()) + 3
    rows, _ = amd.Model.RunBatch(G, po.widen_float(D), seeds, T)
    ids, sc, cnt = np.zeros((3, top_n), dtype=np.int64), np.zeros((3, top_n)), np.zeros(3, dtype=np.int32)
    for k, s in enumerate(seeds):
        L = expected_list(g, rows[k], s, gg.NODE_USER, set(), True)
        assert g["node_type"][s] == gg.NODE_USER and len(L) == top_n - 4   # every user but the seed
        cnt[k], ids[k, :len(L)], sc[k, :len(L)] = len(L), [c[0] for c in L], [c[1] for c in L]
    got = typed(amd, G, seeds, T, top_n, gg.NODE_USER, (), True)
    check(got, (ids, sc, cnt), ("own rows", which))
    for k, s in enumerate(seeds):
        mine = got[0][k, :got[2][k]].tolist()
        assert int(g["node_id"][s]) not in mine, (k, "the seed is in its own list")
        other = 9 if s == 5 else 5                                  # ... and another slot's seed is not marked in this one
        assert int(g["node_id"][other]) in mine, (k, "another position's seed is missing")
    G.close()


# ---- 3. boundaries of the new kernels -----------------------------------------------------------------------------------------

def test_candidate_counts_and_top_n(amd, mixed):
    """node types with 0, 1, 64 and 65 rows (more types than the handle caches: every call after the fourth evicts), and
    top_n around the number of candidates"""
    g0, _ = mixed
    rng = np.random.default_rng(5)
    types = g0["node_type"].copy()
    users = rng.permutation(np.flatnonzero(types == gg.NODE_USER))
    items = rng.permutation(np.flatnonzero(types == gg.NODE_ITEM))
    types[users[:1]] = 8
    types[users[1:65]] = 9
    types[items[:65]] = 10
    g = dict(g0, node_type=types)
    G = built(amd, g)
    seeds = [int(users[0]), int(users[3]), int(items[100]), 0, int(items[7])]
    for round_ in range(2):                                        # (the second round finds some lists cached, some evicted)
        for cand, m in ((7, 0), (8, 1), (9, 64), (10, 65), (gg.NODE_ITEM, 135), (gg.NODE_ETC, 6)):
            assert int((types == cand).sum()) == m
            got = typed(amd, G, seeds, 4, 5, cand, (), False)
            check(got, expected(g, seeds, 4, 5, cand, (), False), ("count", cand, round_))
    for top_n in (1, 64, 65, 66):
        for self_ in (False, True):
            got = typed(amd, G, seeds, 4, top_n, 10, (gg.EDGE_LIKE,), self_)
            check(got, expected(g, seeds, 4, top_n, 10, (gg.EDGE_LIKE,), self_), ("top_n", top_n, self_))
    G.close()


@pytest.mark.parametrize("n", [CAND_BLOCK, CAND_BLOCK + 1])
def test_last_row_is_the_only_match(amd, n):
    g = gg.random_graph(21, n_users=100, n_items=n - 101, n_likes=900, n_friend=60)
    lists = _lists(g)
    lists.append([(2, gg.EDGE_MENTION, 2.5)])
    lists[0].append((n - 1, gg.EDGE_FOLLOW, 1.0))
    lists[4].append((n - 1, gg.EDGE_FOLLOW, 1.0))
    g = _flat(np.concatenate([g["node_id"], [5]]), np.concatenate([g["node_type"], [200]]), lists)
    assert len(g["node_id"]) == n
    G = built(amd, g)
    seeds = [0, 4, 9, n - 1]
    for self_ in (False, True):
        got = typed(amd, G, seeds, 3, 4, 200, (), self_)
        want = expected(g, seeds, 3, 4, 200, (), self_)
        assert want[2].tolist() == ([1, 1, 1, 0] if self_ else [1, 1, 1, 1])
        check(got, want, ("last row", n, self_))
    got = typed(amd, G, seeds, 3, 4, 200, (gg.EDGE_FOLLOW,), False)       # seeds 0 and 4 follow it: no candidate left
    check(got, expected(g, seeds, 3, 4, 200, (gg.EDGE_FOLLOW,), False), ("last row followed", n))
    G.close()


@pytest.mark.parametrize("links", [EXCLUDE_SEG_MAX, EXCLUDE_SEG_MAX + 1])
def test_hub_seed_segments(amd, links):
    """a seed whose raw list is exactly one full exclusion segment, and one link more: the last link, alone in the second
    segment, is the only one that names its target"""
    g = gg.random_graph(31, n_users=300, n_items=80, n_likes=700, n_friend=100)
    lists = _lists(g)
    hub, lonely = 0, 299
    # every raw link of the hub is a masked one (raw lists may name a target more than once)
    lists[hub] = [(1 + k % 297, gg.EDGE_FOLLOW if k % 3 else gg.EDGE_FRIENDSHIP, 1.0) for k in range(EXCLUDE_SEG_MAX)]
    if links > EXCLUDE_SEG_MAX:
        lists[hub].append((lonely, gg.EDGE_FOLLOW, 1.0))
    lists[lonely].append((5, gg.EDGE_FRIENDSHIP, 1.0))
    g = _flat(g["node_id"], g["node_type"], lists)
    assert g["rowptr"][hub + 1] - g["rowptr"][hub] == links
    G = built(amd, g)
    seeds = [hub, 17, hub]
    mask = (gg.EDGE_FRIENDSHIP, gg.EDGE_FOLLOW)
    got = typed(amd, G, seeds, 2, 300, gg.NODE_USER, mask, True)
    want = expected(g, seeds, 2, 300, gg.NODE_USER, mask, True)
    assert (int(g["node_id"][lonely]) in want[0][0, :want[2][0]].tolist()) == (links == EXCLUDE_SEG_MAX)
    check(got, want, ("hub", links))
    G.close()


def test_masks(amd, mixed):
    g, _ = mixed
    G = built(amd, g)
    seeds = [0, 1, 5, 123, 40, 326]
    for cand, mask in ((gg.NODE_USER, ()), (gg.NODE_ITEM, ()),
                       (gg.NODE_ITEM, (gg.EDGE_UNDEFINED, gg.EDGE_LIKE, gg.EDGE_AUTHORSHIP)),
                       (gg.NODE_USER, (gg.EDGE_UNDEFINED, gg.EDGE_FRIENDSHIP, gg.EDGE_MENTION)),
                       (gg.NODE_UNDEFINED, (gg.EDGE_FOLLOW, gg.EDGE_ETC, gg.EDGE_PURCHASE)),
                       (gg.NODE_ETC, (gg.EDGE_MENTION,))):
        got = typed(amd, G, seeds, 5, 30, cand, mask, False)
        check(got, expected(g, seeds, 5, 30, cand, mask, False), ("mask", cand, mask))
    # the UNDEFINED bit alone, from two seeds with UNDEFINED raw links into items: it drops what the empty mask keeps
    src = np.repeat(np.arange(len(g["node_id"])), np.diff(g["rowptr"]))
    und = src[(g["etype"] == gg.EDGE_UNDEFINED) & (g["node_type"][g["dst"]] == gg.NODE_ITEM)]
    seeds = [int(s) for s in np.unique(und)[:2]]
    want = expected(g, seeds, 5, 250, gg.NODE_ITEM, (gg.EDGE_UNDEFINED,), False)
    assert len(seeds) == 2 and (want[2] < expected(g, seeds, 5, 250, gg.NODE_ITEM, (), False)[2]).all()
    check(typed(amd, G, seeds, 5, 250, gg.NODE_ITEM, (gg.EDGE_UNDEFINED,), False), want, "UNDEFINED's bit alone")
    G.close()


def test_link_types_beyond_the_mask_are_never_masked(amd, mixed):
    """link types are unchecked at create: raw links of type 33, 200 and 255 (33 is LIKE's bit modulo 32, 200 UNDEFINED's modulo
    8) are explicit links of the walk and no bit of any mask stands for them"""
    g0, _ = mixed
    et = g0["etype"].copy()
    for seed, ty in ((0, 33), (1, 200), (5, 255)):
        lo, hi = int(g0["rowptr"][seed]), int(g0["rowptr"][seed + 1])
        likes = lo + np.flatnonzero(et[lo:hi] == gg.EDGE_LIKE)
        assert likes.size >= 4
        et[likes[::2]] = ty
    g = dict(g0, etype=et)
    G = built(amd, g)
    seeds = [0, 1, 5, 9]
    every = tuple(range(8))
    for mask in ((gg.EDGE_LIKE,), (gg.EDGE_UNDEFINED, gg.EDGE_LIKE), every):
        want = expected(g, seeds, 4, 250, gg.NODE_ITEM, mask, False)
        assert (want[2][:3] > expected(g0, seeds, 4, 250, gg.NODE_ITEM, mask, False)[2][:3]).all()   # the relabelled targets stay
        check(typed(amd, G, seeds, 4, 250, gg.NODE_ITEM, mask, False), want, ("types beyond the mask", mask))
    G.close()


def test_no_step_all_ties(amd, mixed):
    """T = 0: the seed holds n, every other row +0.0 -- the ids alone order the list"""
    g, _ = mixed
    G = built(amd, g)
    seeds = [0, 5, 123]
    for self_ in (False, True):
        got = typed(amd, G, seeds, 0, 50, gg.NODE_USER, (), self_)
        want = expected(g, seeds, 0, 50, gg.NODE_USER, (), self_)
        assert (want[1][:, 1:] == 0).all() and want[1][0, 0] == (0.0 if self_ else float(len(g["node_id"])))
        check(got, want, ("T=0", self_))
    G.close()


def test_top_1024_of_1025(amd):
    g = gg.random_graph(41, n_users=SEL_MAX_K + 1, n_items=60, n_likes=2500, n_friend=700)
    G = built(amd, g)
    seeds = [3, 1030]
    got = typed(amd, G, seeds, 3, SEL_MAX_K, gg.NODE_USER, (), False)
    want = expected(g, seeds, 3, SEL_MAX_K, gg.NODE_USER, (), False)
    assert want[2].tolist() == [SEL_MAX_K, SEL_MAX_K]
    check(got, want, "top-1024 of 1025")
    got = typed(amd, G, seeds, 3, SEL_MAX_K, gg.NODE_USER, (gg.EDGE_FRIENDSHIP,), True)
    check(got, expected(g, seeds, 3, SEL_MAX_K, gg.NODE_USER, (gg.EDGE_FRIENDSHIP,), True), "top-1024, exclusions")
    G.close()


# ---- 4. the cached candidate list across appends ------------------------------------------------------------------------------

def test_cache_follows_appended_nodes(amd, mixed):
    g, _ = mixed
    n = len(g["node_id"])
    G = built(amd, g)
    seeds = [0, 5, 9, 123]
    mask = (gg.EDGE_FRIENDSHIP, gg.EDGE_FOLLOW)
    before = typed(amd, G, seeds, 4, 25, gg.NODE_USER, mask, True)
    check(before, expected(g, seeds, 4, 25, gg.NODE_USER, mask, True), "before the append")
    # three new users (their ids above every old one: they lead the ties), links to and from them
    G.appendNodes([(90001, gg.NODE_USER), (90002, gg.NODE_ITEM), (90003, gg.NODE_USER), (90004, gg.NODE_USER)],
                  src=[0, 5, n, n + 2, 9, n + 3], dst=[n, n + 2, 5, 0, n + 3, 9],
                  etype=[gg.EDGE_FOLLOW, gg.EDGE_MENTION, gg.EDGE_FRIENDSHIP, gg.EDGE_FOLLOW, gg.EDGE_MENTION, gg.EDGE_FOLLOW],
                  w=[1.0, 2.0, 1.0, 1.0, 0.5, 1.0])
    seeds2 = seeds + [n, n + 3]
    grown = dict(zip(("node_id", "node_type", "rowptr", "dst", "etype", "w"), G._flat))
    fresh = built(amd, grown)
    got = typed(amd, G, seeds2, 4, 25, gg.NODE_USER, mask, True)
    check(got, typed(amd, fresh, seeds2, 4, 25, gg.NODE_USER, mask, True), "after append_nodes: a fresh graph")
    check(got, expected(grown, seeds2, 4, 25, gg.NODE_USER, mask, True), "after append_nodes: the oracle")
    new_ids = {90001, 90003, 90004}
    assert any(new_ids & set(got[0][k, :got[2][k]].tolist()) for k in range(len(seeds2))), "no new user in any list"
    fresh.close()
    # links only: n unchanged, the list is reused
    G.appendLinks([0, 9], [n + 3, n], [gg.EDGE_FRIENDSHIP, gg.EDGE_MENTION], [1.0, 3.0])
    grown = dict(zip(("node_id", "node_type", "rowptr", "dst", "etype", "w"), G._flat))
    fresh = built(amd, grown)
    got = typed(amd, G, seeds2, 4, 25, gg.NODE_USER, mask, True)
    check(got, typed(amd, fresh, seeds2, 4, 25, gg.NODE_USER, mask, True), "after append_links: a fresh graph")
    check(got, expected(grown, seeds2, 4, 25, gg.NODE_USER, mask, True), "after append_links: the oracle")
    fresh.close()
    G.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(amd, mixed):
    from recommendersystems_amd import _lib
    lib = _lib.load()
    g, _ = mixed
    n = len(g["node_id"])
    G = built(amd, g)
    h = G._handle()
    K, top_n = 4, 6
    seeds = np.array([0, 5, 9, 123], dtype=np.int32)
    ids = np.full((K, top_n), -77, dtype=np.int64)
    sc = np.full((K, top_n), -7.5)
    cnt = np.full(K, -9, dtype=np.int32)
    ps, pi, pc, pn = seeds.ctypes.data_as(PI32), ids.ctypes.data_as(PI64), sc.ctypes.data_as(PD), cnt.ctypes.data_as(PI32)
    like = 1 << gg.EDGE_LIKE

    def call(handle=h, s=ps, k=K, d=D, T=3, top=top_n, cand=gg.NODE_USER, mask=like, self_=0, i=pi, c=pc, m=pn):
        return lib.rwr_recommend_typed_batch(handle, s, k, C.c_float(d), T, top, cand, mask, self_, i, c, m), lib.rwr_last_error()

    def untouched():
        return (ids == -77).all() and (sc == -7.5).all() and (cnt == -9).all()

    st, msg = call(handle=None, k=-1, top=0, cand=999)                 # a NULL graph is refused first
    assert st == _lib.RWR_E_INVALID and b"NULL graph" in msg
    assert call(k=0)[0] == _lib.RWR_OK and untouched()                 # a no-op
    assert call(k=0, s=None, i=None, c=None, m=None)[0] == _lib.RWR_OK
    for kw in (dict(k=-1), dict(s=None), dict(i=None), dict(c=None), dict(m=None), dict(cand=-1), dict(cand=256),
               dict(mask=1 << 8), dict(mask=0x80000000), dict(top=0)):
        st, msg = call(**kw)
        assert st == _lib.RWR_E_INVALID and b"rwr_recommend_typed_batch" in msg, (kw, st, msg)
        assert untouched(), kw
    for bad in (-1, n):
        seeds[2] = bad
        st, msg = call()
        assert st == _lib.RWR_E_RANGE and b"batch position 2" in msg, (bad, st, msg)
        assert untouched()
    seeds[2] = 9
    st, msg = call(top=SEL_MAX_K + 1)
    assert st == _lib.RWR_E_UNSUPPORTED and b"1024" in msg and untouched()
    for d in (-0.25, 1.5, float("nan")):
        st, msg = call(d=d)
        assert st == _lib.RWR_E_UNSUPPORTED and b"[0, 1]" in msg and untouched(), d
    assert call(mask=0xFF, cand=255)[0] == _lib.RWR_OK and not untouched()   # every legal bit, the largest type: served
    G.close()
    neg = dict(g, w=g["w"].copy())
    neg["w"][3] = -1.0
    Gn = built(amd, neg)
    ids[:], sc[:], cnt[:] = -77, -7.5, -9
    st, msg = call(handle=Gn._handle())
    assert st == _lib.RWR_E_UNSUPPORTED and b"non-negative" in msg and untouched()
    Gn.close()
