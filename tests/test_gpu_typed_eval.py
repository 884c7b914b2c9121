"""Hits / average precision of typed lists on the device (rwr_recommend_typed_eval_batch /
Recommender.RecommendationTypedEvalBatch).  The expectation is never the code under test: the rank row comes
from oracle/rwr_oracle.py's Model as tests/test_gpu_typed.py derives it, the WHOLE list is filtered and sorted there with
sorted(key=(-score, -id)), and the loop of Experiment.cs:121-128 runs here in Python with the same division and summation order.
n_hits and list_len must be equal, sum_precision bitwise equal.

Graphs: tests/test_gpu_typed.py's mixed graphs (about 330 nodes, weighted and unit-weight) at tile_seeds = 4, tile_group = 2 --
K = 9 is three tiles in two groups, the last with padding slots -- and boundary graphs as small as their boundary allows:
4 100 users (4 096 / 4 097 hits in a slot: the one-workgroup sort against the radix sort, and past the LDS budget of the
counting kernel), 256 / 257 nodes of a type (the compaction's block), a hub seed with 4 096 / 4 097 masked raw links."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import graphgen as gg
from tests.test_golden import load as load_golden
from tests.test_gpu_typed import (CAND_BLOCK, D, EXCLUDE_SEG_MAX, GOLDEN, PD, PI32, PI64, _flat, _lists, _mixed, bits, built,
                                  expected_list, oracle_row, typed)

pytestmark = pytest.mark.gpu

EVAL_SORT_SLOTS = 4096     # eval_plan.h
OPTS = dict(tile_seeds=4, tile_group=2)
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


def harness(L, test, top_n):
    """Experiment.cs:121-128 over the list L = [(id, score), ...], cut to top_n when top_n > 0"""
    if top_n > 0:
        L = L[:top_n]
    ts = set(int(t) for t in test)
    n_hits, sum_precision = 0, 0.0
    for i, (node_id, _) in enumerate(L):
        if node_id in ts:
            n_hits += 1
            sum_precision += float(n_hits) / (i + 1)
    return n_hits, sum_precision, len(L)


def expected_eval(g, seeds, T, tests, cand_type, edge_types, exclude_self, top_n):
    out = [harness(expected_list(g, oracle_row(g, int(s), T), int(s), cand_type, set(edge_types), exclude_self), t, top_n)
           for s, t in zip(seeds, tests)]
    return (np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out], dtype=np.float64),
            np.array([o[2] for o in out], dtype=np.int64))


def typed_eval(amd, G, seeds, T, tests, cand_type, edge_types=(), exclude_self=False, top_n=0):
    return amd.Recommender(G).RecommendationTypedEvalBatch(np.asarray(seeds, dtype=np.int32), D, T, tests, cand_type, edge_types,
                                                           exclude_self, top_n)


def check(got, want, what):
    h, sp, ln = got
    wh, ws, wl = want
    print(what, "hits", h.tolist()[:9], "want", wh.tolist()[:9], "len", ln.tolist()[:9], "sum", sp.tolist()[:3], ws.tolist()[:3])
    assert (ln == wl).all(), (what, "list_len", ln.tolist(), wl.tolist())
    assert (h == wh).all(), (what, "n_hits", h.tolist(), wh.tolist())
    assert (bits(sp) == bits(ws)).all(), (what, "sum_precision not bitwise equal", sp.tolist(), ws.tolist())


def make_sets(g, seeds, rng, cand_type=gg.NODE_USER):
    """one test set per seed: ids of the type with duplicates, absent ids, the ids 17 and 24, an empty set, every id"""
    ids = g["node_id"][g["node_type"] == cand_type]
    sets = []
    for k in range(len(seeds)):
        pick = rng.choice(ids, min(len(ids), 12), replace=False).tolist() if len(ids) else []
        if k % 5 == 0:
            sets.append(pick + pick[:4] + [17, 24, -3, 10 ** 12])          # duplicates, absent ids
        elif k % 5 == 1:
            sets.append([])
        elif k % 5 == 2:
            sets.append(ids.tolist() + [17])                             # every candidate hits
        elif k % 5 == 3:
            sets.append([5, 6, 999999])                                  # ids nobody carries
        else:
            sets.append(pick[:3] + [24, 24])
    return sets



# ---- 1. who to follow, evaluated -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["weighted", "value_free"])
def test_who_to_follow_eval(amd, mixed, unit, which):
    g, (linkless, undef_only) = mixed if which == "weighted" else unit
    G = built(amd, g, **OPTS)
    item_seed = 120 + 3
    assert g["node_type"][item_seed] == gg.NODE_ITEM
    # users, one of them twice, an ITEM seed, the user without raw links, the dangling user with UNDEFINED links only
    all_seeds = [0, 5, 5, item_seed, linkless, undef_only, 7, 9, 21]
    rng = np.random.default_rng(3)
    for K in (1, 3, 9):
        seeds = all_seeds[:K] if K > 1 else [5]
        tests = make_sets(g, seeds, rng)
        for T in (0, 1, 10):
            lens = {}
            for self_ in (False, True):
                want = expected_eval(g, seeds, T, tests, gg.NODE_USER, FOLLOWS, self_, 0)
                check(typed_eval(amd, G, seeds, T, tests, gg.NODE_USER, FOLLOWS, self_, 0), want, (which, K, T, self_, "whole"))
                lens[self_] = want[2]
            # exclude_self shortens a list by exactly one when the seed is of the candidate type, by nothing otherwise
            for k, s in enumerate(seeds):
                assert lens[False][k] - lens[True][k] == (1 if g["node_type"][s] == gg.NODE_USER else 0), (K, T, k)
            L = int(lens[True].max())                                # the longest list: its length, and one more
            for top_n in (1, 7, L, L + 1, 1025, -4):
                want = expected_eval(g, seeds, T, tests, gg.NODE_USER, FOLLOWS, True, top_n)
                check(typed_eval(amd, G, seeds, T, tests, gg.NODE_USER, FOLLOWS, True, top_n), want, (which, K, T, "top", top_n))
    G.close()


def test_similar_items_and_an_empty_type(amd, mixed):
    g, _ = mixed
    G = built(amd, g, **OPTS)
    rng = np.random.default_rng(4)
    seeds = [123, 130, 123, 0, 200]                                    # item seeds (one twice) and a user
    tests = make_sets(g, seeds, rng, gg.NODE_ITEM)
    for T in (1, 10):
        for self_ in (False, True):
            for top_n in (0, 7):
                want = expected_eval(g, seeds, T, tests, gg.NODE_ITEM, (), self_, top_n)
                check(typed_eval(amd, G, seeds, T, tests, gg.NODE_ITEM, (), self_, top_n), want, ("items", T, self_, top_n))
    # a type no node carries: zeros, +0.0 and RWR_OK
    assert not (g["node_type"] == 77).any()
    h, sp, ln = typed_eval(amd, G, seeds, 3, tests, 77, FOLLOWS, True, 0)
    assert not h.any() and not ln.any() and not bits(sp).any()
    G.close()


def test_two_nodes_share_an_id(amd, mixed):
    """node ids need not be unique: every candidate that carries a test id is a hit, whatever its score"""
    g0, _ = mixed
    ids = g0["node_id"].copy()
    users = np.flatnonzero(g0["node_type"] == gg.NODE_USER)
    ids[users[3]], ids[users[40]], ids[users[41]] = 17, 24, 24          # 17 and 24 now name two users each
    g = dict(g0, node_id=ids)
    assert (ids == 17).sum() == 2 and (ids == 24).sum() == 3
    G = built(amd, g, **OPTS)
    seeds = [0, 5, int(users[3]), 9, int(users[40])]
    tests = [[17, 24], [17], [24, 17, 17], [], [24] + g["node_id"][users[:30]].tolist()]
    for T in (0, 10):
        for top_n in (0, 50):
            want = expected_eval(g, seeds, T, tests, gg.NODE_USER, FOLLOWS, True, top_n)
            assert want[0].max() >= 2                                   # (one test id, several hits)
            check(typed_eval(amd, G, seeds, T, tests, gg.NODE_USER, FOLLOWS, True, top_n), want, ("shared ids", T, top_n))
    G.close()


# ---- 2. boundaries -----------------------------------------------------------------------------------------------------------------

def test_sort_boundary_and_global_counters(amd):
    """4 096 hits in one slot (the one-workgroup sort) and 4 097 in the other (the radix sort); 8 193 keys of the tile are past
    the counting kernel's LDS budget, so its global counters run"""
    g = gg.random_graph(51, n_users=EVAL_SORT_SLOTS + 4, n_items=12, n_likes=260, n_friend=220)
    G = built(amd, g, **OPTS)
    user_ids = g["node_id"][:EVAL_SORT_SLOTS + 4]
    seeds = [2, 7]
    tests = [user_ids[:EVAL_SORT_SLOTS].tolist(), user_ids[:EVAL_SORT_SLOTS + 1].tolist()]
    want = expected_eval(g, seeds, 3, tests, gg.NODE_USER, (), False, 0)
    assert want[0].tolist() == [EVAL_SORT_SLOTS, EVAL_SORT_SLOTS + 1] and want[2].tolist() == [EVAL_SORT_SLOTS + 4] * 2
    check(typed_eval(amd, G, seeds, 3, tests, gg.NODE_USER, (), False, 0), want, "4096 / 4097 hits")
    for top_n in (1025, EVAL_SORT_SLOTS + 1):
        want = expected_eval(g, seeds, 3, tests, gg.NODE_USER, FOLLOWS, True, top_n)
        check(typed_eval(amd, G, seeds, 3, tests, gg.NODE_USER, FOLLOWS, True, top_n), want, ("4096 / 4097 hits, top", top_n))
    G.close()


@pytest.mark.parametrize("m", [CAND_BLOCK, CAND_BLOCK + 1])
def test_a_block_of_candidates(amd, m):
    """256 / 257 nodes of the candidate type: one full block of the compaction, and one row more"""
    g = gg.random_graph(52, n_users=m, n_items=90, n_likes=800, n_friend=300)
    G = built(amd, g, **OPTS)
    rng = np.random.default_rng(6)
    seeds = [0, m - 1, m + 5, 3, 3]
    tests = make_sets(g, seeds, rng)
    for top_n in (0, m - 1, m):
        want = expected_eval(g, seeds, 4, tests, gg.NODE_USER, FOLLOWS, True, top_n)
        check(typed_eval(amd, G, seeds, 4, tests, gg.NODE_USER, FOLLOWS, True, top_n), want, ("block", m, top_n))
    G.close()


@pytest.mark.parametrize("links", [EXCLUDE_SEG_MAX, EXCLUDE_SEG_MAX + 1])
def test_hub_seed_segments(amd, links):
    """a seed whose masked raw list is exactly one full exclusion segment, and one link more: the last link, alone in the
    second segment, is the only one that names its target -- a held-out id that then is no candidate"""
    g = gg.random_graph(31, n_users=300, n_items=80, n_likes=700, n_friend=100)
    lists = _lists(g)
    hub, lonely = 0, 299
    lists[hub] = [(1 + k % 297, gg.EDGE_FOLLOW if k % 3 else gg.EDGE_FRIENDSHIP, 1.0) for k in range(EXCLUDE_SEG_MAX)]
    if links > EXCLUDE_SEG_MAX:
        lists[hub].append((lonely, gg.EDGE_FOLLOW, 1.0))
    lists[lonely].append((5, gg.EDGE_FRIENDSHIP, 1.0))
    g = _flat(g["node_id"], g["node_type"], lists)
    assert g["rowptr"][hub + 1] - g["rowptr"][hub] == links
    G = built(amd, g, **OPTS)
    seeds = [hub, 17, hub]
    tests = [[int(g["node_id"][lonely]), int(g["node_id"][298])], g["node_id"][:300].tolist(), [int(g["node_id"][lonely])]]
    want = expected_eval(g, seeds, 2, tests, gg.NODE_USER, FOLLOWS, True, 0)
    assert want[0][2] == (1 if links == EXCLUDE_SEG_MAX else 0) and want[2][0] == (2 if links == EXCLUDE_SEG_MAX else 1)
    check(typed_eval(amd, G, seeds, 2, tests, gg.NODE_USER, FOLLOWS, True, 0), want, ("hub", links))
    G.close()


# ---- 3. identities -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", GOLDEN, ids=lambda p: os.path.basename(p)[:-5])
def test_item_like_is_recommend_eval_batch(amd, path):
    _, g = load_golden(path)
    n = len(g["node_id"])
    item_ids = g["node_id"][g["node_type"] == gg.NODE_ITEM]
    rng = np.random.default_rng(9)
    for tile_seeds in (1, 4):
        G = built(amd, g, tile_seeds=tile_seeds, tile_group=2)
        rec = amd.Recommender(G)
        for K in (1, 3, 9):
            seeds = ((np.arange(K, dtype=np.int64) * 7 + 1) % n).astype(np.int32)
            tests = [(rng.choice(item_ids, min(len(item_ids), 6), replace=False).tolist() if len(item_ids) else []) + [17, 17]
                     for _ in range(K)]
            tests[-1] = []
            for T in (0, 1, 10):
                want = rec.RecommendationEvalBatch(seeds, D, T, tests)
                for top_n in (0, -1):
                    got = typed_eval(amd, G, seeds, T, tests, gg.NODE_ITEM, (gg.EDGE_LIKE,), False, top_n)
                    check(got, want, (os.path.basename(path), tile_seeds, K, T, top_n))
        G.close()


def test_is_the_harness_over_the_ranked_entry_s_lists(amd, mixed):
    """top_n <= 1024: the Hits/AP loop over the lists rwr_recommend_typed_batch returns"""
    g, _ = mixed
    G = built(amd, g, **OPTS)
    rng = np.random.default_rng(10)
    seeds = [0, 5, 5, 123, 7, 9, 21]
    tests = make_sets(g, seeds, rng)
    for top_n in (1, 7, 100, 1024):
        ids, sc, cnt = typed(amd, G, seeds, 10, top_n, gg.NODE_USER, FOLLOWS, True)
        out = [harness(list(zip(ids[k, :cnt[k]].tolist(), sc[k, :cnt[k]].tolist())), tests[k], 0) for k in range(len(seeds))]
        want = (np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int64))
        check(typed_eval(amd, G, seeds, 10, tests, gg.NODE_USER, FOLLOWS, True, top_n), want, ("ranked entry", top_n))
    G.close()


# ---- 4. the cached candidate list across appends ---------------------------------------------------------------------------------

def test_cache_follows_appended_nodes(amd, mixed):
    g, _ = mixed
    n = len(g["node_id"])
    G = built(amd, g, **OPTS)
    seeds = [0, 5, 9]
    tests = [[90001], [90001, 90003], []]
    before = typed_eval(amd, G, seeds, 4, tests, gg.NODE_USER, FOLLOWS, True, 0)
    check(before, expected_eval(g, seeds, 4, tests, gg.NODE_USER, FOLLOWS, True, 0), "before the append")
    assert not before[0].any()
    G.appendNodes([(90001, gg.NODE_USER), (90002, gg.NODE_ITEM), (90003, gg.NODE_USER)],
                  src=[9, n, n + 2], dst=[n, 5, 0], etype=[gg.EDGE_MENTION, gg.EDGE_FRIENDSHIP, gg.EDGE_FOLLOW], w=[1.0, 1.0, 1.0])
    grown = dict(zip(("node_id", "node_type", "rowptr", "dst", "etype", "w"), G._flat))
    got = typed_eval(amd, G, seeds, 4, tests, gg.NODE_USER, FOLLOWS, True, 0)
    check(got, expected_eval(grown, seeds, 4, tests, gg.NODE_USER, FOLLOWS, True, 0), "after append_nodes")
    assert got[0].tolist() == [1, 2, 0] and (got[2] == before[2] + 2).all()
    G.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(amd, mixed):
    from recommendersystems_amd import _lib
    lib = _lib.load()
    name = b"rwr_recommend_typed_eval_batch"
    g, _ = mixed
    n = len(g["node_id"])
    G = built(amd, g, **OPTS)
    h = G._handle()
    K = 4
    seeds = np.array([0, 5, 9, 123], dtype=np.int32)
    tp = np.array([0, 2, 2, 3, 5], dtype=np.int64)
    ti = g["node_id"][[1, 2, 3, 4, 6]].astype(np.int64)
    hits, sp, ln = np.full(K, -77, dtype=np.int64), np.full(K, -7.5), np.full(K, -9, dtype=np.int64)
    ps, pp, pt = seeds.ctypes.data_as(PI32), tp.ctypes.data_as(PI64), ti.ctypes.data_as(PI64)
    ph, pq, pl = hits.ctypes.data_as(PI64), sp.ctypes.data_as(PD), ln.ctypes.data_as(PI64)

    def call(handle=h, s=ps, k=K, d=D, T=3, top=0, cand=gg.NODE_USER, mask=0x0c, self_=1, p=pp, t=pt, nh=ph, q=pq, m=pl):
        return (lib.rwr_recommend_typed_eval_batch(handle, s, k, C.c_float(d), T, top, cand, mask, self_, p, t, nh, q, m),
                lib.rwr_last_error())

    def untouched():
        return (hits == -77).all() and (sp == -7.5).all() and (ln == -9).all()

    st, msg = call(handle=None, k=-1, cand=999, p=None)               # a NULL graph is refused first
    assert st == _lib.RWR_E_INVALID and b"NULL graph" in msg
    assert call(k=0)[0] == _lib.RWR_OK and untouched()                 # then K == 0 is a no-op, whatever else is wrong
    assert call(k=0, s=None, cand=999, mask=1 << 9, p=None, t=None, nh=None, q=None, m=None)[0] == _lib.RWR_OK
    # the typed arguments, each with its word, found before a bad test set
    for kw, word in ((dict(k=-1), b"negative K"), (dict(s=None), b"seeds"), (dict(cand=-1), b"cand_type"), (dict(cand=256), b"cand_type"),
                     (dict(mask=1 << 8), b"excl_edge_mask"), (dict(mask=0x80000000), b"excl_edge_mask")):
        for extra in (dict(), dict(p=None), dict(nh=None)):
            st, msg = call(**kw, **extra)
            assert st == _lib.RWR_E_INVALID and name in msg and word in msg, (kw, extra, st, msg)
            assert untouched(), kw
    for bad in (-1, n):
        seeds[2] = bad
        st, msg = call(p=None)
        assert st == _lib.RWR_E_RANGE and name in msg and b"batch position 2" in msg, (bad, st, msg)
        assert untouched()
    seeds[2] = 9
    # the test sets and result arrays: eval_check's verdicts
    for kw, word in ((dict(p=None), b"NULL test_ptr"), (dict(nh=None), b"n_hits"), (dict(q=None), b"sum_precision"),
                     (dict(t=None), b"NULL test_ids")):
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
    tp[3:] += 2 ** 31
    st, msg = call()
    assert st == _lib.RWR_E_UNSUPPORTED and b"test set 2" in msg and untouched()
    tp[3:] -= 2 ** 31
    # the domain comes last
    for d in (-0.25, 1.5, float("nan")):
        st, msg = call(d=d)
        assert st == _lib.RWR_E_UNSUPPORTED and b"[0, 1]" in msg and untouched(), d
    neg = dict(g, w=g["w"].copy())
    neg["w"][3] = -1.0
    Gn = built(amd, neg)
    st, msg = call(handle=Gn._handle())
    assert st == _lib.RWR_E_UNSUPPORTED and b"non-negative" in msg and untouched()
    Gn.close()
    # a correct call afterwards answers right; list_len may be NULL; top_n 1025 is legal
    tests = [ti[0:2].tolist(), [], ti[2:3].tolist(), ti[3:5].tolist()]
    want = expected_eval(g, seeds.tolist(), 3, tests, gg.NODE_USER, FOLLOWS, True, 0)
    assert call()[0] == _lib.RWR_OK
    check((hits.copy(), sp.copy(), ln.copy()), want, "after the refusals")
    ln[:] = -9
    assert call(m=None, top=1025, mask=0xFF, cand=255)[0] == _lib.RWR_OK and (ln == -9).all() and not hits.any()
    G.close()
