"""Ranked walks with at most m entries per caller-set group of nodes (rwr_recommend_capped_batch,
rwr_recommend_capped_positions_batch / Recommender.RecommendationCappedBatch).  The expectation is never the code
under test: the rank row comes from oracle/rwr_oracle.py's Model (tests/test_gpu_typed.py's graphs and row cache, as
tests/test_gpu_filtered.py uses them), the candidates are filtered and sorted here -- (score descending, id descending, then
row ascending, the cap's documented choice among equal pairs) -- and walked greedily with a counter per label.  Ids must be
equal, scores bitwise equal.  Every case that claims to test the cap first asserts, from the reference alone, that the cap
drops somebody.

The multi-chunk (split) form runs on the same small graphs through the library's RWR_CAP_CHUNK selector, read
per call: a chunk of 4 rows cuts groups of some forty items into ten chunks."""
import ctypes as C

import numpy as np
import pytest

from tests import graphgen as gg
from tests.test_gpu_typed import _mixed, bits, built, oracle_row

pytestmark = pytest.mark.gpu

D = 0.15
SEL_MAX_K = 1024           # rank_keys.h
CAP_MAX = 8                # RWR_GROUP_CAP_MAX, include/rwr.h
PI64, PI32, PD = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
FOLLOWS = (gg.EDGE_FRIENDSHIP, gg.EDGE_FOLLOW)
LIKE = (gg.EDGE_LIKE,)


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

def filtered_rows(g, row, seed, cand_type, edge_types, exclude_self, pool, deny):
    """F_k as rows: the whole filtered list of one seed, best first"""
    lo, hi = int(g["rowptr"][seed]), int(g["rowptr"][seed + 1])
    out = {int(g["dst"][p]) for p in range(lo, hi) if int(g["etype"][p]) in edge_types}
    if exclude_self:
        out.add(int(seed))
    out |= {int(x) for x in deny}
    inside = None if pool is None else {int(x) for x in pool}
    cand = [i for i in range(len(row))
            if (cand_type is None or g["node_type"][i] == cand_type) and (inside is None or i in inside) and i not in out]
    return sorted(cand, key=lambda i: (-float(row[i]), -int(g["node_id"][i]), i))


def greedy(rows, group_of, m):
    """C_k: the walk from the top with a counter per label; group_of None: no cap"""
    if group_of is None:
        return list(rows)
    seen, kept = {}, []
    for i in rows:
        lb = int(group_of[i])
        if lb < 0:
            kept.append(i)
        elif seen.get(lb, 0) < m:
            kept.append(i)
            seen[lb] = seen.get(lb, 0) + 1
    return kept


def lists_of(g, seeds, T, cand_type, edge_types, exclude_self, pool, deny, group_of, m):
    """per batch position (F_k, C_k) as rows"""
    out = []
    for k, s in enumerate(seeds):
        row = oracle_row(g, int(s), T)
        F = filtered_rows(g, row, int(s), cand_type, set(edge_types), exclude_self, pool, () if deny is None else deny[k])
        out.append((F, greedy(F, group_of, m)))
    return out


def as_arrays(g, seeds, T, lists, top_n):
    K = len(seeds)
    ids, sc, cnt = np.zeros((K, top_n), dtype=np.int64), np.zeros((K, top_n)), np.zeros(K, dtype=np.int32)
    for k, s in enumerate(seeds):
        row = oracle_row(g, int(s), T)
        L = lists[k][1][:top_n]
        cnt[k] = len(L)
        ids[k, :len(L)] = [int(g["node_id"][i]) for i in L]
        sc[k, :len(L)] = [float(row[i]) for i in L]
    return ids, sc, cnt


def as_positions(g, seeds, T, lists, tests):
    pos, sc, ln = [], [], np.zeros(len(seeds), dtype=np.int64)
    for k, s in enumerate(seeds):
        row = oracle_row(g, int(s), T)
        first = {}
        for at, i in enumerate(lists[k][1]):
            first.setdefault(int(g["node_id"][i]), (at, float(row[i])))
        pos.append(np.array([first.get(int(t), (-1, 0.0))[0] for t in tests[k]], dtype=np.int64))
        sc.append(np.array([first.get(int(t), (-1, 0.0))[1] for t in tests[k]], dtype=np.float64))
        ln[k] = len(lists[k][1])
    return pos, sc, ln


def cap_bites(lists):
    """from the reference alone: for at least one seed the capped list differs from the uncapped one"""
    return any(F != Cc for F, Cc in lists)


def check(got, want, what):
    ids, sc, cnt = got
    wi, ws, wc = want
    print(what, "counts", cnt.tolist()[:8], "want", wc.tolist()[:8])
    assert (cnt == wc).all(), (what, "counts", cnt.tolist(), wc.tolist())
    bad = np.flatnonzero((ids != wi).any(axis=1))
    assert bad.size == 0, (what, "ids differ in rows", bad.tolist(), ids[bad[0]].tolist()[:12], wi[bad[0]].tolist()[:12])
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


def capped(amd, G, seeds, T, top_n, cand_type, edge_types=(), exclude_self=False, pool=None, deny=None, group_of=None, m=1):
    return amd.Recommender(G).RecommendationCappedBatch(np.asarray(seeds, dtype=np.int32), D, T, top_n, cand_type, edge_types,
                                                        exclude_self, pool, deny, group_of, m)


def rows_of(g, t):
    return np.flatnonzero(g["node_type"] == t)


def labels(g, groups=5):
    """`groups` labels over the items (sparse values), every eleventh row unlabelled, the users in three groups of their own"""
    n = len(g["node_id"])
    lab = np.full(n, -1, dtype=np.int32)
    items, users = rows_of(g, gg.NODE_ITEM), rows_of(g, gg.NODE_USER)
    lab[items] = 1000 * (1 + np.arange(items.size) % groups) + 7
    lab[users] = 3 + (np.arange(users.size) % 3)
    lab[::11] = -1 - (np.arange(0, n, 11) % 4)
    return lab


def run_case(amd, g, G, seeds, T, cand, edges, self_, pool, deny, lab, m, what, whole=400, must_bite=True):
    """top 10, the whole list, and the whole list's length through the positions entry, against the reference"""
    L = lists_of(g, seeds, T, cand, edges, self_, pool, deny, lab, m)
    if must_bite:
        assert cap_bites(L), (what, "the cap is vacuous on this input")
    assert max(len(F) for F, _ in L) <= whole
    for top_n in (10, whole):
        check(capped(amd, G, seeds, T, top_n, cand, edges, self_, pool, deny, lab, m), as_arrays(g, seeds, T, L, top_n), (what, top_n))
    tests = [[int(g["node_id"][i]) for i in F[:6] + F[-3:]] for F, _ in L]
    got = amd.Recommender(G).RecommendationCappedPositionsBatch(seeds, D, T, tests, cand, edges, self_, pool, deny, lab, m)
    check_positions(got, as_positions(g, seeds, T, L, tests), (what, "positions"))
    return L


# ---- 1. the cap on the mixed graphs ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["weighted", "value_free"])
def test_cap_on_the_mixed_graphs(amd, mixed, unit, which):
    g, (linkless, undef_only) = mixed if which == "weighted" else unit
    G = built(amd, g)
    assert G.stats()["uniform_path"] == (0 if which == "weighted" else 1)
    lab = labels(g)
    seeds = [0, 5, 5, 123, linkless, undef_only, 9]
    for T in (0, 1, 5):                                            # (T = 0 / 1: most scores +0.0, ties by id)
        for m in (1, 2, 3, 8):
            run_case(amd, g, G, seeds, T, gg.NODE_ITEM, LIKE, False, None, None, lab, m, (which, T, m))
    run_case(amd, g, G, seeds, 5, None, FOLLOWS, True, None, None, lab, 2, (which, "any type"))
    run_case(amd, g, G, seeds, 5, gg.NODE_USER, FOLLOWS, True, None, None, lab, 1, (which, "users"))
    G.close()


def test_one_seed_mirror(amd, mixed):
    g, _ = mixed
    G = built(amd, g)
    lab = labels(g)
    got = amd.Recommender(G).RecommendationCapped(5, D, 3, 15, amd.NodeType.ITEM, (amd.EdgeType.LIKE,), False, groupOf=lab, groupCap=2)
    L = lists_of(g, [5], 3, gg.NODE_ITEM, LIKE, False, None, None, lab, 2)
    assert cap_bites(L)
    want = as_arrays(g, [5], 3, L, 15)
    assert [r[0] for r in got] == want[0][0, :want[2][0]].tolist()
    assert (bits([r[1] for r in got]) == bits(want[1][0, :want[2][0]])).all()
    G.close()


# ---- 2. segment edges ----------------------------------------------------------------------------------------------------------------

def test_segment_edges(amd, mixed):
    g, _ = mixed
    n = len(g["node_id"])
    G = built(amd, g)
    rec = amd.Recommender(G)
    items = rows_of(g, gg.NODE_ITEM)
    seeds = [0, 5, 9, 123]
    for m in (1, 2, 3, 8):
        # groups of exactly 1, m and m + 1 candidates, the rest in one large group
        lab = np.full(n, -1, dtype=np.int32)
        lab[items] = 9
        lab[items[0]] = 1
        lab[items[1:1 + m]] = 2
        lab[items[1 + m:2 + 2 * m]] = 3
        L = run_case(amd, g, G, seeds, 5, gg.NODE_ITEM, (), False, None, None, lab, m, ("edges", m))
        for F, Cc in L:                                            # (no exclusion: the small groups are whole in F)
            kept = [int(lab[i]) for i in Cc]
            assert kept.count(1) == 1 and kept.count(2) == m and kept.count(3) == m and kept.count(9) == m
    # every candidate in one group
    one = np.full(n, 42, dtype=np.int32)
    L = run_case(amd, g, G, seeds, 5, gg.NODE_ITEM, LIKE, False, None, None, one, 3, "one group")
    assert all(len(Cc) == 3 for _, Cc in L)
    run_case(amd, g, G, seeds, 1, None, (), False, None, None, one, 1, "one group, any type, T = 1")
    # every candidate its own group, and all labels negative: the filtered call's arrays
    own = (np.arange(n, dtype=np.int32) * 3 + 1).astype(np.int32)
    none = np.full(n, -7, dtype=np.int32)
    want = rec.RecommendationFilteredBatch(seeds, D, 5, 50, gg.NODE_ITEM, LIKE, False)
    wantp = rec.RecommendationFilteredPositionsBatch(seeds, D, 5, [[int(x) for x in g["node_id"][items[:9]]]] * 4, gg.NODE_ITEM, LIKE)
    for lab, m in ((own, 1), (none, 1)):
        Lr = lists_of(g, seeds, 5, gg.NODE_ITEM, LIKE, False, None, None, lab, m)
        assert not cap_bites(Lr)
        check(capped(amd, G, seeds, 5, 50, gg.NODE_ITEM, LIKE, False, None, None, lab, m), want, "identity by labels")
        gotp = rec.RecommendationCappedPositionsBatch(seeds, D, 5, [[int(x) for x in g["node_id"][items[:9]]]] * 4, gg.NODE_ITEM, LIKE,
                                                      False, None, None, lab, m)
        check_positions(gotp, wantp, "identity by labels, positions")
    # a cap of at least the largest group's size: the filtered arrays again
    big = np.full(n, -1, dtype=np.int32)
    big[items] = np.arange(items.size) // 8                        # (eight items per label)
    check(capped(amd, G, seeds, 5, 50, gg.NODE_ITEM, LIKE, False, None, None, big, 8), want, "cap = largest group")
    G.close()


# ---- 3. the multi-chunk path ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["weighted", "value_free"])
def test_split_form_equals_fused_form(amd, mixed, unit, which, monkeypatch):
    g, (linkless, _) = mixed if which == "weighted" else unit
    G = built(amd, g)
    lab = labels(g)
    one = np.full(len(g["node_id"]), 5, dtype=np.int32)
    seeds = [0, 5, 5, 123, linkless, 9, 33]
    tests = [[int(x) for x in g["node_id"][rows_of(g, gg.NODE_ITEM)[:30]]]] * len(seeds)
    for la, m, T in ((lab, 1, 5), (lab, 3, 5), (lab, 8, 1), (one, 2, 5), (one, 8, 0)):
        L = lists_of(g, seeds, T, gg.NODE_ITEM, LIKE, False, None, None, la, m)
        assert cap_bites(L)
        want = as_arrays(g, seeds, T, L, 60)
        monkeypatch.delenv("RWR_CAP_CHUNK", raising=False)
        fused = capped(amd, G, seeds, T, 60, gg.NODE_ITEM, LIKE, False, None, None, la, m)
        fp = amd.Recommender(G).RecommendationCappedPositionsBatch(seeds, D, T, tests, gg.NODE_ITEM, LIKE, False, None, None, la, m)
        check(fused, want, ("fused", m, T))
        for chunk in ("4", "1", "13"):                             # (groups of ~40 and of 200 items: 3 .. 200 chunks a segment)
            monkeypatch.setenv("RWR_CAP_CHUNK", chunk)
            split = capped(amd, G, seeds, T, 60, gg.NODE_ITEM, LIKE, False, None, None, la, m)
            check(split, want, ("split", chunk, m, T))
            check(split, fused, ("split against fused", chunk, m, T))
            sp = amd.Recommender(G).RecommendationCappedPositionsBatch(seeds, D, T, tests, gg.NODE_ITEM, LIKE, False, None, None, la, m)
            check_positions(sp, fp, ("split against fused, positions", chunk, m, T))
    monkeypatch.delenv("RWR_CAP_CHUNK", raising=False)
    G.close()


# ---- 4. tile widths and tile groups ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile_seeds", [1, 2, 4, 8, 16, 32, 64])
def test_every_tile_width(amd, mixed, tile_seeds, monkeypatch):
    g, (linkless, _) = mixed
    G = built(amd, g, tile_seeds=tile_seeds)
    lab = labels(g)
    seeds = [0, 5, 5, linkless, 9, 21, 33, 2, 123]
    L = lists_of(g, seeds, 5, gg.NODE_ITEM, LIKE, False, None, None, lab, 2)
    assert cap_bites(L)
    want = as_arrays(g, seeds, 5, L, 40)
    check(capped(amd, G, seeds, 5, 40, gg.NODE_ITEM, LIKE, False, None, None, lab, 2), want, ("tile width", tile_seeds))
    monkeypatch.setenv("RWR_CAP_CHUNK", "7")
    check(capped(amd, G, seeds, 5, 40, gg.NODE_ITEM, LIKE, False, None, None, lab, 2), want, ("tile width, split", tile_seeds))
    assert G.stats()["tile_seeds"] == tile_seeds
    G.close()


@pytest.mark.parametrize("which", ["weighted", "value_free"])
def test_three_tile_groups(amd, mixed, unit, which, monkeypatch):
    """K = 20 on tiles of 8 seeds, one tile a group: three groups, the last with four padding slots"""
    g, (linkless, undef_only) = mixed if which == "weighted" else unit
    G = built(amd, g, tile_seeds=8, tile_group=1)
    lab = labels(g)
    seeds = [int(s) for s in (np.arange(20) * 5) % 120]
    seeds[7], seeds[13], seeds[18] = seeds[2], linkless, undef_only       # a repeated seed, two dangling ones
    items = [int(x) for x in rows_of(g, gg.NODE_ITEM)]
    deny = [items[k:2 * k] for k in range(20)]
    for T in (1, 5):
        run_case(amd, g, G, seeds, T, gg.NODE_ITEM, LIKE, False, None, deny, lab, 2, ("groups", which, T))
    monkeypatch.setenv("RWR_CAP_CHUNK", "5")
    run_case(amd, g, G, seeds, 5, gg.NODE_ITEM, LIKE, False, None, deny, lab, 2, ("groups, split", which))
    st = G.stats()
    assert st["tile_seeds"] == 8 and st["tile_group"] == 1
    G.close()


# ---- 5. interplay: the allowance goes to the group's next candidate ----------------------------------------------------------------------

def test_removed_candidates_do_not_use_the_allowance(amd, mixed):
    g, _ = mixed
    G = built(amd, g)
    lab = labels(g)
    m, T = 2, 5
    seeds = [0, 5, 9]
    items = [int(x) for x in rows_of(g, gg.NODE_ITEM)]
    base = lists_of(g, seeds, T, gg.NODE_ITEM, (), False, None, None, lab, m)
    assert cap_bites(base)

    def moved_on(L):
        """some seed's capped list holds a member that the unfiltered capped list did not hold: the next of its group"""
        return any(set(Cc) - set(Cb) for (_, Cc), (_, Cb) in zip(L, base))

    # a pool without every seed's best member of each labelled group
    best = set()
    for _, Cb in base:
        best |= {i for i in Cb[:8] if lab[i] >= 0}
    pool = [i for i in items if i not in best]
    L = run_case(amd, g, G, seeds, T, gg.NODE_ITEM, (), False, pool, None, lab, m, "pool")
    assert moved_on(L)
    # a deny list per seed that removes that seed's best labelled member
    deny = [[next(i for i in Cb if lab[i] >= 0)] for _, Cb in base]
    L = run_case(amd, g, G, seeds, T, gg.NODE_ITEM, (), False, None, deny, lab, m, "deny")
    assert all(set(Cc) - set(Cb) for (_, Cc), (_, Cb) in zip(L, base))
    # the link mask: the seeds' LIKE targets are their best-ranked items
    L = run_case(amd, g, G, seeds, T, gg.NODE_ITEM, LIKE, False, None, None, lab, m, "mask")
    assert moved_on(L)
    # exclude_self with the seed labelled: ITEM seeds that are their own group's best member (chosen from the reference)
    tried = [i for i in items if lab[i] >= 0][:12]
    tried_lists = lists_of(g, tried, T, gg.NODE_ITEM, (), False, None, None, lab, 1)
    item_seeds = [s for s, (_, Cc) in zip(tried, tried_lists) if s in Cc][:3]
    assert item_seeds, "no ITEM seed is the best of its group"
    with_self = lists_of(g, item_seeds, T, gg.NODE_ITEM, (), False, None, None, lab, 1)
    L = run_case(amd, g, G, item_seeds, T, gg.NODE_ITEM, (), True, None, None, lab, 1, "self")
    for (_, Cc), (_, Cw), s in zip(L, with_self, item_seeds):
        assert s not in Cc and sum(lab[i] == lab[s] for i in Cc) == 1 and set(Cc) - set(Cw)
    G.close()


# ---- 6. appended nodes ------------------------------------------------------------------------------------------------------------------

def test_labels_for_appended_nodes(amd, mixed):
    from recommendersystems_amd import _lib
    g, _ = mixed
    n = len(g["node_id"])
    G = built(amd, g)
    G.appendNodes([(90001, gg.NODE_ITEM), (90002, gg.NODE_ITEM), (90003, gg.NODE_USER), (90004, gg.NODE_ITEM)],
                  src=[0, 5, 0, 5, 9, n + 2], dst=[n, n, n + 1, n + 3, n + 3, n + 1],
                  etype=[gg.EDGE_MENTION, gg.EDGE_MENTION, gg.EDGE_MENTION, gg.EDGE_MENTION, gg.EDGE_MENTION, gg.EDGE_LIKE],
                  w=[5.0, 5.0, 4.0, 5.0, 5.0, 1.0])
    grown = dict(zip(("node_id", "node_type", "rowptr", "dst", "etype", "w"), G._flat))
    lab = np.concatenate([labels(g), np.array([1007, 1007, 3, 1007], dtype=np.int32)])     # the new items join the first group
    seeds = [0, 5, 9, n + 2]
    L = run_case(amd, grown, G, seeds, 4, gg.NODE_ITEM, (), False, None, None, lab, 2, "appended")
    assert any(i >= n for _, Cc in L for i in Cc[:10]), "no appended item near the top of any list"
    assert any(i >= n for F, Cc in L for i in set(F) - set(Cc)), "the cap drops no appended item"
    with pytest.raises(ValueError):                                 # the mirror refuses the shorter array
        capped(amd, G, seeds, 4, 10, gg.NODE_ITEM, (), False, None, None, lab[:n], 2)
    assert _lib.RWR_GROUP_CAP_MAX == CAP_MAX
    G.close()


# ---- 7. positions -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["weighted", "value_free"])
def test_positions_in_the_capped_lists(amd, mixed, unit, which):
    g, (linkless, _) = mixed if which == "weighted" else unit
    G = built(amd, g)
    rec = amd.Recommender(G)
    lab = labels(g)
    seeds = [0, 5, 5, linkless, 9]
    m = 2
    for T in (0, 1, 5):
        L = lists_of(g, seeds, T, gg.NODE_ITEM, LIKE, False, None, None, lab, m)
        assert cap_bites(L)
        tests = []
        for F, Cc in L:
            dropped = [i for i in F if i not in set(Cc)]
            tests.append([int(g["node_id"][i]) for i in dropped[:4] + Cc[:5] + Cc[-2:] + Cc[:1]] + [987654321])
        got = rec.RecommendationCappedPositionsBatch(seeds, D, T, tests, gg.NODE_ITEM, LIKE, False, None, None, lab, m)
        check_positions(got, as_positions(g, seeds, T, L, tests), ("positions", which, T))
        for k, (F, Cc) in enumerate(L):
            nd = min(4, len(F) - len(Cc))
            assert nd > 0 or not F
            assert got[0][k][:nd].tolist() == [-1] * nd and (bits(got[1][k][:nd]) == 0).all()     # dropped by the cap: -1 / +0.0
            assert got[0][k][nd:nd + min(5, len(Cc))].tolist() == list(range(min(5, len(Cc))))       # kept: the place in C_k
            assert got[2][k] == len(Cc) < len(F) or not F
    G.close()


# ---- 8. identities, determinism, the cache ------------------------------------------------------------------------------------------------

def test_no_labels_is_the_filtered_and_the_typed_entry(amd, mixed):
    g, (linkless, undef_only) = mixed
    G = built(amd, g)
    rec = amd.Recommender(G)
    rng = np.random.default_rng(4)
    seeds = np.array([0, 5, 5, 123, linkless, undef_only, 7, 9, 21, 33, 2], dtype=np.int32)
    tests = [[int(x) for x in g["node_id"][k:k + 9]] + [123456789] for k in range(len(seeds))]
    pool = rng.integers(0, len(g["node_id"]), 250)
    deny = [rng.integers(0, len(g["node_id"]), 12) for _ in seeds]
    same = lambda a, b: (a[0] == b[0]).all() and (bits(a[1]) == bits(b[1])).all() and (a[2] == b[2]).all()
    for cand, mask, self_ in ((gg.NODE_USER, FOLLOWS, True), (gg.NODE_ITEM, LIKE, False), (None, (), False)):
        for T in (0, 1, 5):
            want = rec.RecommendationFilteredBatch(seeds, D, T, 20, cand, mask, self_, pool, deny)
            assert same(rec.RecommendationCappedBatch(seeds, D, T, 20, cand, mask, self_, pool, deny, None, 0), want)     # (group_cap ignored)
            assert same(rec.RecommendationCappedBatch(seeds, D, T, 20, cand, mask, self_, pool, deny, None, 99), want)
            wp = rec.RecommendationFilteredPositionsBatch(seeds, D, T, tests, cand, mask, self_, pool, deny)
            gp = rec.RecommendationCappedPositionsBatch(seeds, D, T, tests, cand, mask, self_, pool, deny, None, -4)
            check_positions(gp, wp, ("no labels", cand, T))
            if cand is not None:
                want = rec.RecommendationTypedBatch(seeds, D, T, 20, cand, mask, self_)
                assert same(rec.RecommendationCappedBatch(seeds, D, T, 20, cand, mask, self_), want)
                wp = rec.RecommendationTypedPositionsBatch(seeds, D, T, tests, cand, mask, self_)
                check_positions(rec.RecommendationCappedPositionsBatch(seeds, D, T, tests, cand, mask, self_), wp, ("typed", cand, T))
    G.close()


def test_the_same_call_twice(amd, unit):
    g, _ = unit
    G = built(amd, g)
    rng = np.random.default_rng(8)
    lab = labels(g)
    seeds = [0, 5, 9, 123, 40]
    pool = rng.integers(0, len(g["node_id"]), 400)
    deny = [rng.integers(0, len(g["node_id"]), 30) for _ in seeds]
    tests = [g["node_id"][rng.integers(0, len(g["node_id"]), 20)] for _ in seeds]
    rec = amd.Recommender(G)
    a = rec.RecommendationCappedBatch(seeds, D, 4, 50, None, FOLLOWS, True, pool, deny, lab, 2)
    pa = rec.RecommendationCappedPositionsBatch(seeds, D, 4, tests, None, FOLLOWS, True, pool, deny, lab, 2)
    rec.RecommendationTypedBatch(seeds, D, 4, 50, gg.NODE_USER)              # (another call in between)
    b = rec.RecommendationCappedBatch(seeds, D, 4, 50, None, FOLLOWS, True, pool, deny, lab, 2)
    pb = rec.RecommendationCappedPositionsBatch(seeds, D, 4, tests, None, FOLLOWS, True, pool, deny, lab, 2)
    assert (a[0] == b[0]).all() and (bits(a[1]) == bits(b[1])).all() and (a[2] == b[2]).all()
    check_positions(pa, pb, "twice")
    L = lists_of(g, seeds, 4, None, FOLLOWS, True, pool, deny, lab, 2)
    assert cap_bites(L)
    check(a, as_arrays(g, seeds, 4, L, 50), "twice: the oracle")
    G.close()


def test_capped_calls_leave_the_cached_lists_usable(amd, mixed):
    g, _ = mixed
    G = built(amd, g)
    lab = labels(g)
    seeds = [0, 5, 9]
    rec = amd.Recommender(G)
    before_i = rec.RecommendationTypedBatch(seeds, D, 3, 20, gg.NODE_ITEM, LIKE, False)
    before_u = rec.RecommendationTypedBatch(seeds, D, 3, 20, gg.NODE_USER, FOLLOWS, True)
    L = lists_of(g, seeds, 3, gg.NODE_ITEM, LIKE, False, None, None, lab, 1)
    assert cap_bites(L)
    for _ in range(2):                                             # the cached ITEM list serves the capped call, twice
        check(capped(amd, G, seeds, 3, 20, gg.NODE_ITEM, LIKE, False, None, None, lab, 1), as_arrays(g, seeds, 3, L, 20), "cached list")
    capped(amd, G, seeds, 3, 20, gg.NODE_USER, FOLLOWS, True, None, None, lab, 1)
    capped(amd, G, seeds, 3, 20, None, (), False, [1, 2, 3, 200, 201], None, lab, 1)
    check(rec.RecommendationTypedBatch(seeds, D, 3, 20, gg.NODE_ITEM, LIKE, False), before_i, "typed ITEM after capped")
    check(rec.RecommendationTypedBatch(seeds, D, 3, 20, gg.NODE_USER, FOLLOWS, True), before_u, "typed USER after capped")
    G.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------

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
    lab = labels(g)
    ids, sc, cnt = np.full((K, top_n), -77, dtype=np.int64), np.full((K, top_n), -7.5), np.full(K, -9, dtype=np.int32)
    pos, psc, ln = np.full(3, -77, dtype=np.int64), np.full(3, -7.5), np.full(K, -9, dtype=np.int64)
    like = 1 << gg.EDGE_LIKE
    P = lambda a, t: None if a is None else a.ctypes.data_as(t)

    def ranked(handle=h, s=seeds, k=K, d=D, top=top_n, cand=gg.NODE_USER, mask=like, pc=4, pi=pool, p=dp, i=di, go=lab, cap=2,
               o=(ids, sc, cnt)):
        st = lib.rwr_recommend_capped_batch(handle, P(s, PI32), k, C.c_float(d), 3, top, cand, mask, 0, pc, P(pi, PI32), P(p, PI64),
                                            P(i, PI32), P(go, PI32), cap, P(o[0], PI64), P(o[1], PD), P(o[2], PI32))
        return st, lib.rwr_last_error()

    def positions(handle=h, s=seeds, k=K, d=D, cand=gg.NODE_USER, mask=like, pc=4, pi=pool, p=dp, i=di, go=lab, cap=2, t=tp, ids_=ti,
                  o=pos):
        st = lib.rwr_recommend_capped_positions_batch(handle, P(s, PI32), k, C.c_float(d), 3, cand, mask, 0, pc, P(pi, PI32),
                                                      P(p, PI64), P(i, PI32), P(go, PI32), cap, P(t, PI64), P(ids_, PI64), P(o, PI64),
                                                      P(psc, PD), P(ln, PI64))
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
    tail_ranked = [(dict(cap=0), INV, b"group_cap 0"), (dict(top=SEL_MAX_K + 1), UNS, b"1024"),
                   (dict(cap=CAP_MAX + 1), UNS, b"RWR_GROUP_CAP_MAX = 8"), (dict(d=1.5), UNS, b"[0, 1]")]
    tail_positions = [(dict(t=None), INV, b"NULL test_ptr"), (dict(o=None), INV, b"NULL pos_out"),
                      (dict(t=np.array([0, 2, 1, 3, 3], dtype=np.int64)), INV, b"test_ptr decreases"),
                      (dict(ids_=None), INV, b"NULL test_ids"), (dict(cap=-1), INV, b"group_cap -1"),
                      (dict(cap=CAP_MAX + 1), UNS, b"RWR_GROUP_CAP_MAX = 8"), (dict(d=1.5), UNS, b"[0, 1]")]
    for call, name, order in ((ranked, b"rwr_recommend_capped_batch", steps + tail_ranked),
                              (positions, b"rwr_recommend_capped_positions_batch", steps + tail_positions)):
        for at, (kw, status, text) in enumerate(order):
            later = {}
            for kw2, _, _ in reversed(order[at + 1:]):
                later.update({k: v for k, v in kw2.items() if k not in kw})
            # (a later fault on the same argument cannot ride along: the argument holds this step's fault)
            st, msg = call(**dict(later, **kw))
            assert st == status and text in msg and name in msg, (name, at, kw.keys(), st, msg)
            assert untouched(), (name, at)
    # what is no fault: K == 0 whatever else is there; no labels with any group_cap
    assert ranked(k=0, s=None, pi=None, p=None, i=None, go=None, cap=-3, o=(None, None, None))[0] == _lib.RWR_OK and untouched()
    assert positions(k=0, s=None, t=None, o=None, cap=0)[0] == _lib.RWR_OK and untouched()
    assert ranked(go=None, cap=0, pc=-1, pi=None)[0] == _lib.RWR_OK and (cnt == top_n).all()
    assert positions(go=None, cap=99)[0] == _lib.RWR_OK and (ln >= 0).all()
    assert ranked(cap=CAP_MAX)[0] == _lib.RWR_OK
    G.close()
    neg = dict(g, w=g["w"].copy())
    neg["w"][3] = -1.0
    Gn = built(amd, neg)
    ids[:], sc[:], cnt[:], pos[:], psc[:], ln[:] = -77, -7.5, -9, -77, -7.5, -9
    for call in (ranked, positions):
        st, msg = call(handle=Gn._handle())
        assert st == UNS and b"non-negative" in msg and untouched()
    Gn.close()
